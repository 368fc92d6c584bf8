// levels_core.h -- genome-wide methylation levels (include/walt_amd.h, "methylation levels"): the class of a forward
// position, the CpG-pair predicate and the two integer statistics of a covered site.  Pure inline functions shared by
// the HIP kernel (pileup.hip k_pile_levels) and a g++ unit test (tests/test_levels_cpu.py compiles
// tests/levels_harness.cpp).
#ifndef WALT_AMD_LEVELS_CORE_H_
#define WALT_AMD_LEVELS_CORE_H_

#include "pileup_core.h"

namespace walt {

constexpr uint32_t kLevelRows = 5;      // CpG, CHG, CHH, unknown (walt_meth_site's contexts), CpG pairs
constexpr uint32_t kLevelPair = 4;      // the pairs' row
constexpr uint32_t kLevelNone = 4;      // levels_class of a position that is no site
constexpr uint32_t kLevelBins = 10;
constexpr uint32_t kLevelRowWords = 16; // sites covered meth unmeth max_depth level_sum hist[10]
constexpr uint32_t kLevelWords = kLevelRows * kLevelRowWords + 2;  // walt_levels in 64-bit words: the rows, offref[2]
constexpr uint32_t kLevelMaxWord = 4;   // max_depth: the one word of a row that folds by maximum

// Row (0 CpG, 1 CHG, 2 CHH, 3 unknown) of forward position f inside the chromosome [lo, hi), kLevelNone where R[f] is
// A or T: pile_site's context, so a summary and an extraction cannot classify a position differently.
//   ext   meth_ref_ext(R, f - 2, last)
WALT_HD uint32_t levels_class(unsigned long long ext, uint32_t f, uint32_t lo, uint32_t hi) {
  uint8_t strand = 0, context = 0;
  return pile_site(ext, f, lo, hi, strand, context) ? (uint32_t)context : kLevelNone;
}

// f starts a CpG pair: R[f] is C, R[f + 1] is G and f + 1 lies in f's chromosome (which ends in front of hi).
WALT_HD bool levels_pair(unsigned long long ext, uint32_t f, uint32_t hi) {
  return ((uint32_t)(ext >> 4) & 3u) == 1u && ((uint32_t)(ext >> 6) & 3u) == 2u && (unsigned long long)f + 1ull < hi;
}

// floor((m << 30) / (m + u)) for m + u > 0; m and u below 2^33 (a pair's sums), so the numerator stays below 2^63.
// The quotient is at most 2^30: a double-precision estimate is off by less than one, and the remainder -- in integers
// -- settles it.  (A 64-bit integer division costs the kernel several times this.)
WALT_HD unsigned long long level_q30(unsigned long long m, unsigned long long u) {
  const unsigned long long d = m + u, num = m << 30;
  long long q = (long long)((double)num / (double)d);
  long long r = (long long)num - q * (long long)d;
  if (r < 0) { --q; r += (long long)d; }
  if (r < 0) { --q; r += (long long)d; }
  if (r >= (long long)d) { ++q; r -= (long long)d; }
  if (r >= (long long)d) { ++q; }
  return (unsigned long long)q;
}

// min(9, 10 * m / (m + u)) in integer division, given q = level_q30(m, u): 10 * m / (m + u) lies less than 10 / 2^30
// above 10 * q / 2^30, so its floor is that one's or the next.
WALT_HD uint32_t level_bin_of(unsigned long long m, unsigned long long u, unsigned long long q) {
  unsigned long long b = (10ull * q) >> 30;
  b += 10ull * m >= (b + 1ull) * (m + u) ? 1ull : 0ull;
  return (uint32_t)(b < kLevelBins - 1 ? b : kLevelBins - 1);
}
WALT_HD uint32_t level_bin(unsigned long long m, unsigned long long u) { return level_bin_of(m, u, level_q30(m, u)); }

}  // namespace walt
#endif  // WALT_AMD_LEVELS_CORE_H_
