// overlap_core.h -- the overlap of a proper pair (include/walt_amd.h, "overlap of a pair"): which read positions of
// mate 2 lie on forward positions that mate 1 already calls.  Pure inline functions shared by the HIP kernel
// (overlap.hip) and a g++ unit test (tests/test_overlap_cpu.py compiles tests/overlap_harness.cpp).
#ifndef WALT_AMD_OVERLAP_CORE_H_
#define WALT_AMD_OVERLAP_CORE_H_

#include "chrom_core.h"

namespace walt {

constexpr uint64_t kOverlapMaxRead = 1024;  // walt_max_read_len() of the widest pattern: an interval end fits 16 bits

// what can be decided before the chromosome is known: a unique proper pair of two unique mates, both inside the
// genome, neither read longer than any pattern allows
WALT_HD bool overlap_eligible(uint32_t p1, uint32_t times1, uint32_t p2, uint32_t times2, uint32_t best_times,
                              uint64_t len1, uint64_t len2, uint32_t genome_len) {
  return best_times == 1 && times1 == 1 && times2 == 1 && p1 < genome_len && p2 < genome_len &&
         len1 <= kOverlapMaxRead && len2 <= kOverlapMaxRead;
}

// The excluded interval of mate 2 as ex_lo | ex_hi << 16, 0 when there is none.  [lo, hi): the chromosome that holds
// p1 (the caller has looked it up); limit1 = min(len1, call_len1).  Forward position of strand position q:
// q for '+', lo + hi - 1 - q for '-' (pileup_core.h pile_forward).
// trim5_1 / trim3_1 (include/walt_amd.h, "ignored read ends"): mate 1 calls its read positions [trim5_1, limit1 - trim3_1)
// alone, cut by the chromosome's end -- still one interval of forward positions; where mate 1 is ignored mate 2 keeps
// its calls.
WALT_HD uint32_t overlap_interval(uint32_t p1, bool minus1, uint32_t limit1, uint32_t p2, bool minus2, uint32_t len2,
                                  uint32_t lo, uint32_t hi, uint32_t trim5_1, uint32_t trim3_1) {
  if (p2 < lo || p2 >= hi) return 0u;  // mates on different chromosomes
  const long long room1 = (long long)hi - p1;
  const long long top1 = (long long)limit1 - (long long)trim3_1;  // (negative: nothing is called)
  const long long end1 = top1 < room1 ? top1 : room1;  // mate 1 calls the read positions [trim5_1, end1)
  const long long n1 = end1 - (long long)trim5_1;
  if (n1 <= 0) return 0u;
  const long long mirror = (long long)lo + (long long)hi;
  // mate 1's called span [a1, b1) in forward positions
  const long long a1 = minus1 ? mirror - p1 - end1 : (long long)p1 + (long long)trim5_1;
  const long long b1 = a1 + n1;
  // the read positions j of mate 2 with f(p2 + j) in [a1, b1)
  long long e_lo = minus2 ? mirror - p2 - b1 : a1 - p2;
  long long e_hi = minus2 ? mirror - p2 - a1 : b1 - p2;
  e_lo = e_lo < 0 ? 0 : e_lo;
  e_hi = e_hi > (long long)len2 ? (long long)len2 : e_hi;
  return e_lo < e_hi ? (uint32_t)e_lo | ((uint32_t)e_hi << 16) : 0u;
}
WALT_HD uint32_t overlap_interval(uint32_t p1, bool minus1, uint32_t limit1, uint32_t p2, bool minus2, uint32_t len2,
                                  uint32_t lo, uint32_t hi) {
  return overlap_interval(p1, minus1, limit1, p2, minus2, len2, lo, hi, 0u, 0u);
}

// the positions of an interval word that mate 2 could have been called at -- trim5_2 <= j and j + trim3_2 < limit2, with
// `limit2` = min(len2, call_len2): the calls mate 2 can lose
WALT_HD uint32_t overlap_bases(uint32_t excl, uint32_t limit2, uint32_t trim5_2, uint32_t trim3_2) {
  const uint32_t e_lo = excl & 0xFFFFu, e_hi = excl >> 16;
  const uint32_t end2 = limit2 > trim3_2 ? limit2 - trim3_2 : 0u;
  const uint32_t top = e_hi < end2 ? e_hi : end2;
  const uint32_t low = e_lo > trim5_2 ? e_lo : trim5_2;
  return top > low ? top - low : 0u;
}
WALT_HD uint32_t overlap_bases(uint32_t excl, uint32_t limit2) { return overlap_bases(excl, limit2, 0u, 0u); }

// One pair, as a lane of k_pair_overlap decides it: lds / gs / tab the chromosome look-up of chrom_core.h (one
// chrom_find); call_len1 / call_len2 = the caller's clip points, anything >= the length for none; trim = the ignored
// ends of the two mates: trim5_1, trim3_1, trim5_2, trim3_2.  -> the interval word; bases = overlap_bases of it (0 with
// the word).
WALT_HD uint32_t overlap_pair(const uint32_t* lds, const uint32_t* __restrict__ gs, const ChromTab& tab, uint32_t genome_len,
                              uint32_t p1, uint32_t times1, bool minus1, uint32_t p2, uint32_t times2, bool minus2,
                              uint32_t best_times, uint64_t len1, uint64_t len2, uint32_t call_len1, uint32_t call_len2,
                              uint32_t& bases, uint32_t trim5_1, uint32_t trim3_1, uint32_t trim5_2, uint32_t trim3_2) {
  bases = 0;
  if (!overlap_eligible(p1, times1, p2, times2, best_times, len1, len2, genome_len)) return 0u;
  const uint32_t limit1 = call_len1 < (uint32_t)len1 ? call_len1 : (uint32_t)len1;
  const uint32_t limit2 = call_len2 < (uint32_t)len2 ? call_len2 : (uint32_t)len2;
  uint32_t c_lo, c_hi;
  chrom_bounds(lds, gs, tab, p1, c_lo, c_hi);
  const uint32_t word = overlap_interval(p1, minus1, limit1, p2, minus2, (uint32_t)len2, c_lo, c_hi, trim5_1, trim3_1);
  bases = overlap_bases(word, limit2, trim5_2, trim3_2);
  return word;
}
WALT_HD uint32_t overlap_pair(const uint32_t* lds, const uint32_t* __restrict__ gs, const ChromTab& tab, uint32_t genome_len,
                              uint32_t p1, uint32_t times1, bool minus1, uint32_t p2, uint32_t times2, bool minus2,
                              uint32_t best_times, uint64_t len1, uint64_t len2, uint32_t call_len1, uint32_t call_len2,
                              uint32_t& bases) {
  return overlap_pair(lds, gs, tab, genome_len, p1, times1, minus1, p2, times2, minus2, best_times, len1, len2, call_len1,
                      call_len2, bases, 0u, 0u, 0u, 0u);
}

}  // namespace walt
#endif  // WALT_AMD_OVERLAP_CORE_H_
