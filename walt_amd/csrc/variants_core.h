// variants_core.h -- opposite-strand evidence (include/walt_amd.h, "opposite-strand evidence"): which bases of one
// 16-base slice of a read are evidence, which of them show the reference base, and the rule that judges a position's
// two counters.  Pure inline functions shared by the HIP kernels (variants.hip) and a g++ unit test
// (tests/test_variants_cpu.py compiles tests/variants_harness.cpp).
#ifndef WALT_AMD_VARIANTS_CORE_H_
#define WALT_AMD_VARIANTS_CORE_H_

#include "pileup_core.h"

namespace walt {

struct EvSlice {
  uint32_t match, other;  // field masks of the evidence positions that show the reference base / any other base
};

// One slice (meth_slice's rd, ext, ga and call): the calling rule with the conversion exchanged.
//   ga 0  conversion 'T': evidence where the reference is G, a match where the read base is G
//   ga 1  conversion 'A': evidence where the reference is C, a match where the read base is C
// (reference codes A 0, C 1, G 2, T 3; read fields A 0, C 1, T 2, G 3: meth_read_fields)
WALT_HD EvSlice ev_slice(const uint32_t rd[4], unsigned long long ext, uint32_t ga, uint32_t call) {
  const uint32_t cur = (uint32_t)(ext >> 4);
  const uint32_t e = meth_eq2(cur, ga ? 1u : 2u) & call;
  const uint32_t m = e & meth_eq2(meth_read_fields(rd), ga ? 1u : 3u);
  return {m, e & ~m};
}

// A record that adds evidence at all: the pile-up's validity rule (times == 1, skip byte 0, a position inside the
// genome, a known conversion, 1 to 1024 bases).  len: the read's length as its offsets give it.
WALT_HD bool ev_record_counts(uint32_t times, uint32_t skip, uint32_t pos, uint32_t genome_len, uint32_t cv,
                              unsigned long long len) {
  return times == 1u && !skip && pos < genome_len && (cv == 'T' || cv == 'A') && len >= 1 && len <= 1024;
}

// The slice of a counted read that starts at read position i0 (meth_read_slice's grid: -15 .. total - 1), the read at
// genome position pos of its strand in the chromosome [lo, hi), limit = min(length, call_len).  before / after: the
// bytes of the batch's bases in front of rb and from rb on; a partial slice is loaded whole where its 16 bytes lie
// inside the batch and byte by byte at the batch's two ends, exactly as meth_read_slice loads it.  A slice with no
// position to judge returns before it loads anything.
// kQual: qb = the read's first quality byte, min_qual the floor (include/walt_amd.h, "minimum base quality"): loaded and
// applied as meth_read_slice_q does, a position below the floor adds to neither counter.
template <bool kQual>
WALT_HD EvSlice ev_read_slice_q(const uint8_t* rb, int total, uint32_t limit, uint32_t pos, uint32_t lo, uint32_t hi,
                                uint32_t ga, const uint32_t* ref, uint32_t ref_last, int i0, unsigned long long before,
                                unsigned long long after, const uint8_t* qb, uint32_t min_qual) {
  if (i0 >= (int)limit) return {0u, 0u};
  uint32_t call, v1, v2;
  meth_slice_flags(i0, pos, lo, hi, limit, ga, call, v1, v2);
  if (!call) return {0u, 0u};
  uint32_t rd[4] = {0, 0, 0, 0}, qd[4] = {0, 0, 0, 0};
  if ((i0 >= 0 || (unsigned long long)(-i0) <= before) && (unsigned long long)(i0 + 16) <= after) {
    __builtin_memcpy(rd, rb + i0, 16);
    if (kQual) __builtin_memcpy(qd, qb + i0, 16);  // (the qualities' alignment may differ from the bases')
  } else {
    for (int k = 0; k < 16; ++k) {
      const int i = i0 + k;
      if (i >= 0 && i < total) rd[k >> 2] |= (uint32_t)rb[i] << (8 * (k & 3));
      if (kQual && i >= 0 && i < total) qd[k >> 2] |= (uint32_t)qb[i] << (8 * (k & 3));
    }
  }
  if (kQual) {
    call &= meth_qual_mask(qd, min_qual);
    if (!call) return {0u, 0u};
  }
  return ev_slice(rd, meth_ref_ext(ref, (long long)pos + i0 - 2, ref_last), ga, call);
}
WALT_HD EvSlice ev_read_slice(const uint8_t* rb, int total, uint32_t limit, uint32_t pos, uint32_t lo, uint32_t hi,
                              uint32_t ga, const uint32_t* ref, uint32_t ref_last, int i0, unsigned long long before,
                              unsigned long long after) {
  return ev_read_slice_q<false>(rb, total, limit, pos, lo, hi, ga, ref, ref_last, i0, before, after, nullptr, 0u);
}

// The rule.  A position is judged when its two counters sum to min_depth or more, and flagged when it is judged and
// more than max_percent percent of them are `other`; 64-bit products, so exact up to match = other = 2^32 - 1.
WALT_HD bool ev_judged(uint32_t match, uint32_t other, uint32_t min_depth) {
  return (unsigned long long)match + other >= min_depth;
}
WALT_HD bool ev_flagged(uint32_t match, uint32_t other, uint32_t min_depth, uint32_t max_percent) {
  const unsigned long long total = (unsigned long long)match + other;
  return total >= min_depth && 100ull * other > (unsigned long long)max_percent * total;
}

}  // namespace walt
#endif  // WALT_AMD_VARIANTS_CORE_H_
