// chrom_core.h -- the chromosome of a genome position (getChromID, reference.cpp:43-60) for ANY number of sequences:
// the sampled table of chromosome starts the kernels keep in LDS and the look-up over it.  Pure inline functions
// shared by the HIP kernels (map_common.h includes this file) and a g++ unit test (tests/test_chrom_cpu.py compiles
// tests/chrom_harness.cpp).
#ifndef WALT_AMD_CHROM_CORE_H_
#define WALT_AMD_CHROM_CORE_H_

#include "core.h"

namespace walt {

constexpr uint32_t kLdsChroms = 1023;  // start_index entries staged in LDS when they fit

// getChromID (reference.cpp:43-60) with a fixed number of steps: largest l with
// si[l] <= pos.  top_step = largest power of two <= n_chrom (wave-uniform).
WALT_HD uint32_t chrom_id_steps(const uint32_t* si, uint32_t n_chrom, uint32_t top_step, uint32_t pos) {
  uint32_t l = 0;
  for (uint32_t step = top_step; step; step >>= 1) {
    const uint32_t c = l + step;
    const uint32_t v = si[c <= n_chrom ? c : n_chrom];
    l = (c <= n_chrom && pos >= v) ? c : l;
  }
  return l;
}
WALT_HD uint32_t top_step_of(uint32_t n_chrom) {
#if defined(__HIP_DEVICE_COMPILE__)
  return n_chrom ? 1u << (31 - __clz((int)n_chrom)) : 0u;
#else
  return n_chrom ? 1u << (31 - __builtin_clz(n_chrom)) : 0u;
#endif
}

// Chromosome starts for ANY number of sequences (round 4; an assembly like hg38's analysis set has 3,366).  Up to
// kLdsChroms sequences the LDS array holds every start.  Beyond that it holds every 2^shift-th start (shift the
// smallest that fits) plus the genome's end: getChromID (reference.cpp:43-60: the largest l with start[l] <= pos) is a
// search over the sampled starts in LDS, then over the at most 2^shift starts between two samples -- for shift <= 2
// (up to 4,092 sequences) five neighbouring words of the device array fetched together, no search.  Before, every
// candidate of such an assembly paid a bisection of log2(n) DEPENDENT loads over the device array in every kernel
// (3,000 contigs: pass 1 18.9 against 10.7 ms, stage kernels 38 against 16, verifier 27 against 13).
struct ChromTab {
  uint32_t n_chrom, shift, m, top;  // m = sampled intervals = ceil(n_chrom / 2^shift) <= kLdsChroms, top = top_step_of(m)
};
WALT_HD ChromTab chrom_tab_of(uint32_t n_chrom) {
  ChromTab t;
  t.n_chrom = n_chrom;
  uint32_t sh = 0;
  while (((n_chrom + (1u << sh) - 1u) >> sh) > kLdsChroms) ++sh;  // (uniform: scalar)
  t.shift = sh;
  t.m = (n_chrom + (1u << sh) - 1u) >> sh;
  t.top = top_step_of(t.m);
  return t;
}
// word i (0 .. m) of the staged table is this word of the device array: every 2^shift-th start, then the genome's end
WALT_HD uint32_t chrom_tab_word(const ChromTab& t, uint32_t i) {
  const uint32_t c = i << t.shift;
  return c < t.n_chrom ? c : t.n_chrom;
}
// chr = getChromID(pos); c_lo / c_hi = its first base and the next chromosome's (lds: the staged samples, words 0 .. m;
// gs: the device array, words 0 .. n_chrom)
WALT_HD void chrom_find(const uint32_t* lds, const uint32_t* __restrict__ gs, const ChromTab& t, uint32_t pos,
                        uint32_t& chr, uint32_t& c_lo, uint32_t& c_hi) {
  uint32_t ci = chrom_id_steps(lds, t.m, t.top, pos);
  ci = ci < t.m ? ci : (t.m ? t.m - 1u : 0u);  // (a position at or beyond the genome's end: the last interval)
  if (t.shift == 0) {  // (uniform)
    chr = ci; c_lo = lds[ci]; c_hi = lds[ci + 1];
    return;
  }
  const uint32_t base = ci << t.shift;
  if (t.shift <= 2) {
    uint32_t w[5];
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) w[k] = gs[base + k < t.n_chrom ? base + k : t.n_chrom];  // independent loads, one or two lines
    uint32_t off = 0;
    c_lo = w[0]; c_hi = w[1];
#pragma unroll
    for (uint32_t k = 1; k < 4; ++k) {
      const bool take = k < (1u << t.shift) && base + k < t.n_chrom && pos >= w[k];
      off = take ? k : off;
      c_lo = take ? w[k] : c_lo;
      c_hi = take ? w[k + 1] : c_hi;
    }
    chr = base + off;
    return;
  }
  const uint32_t nsub = t.n_chrom - base < (1u << t.shift) ? t.n_chrom - base : (1u << t.shift);
  uint32_t off = chrom_id_steps(gs + base, nsub, 1u << t.shift, pos);
  off = off < nsub ? off : nsub - 1u;  // (at or beyond the genome's end the search stops ON the end: the last chromosome)
  chr = base + off; c_lo = gs[base + off]; c_hi = gs[base + off + 1];
}
WALT_HD void chrom_bounds(const uint32_t* lds, const uint32_t* __restrict__ gs, const ChromTab& t, uint32_t pos,
                          uint32_t& c_lo, uint32_t& c_hi) {
  uint32_t chr;
  chrom_find(lds, gs, t, pos, chr, c_lo, c_hi);
}

}  // namespace walt
#endif  // WALT_AMD_CHROM_CORE_H_
