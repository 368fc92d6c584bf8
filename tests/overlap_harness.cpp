// overlap_harness.cpp -- CPU build of what the overlap kernel runs per lane (walt_amd/csrc/overlap_core.h over the
// chromosome look-up of chrom_core.h) and of the calling kernel's slices with an excluded interval (the new overloads
// of walt_amd/csrc/meth_core.h), driven the way the HIP kernels drive them.
// Compiled by tests/test_overlap_cpu.py:  g++ -O2 -shared -fPIC -I walt_amd/csrc tests/overlap_harness.cpp
#include <stdint.h>
#include <string.h>

#include <vector>

#include "meth_core.h"
#include "overlap_core.h"

extern "C" {

// One pair.  start: the chromosome starts (n_chrom + 1 words), staged as the kernel stages them; has_cl1 / has_cl2: the
// caller gave a call_len array.  -> the interval word; *bases = the second total's share of the pair.
uint32_t overlap_harness_pair(const uint32_t* start, uint32_t n_chrom, uint32_t genome_len, uint32_t p1, uint32_t times1,
                              uint32_t strand1, uint32_t p2, uint32_t times2, uint32_t strand2, uint32_t best_times, uint64_t len1,
                              uint64_t len2, int has_cl1, uint32_t cl1, int has_cl2, uint32_t cl2, uint32_t* bases) {
  const walt::ChromTab tab = walt::chrom_tab_of(n_chrom);
  std::vector<uint32_t> lds((size_t)tab.m + 1);
  for (uint32_t i = 0; i <= tab.m; ++i) lds[i] = start[walt::chrom_tab_word(tab, i)];
  return walt::overlap_pair(lds.data(), start, tab, genome_len, p1, times1, strand1 == '-', p2, times2, strand2 == '-', best_times,
                            len1, len2, has_cl1 ? cl1 : ~0u, has_cl2 ? cl2 : ~0u, *bases);
}

// One read, as meth_harness.cpp's, with the excluded interval [ex_lo, ex_hi); which = 0: the new overload, 1: the old
// signature with cm / cu, 2: the old signature without (both must give what an empty interval gives).
// cmu: the slices' cm and cu flags OR-ed by read position, one byte per base (bit 0 methylated, bit 1 unmethylated).
void overlap_harness_read(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, uint8_t* calls, uint64_t off,
                          uint64_t total, uint64_t batch_bytes, uint32_t limit, int mapped, uint32_t pos, uint32_t lo, uint32_t hi,
                          uint32_t ga, uint32_t ex_lo, uint32_t ex_hi, int which, uint16_t* counts8, uint8_t* cmu) {
  unsigned long long meth = 0, unmeth = 0;
  const uint8_t* rb = bases + off;
  uint8_t* cb = calls + off;
  const long long head = (long long)((uintptr_t)cb & 15u);
  for (uint32_t sub = 0; sub < 8; ++sub)
    for (int i0 = -(int)head + 16 * (int)sub; i0 < (int)total; i0 += 16 * 8) {
      uint32_t out[4], cm = 0, cu = 0;
      if (which == 0)
        walt::meth_read_slice(rb, (int)total, limit, mapped != 0, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out,
                              meth, unmeth, cm, cu, ex_lo, ex_hi);
      else if (which == 1)
        walt::meth_read_slice(rb, (int)total, limit, mapped != 0, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out,
                              meth, unmeth, cm, cu);
      else
        walt::meth_read_slice(rb, (int)total, limit, mapped != 0, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out,
                              meth, unmeth);
      walt::meth_store_slice(cb, (int)total, i0, out);
      for (int k = 0; k < 16; ++k) {
        const int i = i0 + k;
        if (i >= 0 && i < (int)total) cmu[i] |= (uint8_t)(((cm >> (2 * k)) & 1u) | (((cu >> (2 * k)) & 1u) << 1));
      }
    }
  memcpy(counts8, &meth, 8);
  memcpy(counts8 + 4, &unmeth, 8);
}

// the flag masks alone: new overload against the old signature
void overlap_harness_flags(long long i0, long long p, long long lo, long long hi, long long limit, uint32_t ga, long long ex_lo,
                           long long ex_hi, uint32_t* out6) {
  walt::meth_slice_flags(i0, p, lo, hi, limit, ga, out6[0], out6[1], out6[2], ex_lo, ex_hi);
  walt::meth_slice_flags(i0, p, lo, hi, limit, ga, out6[3], out6[4], out6[5]);
}

}  // extern "C"
