// trim_harness.cpp -- CPU build of what the calling kernel and the overlap kernel run per lane with ignored read ends
// (include/walt_amd.h, "ignored read ends": the new overloads of walt_amd/csrc/meth_core.h and overlap_core.h), driven
// the way the HIP kernels drive them, and of the command line's value parser and <out>.methstats settings line
// (walt_amd/csrc/host/hostio.h).  g++ only: no GPU, no HIP.
// Compiled by tests/test_trim_cpu.py:  g++ -O2 -shared -fPIC -fopenmp -I walt_amd/csrc tests/trim_harness.cpp
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "host/hostio.h"
#include "meth_core.h"
#include "overlap_core.h"

extern "C" {

// One read as a group of eight lanes takes it (meth.hip, meth_call_body): slices cut at the 16-byte boundaries of the
// calls array, the 3' bound taken off the limit, the 5' bound handed to every slice.  limit = min(length, call_len).
// which = 0: the overload with trim5; 1 / 2 / 3: the three older signatures (they take no bounds: the caller passes 0, 0
// and compares).  cmu: the slices' cm and cu flags by read position (bit 0 methylated, bit 1 unmethylated).
void trim_harness_read(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, uint8_t* calls, uint64_t off, uint64_t total,
                       uint64_t batch_bytes, uint32_t limit, uint32_t pos, uint32_t lo, uint32_t hi, uint32_t ga, uint32_t ex_lo,
                       uint32_t ex_hi, uint32_t trim5, uint32_t trim3, int which, uint16_t* counts8, uint8_t* cmu) {
  unsigned long long meth = 0, unmeth = 0;
  const uint8_t* rb = bases + off;
  uint8_t* cb = calls + off;
  const long long head = (long long)((uintptr_t)cb & 15u);
  if (which == 0) limit = walt::meth_trim_limit(limit, trim3);
  const bool mapped = limit != 0;
  for (uint32_t sub = 0; sub < 8; ++sub)
    for (int i0 = -(int)head + 16 * (int)sub; i0 < (int)total; i0 += 16 * 8) {
      uint32_t out[4], cm = 0, cu = 0;
      if (which == 0)
        walt::meth_read_slice(rb, (int)total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out, meth,
                              unmeth, cm, cu, ex_lo, ex_hi, trim5);
      else if (which == 1)
        walt::meth_read_slice(rb, (int)total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out, meth,
                              unmeth, cm, cu, ex_lo, ex_hi);
      else if (which == 2)
        walt::meth_read_slice(rb, (int)total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out, meth,
                              unmeth, cm, cu);
      else
        walt::meth_read_slice(rb, (int)total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out, meth,
                              unmeth);
      walt::meth_store_slice(cb, (int)total, i0, out);
      for (int k = 0; k < 16; ++k) {
        const int i = i0 + k;
        if (cmu && i >= 0 && i < (int)total) cmu[i] |= (uint8_t)(((cm >> (2 * k)) & 1u) | (((cu >> (2 * k)) & 1u) << 1));
      }
    }
  memcpy(counts8, &meth, 8);
  memcpy(counts8 + 4, &unmeth, 8);
}

// A batch of n reads on one chromosome [lo, hi), every read through trim_harness_read with the batch's bounds; recs:
// per read pos, call_len, ga, excl word (four words).  -> the sum of all sixteen-bit counts (something to print).
// tests/trim_sanitize_main.cpp hands over heap blocks that begin or end with the batch.
unsigned long long trim_harness_batch(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, uint8_t* calls,
                                      const uint64_t* offsets, uint32_t n, const uint32_t* recs, uint32_t lo, uint32_t hi,
                                      uint32_t trim5, uint32_t trim3) {
  unsigned long long sum = 0;
  for (uint32_t r = 0; r < n; ++r) {
    const uint64_t len = offsets[r + 1] - offsets[r];
    if (!len) continue;
    const uint32_t* rec = recs + 4 * (size_t)r;
    const uint32_t limit = rec[1] < (uint32_t)len ? rec[1] : (uint32_t)len;
    uint16_t counts[8];
    trim_harness_read(ref, ref_last, bases, calls, offsets[r], len, offsets[n], limit, rec[0], lo, hi, rec[2], rec[3] & 0xFFFFu,
                      rec[3] >> 16, trim5, trim3, 0, counts, nullptr);
    for (int k = 0; k < 8; ++k) sum += counts[k];
  }
  return sum;
}

// the flag masks alone: the overload with trim5 (out[0..2]) against the one without (out[3..5])
void trim_harness_flags(long long i0, long long p, long long lo, long long hi, long long limit, uint32_t ga, long long ex_lo,
                        long long ex_hi, long long trim5, uint32_t* out6) {
  walt::meth_slice_flags(i0, p, lo, hi, limit, ga, out6[0], out6[1], out6[2], ex_lo, ex_hi, trim5);
  walt::meth_slice_flags(i0, p, lo, hi, limit, ga, out6[3], out6[4], out6[5], ex_lo, ex_hi);
}

// One pair as a lane of k_pair_overlap decides it.  trim: trim5_1, trim3_1, trim5_2, trim3_2, or null for the older
// overload.  -> the interval word; *bases = the second total's share of the pair.
uint32_t trim_harness_pair(const uint32_t* start, uint32_t n_chrom, uint32_t genome_len, uint32_t p1, uint32_t times1,
                           uint32_t strand1, uint32_t p2, uint32_t times2, uint32_t strand2, uint32_t best_times, uint64_t len1,
                           uint64_t len2, int has_cl1, uint32_t cl1, int has_cl2, uint32_t cl2, const uint32_t* trim, uint32_t* bases) {
  const walt::ChromTab tab = walt::chrom_tab_of(n_chrom);
  std::vector<uint32_t> lds((size_t)tab.m + 1);
  for (uint32_t i = 0; i <= tab.m; ++i) lds[i] = start[walt::chrom_tab_word(tab, i)];
  if (!trim)
    return walt::overlap_pair(lds.data(), start, tab, genome_len, p1, times1, strand1 == '-', p2, times2, strand2 == '-', best_times,
                              len1, len2, has_cl1 ? cl1 : ~0u, has_cl2 ? cl2 : ~0u, *bases);
  return walt::overlap_pair(lds.data(), start, tab, genome_len, p1, times1, strand1 == '-', p2, times2, strand2 == '-', best_times,
                            len1, len2, has_cl1 ? cl1 : ~0u, has_cl2 ? cl2 : ~0u, *bases, trim[0], trim[1], trim[2], trim[3]);
}

// bin/walt's value parser: -> 1 and *out when `text` is a number from 0 to 1024, else 0
int trim_harness_parse(const char* text, uint32_t* out) { return hostio::parse_ignore_value(text, *out) ? 1 : 0; }

// the settings line of <out>.methstats -> its length (the text in `out`, cap bytes)
uint32_t trim_harness_ignore_line(const uint32_t* v, int n, char* out, uint32_t cap) {
  hostio::Sink s;
  hostio::put_ignore_line(s, v, n);
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}

}  // extern "C"
