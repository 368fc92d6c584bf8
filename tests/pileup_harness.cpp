// pileup_harness.cpp -- CPU build of what the pile-up kernels run per lane (walt_amd/csrc/pileup_core.h on top of
// meth_core.h), driven the way the HIP kernel drives it: slices cut at 16-byte boundaries, eight "lanes" per read,
// every slice's calls added at their forward positions.
// Compiled by tests/test_pileup_cpu.py:  g++ -O2 -shared -fPIC -I walt_amd/csrc tests/pileup_harness.cpp
#include <stdint.h>
#include <string.h>

#include "pileup_core.h"

extern "C" {

// One read.  ref: the packed reference of the record's strand (R or R'), ref_last its last word index; bases: the
// batch's bases (batch_bytes of them), the read at [off, off + total); head: the read's first byte modulo 16 in the
// array the slice grid follows; minus: the record lies on the '-' strand.  meth / unmeth: counters by forward position.
void pileup_harness_read(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, uint32_t head, uint64_t off,
                         uint64_t total, uint64_t batch_bytes, uint32_t limit, int mapped, uint32_t pos, uint32_t lo, uint32_t hi,
                         uint32_t ga, int minus, uint32_t* meth, uint32_t* unmeth) {
  unsigned long long m16 = 0, u16 = 0;
  const uint8_t* rb = bases + off;
  for (uint32_t sub = 0; sub < 8; ++sub)
    for (int i0 = -(int)head + 16 * (int)sub; i0 < (int)total; i0 += 16 * 8) {
      uint32_t out[4], cm, cu;
      walt::meth_read_slice(rb, (int)total, limit, mapped != 0, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out,
                            m16, u16, cm, cu);
      walt::pile_slice(cm, cu, (long long)pos + i0, minus != 0, lo, hi, [&](uint32_t f, bool m) { (m ? meth : unmeth)[f] += 1; });
    }
}

// The site classifier at forward position f of the chromosome [lo, hi); ref: the packed '+' reference.
// -> 0: R[f] is A or T, 1: a site (strand and context written).
int pileup_harness_site(const uint32_t* ref, uint32_t ref_last, uint32_t f, uint32_t lo, uint32_t hi, uint8_t* strand,
                        uint8_t* context) {
  return walt::pile_site(walt::meth_ref_ext(ref, (long long)f - 2, ref_last), f, lo, hi, *strand, *context) ? 1 : 0;
}

}  // extern "C"
