// meth_harness.cpp -- CPU build of the per-slice methylation calling (walt_amd/csrc/meth_core.h), driven the way the
// HIP kernel drives it: slices cut at the 16-byte boundaries of the calls buffer, eight "lanes" per read.
// Compiled by tests/test_meth_cpu.py:  g++ -O2 -shared -fPIC -I walt_amd/csrc tests/meth_harness.cpp
#include <stdint.h>
#include <string.h>

#include "meth_core.h"

extern "C" {

// One read.  ref: packed reference (A 0, C 1, G 2, T 3; 16 bases per word) with ref_last its last word index;
// bases / calls: the batch buffers (batch_bytes of bases), the read at [off, off + total); counts8: meth[4], unmeth[4].
void meth_harness_read(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, uint8_t* calls, uint64_t off,
                       uint64_t total, uint64_t batch_bytes, uint32_t limit, int mapped, uint32_t pos, uint32_t lo, uint32_t hi, uint32_t ga,
                       uint16_t* counts8) {
  unsigned long long meth = 0, unmeth = 0;
  const uint8_t* rb = bases + off;
  uint8_t* cb = calls + off;
  const long long head = (long long)((uintptr_t)cb & 15u);
  for (uint32_t sub = 0; sub < 8; ++sub)
    for (int i0 = -(int)head + 16 * (int)sub; i0 < (int)total; i0 += 16 * 8) {
      uint32_t out[4];
      walt::meth_read_slice(rb, (int)total, limit, mapped != 0, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out,
                            meth, unmeth);
      walt::meth_store_slice(cb, (int)total, i0, out);
    }
  memcpy(counts8, &meth, 8);
  memcpy(counts8 + 4, &unmeth, 8);
}

}  // extern "C"
