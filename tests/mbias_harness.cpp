// mbias_harness.cpp -- CPU test harness (TEST INFRASTRUCTURE) for walt_amd/csrc/mbias_core.h, the per-lane logic of the
// methylation bias kernel, and for the <out>.mbias block writer of walt_amd/csrc/host/hostio.h.  g++ only: no GPU, no
// HIP.  tests/test_mbias_cpu.py compares it with a numpy restatement of include/walt_amd.h, "methylation bias by read
// position".
#include <stdlib.h>
static int mh_alloc(size_t bytes, void** out) { *out = malloc(bytes ? bytes : 1); return *out ? 0 : -5; }
#define HOSTIO_ALLOC(bytes, out) mh_alloc((bytes), (out))
#define HOSTIO_FREE(p) free(p)
#define HOSTIO_ALLOC_ERROR() "out of memory"
#include "../walt_amd/csrc/host/hostio.h"
#include "../walt_amd/csrc/mbias_core.h"

extern "C" {

uint32_t mbias_harness_cell(uint32_t byte) { return walt::mbias_cell(byte); }

// A batch as the kernel takes it: calls is the ADDRESS the offsets index (its low four bits set the slice grid);
// records at records + r * rec_stride (times is the second word); skip null or one byte per record at skip_stride.
// count[8192] is added to.  Returns the number of adds; -1 if an add ever named a word outside the table.
long long mbias_harness_batch(const uint8_t* calls, const uint64_t* offsets, uint32_t n, const uint8_t* records, uint64_t rec_stride,
                              const uint8_t* skip, uint64_t skip_stride, uint64_t* count) {
  long long adds = 0;
  bool bad = false;
  for (uint32_t r = 0; r < n; ++r) {
    const uint64_t off = offsets[r], end = offsets[r + 1];
    uint32_t times;
    memcpy(&times, records + r * rec_stride + 4, 4);
    if (!walt::mbias_counted(times, skip ? skip[r * skip_stride] : 0u, off, end)) continue;
    walt::mbias_read(calls + off, (int)(end - off), off - offsets[0], offsets[n] - off, [&](uint32_t cell, uint32_t pos) {
      if (cell >= walt::kMbiasCells || pos >= walt::kMbiasPositions || pos >= end - off) { bad = true; return; }
      count[cell * walt::kMbiasPositions + pos] += 1;
      ++adds;
    });
  }
  return bad ? -1 : adds;
}

// one slice alone: the sixteen bytes loaded for slice position i0 of a read of `len` calls at rb (0 outside the read),
// with `before` bytes of the batch in front of rb and `after` from rb on
void mbias_harness_slice(const uint8_t* rb, int len, int i0, uint64_t before, uint64_t after, uint8_t* out16) {
  uint32_t w[4];
  walt::mbias_load_slice(rb, len, i0, before, after, w);
  memcpy(out16, w, 16);
}

// the block writer: text into buf (cap bytes); returns the length, or -1 when it does not fit
long long mbias_harness_block(const uint64_t* count, char* buf, uint64_t cap) {
  hostio::Sink s;
  hostio::put_mbias_block(s, count);
  if (s.n > cap) return -1;
  memcpy(buf, s.p, s.n);
  return (long long)s.n;
}

}  // extern "C"
