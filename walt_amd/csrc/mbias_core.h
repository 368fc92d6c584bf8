// mbias_core.h -- methylation bias by read position (include/walt_amd.h, "methylation bias by read position"): which
// counter of a table a call letter belongs to, which records count, and the accumulation of one 16-byte slice of calls.
// Pure inline functions shared by the HIP kernel (mbias.hip) and a g++ unit test (tests/test_mbias_cpu.py compiles
// tests/mbias_harness.cpp).
#ifndef WALT_AMD_MBIAS_CORE_H_
#define WALT_AMD_MBIAS_CORE_H_

#include <stdint.h>
#include <string.h>

#if !defined(WALT_HD)
#if defined(__HIPCC__)
#define WALT_HD __host__ __device__ __forceinline__
#else
#define WALT_HD inline
#endif
#endif

namespace walt {

constexpr uint32_t kMbiasPositions = 1024;              // walt_max_read_len() of the widest pattern (WALT_MBIAS_POSITIONS)
constexpr uint32_t kMbiasCells = 8;                     // (context, m) pairs: cell = 2 * context + m
constexpr uint32_t kMbiasWords = kMbiasCells * kMbiasPositions;  // one table: count[4][2][1024]
constexpr uint32_t kMbiasNoCell = 8;

// The cell 2 * context + m of a call letter, kMbiasNoCell for every other byte.  z 0x7A, x 0x78, h 0x68, u 0x75 and
// their upper-case forms 0x20 below: b | 0x20 is a lower-case letter for exactly those two bytes, so no other byte of
// the 256 reaches a cell.  Upper case is methylated (m = 0).
WALT_HD uint32_t mbias_cell(uint32_t b) {
  const uint32_t low = b | 0x20u;
  const uint32_t ctx = low == 'z' ? 0u : low == 'x' ? 1u : low == 'h' ? 2u : low == 'u' ? 3u : 4u;
  return ctx < 4u ? 2u * ctx + ((b >> 5) & 1u) : kMbiasNoCell;
}

// A record adds to the table when it is unique, not skipped, and its read fits the table; tested before any index is formed.
WALT_HD bool mbias_counted(uint32_t times, uint32_t skip_byte, uint64_t off, uint64_t end) {
  return times == 1u && skip_byte == 0u && end > off && end - off <= (uint64_t)kMbiasPositions;
}

// Slices are cut at the 16-byte boundaries of the calls ARRAY, as the calling kernel cuts the slices it stores: slice
// position k is read position i0 + k, i0 = 16 * s - head with head = the low four address bits of the read's first
// call.  A slice is one aligned 16-byte load wherever its sixteen bytes lie inside the batch's calls -- `before` bytes of
// the batch precede rb, `after` bytes follow from rb on (the read's own included) -- and the bytes of a partial first or
// last slice that belong to a neighbouring read are masked to 0, no letter.  Only a slice that would reach outside the
// batch (the first of its first read, the last of its last) is read byte by byte, so nothing outside the batch's own
// bytes is touched, at any address of the array.
WALT_HD uint32_t mbias_keep_mask(int lo, int hi) {  // the bytes [lo, hi) of a word, lo and hi clamped to 0 .. 4
  lo = lo < 0 ? 0 : lo > 4 ? 4 : lo;
  hi = hi < 0 ? 0 : hi > 4 ? 4 : hi;
  const uint32_t below_hi = hi >= 4 ? ~0u : (1u << (8 * hi)) - 1u;
  const uint32_t below_lo = lo >= 4 ? ~0u : (1u << (8 * lo)) - 1u;
  return below_hi & ~below_lo;
}
WALT_HD void mbias_load_slice(const uint8_t* __restrict__ rb, int len, int i0, uint64_t before, uint64_t after, uint32_t w[4]) {
  if ((long long)i0 >= -(long long)(before < 16 ? before : 16) && (uint64_t)((long long)i0 + 16 > 0 ? i0 + 16 : 0) <= after) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 q = *reinterpret_cast<const uint4*>(rb + i0);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
#else
    memcpy(w, rb + i0, 16);
#endif
    if (i0 < 0 || i0 + 16 > len) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int j = 0; j < 4; ++j) w[j] &= mbias_keep_mask(-i0 - 4 * j, len - i0 - 4 * j);
    }
    return;
  }
  w[0] = w[1] = w[2] = w[3] = 0u;
  for (int k = 0; k < 16; ++k) {
    const int i = i0 + k;
    if (i >= 0 && i < len) w[k >> 2] |= (uint32_t)rb[i] << (8 * (k & 3));
  }
}
// a read on its own: nothing before it, nothing after
WALT_HD void mbias_load_slice(const uint8_t* __restrict__ rb, int len, int i0, uint32_t w[4]) {
  mbias_load_slice(rb, len, i0, 0, (uint64_t)len, w);
}

// bit 7 of every byte of w that is NOT '.': the calls of a read are mostly '.', and a word of four costs one test
WALT_HD uint32_t mbias_not_dot(uint32_t w) {
  const uint32_t x = w ^ 0x2E2E2E2Eu;  // a '.' becomes 0
  return ((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

// The calls of one slice: add(cell, read position) once per letter, in slice order.  Every position handed to add lies
// in [0, len) of a read that mbias_counted accepted, so cell * kMbiasPositions + position indexes one table.
template <class Add>
WALT_HD void mbias_slice(const uint32_t w[4], int i0, Add&& add) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 4; ++j) {
    uint32_t bits = mbias_not_dot(w[j]);
    while (bits) {
      const int k = __builtin_ctz(bits) >> 3;
      bits &= bits - 1u;
      const uint32_t cell = mbias_cell((w[j] >> (8 * k)) & 0xFFu);
      if (cell != kMbiasNoCell) add(cell, (uint32_t)(i0 + 4 * j + k));
    }
  }
}

// One read as a group of the kernel takes it: every slice from -head in steps of 16 (the kernel spreads them over
// the lanes of a group; the order does not matter to a sum).  before / after: as in mbias_load_slice.
template <class Add>
WALT_HD void mbias_read(const uint8_t* __restrict__ rb, int len, uint64_t before, uint64_t after, Add&& add) {
  const int head = (int)((uintptr_t)rb & 15u);
  for (int i0 = -head; i0 < len; i0 += 16) {
    uint32_t w[4];
    mbias_load_slice(rb, len, i0, before, after, w);
    mbias_slice(w, i0, add);
  }
}

}  // namespace walt
#endif  // WALT_AMD_MBIAS_CORE_H_
