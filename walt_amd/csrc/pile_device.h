// pile_device.h -- the adds of the kernels that feed a walt_pileup's counters from a batch of reads, eight lanes per read
// (meth.hip k_meth_pile*, variants.hip k_evidence*): one no-return atomic per update, and the two shapes the option
// pile_rows chooses between.
#ifndef WALT_AMD_PILE_DEVICE_H_
#define WALT_AMD_PILE_DEVICE_H_

#include <hip/hip_runtime.h>

#include "pileup_core.h"

namespace walt {

constexpr uint32_t kMethGroup = 8;       // lanes that share a read

// One call of the pile-up: a 32-bit add whose result nobody reads (no value comes back from the memory side).
__device__ __forceinline__ void pile_add(uint32_t* __restrict__ plane, uint32_t f) {
  (void)__hip_atomic_fetch_add(plane + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// kPile = 2: the eight slices of a group's trip taken one after the other, lane t of the group adding the calls at
// slice positions t and t + 8: the lanes of one instruction hold neighbouring positions (8 x 4 bytes of one plane),
// where kPile = 1 has every lane walk its own slice (16 positions apart from its neighbour's).  All eight lanes of a
// group arrive together (the trip count is the group's); q0 = the genome position of slice 0, position 0.
__device__ __forceinline__ void pile_rows(uint32_t cm, uint32_t cu, long long q0, uint32_t sub, bool minus, uint32_t lo,
                                          uint32_t hi, uint32_t* const plane[2]) {
#pragma unroll
  for (uint32_t s = 0; s < kMethGroup; ++s) {
    const uint32_t bm = (uint32_t)__shfl((int)cm, (int)s, kMethGroup), bu = (uint32_t)__shfl((int)cu, (int)s, kMethGroup);
    if (!(bm | bu)) continue;  // (the same for the whole group)
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
      const uint32_t k = sub + 8u * half;
      const uint32_t f = pile_forward(q0 + 16 * (long long)s + k, minus, lo, hi);
      if ((bm >> (2u * k)) & 1u) pile_add(plane[0], f);
      if ((bu >> (2u * k)) & 1u) pile_add(plane[1], f);
    }
  }
}

}  // namespace walt
#endif  // WALT_AMD_PILE_DEVICE_H_
