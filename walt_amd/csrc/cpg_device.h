// cpg_device.h -- what the two tables keyed by CpG pair number share on the device side (cpgpairs.hip defines it,
// epialleles.hip uses it): the builder of the pair bitmap and its rank directory, the extraction's launch shape and scan,
// and the block helpers of the count / scan / write passes.
#ifndef WALT_AMD_CPG_DEVICE_H_
#define WALT_AMD_CPG_DEVICE_H_

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "cpgpairs_core.h"

namespace walt {

// the bitmap (n_words words with its zero padding), the directory and the scan words of one object
struct CpgRank {
  uint32_t* bits = nullptr;
  uint32_t* dir = nullptr;
  unsigned long long* scan = nullptr;
  uint64_t n_words = 0;
  uint32_t n_pairs = 0;
};
uint64_t cpg_rank_bytes(const walt_index* idx);
bool cpg_rank_build(const walt_index* idx, CpgRank& r, hipError_t& e);
void cpg_rank_free(CpgRank& r);

struct CpgShape {
  uint64_t w_lo, w_hi;  // the bitmap words that hold [pos_lo, pos_hi)
  uint64_t chunk;       // words per block
  uint32_t n_blocks;
};
CpgShape cpg_extract_shape(const walt_index* idx, uint32_t pos_lo, uint32_t pos_hi);
void cpg_scan_launch(unsigned long long* table, uint32_t n, unsigned long long* total_out, hipStream_t stream);

__device__ __forceinline__ uint32_t cpg_block_sum(uint32_t v, uint32_t* s_red) {  // the block's sum, in every thread
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_red[w];
  return t;
}

// Where the entries of a thread's word go in an ascending write: v entries of this thread -> the entries of the block's
// threads in front of it; total = the block's.  Every thread of the block calls it; s_wave may be rewritten after the
// next __syncthreads.
__device__ __forceinline__ uint32_t cpg_block_before(uint32_t v, uint32_t* s_wave, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d);
    incl += lane >= (uint32_t)d ? o : 0u;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t k = 0; k < kBlock / 64; ++k) {
    before += k < wave ? s_wave[k] : 0u;
    total += s_wave[k];
  }
  return before + incl - v;
}

}  // namespace walt
#endif  // WALT_AMD_CPG_DEVICE_H_
