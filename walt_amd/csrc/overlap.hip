// overlap.hip -- the overlap of a proper pair on the device (include/walt_amd.h, "overlap of a pair"): one kernel that
// turns every walt_pair_result of a batch into the interval of mate 2's read positions whose forward positions mate 1
// already calls.  The per-lane logic is overlap_core.h's.  The reference has no such mode; the contract is the header's.
#include <string.h>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "overlap_core.h"

namespace walt {

constexpr uint32_t kOverlapTotals = 2;  // pairs with a non-empty interval, mate-2 bases excluded
static_assert(sizeof(walt_pair_result) == 64 && offsetof(walt_pair_result, m2) == 16 && offsetof(walt_pair_result, best_times) == 32,
              "k_pair_overlap reads a walt_pair_result by word");

struct OverlapArgs {
  const uint32_t* start_index;
  uint32_t n_chrom;
  uint32_t genome_len;
  const uint32_t* pairs;       // walt_pair_result[n], sixteen words each
  const uint64_t* offsets1;    // n + 1 each: only the differences are used
  const uint64_t* offsets2;
  const uint32_t* call_len1;   // null: the whole read
  const uint32_t* call_len2;
  uint32_t n;
  uint32_t* excl;
  unsigned long long* totals;  // null: not wanted
  uint32_t trim[4];            // the ignored read ends: trim5_1, trim3_1, trim5_2, trim3_2 (all 0: none)
};

// One pair per lane: 64 bytes of record, two offsets per mate, the optional clip points, one look-up over the staged
// chromosome starts, one word out.
__global__ __launch_bounds__(kBlock) void k_pair_overlap(const OverlapArgs a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  __shared__ unsigned long long s_red[kBlock / 64][kOverlapTotals];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t word = 0, bases = 0;
  if (i < a.n) {
    const uint32_t* rec = a.pairs + i * 16;
    const uint32_t p1 = rec[0], t1 = rec[1], s1 = rec[2] & 0xFFu;
    const uint32_t p2 = rec[4], t2 = rec[5], s2 = rec[6] & 0xFFu;
    const uint32_t best_times = rec[8];
    const uint64_t b1 = a.offsets1[i], e1 = a.offsets1[i + 1], b2 = a.offsets2[i], e2 = a.offsets2[i + 1];
    const uint64_t len1 = e1 > b1 ? e1 - b1 : 0, len2 = e2 > b2 ? e2 - b2 : 0;
    word = overlap_pair(s_start, a.start_index, tab, a.genome_len, p1, t1, s1 == '-', p2, t2, s2 == '-', best_times, len1, len2,
                        a.call_len1 ? a.call_len1[i] : ~0u, a.call_len2 ? a.call_len2[i] : ~0u, bases, a.trim[0], a.trim[1], a.trim[2], a.trim[3]);
    a.excl[i] = word;
  }
  if (!a.totals) return;  // (uniform)
  // wavefront, block, then one add per block and total
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long v[kOverlapTotals] = {word ? 1ull : 0ull, bases};
#pragma unroll
  for (uint32_t k = 0; k < kOverlapTotals; ++k) {
    for (int d = 32; d > 0; d >>= 1) v[k] += __shfl_down(v[k], d);
    if (lane == 0) s_red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < kOverlapTotals) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_red[w][threadIdx.x];
    if (t) atomicAdd(&a.totals[threadIdx.x], t);
  }
}

// one batch as the kernel reads it (device arrays)
struct OverlapBatch {
  const void *pairs, *offsets1, *offsets2;
  uint32_t n;
  const void *call_len1, *call_len2;
  void *excl, *totals;
  uint32_t trim[4] = {0, 0, 0, 0};  // trim5_1, trim3_1, trim5_2, trim3_2
};

static int overlap_launch(walt_index* idx, const OverlapBatch& b, hipStream_t stream) {
  if (b.n == 0) return WALT_OK;
  WALT_HIP(hipSetDevice(idx->device));
  OverlapArgs a;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  a.genome_len = idx->head.genome_len;
  a.pairs = static_cast<const uint32_t*>(b.pairs);
  a.offsets1 = static_cast<const uint64_t*>(b.offsets1);
  a.offsets2 = static_cast<const uint64_t*>(b.offsets2);
  a.call_len1 = static_cast<const uint32_t*>(b.call_len1);
  a.call_len2 = static_cast<const uint32_t*>(b.call_len2);
  a.n = b.n;
  a.excl = static_cast<uint32_t*>(b.excl);
  a.totals = static_cast<unsigned long long*>(b.totals);
  for (int k = 0; k < 4; ++k) a.trim[k] = b.trim[k];
  hipLaunchKernelGGL(k_pair_overlap, dim3(grid_for(b.n)), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

// the two device forms: asynchronous on the caller's stream (b: the caller's arrays, on the device)
static int overlap_batch_device(const char* name, walt_index* idx, const OverlapBatch& b, void* stream) {
  const std::string who(name);
  const void *d_pairs = b.pairs, *d_offsets1 = b.offsets1, *d_offsets2 = b.offsets2, *d_call_len1 = b.call_len1, *d_call_len2 = b.call_len2;
  const void *d_excl = b.excl, *d_totals = b.totals;
  const uint32_t n = b.n;
  if (!idx) return fail(WALT_EINVAL, who + ": bad argument (null index)");
  if (n && (!d_pairs || !d_offsets1 || !d_offsets2 || !d_excl)) return fail(WALT_EINVAL, who + ": bad argument");
  if (((uintptr_t)d_pairs & 3u) || ((uintptr_t)d_call_len1 & 3u) || ((uintptr_t)d_call_len2 & 3u) || ((uintptr_t)d_excl & 3u) ||
      ((uintptr_t)d_offsets1 & 7u) || ((uintptr_t)d_offsets2 & 7u) || ((uintptr_t)d_totals & 7u))
    return fail(WALT_EINVAL, who + ": pairs, call_len and excl must be 4-byte aligned, offsets and totals 8-byte aligned");
  return overlap_launch(idx, b, reinterpret_cast<hipStream_t>(stream));
}

// the two host forms: the batch into device temporaries of this call, the kernel on the null stream, the results back
static int overlap_batch_host(const char* name, walt_index* idx, const OverlapBatch& b) {
  const std::string who(name);
  const walt_pair_result* pairs = static_cast<const walt_pair_result*>(b.pairs);
  const uint64_t *offsets1 = static_cast<const uint64_t*>(b.offsets1), *offsets2 = static_cast<const uint64_t*>(b.offsets2);
  const uint32_t *call_len1 = static_cast<const uint32_t*>(b.call_len1), *call_len2 = static_cast<const uint32_t*>(b.call_len2);
  uint32_t* excl = static_cast<uint32_t*>(b.excl);
  uint64_t* totals = static_cast<uint64_t*>(b.totals);
  const uint32_t n = b.n;
  if (!idx) return fail(WALT_EINVAL, who + ": bad argument (null index)");
  if (n == 0) return WALT_OK;
  if (!pairs || !offsets1 || !offsets2 || !excl) return fail(WALT_EINVAL, who + ": bad argument");
  for (uint32_t i = 0; i < n; ++i)
    if (offsets1[i + 1] < offsets1[i] || offsets2[i + 1] < offsets2[i]) return fail(WALT_EINVAL, who + ": offsets not non-decreasing");
  WALT_HIP(hipSetDevice(idx->device));
  const char* what = "overlap of a pair";
  DeviceTemp d_pairs, d_off1, d_off2, d_len1, d_len2, d_excl, d_totals;
  int rc;
  const size_t off_bytes = ((size_t)n + 1) * 8;
  // (only the differences of the offsets are used: relative to offsets[0] or not is the same)
  if ((rc = d_pairs.put(pairs, (size_t)n * 64, what)) || (rc = d_off1.put(offsets1, off_bytes, what)) ||
      (rc = d_off2.put(offsets2, off_bytes, what)) || (rc = d_excl.get((size_t)n * 4, what)))
    return rc;
  if (call_len1 && (rc = d_len1.put(call_len1, (size_t)n * 4, what))) return rc;
  if (call_len2 && (rc = d_len2.put(call_len2, (size_t)n * 4, what))) return rc;
  if (totals && (rc = d_totals.get(kOverlapTotals * 8, what))) return rc;
  if (totals) WALT_HIP(hipMemset(d_totals.p, 0, kOverlapTotals * 8));
  OverlapBatch d = b;  // the same batch on the device copies
  d.pairs = d_pairs.p; d.offsets1 = d_off1.p; d.offsets2 = d_off2.p; d.call_len1 = d_len1.p; d.call_len2 = d_len2.p;
  d.excl = d_excl.p; d.totals = d_totals.p;
  if ((rc = overlap_launch(idx, d, nullptr))) return rc;
  WALT_HIP(hipStreamSynchronize(nullptr));
  WALT_HIP(hipMemcpy(excl, d_excl.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (totals) {
    uint64_t t[kOverlapTotals];
    WALT_HIP(hipMemcpy(t, d_totals.p, sizeof t, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < kOverlapTotals; ++k) totals[k] += t[k];
  }
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_pair_overlap_batch_device(walt_index* idx, const void* d_pairs, const void* d_offsets1, const void* d_offsets2,
                                   uint32_t n, const void* d_call_len1, const void* d_call_len2, void* d_excl, void* d_totals,
                                   void* stream) {
  return overlap_batch_device("walt_pair_overlap_batch_device", idx, {d_pairs, d_offsets1, d_offsets2, n, d_call_len1, d_call_len2,
                                                                      d_excl, d_totals}, stream);
}

int walt_pair_overlap_batch(walt_index* idx, const walt_pair_result* pairs, const uint64_t* offsets1, const uint64_t* offsets2,
                            uint32_t n, const uint32_t* call_len1, const uint32_t* call_len2, uint32_t* excl, uint64_t* totals) {
  return overlap_batch_host("walt_pair_overlap_batch", idx, {pairs, offsets1, offsets2, n, call_len1, call_len2, excl, totals});
}

// the same with the ignored read ends of the two mates (include/walt_amd.h, "ignored read ends"); all 0: the calls above
int walt_pair_overlap_batch_trim_device(walt_index* idx, const void* d_pairs, const void* d_offsets1, const void* d_offsets2,
                                        uint32_t n, const void* d_call_len1, const void* d_call_len2, void* d_excl, void* d_totals,
                                        uint32_t trim5_1, uint32_t trim3_1, uint32_t trim5_2, uint32_t trim3_2, void* stream) {
  return overlap_batch_device("walt_pair_overlap_batch_trim_device", idx,
                              {d_pairs, d_offsets1, d_offsets2, n, d_call_len1, d_call_len2, d_excl, d_totals,
                               {trim5_1, trim3_1, trim5_2, trim3_2}}, stream);
}

int walt_pair_overlap_batch_trim(walt_index* idx, const walt_pair_result* pairs, const uint64_t* offsets1, const uint64_t* offsets2,
                                 uint32_t n, const uint32_t* call_len1, const uint32_t* call_len2, uint32_t* excl, uint64_t* totals,
                                 uint32_t trim5_1, uint32_t trim3_1, uint32_t trim5_2, uint32_t trim3_2) {
  return overlap_batch_host("walt_pair_overlap_batch_trim", idx,
                            {pairs, offsets1, offsets2, n, call_len1, call_len2, excl, totals, {trim5_1, trim3_1, trim5_2, trim3_2}});
}

}  // extern "C"
