// nonconv.hip -- non-converted reads on the device (include/walt_amd.h, "non-converted reads"): one streaming kernel
// over the calls of a batch that tallies each read's non-CpG calls -- methylated, all, and the longest run of methylated
// ones -- and judges the read by the caller's rule, and the pair rule over the verdicts of a batch of pairs.  The
// per-lane logic is nonconv_core.h's.  The reference has no such mode; the contract is the header's.
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "device_common.h"
#include "nonconv_core.h"

namespace walt {

constexpr uint32_t kNonconvBlocksPerCu = 8;  // no LDS, few registers: the grid is bounded by the device, the loop strides

struct NonconvArgs {
  CallsView v;                // (no skip bytes: a verdict is written for every read)
  walt_nonconv_rule rule;
  uint8_t* filt;
  uint64_t filt_stride;
  unsigned long long* tally;  // null: not wanted (one 8-byte walt_nonconv_tally per read)
};

// A followed by what lane sub + d of the group holds (a lane with no such neighbour gets its own back: its result is
// never read).  All eight lanes of the group are active here.
__device__ __forceinline__ NonconvSum nonconv_step(const NonconvSum& s, int d) {
  uint32_t w0, w1;
  nonconv_pack(s, w0, w1);
  w0 = (uint32_t)__shfl_down((int)w0, (unsigned)d, (int)kNonconvGroup);
  w1 = (uint32_t)__shfl_down((int)w1, (unsigned)d, (int)kNonconvGroup);
  return nonconv_combine(s, nonconv_unpack(w0, w1));
}

// k_mbias's access shape (mbias.hip): eight lanes per read, one aligned 16-byte slice of its calls per lane and trip,
// the neighbours' bytes of a partial first or last slice masked, only the two slices at the batch's ends byte by byte.
// Here order matters: each lane turns its slice into a summary, the eight summaries of a trip are folded in lane order
// by three cross-lane steps (after step d lane k, k a multiple of 2 d, holds slices k .. k + 2 d - 1), and lane 0 folds
// the trip onto the read's running summary.  The trip count comes from the read's length and head alone, so the eight
// lanes of a group take every trip together (a lane beyond the read's end contributes the identity); the groups of a
// wavefront may diverge from each other -- a shuffle of width 8 stays inside its group.
__global__ __launch_bounds__(kBlock) void k_nonconv(const NonconvArgs a) {
  const uint32_t sub = threadIdx.x & (kNonconvGroup - 1);
  const uint64_t groups = (uint64_t)gridDim.x * (kBlock / kNonconvGroup);
  const uint64_t batch_lo = a.v.offsets[0], batch_hi = a.v.offsets[a.v.n];  // the calls the batch owns: a slice stays inside them
  for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / kNonconvGroup) + threadIdx.x / kNonconvGroup; r < a.v.n; r += groups) {
    const uint64_t off = a.v.offsets[r], end = a.v.offsets[r + 1];
    const uint32_t times = reinterpret_cast<const uint32_t*>(a.v.records + r * a.v.rec_stride)[1];
    NonconvSum run = nonconv_identity();
    uint32_t fails = 0u;
    if (nonconv_judged(times, off, end) && off >= batch_lo && end <= batch_hi) {  // (before any address; the same for the group)
      const uint8_t* rb = a.v.calls + off;
      const int len = (int)(end - off);
      const int head = (int)((uintptr_t)rb & 15u);
      const int trips = nonconv_trips(len, head);
      for (int t = 0; t < trips; ++t) {
        const int i0 = -head + 16 * ((int)kNonconvGroup * t + (int)sub);
        NonconvSum s = nonconv_identity();
        if (i0 < len) {
          uint32_t w[4];
          mbias_load_slice(rb, len, i0, off - batch_lo, batch_hi - off, w);
          s = nonconv_slice(w);
        }
#pragma unroll
        for (int d = 1; d < (int)kNonconvGroup; d <<= 1) s = nonconv_step(s, d);
        run = nonconv_combine(run, s);  // (lane 0's is the read's)
      }
      fails = nonconv_fails(run.meth, run.total, run.best, a.rule);
    }
    if (sub == 0) {  // (not judged: the identity's zeros and a verdict of 0)
      if (a.tally) a.tally[r] = (unsigned long long)run.meth | (unsigned long long)run.total << 16 | (unsigned long long)run.best << 32;
      a.filt[r * a.filt_stride] = (uint8_t)fails;
    }
  }
}

// one pair per lane: best_times is the word behind the two 16-byte mates of a walt_pair_result
__global__ __launch_bounds__(kBlock) void k_nonconv_pairs(const uint8_t* __restrict__ pairs, uint32_t n, uint8_t* __restrict__ filt) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t best_times = reinterpret_cast<const uint32_t*>(pairs + i * sizeof(walt_pair_result))[8];
    uint8_t f1 = filt[2 * i], f2 = filt[2 * i + 1];
    nonconv_pair(best_times, f1, f2);
    filt[2 * i] = f1;
    filt[2 * i + 1] = f2;
  }
}

int nonconv_launch(const walt_index* idx, const NonconvBatch& b, hipStream_t stream) {
  if (b.n == 0) return WALT_OK;
  WALT_HIP(hipSetDevice(idx->device));
  const NonconvArgs a = {calls_view({b.calls, b.offsets, b.n, b.records, b.rec_stride, nullptr, 0}), b.rule, static_cast<uint8_t*>(b.filt),
                         b.filt_stride, static_cast<unsigned long long*>(b.tally)};
  const uint64_t want = ((uint64_t)b.n + kBlock / kNonconvGroup - 1) / (kBlock / kNonconvGroup);
  const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)idx->n_cu * kNonconvBlocksPerCu);
  hipLaunchKernelGGL(k_nonconv, dim3(grid), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

std::string nonconv_refusal(const walt_nonconv_rule* rule, const void* filt, size_t filt_stride) {
  if (!rule) return "bad argument (null rule)";
  if (!nonconv_rule_ok(*rule)) return "min_percent " + std::to_string(rule->min_percent) + " is above 100";
  if (filt && filt_stride < 1) return "filt stride 0 is smaller than its element (1)";
  return std::string();
}

static int nonconv_pairs_launch(const walt_index* idx, const void* d_pairs, uint32_t n, void* d_filt, hipStream_t stream) {
  if (n == 0) return WALT_OK;
  WALT_HIP(hipSetDevice(idx->device));
  const unsigned grid = (unsigned)std::min<uint64_t>(grid_for(n), (uint64_t)idx->n_cu * kNonconvBlocksPerCu);
  hipLaunchKernelGGL(k_nonconv_pairs, dim3(grid), dim3(kBlock), 0, stream, static_cast<const uint8_t*>(d_pairs), n,
                     static_cast<uint8_t*>(d_filt));
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

// what both forms of walt_nonconv_batch refuse before they look at the batch
static int nonconv_check(const walt_index* idx, const std::string& who, size_t rec_stride, const walt_nonconv_rule* rule,
                         const void* filt, size_t filt_stride) {
  if (!idx) return fail(WALT_EINVAL, who + ": bad argument (null index)");
  std::string bad = record_stride_refusal(rec_stride);
  if (bad.empty()) bad = nonconv_refusal(rule, filt, filt_stride);
  return bad.empty() ? WALT_OK : fail(WALT_EINVAL, who + ": " + bad);
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_nonconv_batch_device(walt_index* idx, const void* d_calls, const void* d_offsets, uint32_t n, const void* d_records,
                              size_t record_stride, const walt_nonconv_rule* rule, void* d_filt, size_t filt_stride,
                              void* d_tally, void* stream) {
  const std::string who = "walt_nonconv_batch_device";
  if (const int rc = nonconv_check(idx, who, record_stride, rule, d_filt, filt_stride)) return rc;
  const void* const out[2] = {d_filt, d_tally};
  if (const int rc = calls_device_check(who, {d_calls, d_offsets, n, d_records, record_stride, nullptr, 0}, out)) return rc;
  return nonconv_launch(idx, {d_calls, d_offsets, n, d_records, record_stride, *rule, d_filt, filt_stride, d_tally},
                        reinterpret_cast<hipStream_t>(stream));
}

int walt_nonconv_batch(walt_index* idx, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                       size_t record_stride, const walt_nonconv_rule* rule, uint8_t* filt, size_t filt_stride,
                       walt_nonconv_tally* tally) {
  const std::string who = "walt_nonconv_batch";
  int rc = nonconv_check(idx, who, record_stride, rule, filt, filt_stride);
  if (rc || n == 0) return rc;
  // (any_length: a read of more than 1024 calls is legal here: it is not judged)
  const char* what = "non-converted reads";
  DeviceTemp d_filt, d_tally;
  rc = calls_host_batch(who, what, {calls, offsets, n, records, record_stride, nullptr, 0}, true, filt, idx->device, [&](const CallsBatch& b) {
    int e;
    if ((e = d_filt.get(n, what)) || (tally && (e = d_tally.get((size_t)n * sizeof(walt_nonconv_tally), what)))) return e;
    return nonconv_launch(idx, {b.calls, b.offsets, n, b.records, b.rec_stride, *rule, d_filt.p, 1, d_tally.p}, nullptr);
  });
  return rc ? rc : nonconv_results(d_filt.p, d_tally.p, n, filt, filt_stride, tally);
}

int walt_nonconv_pairs_batch_device(walt_index* idx, const void* d_pairs, uint32_t n, void* d_filt, void* stream) {
  const std::string who = "walt_nonconv_pairs_batch_device";
  if (!idx) return fail(WALT_EINVAL, who + ": bad argument (null index)");
  if (n && (!d_pairs || !d_filt)) return fail(WALT_EINVAL, who + ": bad argument (null pairs or filt)");
  if ((uintptr_t)d_pairs & 3u) return fail(WALT_EINVAL, who + ": pairs must be 4-byte aligned");
  return nonconv_pairs_launch(idx, d_pairs, n, d_filt, reinterpret_cast<hipStream_t>(stream));
}

int walt_nonconv_pairs_batch(walt_index* idx, const walt_pair_result* pairs, uint32_t n, uint8_t* filt) {
  const std::string who = "walt_nonconv_pairs_batch";
  if (!idx) return fail(WALT_EINVAL, who + ": bad argument (null index)");
  if (n == 0) return WALT_OK;
  if (!pairs || !filt) return fail(WALT_EINVAL, who + ": bad argument (null pairs or filt)");
  WALT_HIP(hipSetDevice(idx->device));
  const char* what = "non-converted reads";
  DeviceTemp d_pairs, d_filt;
  int rc;
  if ((rc = d_pairs.put(pairs, (size_t)n * sizeof(walt_pair_result), what)) || (rc = d_filt.put(filt, 2 * (size_t)n, what))) return rc;
  if ((rc = nonconv_pairs_launch(idx, d_pairs.p, n, d_filt.p, nullptr))) return rc;
  WALT_HIP(hipStreamSynchronize(nullptr));
  WALT_HIP(hipMemcpy(filt, d_filt.p, 2 * (size_t)n, hipMemcpyDeviceToHost));
  return WALT_OK;
}

}  // extern "C"

namespace walt {

// the end of a host form: the packed verdicts into the caller's strided bytes, the tallies as they are
int nonconv_results(const void* d_filt, const void* d_tally, uint32_t n, uint8_t* filt, size_t filt_stride, walt_nonconv_tally* tally) {
  std::vector<uint8_t> packed(n);
  WALT_HIP(hipMemcpy(packed.data(), d_filt, n, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) filt[(size_t)i * filt_stride] = packed[i];
  if (tally) WALT_HIP(hipMemcpy(tally, d_tally, (size_t)n * sizeof(walt_nonconv_tally), hipMemcpyDeviceToHost));
  return WALT_OK;
}

}  // namespace walt
