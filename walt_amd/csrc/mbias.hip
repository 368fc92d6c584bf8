// mbias.hip -- methylation bias by read position on the device (include/walt_amd.h, "methylation bias by read
// position"): one streaming kernel over the calls of a batch that sums, per read position, context and state, how many
// calls there are -- in a block-private table in LDS first, then once per block into replica tables in HBM.  The
// per-lane logic is mbias_core.h's.  The reference has no such mode; the contract is the header's.
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "device_common.h"
#include "mbias_core.h"

namespace walt {

constexpr uint32_t kMbiasGroup = 8;        // lanes that share a read, as in the calling kernel: 128 contiguous bytes per group
constexpr uint32_t kMbiasReplicas = 8;     // replica tables per table in HBM (walt_mbias_read folds them)
constexpr uint32_t kMbiasBlocksPerCu = 4;  // 32 KB of LDS per block: five fit a compute unit, four are launched
constexpr uint32_t kMbiasMaxTables = 8;
static_assert(kMbiasPositions == WALT_MBIAS_POSITIONS && kMbiasWords == WALT_MBIAS_WORDS, "the header's table is mbias_core.h's");

struct MbiasArgs {
  CallsView v;
  unsigned long long* tabs;    // the kMbiasReplicas replicas of the table that is fed
};

// Eight lanes per read, one 16-byte slice of its calls per lane and trip, cut at the 16-byte boundaries of the calls
// array (mbias_core.h): a group reads 128 contiguous bytes, a wavefront eight reads.  A partial first or last slice of a
// read is the same aligned load with the neighbour's bytes masked; only the two slices at the batch's ends go byte by byte.
//
// How lanes meet: LDS atomics whose result nobody reads (ds_add_u32), one per call letter.  With this layout the 64
// lanes of one instruction hold eight DIFFERENT slices of eight reads, so at most eight lanes -- one per read of the
// wavefront -- can name the same word, however uniform the library is; a layout with one read per lane would have all
// 64 on one word at every step.  DESIGN.md section 19 has the reasoning and the alternatives.
//
// Overflow bound of the LDS table: a read adds at most 1 to a word (a position of a read has one letter), so a word is
// at most the number of reads its block takes, which is at most n < 2^32: a 32-bit word cannot wrap, for any grid.
// The flush widens to 64 bits.
__global__ __launch_bounds__(kBlock) void k_mbias(const MbiasArgs a) {
  __shared__ uint32_t s_tab[kMbiasWords];
  for (uint32_t w = threadIdx.x; w < kMbiasWords; w += kBlock) s_tab[w] = 0u;
  __syncthreads();
  const uint32_t sub = threadIdx.x & (kMbiasGroup - 1);
  const uint64_t groups = (uint64_t)gridDim.x * (kBlock / kMbiasGroup);
  const uint64_t batch_lo = a.v.offsets[0], batch_hi = a.v.offsets[a.v.n];  // the calls the batch owns: a slice stays inside them
  for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / kMbiasGroup) + threadIdx.x / kMbiasGroup; r < a.v.n; r += groups) {
    const uint64_t off = a.v.offsets[r], end = a.v.offsets[r + 1];
    const uint32_t times = reinterpret_cast<const uint32_t*>(a.v.records + r * a.v.rec_stride)[1];
    const uint32_t skip = a.v.skip ? a.v.skip[r * a.v.skip_stride] : 0u;
    if (!mbias_counted(times, skip, off, end) || off < batch_lo || end > batch_hi) continue;  // (before any index or address)
    const uint8_t* rb = a.v.calls + off;
    const int len = (int)(end - off);
    const int head = (int)((uintptr_t)rb & 15u);
    for (int i0 = -head + 16 * (int)sub; i0 < len; i0 += 16 * (int)kMbiasGroup) {
      uint32_t w[4];
      mbias_load_slice(rb, len, i0, off - batch_lo, batch_hi - off, w);
      mbias_slice(w, i0, [&](uint32_t cell, uint32_t pos) {
        (void)__hip_atomic_fetch_add(&s_tab[cell * kMbiasPositions + pos], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      });
    }
  }
  __syncthreads();
  // once per block, non-zero words only (reads of 100 bases leave nine tenths of the table at zero)
  unsigned long long* rep = a.tabs + (uint64_t)(blockIdx.x % kMbiasReplicas) * kMbiasWords;
  for (uint32_t w = threadIdx.x; w < kMbiasWords; w += kBlock) {
    const uint32_t v = s_tab[w];
    if (v) (void)__hip_atomic_fetch_add(rep + w, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

static uint64_t mbias_bytes(uint32_t n_tables) { return (uint64_t)n_tables * kMbiasReplicas * kMbiasWords * 8; }

// what both forms refuse before they look at the batch
static int mbias_set_check(const walt_mbias* mb, const std::string& who, uint32_t table, const CallsBatch& b) {
  if (!mb) return fail(WALT_EINVAL, who + ": bad argument (null bias set)");
  if (table >= mb->n_tables)
    return fail(WALT_EINVAL, who + ": table " + std::to_string(table) + " of a bias set with " + std::to_string(mb->n_tables));
  std::string bad = record_stride_refusal(b.rec_stride);
  if (bad.empty()) bad = skip_stride_refusal(b.skip, b.skip_stride);
  return bad.empty() ? WALT_OK : fail(WALT_EINVAL, who + ": " + bad);
}

int mbias_launch(walt_mbias* mb, uint32_t table, const CallsBatch& b, hipStream_t stream) {
  if (b.n == 0) return WALT_OK;
  WALT_HIP(hipSetDevice(mb->device));
  const MbiasArgs a = {calls_view(b), mb->tabs + (uint64_t)table * kMbiasReplicas * kMbiasWords};
  const uint64_t want = ((uint64_t)b.n + kBlock / kMbiasGroup - 1) / (kBlock / kMbiasGroup);
  const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)mb->n_cu * kMbiasBlocksPerCu);
  hipLaunchKernelGGL(k_mbias, dim3(grid), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_mbias_create(int device, uint32_t n_tables, walt_mbias** out) {
  if (!out) return fail(WALT_EINVAL, "walt_mbias_create: bad argument");
  *out = nullptr;
  if (n_tables < 1 || n_tables > kMbiasMaxTables)
    return fail(WALT_EINVAL, "walt_mbias_create: " + std::to_string(n_tables) + " tables (a set holds 1 to 8)");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(WALT_EHIP, "walt_mbias_create: no HIP device (no CPU fallback exists)");
  }
  if (device < 0 || device >= n_dev)
    return fail(WALT_EINVAL, "walt_mbias_create: device " + std::to_string(device) + " of " + std::to_string(n_dev));
  WALT_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  WALT_HIP(hipGetDeviceProperties(&prop, device));
  void* tabs = nullptr;
  const uint64_t bytes = mbias_bytes(n_tables);
  if (hipMalloc(&tabs, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(WALT_ENOMEM, "walt_mbias_create: hipMalloc of " + std::to_string(bytes) + " bytes failed");
  }
  if (hipMemset(tabs, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(tabs);
    return fail(WALT_EHIP, "walt_mbias_create: the tables could not be cleared");
  }
  walt_mbias* mb = new walt_mbias;
  mb->device = device;
  mb->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
  mb->n_tables = n_tables;
  mb->tabs = static_cast<unsigned long long*>(tabs);
  *out = mb;
  return WALT_OK;
}

void walt_mbias_destroy(walt_mbias* mb) {
  if (!mb) return;
  (void)hipSetDevice(mb->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(mb->tabs);
  delete mb;
}

int walt_mbias_clear(walt_mbias* mb) {
  if (!mb) return fail(WALT_EINVAL, "walt_mbias_clear: bad argument (null bias set)");
  WALT_HIP(hipSetDevice(mb->device));
  WALT_HIP(hipDeviceSynchronize());  // calls of any stream come first
  WALT_HIP(hipMemset(mb->tabs, 0, mbias_bytes(mb->n_tables)));
  WALT_HIP(hipDeviceSynchronize());
  return WALT_OK;
}

uint64_t walt_mbias_device_bytes(const walt_mbias* mb) { return mb ? mbias_bytes(mb->n_tables) : 0; }

int walt_mbias_read(walt_mbias* mb, uint32_t table, uint64_t* out) {
  if (!mb || !out) return fail(WALT_EINVAL, "walt_mbias_read: bad argument");
  if (table >= mb->n_tables)
    return fail(WALT_EINVAL, "walt_mbias_read: table " + std::to_string(table) + " of a bias set with " + std::to_string(mb->n_tables));
  WALT_HIP(hipSetDevice(mb->device));
  WALT_HIP(hipDeviceSynchronize());
  std::vector<unsigned long long> rep((size_t)kMbiasReplicas * kMbiasWords);
  WALT_HIP(hipMemcpy(rep.data(), mb->tabs + (uint64_t)table * kMbiasReplicas * kMbiasWords, rep.size() * 8, hipMemcpyDeviceToHost));
  for (uint32_t w = 0; w < kMbiasWords; ++w) {
    uint64_t sum = 0;
    for (uint32_t k = 0; k < kMbiasReplicas; ++k) sum += rep[(size_t)k * kMbiasWords + w];
    out[w] = sum;
  }
  return WALT_OK;
}

int walt_mbias_batch_device(walt_mbias* mb, uint32_t table, const void* d_calls, const void* d_offsets, uint32_t n,
                            const void* d_records, size_t record_stride, const void* d_skip, size_t skip_stride, void* stream) {
  const std::string who = "walt_mbias_batch_device";
  const CallsBatch b = {d_calls, d_offsets, n, d_records, record_stride, d_skip, skip_stride};
  if (const int rc = mbias_set_check(mb, who, table, b)) return rc;
  if (const int rc = calls_device_check(who, b)) return rc;
  return mbias_launch(mb, table, b, reinterpret_cast<hipStream_t>(stream));
}

int walt_mbias_batch(walt_mbias* mb, uint32_t table, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                     size_t record_stride, const uint8_t* skip, size_t skip_stride) {
  const std::string who = "walt_mbias_batch";
  const CallsBatch host = {calls, offsets, n, records, record_stride, skip, skip_stride};
  if (const int rc = mbias_set_check(mb, who, table, host)) return rc;
  static_assert(kMbiasPositions == 1024, "scan_offsets refuses what the table has no position for");
  return calls_host_batch(who, "methylation bias", host, false, nullptr, mb->device,
                          [&](const CallsBatch& b) { return mbias_launch(mb, table, b, nullptr); });
}

}  // extern "C"
