// dedup.hip -- PCR-duplicate marking on the device (include/walt_amd.h, "duplicates"): an open-addressing set of 64-bit
// record keys, each remembering the ordinal of the first record that produced it; an insert kernel, a mark kernel that
// follows it in stream order, and a rehash into a larger table.  Keys, hash and probe sequences are dedup_core.h's.
// The reference has no such mode; the contract is the header's.
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "device_common.h"
#include "dedup_core.h"

// A duplicate set: two planes of `slots` 64-bit words (keys; ordinal of the first record of each key), both all ones
// when empty, and two control words on the device: [0] occupied slots, [1] error (a probe ran through the whole table).
struct walt_dedup {
  int device = 0;
  uint64_t slots = 0;
  uint64_t* key = nullptr;
  uint64_t* first = nullptr;
  unsigned long long* ctl = nullptr;
  uint64_t fed = 0;         // records numbered so far (host side: a call's ordinals are known when it is enqueued)
  uint64_t known_keys = 0;  // occupied slots when the counter was last read
  uint64_t maybe_keys = 0;  // keys the calls enqueued since then can have added at most
};

namespace walt {

constexpr uint64_t kDedupDefaultSlots = 1ull << 25;  // 10 M records (the default batch) at a load below 1/2; 512 MiB
constexpr uint32_t kPairStride = (uint32_t)sizeof(walt_pair_result);
static_assert(sizeof(walt_pair_result) == 64 && offsetof(walt_pair_result, m2) == 16 &&
              offsetof(walt_pair_result, best_times) == 32 && offsetof(walt_pair_result, frag_len) == 36,
              "k_dedup_* read a walt_pair_result by word");

struct DevOps {
  static __device__ __forceinline__ uint64_t load(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
    return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expect, (unsigned long long)v);
  }
  static __device__ __forceinline__ void min(uint64_t* p, uint64_t v) {  // nobody reads the result
    (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

struct DedupArgs {
  uint64_t* key;
  uint64_t* first;
  uint64_t mask;               // slots - 1
  unsigned long long* ctl;
  const uint8_t* records;      // walt_best_match at records + i * rec_stride, or walt_pair_result (stride 64)
  uint64_t rec_stride;
  const uint8_t* conv;         // null: `conversion` (pairs: for mate 1, its complement for mate 2)
  uint64_t conv_stride;
  uint32_t conversion;
  uint32_t kind;               // single records
  uint32_t n;
  uint64_t ordinal0;           // record i is number ordinal0 + i
  uint8_t* dup;
};

__device__ __forceinline__ bool single_key_of(const DedupArgs& a, uint32_t i, uint64_t& key) {
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.records + (uint64_t)i * a.rec_stride);
  const uint32_t cv = a.conv ? a.conv[(uint64_t)i * a.conv_stride] : a.conversion;
  return dedup_single_key(rec[0], rec[1], rec[2] & 0xFFu, cv, a.kind, key);
}
__device__ __forceinline__ DedupPairKeys pair_keys_of(const DedupArgs& a, uint32_t i) {
  const uint4* rec = reinterpret_cast<const uint4*>(a.records + (uint64_t)i * kPairStride);  // (16-byte aligned: checked on the host)
  const uint4 m1 = rec[0], m2 = rec[1], tail = rec[2];
  const uint32_t c1 = a.conv ? a.conv[2ull * i] : a.conversion;
  const uint32_t c2 = a.conv ? a.conv[2ull * i + 1] : dedup_conv_complement(a.conversion);
  return dedup_pair_keys(m1.x, m1.y, m1.z & 0xFFu, m2.x, m2.y, m2.z & 0xFFu, tail.x, (int32_t)tail.y, c1, c2);
}
// the wavefront's newly occupied slots in one add; every lane of the wavefront arrives
__device__ __forceinline__ void count_fresh(uint32_t fresh, bool failed, unsigned long long* ctl) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) fresh += __shfl_xor(fresh, off);
  if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(&ctl[0], (unsigned long long)fresh);
  if (failed) ctl[1] = 1ull;
}

// one record (kPairs: one pair) per lane
template <bool kPairs>
__global__ __launch_bounds__(kBlock) void k_dedup_insert(const DedupArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t fresh = 0;
  bool failed = false;
  if (i < a.n) {
    const uint64_t ordinal = a.ordinal0 + i;
    if (kPairs) {
      const DedupPairKeys k = pair_keys_of(a, (uint32_t)i);
      if (k.has[0]) failed |= !dedup_insert<DevOps>(a.key, a.first, a.mask, k.key[0], ordinal, fresh);
      if (k.has[1] && k.key[1] != k.key[0]) failed |= !dedup_insert<DevOps>(a.key, a.first, a.mask, k.key[1], ordinal, fresh);
    } else {
      uint64_t key;
      if (single_key_of(a, (uint32_t)i, key)) failed = !dedup_insert<DevOps>(a.key, a.first, a.mask, key, ordinal, fresh);
    }
  }
  count_fresh(fresh, failed, a.ctl);
}

template <bool kPairs>
__global__ __launch_bounds__(kBlock) void k_dedup_mark(const DedupArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t ordinal = a.ordinal0 + i;
  if (kPairs) {
    const DedupPairKeys k = pair_keys_of(a, (uint32_t)i);
    uint8_t d[2];
    d[0] = k.has[0] && dedup_is_dup<DevOps>(a.key, a.first, a.mask, k.key[0], ordinal) ? 1 : 0;
    d[1] = !k.has[1] ? 0 : k.key[1] == k.key[0] && k.has[0] ? d[0]  // a unique pair: one key, one verdict
                         : dedup_is_dup<DevOps>(a.key, a.first, a.mask, k.key[1], ordinal) ? 1 : 0;
    a.dup[2 * i] = d[0];
    a.dup[2 * i + 1] = d[1];
  } else {
    uint64_t key;
    a.dup[i] = single_key_of(a, (uint32_t)i, key) && dedup_is_dup<DevOps>(a.key, a.first, a.mask, key, ordinal) ? 1 : 0;
  }
}

// one old slot per lane into the new planes (all ones before)
__global__ __launch_bounds__(kBlock) void k_dedup_rehash(const uint64_t* __restrict__ old_key, const uint64_t* __restrict__ old_first,
                                                         uint64_t old_slots, uint64_t* key, uint64_t* first, uint64_t mask,
                                                         unsigned long long* ctl) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= old_slots) return;
  const uint64_t k = old_key[s];
  if (k == kDedupEmpty) return;
  if (!dedup_move<DevOps>(key, first, mask, k, old_first[s])) ctl[1] = 1ull;
}

static int dd_check(const walt_dedup* dd, const char* who) {
  if (!dd) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null duplicate set)");
  return WALT_OK;
}
static uint64_t dd_bytes(uint64_t slots) { return 16ull * slots + 16; }

// both planes of `slots` words, all ones; WALT_ENOMEM names the bytes and nothing is kept
static int dd_alloc_planes(const char* who, uint64_t slots, uint64_t** key, uint64_t** first) {
  void* got[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; ++i) {
    const hipError_t e = hipMalloc(&got[i], 8ull * slots);
    if (e != hipSuccess || hipMemset(got[i], 0xFF, 8ull * slots) != hipSuccess) {
      (void)hipGetLastError();
      for (void* q : got) if (q) (void)hipFree(q);
      return fail(WALT_ENOMEM, std::string(who) + ": a table of " + std::to_string(slots) + " slots wants " +
                                   std::to_string(16ull * slots) + " bytes of device memory: " + hipGetErrorString(e));
    }
  }
  *key = static_cast<uint64_t*>(got[0]);
  *first = static_cast<uint64_t*>(got[1]);
  return WALT_OK;
}

// waits for the device, reads the control words: the occupied count becomes the host's known count
static int dd_sync_count(walt_dedup* dd, const char* who) {
  WALT_HIP(hipSetDevice(dd->device));
  WALT_HIP(hipDeviceSynchronize());  // inserts of any stream come first
  unsigned long long ctl[2];
  WALT_HIP(hipMemcpy(ctl, dd->ctl, sizeof ctl, hipMemcpyDeviceToHost));
  if (ctl[1])
    return fail(WALT_EHIP, std::string(who) + ": a probe ran through all " + std::to_string(dd->slots) +
                               " slots of the table (internal: the load limit was not kept)");
  dd->known_keys = ctl[0];
  dd->maybe_keys = 0;
  return WALT_OK;
}

static int dd_reserve(walt_dedup* dd, const char* who, uint64_t n_more) {
  int rc = dd_sync_count(dd, who);
  if (rc) return rc;
  const uint64_t want = dedup_slots_for(dd->slots, dd->known_keys + n_more);
  if (want == dd->slots) return WALT_OK;
  uint64_t *key = nullptr, *first = nullptr;
  if ((rc = dd_alloc_planes(who, want, &key, &first))) return rc;  // the set stays as it was
  hipLaunchKernelGGL(k_dedup_rehash, dim3(grid_for(dd->slots)), dim3(kBlock), 0, nullptr, dd->key, dd->first, dd->slots, key,
                     first, want - 1, dd->ctl);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned long long err = 0;
  if (e == hipSuccess) e = hipMemcpy(&err, dd->ctl + 1, sizeof err, hipMemcpyDeviceToHost);
  if (e != hipSuccess || err) {
    (void)hipFree(key);
    (void)hipFree(first);
    return fail(WALT_EHIP, std::string(who) + ": moving the table failed" + (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : ""));
  }
  (void)hipFree(dd->key);
  (void)hipFree(dd->first);
  dd->key = key;
  dd->first = first;
  dd->slots = want;
  return WALT_OK;
}

static int dd_args_check(const char* who, size_t rec_stride, const void* conv, size_t conv_stride, int conversion) {
  std::string bad = record_stride_refusal(rec_stride);
  if (bad.empty()) bad = conv_refusal(conv, conv_stride, conversion);
  return bad.empty() ? WALT_OK : fail(WALT_EINVAL, std::string(who) + ": " + bad);
}

// one batch as the kernels read it (device arrays); pairs: walt_pair_result records, two conversions and two verdicts each
struct DedupBatch {
  bool pairs;
  const void* records;
  size_t rec_stride;
  const void* conv;
  size_t conv_stride;
  int conversion, kind;
  uint32_t n;
  void* dup;
};

// insert, then mark, on `stream`; the host's bound on the keys moves by what the call can add
static int dd_launch(walt_dedup* dd, const char* who, const DedupBatch& b, hipStream_t stream) {
  const uint32_t n = b.n;
  if (n == 0) return WALT_OK;
  const uint64_t can_add = b.pairs ? 2ull * n : (uint64_t)n;
  if (dd->known_keys + dd->maybe_keys + can_add > dd->slots / 2)
    return fail(WALT_EINVAL, std::string(who) + ": the set may hold " + std::to_string(dd->known_keys + dd->maybe_keys) + " keys and this call may add " +
                                 std::to_string(can_add) + ", more than half of its " + std::to_string(dd->slots) +
                                 " slots: call walt_dedup_reserve first (a device form cannot grow the table)");
  WALT_HIP(hipSetDevice(dd->device));
  DedupArgs a;
  a.key = dd->key; a.first = dd->first; a.mask = dd->slots - 1; a.ctl = dd->ctl;
  a.records = static_cast<const uint8_t*>(b.records);
  a.rec_stride = b.rec_stride;
  a.conv = static_cast<const uint8_t*>(b.conv);
  a.conv_stride = b.conv_stride;
  a.conversion = (uint32_t)b.conversion;
  a.kind = (uint32_t)b.kind;
  a.n = n;
  a.ordinal0 = dd->fed;
  a.dup = static_cast<uint8_t*>(b.dup);
  const dim3 grid(grid_for(n)), block(kBlock);
  if (b.pairs) {
    hipLaunchKernelGGL(k_dedup_insert<true>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(k_dedup_mark<true>, grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL(k_dedup_insert<false>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(k_dedup_mark<false>, grid, block, 0, stream, a);
  }
  WALT_HIP(hipGetLastError());
  dd->fed += n;
  dd->maybe_keys += can_add;
  return WALT_OK;
}

constexpr const char* kWhat = "duplicates";  // a host form's device temporaries, as its out-of-memory message names them

// the end of a host form: wait, the error word, the verdicts
static int dd_finish(walt_dedup* dd, const char* who, uint8_t* dup, const void* d_dup, size_t bytes) {
  const int rc = dd_sync_count(dd, who);
  if (rc) return rc;
  WALT_HIP(hipMemcpy(dup, d_dup, bytes, hipMemcpyDeviceToHost));
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_dedup_create(int device, uint64_t initial_slots, walt_dedup** out) {
  if (!out) return fail(WALT_EINVAL, "walt_dedup_create: bad argument");
  *out = nullptr;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(WALT_EHIP, "walt_dedup_create: no HIP device (no CPU fallback exists)");
  }
  if (device < 0 || device >= n_dev)
    return fail(WALT_EINVAL, "walt_dedup_create: device " + std::to_string(device) + " of " + std::to_string(n_dev));
  WALT_HIP(hipSetDevice(device));
  const uint64_t slots = dedup_round_slots(initial_slots ? initial_slots : kDedupDefaultSlots);
  uint64_t *key = nullptr, *first = nullptr;
  int rc = dd_alloc_planes("walt_dedup_create", slots, &key, &first);
  if (rc) return rc;
  void* ctl = nullptr;
  if (hipMalloc(&ctl, 16) != hipSuccess || hipMemset(ctl, 0, 16) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipGetLastError();
    if (ctl) (void)hipFree(ctl);
    (void)hipFree(key);
    (void)hipFree(first);
    return fail(WALT_EHIP, "walt_dedup_create: the control words could not be set up");
  }
  walt_dedup* dd = new walt_dedup;
  dd->device = device;
  dd->slots = slots;
  dd->key = key;
  dd->first = first;
  dd->ctl = static_cast<unsigned long long*>(ctl);
  *out = dd;
  return WALT_OK;
}

void walt_dedup_destroy(walt_dedup* dd) {
  if (!dd) return;
  (void)hipSetDevice(dd->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(dd->key);
  (void)hipFree(dd->first);
  (void)hipFree(dd->ctl);
  delete dd;
}

int walt_dedup_clear(walt_dedup* dd) {
  const int rc = dd_check(dd, "walt_dedup_clear");
  if (rc) return rc;
  WALT_HIP(hipSetDevice(dd->device));
  WALT_HIP(hipDeviceSynchronize());  // calls of any stream come first
  WALT_HIP(hipMemset(dd->key, 0xFF, 8ull * dd->slots));
  WALT_HIP(hipMemset(dd->first, 0xFF, 8ull * dd->slots));
  WALT_HIP(hipMemset(dd->ctl, 0, 16));
  WALT_HIP(hipDeviceSynchronize());
  dd->fed = dd->known_keys = dd->maybe_keys = 0;
  return WALT_OK;
}

int walt_dedup_reserve(walt_dedup* dd, uint64_t n_more) {
  const int rc = dd_check(dd, "walt_dedup_reserve");
  if (rc) return rc;
  return dd_reserve(dd, "walt_dedup_reserve", n_more);
}

int walt_dedup_count(walt_dedup* dd, uint64_t* keys, uint64_t* fed) {
  int rc = dd_check(dd, "walt_dedup_count");
  if (rc) return rc;
  if ((rc = dd_sync_count(dd, "walt_dedup_count"))) return rc;
  if (keys) *keys = dd->known_keys;
  if (fed) *fed = dd->fed;
  return WALT_OK;
}

uint64_t walt_dedup_device_bytes(const walt_dedup* dd) { return dd ? dd_bytes(dd->slots) : 0; }

int walt_dedup_batch_device(walt_dedup* dd, const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                            int conversion, int kind, uint32_t n, void* d_dup, void* stream) {
  const char* who = "walt_dedup_batch_device";
  int rc = dd_check(dd, who);
  if (rc || (rc = dd_args_check(who, record_stride, d_conv, conv_stride, conversion))) return rc;
  if (kind < 0 || kind > 2) return fail(WALT_EINVAL, std::string(who) + ": kind " + std::to_string(kind) + " is not 0, 1 or 2");
  if (n && (!d_records || !d_dup)) return fail(WALT_EINVAL, std::string(who) + ": bad argument");
  if ((uintptr_t)d_records & 3u) return fail(WALT_EINVAL, std::string(who) + ": records must be 4-byte aligned");
  return dd_launch(dd, who, {false, d_records, record_stride, d_conv, conv_stride, conversion, kind, n, d_dup},
                   reinterpret_cast<hipStream_t>(stream));
}

int walt_dedup_pairs_batch_device(walt_dedup* dd, const void* d_pairs, const void* d_conv, int conversion, uint32_t n, void* d_dup,
                                  void* stream) {
  const char* who = "walt_dedup_pairs_batch_device";
  int rc = dd_check(dd, who);
  if (rc || (rc = dd_args_check(who, kPairStride, d_conv, 2, conversion))) return rc;
  if (n && (!d_pairs || !d_dup)) return fail(WALT_EINVAL, std::string(who) + ": bad argument");
  if ((uintptr_t)d_pairs & 15u) return fail(WALT_EINVAL, std::string(who) + ": pairs must be 16-byte aligned");
  return dd_launch(dd, who, {true, d_pairs, kPairStride, d_conv, 2, conversion, 0, n, d_dup}, reinterpret_cast<hipStream_t>(stream));
}

int walt_dedup_batch(walt_dedup* dd, const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                     int conversion, int kind, uint32_t n, uint8_t* dup) {
  const char* who = "walt_dedup_batch";
  int rc = dd_check(dd, who);
  if (rc || (rc = dd_args_check(who, record_stride, conv, conv_stride, conversion))) return rc;
  if (kind < 0 || kind > 2) return fail(WALT_EINVAL, std::string(who) + ": kind " + std::to_string(kind) + " is not 0, 1 or 2");
  if (n == 0) return WALT_OK;
  if (!records || !dup) return fail(WALT_EINVAL, std::string(who) + ": bad argument");
  if ((rc = dd_reserve(dd, who, n))) return rc;
  // the records and conversions as the kernel reads them: packed (the caller's strides stay on the host)
  const std::vector<walt_best_match> rec = pack_strided<walt_best_match>(records, record_stride, n);
  const std::vector<uint8_t> cv = pack_strided<uint8_t>(conv, conv_stride, conv ? n : 0);
  DeviceTemp d_rec, d_conv, d_dup;
  if ((rc = d_rec.put(rec.data(), (size_t)n * 16, kWhat)) || (rc = d_dup.get(n, kWhat)) || (conv && (rc = d_conv.put(cv.data(), n, kWhat))))
    return rc;
  if ((rc = dd_launch(dd, who, {false, d_rec.p, 16, d_conv.p, 1, conversion, kind, n, d_dup.p}, nullptr))) return rc;
  return dd_finish(dd, who, dup, d_dup.p, n);
}

int walt_dedup_pairs_batch(walt_dedup* dd, const walt_pair_result* pairs, const uint8_t* conv, int conversion, uint32_t n,
                           uint8_t* dup) {
  const char* who = "walt_dedup_pairs_batch";
  int rc = dd_check(dd, who);
  if (rc || (rc = dd_args_check(who, kPairStride, conv, 2, conversion))) return rc;
  if (n == 0) return WALT_OK;
  if (!pairs || !dup) return fail(WALT_EINVAL, std::string(who) + ": bad argument");
  if ((rc = dd_reserve(dd, who, 2ull * n))) return rc;
  DeviceTemp d_rec, d_conv, d_dup;
  if ((rc = d_rec.put(pairs, (size_t)n * kPairStride, kWhat)) || (rc = d_dup.get(2 * (size_t)n, kWhat)) ||
      (conv && (rc = d_conv.put(conv, 2 * (size_t)n, kWhat))))
    return rc;
  if ((rc = dd_launch(dd, who, {true, d_rec.p, kPairStride, d_conv.p, 2, conversion, 0, n, d_dup.p}, nullptr))) return rc;
  return dd_finish(dd, who, dup, d_dup.p, 2 * (size_t)n);
}

}  // extern "C"
