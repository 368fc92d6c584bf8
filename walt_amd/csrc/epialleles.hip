// epialleles.hip -- four-CpG epialleles on the device (include/walt_amd.h, "four-CpG epialleles"): one streaming kernel
// over the calls of a batch that folds each read's CpG calls in read order into a table of sixteen counters per pair
// number -- the patterns the four neighbouring CpGs from that pair on showed on one read -- and the deterministic
// two-pass extraction of the entries with enough reads.  The pair bitmap, its rank directory, the scan and the launch
// shapes are cpgpairs.hip's (cpg_device.h); the per-lane logic is epialleles_core.h's.  The reference has no such mode;
// the contract is the header's.
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "epialleles_core.h"
#include "cpg_device.h"

namespace walt {

constexpr uint32_t kEpiBlocksPerCu = 8;  // no LDS beyond the chromosome starts: the grid is bounded by the device
static_assert(sizeof(walt_epiallele_site) == 72, "walt_epiallele_site is 72 bytes");
static_assert(kEpiColumns == 16, "an entry is four 16-byte loads");

// ---------------------------------------------------------------------------
// the window kernel
// ---------------------------------------------------------------------------
struct EpiArgs {
  const uint8_t* calls;
  const uint64_t* offsets;
  uint32_t n;
  const uint8_t* records;
  uint64_t rec_stride;
  const uint8_t* skip;         // null: none
  uint64_t skip_stride;
  const uint32_t* bits;
  const uint32_t* dir;
  uint32_t* table;             // count[n_pairs][16]
  uint32_t genome_len;
  const uint32_t* start_index;
  uint32_t n_chrom;
};

// One window: a 32-bit add whose result nobody reads (cpgpairs.hip cpg_add).
__device__ __forceinline__ void epi_add(uint32_t* __restrict__ table, uint32_t entry, uint32_t column) {
  (void)__hip_atomic_fetch_add(table + (uint64_t)kEpiColumns * entry + column, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_cpg_pairs's shape (cpgpairs.hip): eight lanes per read, one aligned 16-byte slice of its calls per lane and trip, the
// rank of a call gathered once.  The fold has a depth of three calls instead of one: a lane adds the windows that lie
// wholly inside its slice and keeps the slice's head chain (its first calls, at most three) and tail chain (chain(slice),
// epialleles_core.h); the tails are scanned across the group in lane order with epi_combine (after step d lane s holds
// chain(slices s - 2 d + 1 .. s)), so that every lane learns the chain that reaches its slice -- from the lanes to its
// left or, through `carry`, from earlier trips, empty ones included -- and adds the windows that end on its head calls:
// a window belongs to the lane that holds its last call, at most three per lane and trip.  All eight lanes of a group
// take every trip together (nonconv_trips); the groups of a wavefront may diverge from each other: a shuffle of width 8
// stays inside its group.  A call that has no pair is skipped by number(), so the chain runs over it as the contract's
// "calls that have a pair" do; a '.' leaves no call and the pair numbers on its two sides are no neighbours.
__global__ __launch_bounds__(kBlock) void k_epialleles(const EpiArgs a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  __syncthreads();
  const uint32_t sub = threadIdx.x & (kCpgGroup - 1);
  const uint64_t groups = (uint64_t)gridDim.x * (kBlock / kCpgGroup);
  const uint64_t batch_lo = a.offsets[0], batch_hi = a.offsets[a.n];  // the calls the batch owns: a slice stays inside them
  for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / kCpgGroup) + threadIdx.x / kCpgGroup; r < a.n; r += groups) {
    const uint64_t off = a.offsets[r], end = a.offsets[r + 1];
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.records + r * a.rec_stride);
    const uint32_t pos = rec[0], times = rec[1];
    const bool minus = (rec[2] & 0xFFu) == '-';
    const uint32_t skip = a.skip ? a.skip[r * a.skip_stride] : 0u;
    // (before any index or address; the same for the group)
    if (!cpg_counted(times, skip, off, end, pos, a.genome_len) || off < batch_lo || end > batch_hi) continue;
    uint32_t c_lo = 0, c_hi = 0;
    chrom_bounds(s_start, a.start_index, tab, pos, c_lo, c_hi);
    const uint8_t* rb = a.calls + off;
    const int len = (int)(end - off);
    const int head = (int)((uintptr_t)rb & 15u);
    const int trips = nonconv_trips(len, head);
    const auto number = [&](int i) -> long long {
      const long long c = cpg_call_pair(a.bits, pos, i, minus, c_lo, c_hi);
      return c < 0 ? -1ll : (long long)cpg_rank(a.bits, a.dir, (uint32_t)c);
    };
    const auto add = [&](uint32_t entry, uint32_t column) { epi_add(a.table, entry, column); };
    unsigned long long carry = 0ull;
    for (int t = 0; t < trips; ++t) {
      const int i0 = -head + 16 * ((int)kCpgGroup * t + (int)sub);
      unsigned long long first = 0ull, incl = 0ull;
      if (i0 < len) {
        uint32_t w[4];
        mbias_load_slice(rb, len, i0, off - batch_lo, batch_hi - off, w);
        if (mbias_not_dot(w[0]) | mbias_not_dot(w[1]) | mbias_not_dot(w[2]) | mbias_not_dot(w[3]))
          epi_slice(w, i0, number, add, first, incl);
      }
#pragma unroll
      for (int d = 1; d < (int)kCpgGroup; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, (unsigned)d, (int)kCpgGroup);
        incl = epi_combine(sub >= (uint32_t)d ? o : 0ull, incl);
      }
      const unsigned long long left = __shfl_up(incl, 1u, (int)kCpgGroup);
      if (first) epi_straddle(epi_combine(carry, sub ? left : 0ull), first, add);
      carry = epi_combine(carry, __shfl(incl, (int)kCpgGroup - 1, (int)kCpgGroup));
    }
  }
}

// ---------------------------------------------------------------------------
// the extraction
// ---------------------------------------------------------------------------
struct EpiExtract {
  const uint32_t* bits;
  const uint32_t* dir;
  const uint32_t* table;
  uint64_t n_words;            // the bitmap's words with its padding (cpg_next)
  uint32_t pos_lo, pos_hi;
  uint64_t w_lo, w_hi;         // the bitmap words that hold [pos_lo, pos_hi)
  uint64_t chunk;              // words per block
  unsigned long long min_total;
  unsigned long long* scan;
  walt_epiallele_site* out;
  unsigned long long cap;
};

__device__ __forceinline__ void epi_block_words(const EpiExtract& a, uint64_t& lo, uint64_t& hi) {
  lo = a.w_lo + (uint64_t)blockIdx.x * a.chunk;
  hi = lo + a.chunk;
  lo = lo < a.w_hi ? lo : a.w_hi;
  hi = hi < a.w_hi ? hi : a.w_hi;
}
// entry j (64 bytes at a 64-byte aligned place) and the sum of its counters
__device__ __forceinline__ unsigned long long epi_entry(const EpiExtract& a, uint32_t j, uint4 e[4]) {
  const uint4* p = reinterpret_cast<const uint4*>(a.table) + 4ull * j;
  unsigned long long sum = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k] = p[k];
    sum += (unsigned long long)e[k].x + e[k].y + e[k].z + e[k].w;
  }
  return sum;
}
// the pairs of bitmap word w inside the range, and the number of the first of them
__device__ __forceinline__ uint32_t epi_word_pairs(const EpiExtract& a, uint64_t w, uint32_t& j0) {
  const uint32_t word = a.bits[w] & cpg_range_mask(w, a.pos_lo, a.pos_hi);
  if (word) j0 = cpg_rank(a.bits, a.dir, (uint32_t)(32u * w) + (uint32_t)__builtin_ctz(word));
  return word;
}
__device__ __forceinline__ uint32_t epi_word_count(const EpiExtract& a, uint64_t w) {
  uint32_t j = 0, n = 0;
  uint4 e[4];
  for (uint32_t word = epi_word_pairs(a, w, j); word; word &= word - 1u, ++j) n += epi_entry(a, j, e) >= a.min_total;
  return n;
}
// c_{j+3} from c_j: three steps along the bitmap (kCpgNoNext when one finds nothing: no entry that a read added to)
__device__ __forceinline__ uint32_t epi_window_last(const EpiExtract& a, uint32_t pos) {
#pragma unroll 1
  for (uint32_t k = 0; k < kEpiWindow - 1 && pos != kCpgNoNext; ++k) pos = cpg_next(a.bits, pos, a.n_words);
  return pos;
}

// pass 1: entries with min_total reads per block
__global__ __launch_bounds__(kBlock) void k_epi_count(const EpiExtract a) {
  __shared__ uint32_t s_red[kBlock / 64];
  uint64_t lo, hi;
  epi_block_words(a, lo, hi);
  uint32_t v = 0;
  for (uint64_t w = lo + threadIdx.x; w < hi; w += kBlock) v += epi_word_count(a, w);
  const uint32_t t = cpg_block_sum(v, s_red);
  if (threadIdx.x == 0) a.scan[blockIdx.x] = t;
}

// pass 2: the records, ascending by position: a block walks its words kBlock at a time, a thread writes the entries of
// its word behind those of the threads in front of it
__global__ __launch_bounds__(kBlock) void k_epi_write(const EpiExtract a, uint32_t n_blocks) {
  __shared__ uint32_t s_wave[kBlock / 64];
  if (a.scan[n_blocks] > a.cap) return;  // (uniform) too many for the caller's array: nothing is written
  uint64_t lo, hi;
  epi_block_words(a, lo, hi);
  unsigned long long at = a.scan[blockIdx.x];
  for (uint64_t w0 = lo; w0 < hi; w0 += kBlock) {  // (uniform trip count)
    const uint64_t w = w0 + threadIdx.x;
    const uint32_t v = w < hi ? epi_word_count(a, w) : 0u;
    uint32_t total = 0;
    const uint32_t before = cpg_block_before(v, s_wave, total);
    if (v) {
      unsigned long long slot = at + before;
      uint32_t j = 0;
      uint4 e[4];
      for (uint32_t word = epi_word_pairs(a, w, j); word; word &= word - 1u, ++j) {
        if (epi_entry(a, j, e) < a.min_total) continue;
        const uint32_t pos = (uint32_t)(32u * w) + (uint32_t)__builtin_ctz(word);
        uint2* rec = reinterpret_cast<uint2*>(a.out + slot);  // (72-byte records at an 8-byte aligned base)
        rec[0] = make_uint2(pos, epi_window_last(a, pos));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          rec[1 + 2 * k] = make_uint2(e[k].x, e[k].y);
          rec[2 + 2 * k] = make_uint2(e[k].z, e[k].w);
        }
        ++slot;
      }
    }
    at += total;
    __syncthreads();  // s_wave is rewritten by the next step
  }
}

static uint64_t epi_table_bytes(const walt_epialleles* ep) { return 4ull * kEpiColumns * std::max<uint32_t>(ep->n_pairs, 1u); }

int epialleles_launch(walt_epialleles* ep, const MbiasBatch& b, hipStream_t stream) {
  if (b.n == 0) return WALT_OK;
  const walt_index* idx = ep->idx;
  WALT_HIP(hipSetDevice(idx->device));
  EpiArgs a;
  a.calls = static_cast<const uint8_t*>(b.calls);
  a.offsets = static_cast<const uint64_t*>(b.offsets);
  a.n = b.n;
  a.records = static_cast<const uint8_t*>(b.records);
  a.rec_stride = b.rec_stride;
  a.skip = static_cast<const uint8_t*>(b.skip);
  a.skip_stride = b.skip_stride;
  a.bits = ep->bits;
  a.dir = ep->dir;
  a.table = ep->table;
  a.genome_len = idx->head.genome_len;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  const uint64_t want = ((uint64_t)b.n + kBlock / kCpgGroup - 1) / (kBlock / kCpgGroup);
  const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)idx->n_cu * kEpiBlocksPerCu);
  hipLaunchKernelGGL(k_epialleles, dim3(grid), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

// what both batch forms refuse before they look at the batch
static int epi_batch_check(const walt_epialleles* ep, const std::string& who, const MbiasBatch& b) {
  if (!ep) return fail(WALT_EINVAL, who + ": bad argument (null epiallele table)");
  std::string bad = record_stride_refusal(b.rec_stride);
  if (bad.empty()) bad = skip_stride_refusal(b.skip, b.skip_stride);
  return bad.empty() ? WALT_OK : fail(WALT_EINVAL, who + ": " + bad);
}

static int epi_range_check(const walt_epialleles* ep, const char* who, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total) {
  if (!ep) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null epiallele table)");
  if (pos_lo > pos_hi || pos_hi > ep->idx->head.genome_len)
    return fail(WALT_EINVAL, std::string(who) + ": range [" + std::to_string(pos_lo) + ", " + std::to_string(pos_hi) +
                                 ") is not inside the genome's " + std::to_string(ep->idx->head.genome_len) + " positions");
  if (!min_total) return fail(WALT_EINVAL, std::string(who) + ": min_total must be at least 1");
  return WALT_OK;
}

static EpiExtract epi_extract_args(const walt_epialleles* ep, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, uint32_t& n_blocks) {
  EpiExtract a;
  a.bits = ep->bits; a.dir = ep->dir; a.table = ep->table;
  a.n_words = ep->n_words;
  a.pos_lo = pos_lo; a.pos_hi = pos_hi;
  const CpgShape sh = cpg_extract_shape(ep->idx, pos_lo, pos_hi);
  a.w_lo = sh.w_lo; a.w_hi = sh.w_hi; a.chunk = sh.chunk;
  n_blocks = sh.n_blocks;
  a.min_total = min_total;
  a.scan = ep->scan;
  a.out = nullptr; a.cap = 0;
  return a;
}

// count and scan on `stream`; the total lands in scan[n_blocks] and, when given, in *d_n_out
static int epi_count_launch(const EpiExtract& a, uint32_t n_blocks, void* d_n_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_epi_count, dim3(n_blocks), dim3(kBlock), 0, stream, a);
  cpg_scan_launch(a.scan, n_blocks, static_cast<unsigned long long*>(d_n_out), stream);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_epialleles_create(walt_index* idx, walt_epialleles** out) {
  if (!idx || !out) return fail(WALT_EINVAL, "walt_epialleles_create: bad argument");
  *out = nullptr;
  if (!idx->ref[0])
    return fail(WALT_EINVAL, "walt_epialleles_create: the index holds no reference (open it with WALT_WITH_REFERENCE or call "
                             "walt_index_enable_reference)");
  WALT_HIP(hipSetDevice(idx->device));
  walt_epialleles* ep = new walt_epialleles;
  ep->idx = idx;
  CpgRank rank;
  uint64_t wanted = cpg_rank_bytes(idx);
  const auto give_up = [&](int code, const std::string& msg) {  // the index stays as it was
    (void)hipGetLastError();
    cpg_rank_free(rank);
    (void)hipFree(ep->table);
    delete ep;
    return fail(code, msg);
  };
  const auto no_memory = [&]() {
    return give_up(WALT_ENOMEM, "walt_epialleles_create: the epiallele table wants " + std::to_string(wanted) +
                                    " bytes of device memory (genome_len / 8 + genome_len / 32 + 64 per CpG pair)");
  };
  hipError_t e = hipSuccess;
  if (!cpg_rank_build(idx, rank, e)) {
    if (e == hipSuccess) return no_memory();
    return give_up(WALT_EHIP, std::string("walt_epialleles_create: building the pair bitmap failed: ") + hipGetErrorString(e));
  }
  ep->bits = rank.bits; ep->dir = rank.dir; ep->scan = rank.scan;
  ep->n_words = rank.n_words;
  ep->n_pairs = rank.n_pairs;
  wanted += epi_table_bytes(ep);
  if (hipMalloc(reinterpret_cast<void**>(&ep->table), epi_table_bytes(ep)) != hipSuccess) return no_memory();
  if (hipMemset(ep->table, 0, epi_table_bytes(ep)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return give_up(WALT_EHIP, "walt_epialleles_create: the table could not be cleared");
  ep->device_bytes = wanted;
  *out = ep;
  return WALT_OK;
}

void walt_epialleles_destroy(walt_epialleles* ep) {
  if (!ep) return;
  (void)hipSetDevice(ep->idx->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(ep->bits);
  (void)hipFree(ep->dir);
  (void)hipFree(ep->scan);
  (void)hipFree(ep->table);
  delete ep;
}

int walt_epialleles_clear(walt_epialleles* ep) {
  if (!ep) return fail(WALT_EINVAL, "walt_epialleles_clear: bad argument (null epiallele table)");
  WALT_HIP(hipSetDevice(ep->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  WALT_HIP(hipMemset(ep->table, 0, epi_table_bytes(ep)));
  WALT_HIP(hipDeviceSynchronize());
  return WALT_OK;
}

uint64_t walt_epialleles_device_bytes(const walt_epialleles* ep) { return ep ? ep->device_bytes : 0; }
uint64_t walt_epialleles_n_pairs(const walt_epialleles* ep) { return ep ? ep->n_pairs : 0; }

int walt_epialleles_batch_device(walt_epialleles* ep, const void* d_calls, const void* d_offsets, uint32_t n, const void* d_records,
                                 size_t record_stride, const void* d_skip, size_t skip_stride, void* stream) {
  const std::string who = "walt_epialleles_batch_device";
  const MbiasBatch b = {d_calls, d_offsets, n, d_records, record_stride, d_skip, skip_stride};
  if (const int rc = epi_batch_check(ep, who, b)) return rc;
  if (n && (!d_calls || !d_offsets || !d_records)) return fail(WALT_EINVAL, who + ": bad argument (null calls, offsets or records)");
  if (((uintptr_t)d_records & 3u) || ((uintptr_t)d_offsets & 7u))
    return fail(WALT_EINVAL, who + ": records must be 4-byte aligned, offsets 8-byte aligned");
  return epialleles_launch(ep, b, reinterpret_cast<hipStream_t>(stream));
}

int walt_epialleles_batch(walt_epialleles* ep, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                          size_t record_stride, const uint8_t* skip, size_t skip_stride) {
  const std::string who = "walt_epialleles_batch";
  // (host arrays: no alignment is asked of them; the device copies below are aligned)
  int rc = epi_batch_check(ep, who, {calls, offsets, n, records, record_stride, skip, skip_stride});
  if (rc) return rc;
  if (n == 0) return WALT_OK;
  if (!offsets || !records || (!calls && offsets[n] > offsets[0])) return fail(WALT_EINVAL, who + ": bad argument (null calls, offsets or records)");
  uint32_t max_len = 0;
  if (const char* bad = scan_offsets(offsets, n, &max_len)) return fail(WALT_EINVAL, who + ": " + bad);
  WALT_HIP(hipSetDevice(ep->idx->device));
  const uint64_t nbytes = offsets[n] - offsets[0];
  // records and skip bytes as the kernel reads them: packed (the caller's strides stay on the host)
  const std::vector<walt_best_match> rec = pack_strided<walt_best_match>(records, record_stride, n);
  const std::vector<uint8_t> sk = pack_strided<uint8_t>(skip, skip_stride, skip ? n : 0);
  std::vector<uint64_t> rel;
  const uint64_t* off = rebase_offsets(offsets, n, rel);
  const char* what = "four-CpG epialleles";
  DeviceTemp d_calls, d_off, d_rec, d_skip;
  if ((rc = d_calls.put(nbytes ? calls + offsets[0] : nullptr, nbytes, what)) || (rc = d_off.put(off, ((size_t)n + 1) * 8, what)) ||
      (rc = d_rec.put(rec.data(), (size_t)n * 16, what)) || (skip && (rc = d_skip.put(sk.data(), n, what))))
    return rc;
  if ((rc = epialleles_launch(ep, {d_calls.p, d_off.p, n, d_rec.p, 16, d_skip.p, 1}, nullptr))) return rc;
  WALT_HIP(hipStreamSynchronize(nullptr));
  return WALT_OK;
}

int walt_epialleles_extract_device(walt_epialleles* ep, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, void* d_out,
                                   uint64_t cap, void* d_n_out, void* stream) {
  int rc = epi_range_check(ep, "walt_epialleles_extract_device", pos_lo, pos_hi, min_total);
  if (rc) return rc;
  if (!d_n_out || (cap && !d_out)) return fail(WALT_EINVAL, "walt_epialleles_extract_device: bad argument");
  if (((uintptr_t)d_out & 7u) || ((uintptr_t)d_n_out & 7u))
    return fail(WALT_EINVAL, "walt_epialleles_extract_device: out and n_out must be 8-byte aligned");
  WALT_HIP(hipSetDevice(ep->idx->device));
  uint32_t n_blocks;
  EpiExtract a = epi_extract_args(ep, pos_lo, pos_hi, min_total, n_blocks);
  a.out = static_cast<walt_epiallele_site*>(d_out);
  a.cap = cap;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if ((rc = epi_count_launch(a, n_blocks, d_n_out, s))) return rc;
  if (cap) hipLaunchKernelGGL(k_epi_write, dim3(n_blocks), dim3(kBlock), 0, s, a, n_blocks);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

int walt_epialleles_extract(walt_epialleles* ep, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, walt_epiallele_site* out,
                            uint64_t cap, uint64_t* n_out) {
  int rc = epi_range_check(ep, "walt_epialleles_extract", pos_lo, pos_hi, min_total);
  if (rc) return rc;
  if (!n_out || (cap && !out)) return fail(WALT_EINVAL, "walt_epialleles_extract: bad argument");
  WALT_HIP(hipSetDevice(ep->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  uint32_t n_blocks;
  EpiExtract a = epi_extract_args(ep, pos_lo, pos_hi, min_total, n_blocks);
  if ((rc = epi_count_launch(a, n_blocks, nullptr, nullptr))) return rc;
  unsigned long long total = 0;
  WALT_HIP(hipMemcpy(&total, ep->scan + n_blocks, 8, hipMemcpyDeviceToHost));
  *n_out = total;
  if (total > cap)
    return fail(WALT_EINVAL, "walt_epialleles_extract: the range holds " + std::to_string(total) + " entries, the array has room for " +
                                 std::to_string(cap));
  if (!total) return WALT_OK;
  DeviceTemp d_out;
  if (hipMalloc(&d_out.p, total * sizeof(walt_epiallele_site)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(WALT_ENOMEM, "walt_epialleles_extract: hipMalloc of " + std::to_string(total * sizeof(walt_epiallele_site)) + " bytes failed");
  }
  a.out = static_cast<walt_epiallele_site*>(d_out.p);
  a.cap = total;
  hipLaunchKernelGGL(k_epi_write, dim3(n_blocks), dim3(kBlock), 0, nullptr, a, n_blocks);
  WALT_HIP(hipGetLastError());
  WALT_HIP(hipMemcpy(out, d_out.p, total * sizeof(walt_epiallele_site), hipMemcpyDeviceToHost));
  return WALT_OK;
}

}  // extern "C"
