// cpg_device.h -- the one implementation of the two tables keyed by CpG pair number (adjacent CpG pairs, cpgpairs.hip;
// four-CpG epialleles, epialleles.hip).  A table is a CpgTable (device_common.h) and two policies:
//   Fold  what a read's calls add to the table: the columns of an entry, the fold of a 16-byte slice, how two stretches
//         meet, what straddles a slice's left boundary (CpgPairFold in cpgpairs_core.h, EpiFold in epialleles_core.h;
//         cpg_fold_read<Fold> there is the one-thread model of k_cpg_fold<Fold>);
//   Tab   the table as its .hip file describes it: its handle, Fold and record types, the nouns of its messages, and for
//         the extraction how an entry is loaded, whether it is kept, and how its record is written.
// Here: the builder of the pair bitmap and its rank directory (defined in cpgpairs.hip), the fold kernel, the
// extraction's count / scan / write passes, and everything the host does around them.  The extern "C" functions of the
// two .hip files forward to the cpg_table_* templates.
#ifndef WALT_AMD_CPG_DEVICE_H_
#define WALT_AMD_CPG_DEVICE_H_

#include <algorithm>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "cpgpairs_core.h"

namespace walt {

constexpr uint32_t kCpgBlocksPerCu = 8;      // no LDS beyond the chromosome starts: the grid is bounded by the device
constexpr uint32_t kCpgMaxBlocks = 65536;    // blocks of an extraction at most
constexpr uint32_t kCpgTileWords = 128;      // bitmap words (4096 positions) per block the default grid aims at
constexpr uint32_t kCpgScanWords = kCpgMaxBlocks + 2;  // block offsets, the total behind them

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
// k_cpg_scan over table[0 .. n) on `stream` (total_out: null, or a device word that gets the sum too)
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

// ---------------------------------------------------------------------------
// the fold kernel
// ---------------------------------------------------------------------------
struct CpgFoldArgs {
  CallsView v;
  const uint32_t* bits;
  const uint32_t* dir;
  uint32_t* table;             // count[n_pairs][Fold::kColumns]
  uint32_t genome_len;
  const uint32_t* start_index;
  uint32_t n_chrom;
};

// k_mbias's access shape (mbias.hip): eight lanes per read, one aligned 16-byte slice of its calls per lane and trip.
// Order matters, as in k_nonconv: a lane folds its slice -- it adds what lies wholly inside it (couples; windows) and
// keeps what its first calls and its last calls leave (`first`, `incl`: a call for the pair table, a chain of up to three
// for the epialleles, epialleles_core.h); the `incl` are scanned across the group in lane order with Fold::combine (after
// step d lane s holds the fold of slices s - 2 d + 1 .. s), so that every lane learns what reaches its slice -- from the
// lanes to its left or, through `carry`, from earlier trips, empty ones included -- and Fold::straddle adds what ends on
// its first calls: the couple, or at most three windows, that straddle its left boundary.  All eight lanes of a group
// take every trip together (nonconv_trips); the groups of a wavefront may diverge from each other: a shuffle of width 8
// stays inside its group.  A call that has no pair is skipped by number(), so a chain runs over it as the contract's
// "calls that have a pair" do; a '.' leaves no call and the pair numbers on its two sides are no neighbours.
// What is read per call: the bitmap word of the call's position (and its left neighbour's at a word boundary), then the
// rank: one directory word and one 16-byte block of the bitmap.  Calls are sparse -- a CpG every 50 to 100 bases of a
// mammalian genome -- and a slice without z / Z costs its load and four word tests.  An add is a 32-bit atomic whose
// result nobody reads (meth.hip pile_add).
template <class Fold>
__global__ __launch_bounds__(kBlock) void k_cpg_fold(const CpgFoldArgs a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  __syncthreads();
  const uint32_t sub = threadIdx.x & (kCpgGroup - 1);
  const uint64_t groups = (uint64_t)gridDim.x * (kBlock / kCpgGroup);
  const uint64_t batch_lo = a.v.offsets[0], batch_hi = a.v.offsets[a.v.n];  // the calls the batch owns: a slice stays inside them
  for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / kCpgGroup) + threadIdx.x / kCpgGroup; r < a.v.n; r += groups) {
    const uint64_t off = a.v.offsets[r], end = a.v.offsets[r + 1];
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.v.records + r * a.v.rec_stride);
    const uint32_t pos = rec[0], times = rec[1];
    const bool minus = (rec[2] & 0xFFu) == '-';
    const uint32_t skip = a.v.skip ? a.v.skip[r * a.v.skip_stride] : 0u;
    // (before any index or address; the same for the group)
    if (!cpg_counted(times, skip, off, end, pos, a.genome_len) || off < batch_lo || end > batch_hi) continue;
    uint32_t c_lo = 0, c_hi = 0;
    chrom_bounds(s_start, a.start_index, tab, pos, c_lo, c_hi);
    const uint8_t* rb = a.v.calls + off;
    const int len = (int)(end - off);
    const int head = (int)((uintptr_t)rb & 15u);
    const int trips = nonconv_trips(len, head);
    const auto number = [&](int i) -> long long {
      const long long c = cpg_call_pair(a.bits, pos, i, minus, c_lo, c_hi);
      return c < 0 ? -1ll : (long long)cpg_rank(a.bits, a.dir, (uint32_t)c);
    };
    const auto add = [&](uint32_t entry, uint32_t column) {
      (void)__hip_atomic_fetch_add(a.table + (uint64_t)Fold::kColumns * entry + column, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    unsigned long long carry = 0ull;
    for (int t = 0; t < trips; ++t) {
      const int i0 = -head + 16 * ((int)kCpgGroup * t + (int)sub);
      unsigned long long first = 0ull, incl = 0ull;
      if (i0 < len) {
        uint32_t w[4];
        mbias_load_slice(rb, len, i0, off - batch_lo, batch_hi - off, w);
        if (mbias_not_dot(w[0]) | mbias_not_dot(w[1]) | mbias_not_dot(w[2]) | mbias_not_dot(w[3]))
          Fold::slice(w, i0, number, add, first, incl);
      }
#pragma unroll
      for (int d = 1; d < (int)kCpgGroup; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, (unsigned)d, (int)kCpgGroup);
        incl = Fold::combine(sub >= (uint32_t)d ? o : 0ull, incl);
      }
      const unsigned long long left = __shfl_up(incl, 1u, (int)kCpgGroup);
      Fold::straddle(carry, sub ? left : 0ull, first, add);
      carry = Fold::combine(carry, __shfl(incl, (int)kCpgGroup - 1, (int)kCpgGroup));
    }
  }
}

// k_cpg_fold<Fold> over a batch on `stream` of the table's index's device
template <class Fold>
int cpg_fold_launch(CpgTable* t, const CallsBatch& b, hipStream_t stream) {
  if (b.n == 0) return WALT_OK;
  const walt_index* idx = t->idx;
  WALT_HIP(hipSetDevice(idx->device));
  const CpgFoldArgs a = {calls_view(b), t->bits, t->dir, t->table, idx->head.genome_len, idx->view.start_index, idx->view.n_chrom};
  const uint64_t want = ((uint64_t)b.n + kBlock / kCpgGroup - 1) / (kBlock / kCpgGroup);
  const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)idx->n_cu * kCpgBlocksPerCu);
  hipLaunchKernelGGL(k_cpg_fold<Fold>, dim3(grid), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

// ---------------------------------------------------------------------------
// the extraction
// ---------------------------------------------------------------------------
struct CpgExtract {
  const uint32_t* bits;
  const uint32_t* dir;
  const uint32_t* table;
  uint64_t n_words;            // the bitmap's words with its padding (cpg_next)
  uint32_t pos_lo, pos_hi;
  uint64_t w_lo, w_hi;         // the bitmap words that hold [pos_lo, pos_hi)
  uint64_t chunk;              // words per block
  unsigned long long min_total;  // the reads an entry needs to be kept, for a table that asks (the pair table keeps the non-zero ones)
  unsigned long long* scan;
  void* out;                   // Tab::Site records
  unsigned long long cap;
};

__device__ __forceinline__ void cpg_block_words(const CpgExtract& a, uint64_t& lo, uint64_t& hi) {
  lo = a.w_lo + (uint64_t)blockIdx.x * a.chunk;
  hi = lo + a.chunk;
  lo = lo < a.w_hi ? lo : a.w_hi;
  hi = hi < a.w_hi ? hi : a.w_hi;
}
// the pairs of bitmap word w inside the range, and the number of the first of them
__device__ __forceinline__ uint32_t cpg_word_pairs(const CpgExtract& a, uint64_t w, uint32_t& j0) {
  const uint32_t word = a.bits[w] & cpg_range_mask(w, a.pos_lo, a.pos_hi);
  if (word) j0 = cpg_rank(a.bits, a.dir, (uint32_t)(32u * w) + (uint32_t)__builtin_ctz(word));
  return word;
}
// the entries of word w that are kept (Tab::load: entry j into e, -> whether it is kept)
template <class Tab>
__device__ __forceinline__ uint32_t cpg_word_count(const CpgExtract& a, uint64_t w) {
  uint32_t j = 0, n = 0;
  typename Tab::Entry e;
  for (uint32_t word = cpg_word_pairs(a, w, j); word; word &= word - 1u, ++j) n += Tab::load(a, j, e);
  return n;
}

// pass 1: kept entries per block
template <class Tab>
__global__ __launch_bounds__(kBlock) void k_cpg_count(const CpgExtract a) {
  __shared__ uint32_t s_red[kBlock / 64];
  uint64_t lo, hi;
  cpg_block_words(a, lo, hi);
  uint32_t v = 0;
  for (uint64_t w = lo + threadIdx.x; w < hi; w += kBlock) v += cpg_word_count<Tab>(a, w);
  const uint32_t t = cpg_block_sum(v, s_red);
  if (threadIdx.x == 0) a.scan[blockIdx.x] = t;
}

// pass 2: the records, ascending by position: a block walks its words kBlock at a time, a thread writes the entries of
// its word behind those of the threads in front of it (Tab::store: the record of entry e, whose pair starts at pos)
template <class Tab>
__global__ __launch_bounds__(kBlock) void k_cpg_write(const CpgExtract a, uint32_t n_blocks) {
  __shared__ uint32_t s_wave[kBlock / 64];
  if (a.scan[n_blocks] > a.cap) return;  // (uniform) too many for the caller's array: nothing is written
  uint64_t lo, hi;
  cpg_block_words(a, lo, hi);
  unsigned long long at = a.scan[blockIdx.x];
  for (uint64_t w0 = lo; w0 < hi; w0 += kBlock) {  // (uniform trip count)
    const uint64_t w = w0 + threadIdx.x;
    const uint32_t v = w < hi ? cpg_word_count<Tab>(a, w) : 0u;
    uint32_t total = 0;
    const uint32_t before = cpg_block_before(v, s_wave, total);
    if (v) {
      unsigned long long slot = at + before;
      uint32_t j = 0;
      typename Tab::Entry e;
      for (uint32_t word = cpg_word_pairs(a, w, j); word; word &= word - 1u, ++j) {
        if (!Tab::load(a, j, e)) continue;
        Tab::store(a, slot, (uint32_t)(32u * w) + (uint32_t)__builtin_ctz(word), e);
        ++slot;
      }
    }
    at += total;
    __syncthreads();  // s_wave is rewritten by the next step
  }
}

// ---------------------------------------------------------------------------
// the host side
// ---------------------------------------------------------------------------
template <class Tab>
uint64_t cpg_table_bytes(const CpgTable* t) { return 4ull * Tab::Fold::kColumns * std::max<uint32_t>(t->n_pairs, 1u); }

template <class Tab>
int cpg_table_create(const std::string& who, walt_index* idx, typename Tab::Handle** out) {
  if (!idx || !out) return fail(WALT_EINVAL, who + ": bad argument");
  *out = nullptr;
  if (!idx->ref[0])
    return fail(WALT_EINVAL, who + ": the index holds no reference (open it with WALT_WITH_REFERENCE or call "
                                   "walt_index_enable_reference)");
  WALT_HIP(hipSetDevice(idx->device));
  typename Tab::Handle* t = new typename Tab::Handle;
  t->idx = idx;
  CpgRank rank;
  uint64_t wanted = cpg_rank_bytes(idx);
  const auto give_up = [&](int code, const std::string& msg) {  // the index stays as it was
    (void)hipGetLastError();
    cpg_rank_free(rank);
    (void)hipFree(t->table);
    delete t;
    return fail(code, msg);
  };
  const auto no_memory = [&]() {
    return give_up(WALT_ENOMEM, who + ": the " + Tab::kNoun + " wants " + std::to_string(wanted) +
                                    " bytes of device memory (genome_len / 8 + genome_len / 32 + " +
                                    std::to_string(4 * Tab::Fold::kColumns) + " per CpG pair)");
  };
  hipError_t e = hipSuccess;
  if (!cpg_rank_build(idx, rank, e)) {
    if (e == hipSuccess) return no_memory();
    return give_up(WALT_EHIP, who + ": building the pair bitmap failed: " + hipGetErrorString(e));
  }
  t->bits = rank.bits; t->dir = rank.dir; t->scan = rank.scan;
  t->n_words = rank.n_words;
  t->n_pairs = rank.n_pairs;
  wanted += cpg_table_bytes<Tab>(t);
  if (hipMalloc(reinterpret_cast<void**>(&t->table), cpg_table_bytes<Tab>(t)) != hipSuccess) return no_memory();
  if (hipMemset(t->table, 0, cpg_table_bytes<Tab>(t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return give_up(WALT_EHIP, who + ": the table could not be cleared");
  t->device_bytes = wanted;
  *out = t;
  return WALT_OK;
}

template <class Tab>
void cpg_table_destroy(typename Tab::Handle* t) {
  if (!t) return;
  (void)hipSetDevice(t->idx->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(t->bits);
  (void)hipFree(t->dir);
  (void)hipFree(t->scan);
  (void)hipFree(t->table);
  delete t;
}

template <class Tab>
int cpg_table_clear(const std::string& who, CpgTable* t) {
  if (!t) return fail(WALT_EINVAL, who + ": bad argument (null " + Tab::kNoun + ")");
  WALT_HIP(hipSetDevice(t->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  WALT_HIP(hipMemset(t->table, 0, cpg_table_bytes<Tab>(t)));
  WALT_HIP(hipDeviceSynchronize());
  return WALT_OK;
}

// what both batch forms refuse before they look at the batch
template <class Tab>
int cpg_batch_check(const CpgTable* t, const std::string& who, const CallsBatch& b) {
  if (!t) return fail(WALT_EINVAL, who + ": bad argument (null " + Tab::kNoun + ")");
  std::string bad = record_stride_refusal(b.rec_stride);
  if (bad.empty()) bad = skip_stride_refusal(b.skip, b.skip_stride);
  return bad.empty() ? WALT_OK : fail(WALT_EINVAL, who + ": " + bad);
}

template <class Tab>
int cpg_table_batch_device(const std::string& who, CpgTable* t, const CallsBatch& b, void* stream) {
  if (const int rc = cpg_batch_check<Tab>(t, who, b)) return rc;
  if (const int rc = calls_device_check(who, b)) return rc;
  return cpg_fold_launch<typename Tab::Fold>(t, b, reinterpret_cast<hipStream_t>(stream));
}

template <class Tab>
int cpg_table_batch(const std::string& who, CpgTable* t, const CallsBatch& host) {
  if (const int rc = cpg_batch_check<Tab>(t, who, host)) return rc;
  return calls_host_batch(who, Tab::kWhat, host, false, nullptr, t->idx->device,
                          [&](const CallsBatch& b) { return cpg_fold_launch<typename Tab::Fold>(t, b, nullptr); });
}

// An extraction of [pos_lo, pos_hi): the bitmap words that hold the range, cut into n_blocks chunks (extract_blocks)
template <class Tab>
CpgExtract cpg_extract_args(const CpgTable* t, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, uint32_t& n_blocks) {
  CpgExtract a;
  a.bits = t->bits; a.dir = t->dir; a.table = t->table;
  a.n_words = t->n_words;
  a.pos_lo = pos_lo; a.pos_hi = pos_hi;
  a.w_lo = pos_lo >> 5;
  a.w_hi = pos_hi > pos_lo ? ((uint64_t)pos_hi + 31u) >> 5 : a.w_lo;
  n_blocks = extract_blocks(t->idx, a.w_hi - a.w_lo, kCpgTileWords, kCpgMaxBlocks, &a.chunk);
  a.min_total = min_total;
  a.scan = t->scan;
  a.out = nullptr; a.cap = 0;
  return a;
}

// count and scan on `stream`; the total lands in scan[n_blocks] and, when given, in *d_n_out
template <class Tab>
int cpg_count_launch(const CpgExtract& a, uint32_t n_blocks, void* d_n_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_cpg_count<Tab>, dim3(n_blocks), dim3(kBlock), 0, stream, a);
  cpg_scan_launch(a.scan, n_blocks, static_cast<unsigned long long*>(d_n_out), stream);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

// The two extractions, after the caller's range check (range_refusal with Tab::kNoun, and what the table asks of
// min_total; a table without one passes 1).
template <class Tab>
int cpg_table_extract_device(const std::string& who, CpgTable* t, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, void* d_out,
                             uint64_t cap, void* d_n_out, void* stream) {
  if (!d_n_out || (cap && !d_out)) return fail(WALT_EINVAL, who + ": bad argument");
  if (((uintptr_t)d_out & 7u) || ((uintptr_t)d_n_out & 7u)) return fail(WALT_EINVAL, who + ": out and n_out must be 8-byte aligned");
  WALT_HIP(hipSetDevice(t->idx->device));
  uint32_t n_blocks;
  CpgExtract a = cpg_extract_args<Tab>(t, pos_lo, pos_hi, min_total, n_blocks);
  a.out = d_out;
  a.cap = cap;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (const int rc = cpg_count_launch<Tab>(a, n_blocks, d_n_out, s)) return rc;
  if (cap) hipLaunchKernelGGL(k_cpg_write<Tab>, dim3(n_blocks), dim3(kBlock), 0, s, a, n_blocks);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

template <class Tab>
int cpg_table_extract(const std::string& who, CpgTable* t, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total,
                      typename Tab::Site* out, uint64_t cap, uint64_t* n_out) {
  if (!n_out || (cap && !out)) return fail(WALT_EINVAL, who + ": bad argument");
  WALT_HIP(hipSetDevice(t->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  uint32_t n_blocks;
  CpgExtract a = cpg_extract_args<Tab>(t, pos_lo, pos_hi, min_total, n_blocks);
  if (const int rc = cpg_count_launch<Tab>(a, n_blocks, nullptr, nullptr)) return rc;
  unsigned long long total = 0;
  WALT_HIP(hipMemcpy(&total, t->scan + n_blocks, 8, hipMemcpyDeviceToHost));
  *n_out = total;
  if (total > cap)
    return fail(WALT_EINVAL, who + ": the range holds " + std::to_string(total) + " entries, the array has room for " + std::to_string(cap));
  if (!total) return WALT_OK;
  const size_t bytes = total * sizeof(typename Tab::Site);
  DeviceTemp d_out;
  if (hipMalloc(&d_out.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(WALT_ENOMEM, who + ": hipMalloc of " + std::to_string(bytes) + " bytes failed");
  }
  a.out = d_out.p;
  a.cap = total;
  hipLaunchKernelGGL(k_cpg_write<Tab>, dim3(n_blocks), dim3(kBlock), 0, nullptr, a, n_blocks);
  WALT_HIP(hipGetLastError());
  WALT_HIP(hipMemcpy(out, d_out.p, bytes, hipMemcpyDeviceToHost));
  return WALT_OK;
}

}  // namespace walt
#endif  // WALT_AMD_CPG_DEVICE_H_
