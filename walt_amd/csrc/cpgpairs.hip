// cpgpairs.hip -- adjacent CpG pairs on the device (include/walt_amd.h, "adjacent CpG pairs"): the pair bitmap and its
// rank directory built from the '+' reference, one streaming kernel over the calls of a batch that folds each read's
// CpG calls in read order into a table keyed by pair number, and the deterministic two-pass extraction of the non-zero
// entries.  The per-lane logic is cpgpairs_core.h's.  The reference has no such mode; the contract is the header's.
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "cpgpairs_core.h"
#include "cpg_device.h"

namespace walt {

constexpr uint32_t kCpgBlocksPerCu = 8;      // no LDS beyond the chromosome starts: the grid is bounded by the device
constexpr uint32_t kCpgMaxBlocks = 65536;    // blocks of an extraction at most
constexpr uint32_t kCpgTileWords = 128;      // bitmap words (4096 positions) per block the default grid aims at
constexpr uint32_t kCpgScanWords = kCpgMaxBlocks + 2;  // block offsets, the total behind them
constexpr uint32_t kCpgRefPadWords = 16;     // as meth.hip: zero words behind a packed reference
static_assert(sizeof(walt_cpgpair_site) == 24, "walt_cpgpair_site is 24 bytes");
static_assert(kCpgMaxCalls == WALT_MBIAS_POSITIONS, "the reads that add are the reads the bias table counts");

// ---------------------------------------------------------------------------
// the bitmap and its directory
// ---------------------------------------------------------------------------
// one bitmap word per thread, from three words of the '+' reference (ref_last: the last word the array holds)
__global__ __launch_bounds__(kBlock) void k_cpg_bits(const uint32_t* __restrict__ ref, uint32_t ref_last, uint64_t n_words,
                                                      uint32_t* __restrict__ bits) {
  const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= n_words) return;
  uint32_t r[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) r[k] = 2 * w + k <= ref_last ? ref[2 * w + k] : 0u;
  bits[w] = cpg_pair_word(r[0], r[1], r[2]);
}
// one chromosome per thread: its last position starts no pair (the words were written by the launch in front)
__global__ __launch_bounds__(kBlock) void k_cpg_ends(const uint32_t* __restrict__ start_index, uint32_t n_chrom,
                                                      uint32_t* __restrict__ bits) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_chrom) return;
  const uint32_t end = start_index[i + 1];
  if (end) (void)atomicAnd(bits + cpg_end_word(end), cpg_end_mask(end));
}

// scan, launch 1 of 3: the pairs of kBlock neighbouring directory blocks -> sums[block]
__global__ __launch_bounds__(kBlock) void k_cpg_dir_sums(const uint32_t* __restrict__ bits, uint64_t n_dir,
                                                          unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_red[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t t = cpg_block_sum(i < n_dir ? cpg_block_count(bits, i) : 0u, s_red);
  if (threadIdx.x == 0) sums[blockIdx.x] = t;
}
// scan, launch 2 of 3 and the extraction's scan: exclusive prefix of table[0 .. n) in place (one block), table[n] = the sum
__global__ __launch_bounds__(1024) void k_cpg_scan(unsigned long long* __restrict__ table, uint32_t n,
                                                    unsigned long long* __restrict__ total_out) {
  __shared__ unsigned long long s_sum[1024];
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t b0 = threadIdx.x * per < n ? threadIdx.x * per : n, b1 = b0 + per < n ? b0 + per : n;
  unsigned long long mine = 0;
  for (uint32_t b = b0; b < b1; ++b) mine += table[b];
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (uint32_t t = 0; t < 1024; ++t) { const unsigned long long x = s_sum[t]; s_sum[t] = run; run += x; }
    table[n] = run;
    if (total_out) *total_out = run;
  }
  __syncthreads();
  unsigned long long run = s_sum[threadIdx.x];
  for (uint32_t b = b0; b < b1; ++b) { const unsigned long long x = table[b]; table[b] = run; run += x; }
}
// scan, launch 3 of 3: dir[i] = the block's scanned sum + the pairs of the block's directory blocks in front of i
__global__ __launch_bounds__(kBlock) void k_cpg_dir_apply(const uint32_t* __restrict__ bits, uint64_t n_dir,
                                                           const unsigned long long* __restrict__ sums, uint32_t* __restrict__ dir) {
  __shared__ uint32_t s_wave[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t v = i < n_dir ? cpg_block_count(bits, i) : 0u;
  uint32_t incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d);
    incl += lane >= (uint32_t)d ? o : 0u;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before = (uint32_t)sums[blockIdx.x];
  for (uint32_t w = 0; w < kBlock / 64; ++w) before += w < wave ? s_wave[w] : 0u;
  if (i < n_dir) dir[i] = before + incl - v;
}

// what cpg_rank_build allocates for idx's genome: the bitmap with its padding, the directory, the scan words
uint64_t cpg_rank_bytes(const walt_index* idx) {
  const uint64_t genome_len = idx->head.genome_len;
  const uint64_t n_dir = cpg_dir_entries(genome_len), n_sums = (n_dir + kBlock - 1) / kBlock;
  return 4 * (cpg_bit_words(genome_len) + kCpgPadWords) + 4 * std::max<uint64_t>(n_dir, 1) +
         8ull * std::max<uint64_t>(kCpgScanWords, n_sums + 2);
}
void cpg_rank_free(CpgRank& r) {
  (void)hipFree(r.bits); (void)hipFree(r.dir); (void)hipFree(r.scan);
  r = CpgRank();
}
// The pair bitmap, its directory and the scan words of one object on idx's device (the current device), built from the
// '+' reference the index holds: what walt_cpgpairs_create and walt_epialleles_create share.  false: nothing is left
// allocated; e == hipSuccess then means the device had no room for cpg_rank_bytes(idx), else e is the error.
bool cpg_rank_build(const walt_index* idx, CpgRank& r, hipError_t& e) {
  const uint64_t genome_len = idx->head.genome_len;
  const uint64_t n_bit_words = cpg_bit_words(genome_len), n_dir = cpg_dir_entries(genome_len);
  const uint64_t n_sums = (n_dir + kBlock - 1) / kBlock;
  const uint64_t bits_bytes = 4 * (n_bit_words + kCpgPadWords), dir_bytes = 4 * std::max<uint64_t>(n_dir, 1);
  const uint64_t scan_bytes = 8ull * std::max<uint64_t>(kCpgScanWords, n_sums + 2);
  r = CpgRank();
  r.n_words = n_bit_words + kCpgPadWords;
  e = hipSuccess;
  if (hipMalloc(reinterpret_cast<void**>(&r.bits), bits_bytes) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&r.dir), dir_bytes) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&r.scan), scan_bytes) != hipSuccess) {
    (void)hipGetLastError();
    cpg_rank_free(r);
    return false;
  }
  const uint32_t ref_last = (uint32_t)((genome_len + 15) / 16 + kCpgRefPadWords - 1);
  e = hipMemset(r.bits, 0, bits_bytes);
  if (e == hipSuccess) e = hipMemset(r.dir, 0, dir_bytes);
  if (e == hipSuccess && genome_len) {
    const uint64_t n_src = (genome_len + 31) / 32;  // the words that hold a position
    hipLaunchKernelGGL(k_cpg_bits, dim3(grid_for(n_src)), dim3(kBlock), 0, nullptr, idx->ref[0], ref_last, n_src, r.bits);
    hipLaunchKernelGGL(k_cpg_ends, dim3(grid_for(idx->view.n_chrom)), dim3(kBlock), 0, nullptr, idx->view.start_index,
                       idx->view.n_chrom, r.bits);
    hipLaunchKernelGGL(k_cpg_dir_sums, dim3((unsigned)n_sums), dim3(kBlock), 0, nullptr, r.bits, n_dir, r.scan);
    hipLaunchKernelGGL(k_cpg_scan, dim3(1), dim3(1024), 0, nullptr, r.scan, (uint32_t)n_sums, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(k_cpg_dir_apply, dim3((unsigned)n_sums), dim3(kBlock), 0, nullptr, r.bits, n_dir, r.scan, r.dir);
    e = hipGetLastError();
    unsigned long long total = 0;
    if (e == hipSuccess) e = hipMemcpy(&total, r.scan + n_sums, 8, hipMemcpyDeviceToHost);
    r.n_pairs = (uint32_t)total;
  }
  if (e != hipSuccess) {
    cpg_rank_free(r);
    return false;
  }
  return true;
}

// ---------------------------------------------------------------------------
// the pair kernel
// ---------------------------------------------------------------------------
struct CpgArgs {
  const uint8_t* calls;
  const uint64_t* offsets;
  uint32_t n;
  const uint8_t* records;
  uint64_t rec_stride;
  const uint8_t* skip;         // null: none
  uint64_t skip_stride;
  const uint32_t* bits;
  const uint32_t* dir;
  uint32_t* table;             // count[n_pairs][4]
  uint32_t genome_len;
  const uint32_t* start_index;
  uint32_t n_chrom;
};

// One couple: a 32-bit add whose result nobody reads (meth.hip pile_add).
__device__ __forceinline__ void cpg_add(uint32_t* __restrict__ table, uint32_t entry, uint32_t column) {
  (void)__hip_atomic_fetch_add(table + 4ull * entry + column, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_mbias's access shape (mbias.hip): eight lanes per read, one aligned 16-byte slice of its calls per lane and trip.
// Order matters, as in k_nonconv: a lane adds the couples that lie wholly inside its slice and keeps the slice's first
// and last call; the last calls are scanned across the group in lane order with the rightmost-that-exists monoid (after
// step d lane s holds the rightmost call of slices s - 2 d + 1 .. s), so that every lane learns the call in front of
// its slice -- from a lane to its left or, through `carry`, from an earlier trip -- and adds the couple that straddles
// its left boundary.  All eight lanes of a group take every trip together (nonconv_trips); the groups of a wavefront may
// diverge from each other: a shuffle of width 8 stays inside its group.
// What is read per call: the bitmap word of the call's position (and its left neighbour's at a word boundary), then the
// rank: one directory word and one 16-byte block of the bitmap.  Calls are sparse -- a CpG every 50 to 100 bases of a
// mammalian genome -- and a slice without z / Z costs its load and four word tests.
__global__ __launch_bounds__(kBlock) void k_cpg_pairs(const CpgArgs a) {
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
    const auto add = [&](uint32_t entry, uint32_t column) { cpg_add(a.table, entry, column); };
    unsigned long long carry = 0ull;
    for (int t = 0; t < trips; ++t) {
      const int i0 = -head + 16 * ((int)kCpgGroup * t + (int)sub);
      unsigned long long first = 0ull, incl = 0ull;
      if (i0 < len) {
        uint32_t w[4];
        mbias_load_slice(rb, len, i0, off - batch_lo, batch_hi - off, w);
        if (mbias_not_dot(w[0]) | mbias_not_dot(w[1]) | mbias_not_dot(w[2]) | mbias_not_dot(w[3]))
          cpg_slice(w, i0, number, add, first, incl);
      }
#pragma unroll
      for (int d = 1; d < (int)kCpgGroup; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, (unsigned)d, (int)kCpgGroup);
        incl = cpg_combine(sub >= (uint32_t)d ? o : 0ull, incl);
      }
      const unsigned long long left = __shfl_up(incl, 1u, (int)kCpgGroup);
      cpg_couple(cpg_combine(carry, sub ? left : 0ull), first, add);
      carry = cpg_combine(carry, __shfl(incl, (int)kCpgGroup - 1, (int)kCpgGroup));
    }
  }
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
  unsigned long long* scan;
  walt_cpgpair_site* out;
  unsigned long long cap;
};

__device__ __forceinline__ void cpg_block_words(const CpgExtract& a, uint64_t& lo, uint64_t& hi) {
  lo = a.w_lo + (uint64_t)blockIdx.x * a.chunk;
  hi = lo + a.chunk;
  lo = lo < a.w_hi ? lo : a.w_hi;
  hi = hi < a.w_hi ? hi : a.w_hi;
}
__device__ __forceinline__ uint4 cpg_entry(const CpgExtract& a, uint32_t j) { return reinterpret_cast<const uint4*>(a.table)[j]; }
// the pairs of bitmap word w inside the range, and the number of the first of them
__device__ __forceinline__ uint32_t cpg_word_pairs(const CpgExtract& a, uint64_t w, uint32_t& j0) {
  const uint32_t word = a.bits[w] & cpg_range_mask(w, a.pos_lo, a.pos_hi);
  if (word) j0 = cpg_rank(a.bits, a.dir, (uint32_t)(32u * w) + (uint32_t)__builtin_ctz(word));
  return word;
}
__device__ __forceinline__ uint32_t cpg_word_count(const CpgExtract& a, uint64_t w) {
  uint32_t j = 0, n = 0;
  for (uint32_t word = cpg_word_pairs(a, w, j); word; word &= word - 1u, ++j) {
    const uint4 e = cpg_entry(a, j);
    n += (e.x | e.y | e.z | e.w) != 0u;
  }
  return n;
}

// pass 1: non-zero entries per block
__global__ __launch_bounds__(kBlock) void k_cpg_count(const CpgExtract a) {
  __shared__ uint32_t s_red[kBlock / 64];
  uint64_t lo, hi;
  cpg_block_words(a, lo, hi);
  uint32_t v = 0;
  for (uint64_t w = lo + threadIdx.x; w < hi; w += kBlock) v += cpg_word_count(a, w);
  const uint32_t t = cpg_block_sum(v, s_red);
  if (threadIdx.x == 0) a.scan[blockIdx.x] = t;
}

// pass 2: the records, ascending by position: a block walks its words kBlock at a time, a thread writes the entries of
// its word behind those of the threads in front of it
__global__ __launch_bounds__(kBlock) void k_cpg_write(const CpgExtract a, uint32_t n_blocks) {
  __shared__ uint32_t s_wave[kBlock / 64];
  if (a.scan[n_blocks] > a.cap) return;  // (uniform) too many for the caller's array: nothing is written
  uint64_t lo, hi;
  cpg_block_words(a, lo, hi);
  unsigned long long at = a.scan[blockIdx.x];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t w0 = lo; w0 < hi; w0 += kBlock) {  // (uniform trip count)
    const uint64_t w = w0 + threadIdx.x;
    const uint32_t v = w < hi ? cpg_word_count(a, w) : 0u;
    uint32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(incl, d);
      incl += lane >= (uint32_t)d ? o : 0u;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kBlock / 64; ++k) {
      before += k < wave ? s_wave[k] : 0u;
      total += s_wave[k];
    }
    if (v) {
      unsigned long long slot = at + before + incl - v;
      uint32_t j = 0;
      for (uint32_t word = cpg_word_pairs(a, w, j); word; word &= word - 1u, ++j) {
        const uint4 e = cpg_entry(a, j);
        if (!(e.x | e.y | e.z | e.w)) continue;
        const uint32_t pos = (uint32_t)(32u * w) + (uint32_t)__builtin_ctz(word);
        uint2* rec = reinterpret_cast<uint2*>(a.out + slot);  // (24-byte records at an 8-byte aligned base)
        rec[0] = make_uint2(pos, cpg_next(a.bits, pos, a.n_words));
        rec[1] = make_uint2(e.x, e.y);
        rec[2] = make_uint2(e.z, e.w);
        ++slot;
      }
    }
    at += total;
    __syncthreads();  // s_wave is rewritten by the next step
  }
}

static uint64_t cpg_table_bytes(const walt_cpgpairs* ap) { return 16ull * std::max<uint32_t>(ap->n_pairs, 1u); }

int cpgpairs_launch(walt_cpgpairs* ap, const MbiasBatch& b, hipStream_t stream) {
  if (b.n == 0) return WALT_OK;
  const walt_index* idx = ap->idx;
  WALT_HIP(hipSetDevice(idx->device));
  CpgArgs a;
  a.calls = static_cast<const uint8_t*>(b.calls);
  a.offsets = static_cast<const uint64_t*>(b.offsets);
  a.n = b.n;
  a.records = static_cast<const uint8_t*>(b.records);
  a.rec_stride = b.rec_stride;
  a.skip = static_cast<const uint8_t*>(b.skip);
  a.skip_stride = b.skip_stride;
  a.bits = ap->bits;
  a.dir = ap->dir;
  a.table = ap->table;
  a.genome_len = idx->head.genome_len;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  const uint64_t want = ((uint64_t)b.n + kBlock / kCpgGroup - 1) / (kBlock / kCpgGroup);
  const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)idx->n_cu * kCpgBlocksPerCu);
  hipLaunchKernelGGL(k_cpg_pairs, dim3(grid), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

// what both batch forms refuse before they look at the batch
static int cpg_batch_check(const walt_cpgpairs* ap, const std::string& who, const MbiasBatch& b) {
  if (!ap) return fail(WALT_EINVAL, who + ": bad argument (null pair table)");
  std::string bad = record_stride_refusal(b.rec_stride);
  if (bad.empty()) bad = skip_stride_refusal(b.skip, b.skip_stride);
  return bad.empty() ? WALT_OK : fail(WALT_EINVAL, who + ": " + bad);
}

static int cpg_range_check(const walt_cpgpairs* ap, const char* who, uint32_t pos_lo, uint32_t pos_hi) {
  if (!ap) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null pair table)");
  if (pos_lo > pos_hi || pos_hi > ap->idx->head.genome_len)
    return fail(WALT_EINVAL, std::string(who) + ": range [" + std::to_string(pos_lo) + ", " + std::to_string(pos_hi) +
                                 ") is not inside the genome's " + std::to_string(ap->idx->head.genome_len) + " positions");
  return WALT_OK;
}

// The launch shape of an extraction of [pos_lo, pos_hi): the bitmap words that hold the range, cut into n_blocks chunks
// (option pile_extract_blocks, else one block per kCpgTileWords words up to eight per CU).
CpgShape cpg_extract_shape(const walt_index* idx, uint32_t pos_lo, uint32_t pos_hi) {
  CpgShape sh;
  sh.w_lo = pos_lo >> 5;
  sh.w_hi = pos_hi > pos_lo ? ((uint64_t)pos_hi + 31u) >> 5 : sh.w_lo;
  const uint64_t range = sh.w_hi - sh.w_lo;
  uint64_t want = idx->opt.pile_extract_blocks ? (uint64_t)idx->opt.pile_extract_blocks
                                               : std::min<uint64_t>((range + kCpgTileWords - 1) / kCpgTileWords, (uint64_t)idx->n_cu * 8);
  want = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(want, kCpgMaxBlocks), std::max<uint64_t>(range, 1)));
  sh.n_blocks = (uint32_t)want;
  sh.chunk = (range + want - 1) / want;
  return sh;
}

// k_cpg_scan over table[0 .. n) on `stream` (total_out: null, or a device word that gets the sum too)
void cpg_scan_launch(unsigned long long* table, uint32_t n, unsigned long long* total_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_cpg_scan, dim3(1), dim3(1024), 0, stream, table, n, total_out);
}

static CpgExtract cpg_extract_args(const walt_cpgpairs* ap, uint32_t pos_lo, uint32_t pos_hi, uint32_t& n_blocks) {
  const walt_index* idx = ap->idx;
  CpgExtract a;
  a.bits = ap->bits; a.dir = ap->dir; a.table = ap->table;
  a.n_words = ap->n_words;
  a.pos_lo = pos_lo; a.pos_hi = pos_hi;
  const CpgShape sh = cpg_extract_shape(idx, pos_lo, pos_hi);
  a.w_lo = sh.w_lo; a.w_hi = sh.w_hi; a.chunk = sh.chunk;
  n_blocks = sh.n_blocks;
  a.scan = ap->scan;
  a.out = nullptr; a.cap = 0;
  return a;
}

// count and scan on `stream`; the total lands in scan[n_blocks] and, when given, in *d_n_out
static int cpg_count_launch(const CpgExtract& a, uint32_t n_blocks, void* d_n_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_cpg_count, dim3(n_blocks), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(k_cpg_scan, dim3(1), dim3(1024), 0, stream, a.scan, n_blocks, static_cast<unsigned long long*>(d_n_out));
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_cpgpairs_create(walt_index* idx, walt_cpgpairs** out) {
  if (!idx || !out) return fail(WALT_EINVAL, "walt_cpgpairs_create: bad argument");
  *out = nullptr;
  if (!idx->ref[0])
    return fail(WALT_EINVAL, "walt_cpgpairs_create: the index holds no reference (open it with WALT_WITH_REFERENCE or call "
                             "walt_index_enable_reference)");
  WALT_HIP(hipSetDevice(idx->device));
  walt_cpgpairs* ap = new walt_cpgpairs;
  ap->idx = idx;
  CpgRank rank;
  uint64_t wanted = cpg_rank_bytes(idx);
  const auto give_up = [&](int code, const std::string& msg) {  // the index stays as it was
    (void)hipGetLastError();
    cpg_rank_free(rank);
    (void)hipFree(ap->table);
    delete ap;
    return fail(code, msg);
  };
  const auto no_memory = [&]() {
    return give_up(WALT_ENOMEM, "walt_cpgpairs_create: the pair table wants " + std::to_string(wanted) +
                                    " bytes of device memory (genome_len / 8 + genome_len / 32 + 16 per CpG pair)");
  };
  hipError_t e = hipSuccess;
  if (!cpg_rank_build(idx, rank, e)) {
    if (e == hipSuccess) return no_memory();
    return give_up(WALT_EHIP, std::string("walt_cpgpairs_create: building the pair bitmap failed: ") + hipGetErrorString(e));
  }
  ap->bits = rank.bits; ap->dir = rank.dir; ap->scan = rank.scan;
  ap->n_words = rank.n_words;
  ap->n_pairs = rank.n_pairs;
  wanted += cpg_table_bytes(ap);
  if (hipMalloc(reinterpret_cast<void**>(&ap->table), cpg_table_bytes(ap)) != hipSuccess) return no_memory();
  if (hipMemset(ap->table, 0, cpg_table_bytes(ap)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return give_up(WALT_EHIP, "walt_cpgpairs_create: the table could not be cleared");
  ap->device_bytes = wanted;
  *out = ap;
  return WALT_OK;
}

void walt_cpgpairs_destroy(walt_cpgpairs* ap) {
  if (!ap) return;
  (void)hipSetDevice(ap->idx->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(ap->bits);
  (void)hipFree(ap->dir);
  (void)hipFree(ap->scan);
  (void)hipFree(ap->table);
  delete ap;
}

int walt_cpgpairs_clear(walt_cpgpairs* ap) {
  if (!ap) return fail(WALT_EINVAL, "walt_cpgpairs_clear: bad argument (null pair table)");
  WALT_HIP(hipSetDevice(ap->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  WALT_HIP(hipMemset(ap->table, 0, cpg_table_bytes(ap)));
  WALT_HIP(hipDeviceSynchronize());
  return WALT_OK;
}

uint64_t walt_cpgpairs_device_bytes(const walt_cpgpairs* ap) { return ap ? ap->device_bytes : 0; }
uint64_t walt_cpgpairs_n_pairs(const walt_cpgpairs* ap) { return ap ? ap->n_pairs : 0; }

int walt_cpgpairs_batch_device(walt_cpgpairs* ap, const void* d_calls, const void* d_offsets, uint32_t n, const void* d_records,
                               size_t record_stride, const void* d_skip, size_t skip_stride, void* stream) {
  const std::string who = "walt_cpgpairs_batch_device";
  const MbiasBatch b = {d_calls, d_offsets, n, d_records, record_stride, d_skip, skip_stride};
  if (const int rc = cpg_batch_check(ap, who, b)) return rc;
  if (n && (!d_calls || !d_offsets || !d_records)) return fail(WALT_EINVAL, who + ": bad argument (null calls, offsets or records)");
  if (((uintptr_t)d_records & 3u) || ((uintptr_t)d_offsets & 7u))
    return fail(WALT_EINVAL, who + ": records must be 4-byte aligned, offsets 8-byte aligned");
  return cpgpairs_launch(ap, b, reinterpret_cast<hipStream_t>(stream));
}

int walt_cpgpairs_batch(walt_cpgpairs* ap, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                        size_t record_stride, const uint8_t* skip, size_t skip_stride) {
  const std::string who = "walt_cpgpairs_batch";
  // (host arrays: no alignment is asked of them; the device copies below are aligned)
  int rc = cpg_batch_check(ap, who, {calls, offsets, n, records, record_stride, skip, skip_stride});
  if (rc) return rc;
  if (n == 0) return WALT_OK;
  if (!offsets || !records || (!calls && offsets[n] > offsets[0])) return fail(WALT_EINVAL, who + ": bad argument (null calls, offsets or records)");
  uint32_t max_len = 0;
  if (const char* bad = scan_offsets(offsets, n, &max_len)) return fail(WALT_EINVAL, who + ": " + bad);
  WALT_HIP(hipSetDevice(ap->idx->device));
  const uint64_t nbytes = offsets[n] - offsets[0];
  // records and skip bytes as the kernel reads them: packed (the caller's strides stay on the host)
  const std::vector<walt_best_match> rec = pack_strided<walt_best_match>(records, record_stride, n);
  const std::vector<uint8_t> sk = pack_strided<uint8_t>(skip, skip_stride, skip ? n : 0);
  std::vector<uint64_t> rel;
  const uint64_t* off = rebase_offsets(offsets, n, rel);
  const char* what = "adjacent CpG pairs";
  DeviceTemp d_calls, d_off, d_rec, d_skip;
  if ((rc = d_calls.put(nbytes ? calls + offsets[0] : nullptr, nbytes, what)) || (rc = d_off.put(off, ((size_t)n + 1) * 8, what)) ||
      (rc = d_rec.put(rec.data(), (size_t)n * 16, what)) || (skip && (rc = d_skip.put(sk.data(), n, what))))
    return rc;
  if ((rc = cpgpairs_launch(ap, {d_calls.p, d_off.p, n, d_rec.p, 16, d_skip.p, 1}, nullptr))) return rc;
  WALT_HIP(hipStreamSynchronize(nullptr));
  return WALT_OK;
}

int walt_cpgpairs_extract_device(walt_cpgpairs* ap, uint32_t pos_lo, uint32_t pos_hi, void* d_out, uint64_t cap, void* d_n_out,
                                 void* stream) {
  int rc = cpg_range_check(ap, "walt_cpgpairs_extract_device", pos_lo, pos_hi);
  if (rc) return rc;
  if (!d_n_out || (cap && !d_out)) return fail(WALT_EINVAL, "walt_cpgpairs_extract_device: bad argument");
  if (((uintptr_t)d_out & 7u) || ((uintptr_t)d_n_out & 7u))
    return fail(WALT_EINVAL, "walt_cpgpairs_extract_device: out and n_out must be 8-byte aligned");
  WALT_HIP(hipSetDevice(ap->idx->device));
  uint32_t n_blocks;
  CpgExtract a = cpg_extract_args(ap, pos_lo, pos_hi, n_blocks);
  a.out = static_cast<walt_cpgpair_site*>(d_out);
  a.cap = cap;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if ((rc = cpg_count_launch(a, n_blocks, d_n_out, s))) return rc;
  if (cap) hipLaunchKernelGGL(k_cpg_write, dim3(n_blocks), dim3(kBlock), 0, s, a, n_blocks);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

int walt_cpgpairs_extract(walt_cpgpairs* ap, uint32_t pos_lo, uint32_t pos_hi, walt_cpgpair_site* out, uint64_t cap, uint64_t* n_out) {
  int rc = cpg_range_check(ap, "walt_cpgpairs_extract", pos_lo, pos_hi);
  if (rc) return rc;
  if (!n_out || (cap && !out)) return fail(WALT_EINVAL, "walt_cpgpairs_extract: bad argument");
  WALT_HIP(hipSetDevice(ap->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  uint32_t n_blocks;
  CpgExtract a = cpg_extract_args(ap, pos_lo, pos_hi, n_blocks);
  if ((rc = cpg_count_launch(a, n_blocks, nullptr, nullptr))) return rc;
  unsigned long long total = 0;
  WALT_HIP(hipMemcpy(&total, ap->scan + n_blocks, 8, hipMemcpyDeviceToHost));
  *n_out = total;
  if (total > cap)
    return fail(WALT_EINVAL, "walt_cpgpairs_extract: the range holds " + std::to_string(total) + " entries, the array has room for " +
                                 std::to_string(cap));
  if (!total) return WALT_OK;
  DeviceTemp d_out;
  if (hipMalloc(&d_out.p, total * sizeof(walt_cpgpair_site)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(WALT_ENOMEM, "walt_cpgpairs_extract: hipMalloc of " + std::to_string(total * sizeof(walt_cpgpair_site)) + " bytes failed");
  }
  a.out = static_cast<walt_cpgpair_site*>(d_out.p);
  a.cap = total;
  hipLaunchKernelGGL(k_cpg_write, dim3(n_blocks), dim3(kBlock), 0, nullptr, a, n_blocks);
  WALT_HIP(hipGetLastError());
  WALT_HIP(hipMemcpy(out, d_out.p, total * sizeof(walt_cpgpair_site), hipMemcpyDeviceToHost));
  return WALT_OK;
}

}  // extern "C"
