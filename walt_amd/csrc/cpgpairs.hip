// cpgpairs.hip -- adjacent CpG pairs on the device (include/walt_amd.h, "adjacent CpG pairs"): the pair bitmap and its
// rank directory built from the '+' reference (for the epiallele table too), one streaming kernel over the calls of a
// batch that folds each read's CpG calls in read order into a table keyed by pair number, and the deterministic two-pass
// extraction of the non-zero entries.  Kernel, extraction and host side are cpg_device.h's, shared with epialleles.hip,
// here with CpgPairFold (cpgpairs_core.h: the per-lane logic) and PairTab below.  The reference has no such mode; the
// contract is the header's.
#include <string.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "cpgpairs_core.h"
#include "cpg_device.h"

namespace walt {

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


void cpg_scan_launch(unsigned long long* table, uint32_t n, unsigned long long* total_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_cpg_scan, dim3(1), dim3(1024), 0, stream, table, n, total_out);
}

// ---------------------------------------------------------------------------
// the pair table: cpg_device.h's implementation with CpgPairFold (cpgpairs_core.h) and this
// ---------------------------------------------------------------------------
struct PairTab {
  using Handle = walt_cpgpairs;
  using Fold = CpgPairFold;
  using Site = walt_cpgpair_site;
  static constexpr const char* kNoun = "pair table";
  static constexpr const char* kWhat = "adjacent CpG pairs";
  using Entry = uint4;
  // entry j; kept: any counter non-zero
  static __device__ __forceinline__ bool load(const CpgExtract& a, uint32_t j, Entry& e) {
    e = reinterpret_cast<const uint4*>(a.table)[j];
    return (e.x | e.y | e.z | e.w) != 0u;
  }
  static __device__ __forceinline__ void store(const CpgExtract& a, unsigned long long slot, uint32_t pos, const Entry& e) {
    uint2* rec = reinterpret_cast<uint2*>(static_cast<Site*>(a.out) + slot);  // (24-byte records at an 8-byte aligned base)
    rec[0] = make_uint2(pos, cpg_next(a.bits, pos, a.n_words));
    rec[1] = make_uint2(e.x, e.y);
    rec[2] = make_uint2(e.z, e.w);
  }
};
// (named here so that the instances are this file's whatever calls them)
template __global__ void k_cpg_fold<CpgPairFold>(const CpgFoldArgs);
template __global__ void k_cpg_count<PairTab>(const CpgExtract);
template __global__ void k_cpg_write<PairTab>(const CpgExtract, uint32_t);

int cpgpairs_launch(walt_cpgpairs* ap, const CallsBatch& b, hipStream_t stream) { return cpg_fold_launch<CpgPairFold>(ap, b, stream); }

}  // namespace walt

using namespace walt;

extern "C" {

int walt_cpgpairs_create(walt_index* idx, walt_cpgpairs** out) { return cpg_table_create<PairTab>("walt_cpgpairs_create", idx, out); }
void walt_cpgpairs_destroy(walt_cpgpairs* ap) { cpg_table_destroy<PairTab>(ap); }
int walt_cpgpairs_clear(walt_cpgpairs* ap) { return cpg_table_clear<PairTab>("walt_cpgpairs_clear", ap); }
uint64_t walt_cpgpairs_device_bytes(const walt_cpgpairs* ap) { return ap ? ap->device_bytes : 0; }
uint64_t walt_cpgpairs_n_pairs(const walt_cpgpairs* ap) { return ap ? ap->n_pairs : 0; }

int walt_cpgpairs_batch_device(walt_cpgpairs* ap, const void* d_calls, const void* d_offsets, uint32_t n, const void* d_records,
                               size_t record_stride, const void* d_skip, size_t skip_stride, void* stream) {
  return cpg_table_batch_device<PairTab>("walt_cpgpairs_batch_device", ap, {d_calls, d_offsets, n, d_records, record_stride, d_skip, skip_stride},
                                         stream);
}

int walt_cpgpairs_batch(walt_cpgpairs* ap, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                        size_t record_stride, const uint8_t* skip, size_t skip_stride) {
  return cpg_table_batch<PairTab>("walt_cpgpairs_batch", ap, {calls, offsets, n, records, record_stride, skip, skip_stride});
}

// (no min_total here: an entry is kept when it is non-zero, and PairTab::load never looks at the 1 that is passed)
int walt_cpgpairs_extract_device(walt_cpgpairs* ap, uint32_t pos_lo, uint32_t pos_hi, void* d_out, uint64_t cap, void* d_n_out,
                                 void* stream) {
  const char* who = "walt_cpgpairs_extract_device";
  if (const int rc = range_refusal(ap, who, PairTab::kNoun, pos_lo, pos_hi)) return rc;
  return cpg_table_extract_device<PairTab>(who, ap, pos_lo, pos_hi, 1, d_out, cap, d_n_out, stream);
}

int walt_cpgpairs_extract(walt_cpgpairs* ap, uint32_t pos_lo, uint32_t pos_hi, walt_cpgpair_site* out, uint64_t cap, uint64_t* n_out) {
  const char* who = "walt_cpgpairs_extract";
  if (const int rc = range_refusal(ap, who, PairTab::kNoun, pos_lo, pos_hi)) return rc;
  return cpg_table_extract<PairTab>(who, ap, pos_lo, pos_hi, 1, out, cap, n_out);
}

}  // extern "C"
