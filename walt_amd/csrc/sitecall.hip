// sitecall.hip -- called sites (include/walt_amd.h, "called sites"): the joint histogram of (depth, meth) per context over
// a pile-up's counters, and the extraction of the sites that meet a table "smallest significant meth per depth" (count /
// scan / write, the pile-up's compaction with the table as predicate).  Integers only: the p-values, Benjamini-Hochberg
// and the table are the host's (sitecall_core.h).  The reference has no such mode; the contract is the header's.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "pileup_core.h"
#include "sitecall_core.h"

namespace walt {

constexpr uint32_t kRefPadWords = 16;  // as meth.hip: zero words behind a packed reference
static_assert(WALT_SITECALL_DEPTH == kSiteDepth && WALT_SITECALL_BINS == kSiteBins, "the header's constants are sitecall_core.h's");
static_assert(sizeof(walt_meth_site) == 16, "walt_meth_site is 16 bytes");

struct SiteArgs {
  const uint32_t* plane[2];
  const uint32_t* ref;         // the '+' reference
  uint32_t ref_last;
  const uint32_t* start_index;
  uint32_t n_chrom;
  uint32_t pos_lo, pos_hi;     // [pos_lo, pos_hi), pos_hi <= genome_len
  uint64_t chunk;              // positions per block
  unsigned long long* hist;    // [4][kSiteBins], the caller's (the histogram pass)
  unsigned long long* deep;    // [4]
  const uint32_t* min_meth;    // [4][128] (the extraction)
  unsigned long long* table;   // the pile-up's: block offsets
  walt_meth_site* sites;
  unsigned long long cap;
};

__device__ __forceinline__ void site_block_range(const SiteArgs& a, uint64_t& lo, uint64_t& hi) {
  lo = (uint64_t)a.pos_lo + (uint64_t)blockIdx.x * a.chunk;
  hi = lo + a.chunk;
  lo = lo < a.pos_hi ? lo : a.pos_hi;
  hi = hi < a.pos_hi ? hi : a.pos_hi;
}

// The chromosome a wavefront is in, kept while it stays inside it (k_pile_levels' scheme): uniform values.
struct WaveChrom {
  uint32_t lo = 1, hi = 0;  // none yet
};
// One lane's position f < hi of a wavefront whose 64 positions start at wf and end at wl: its counters, and its strand
// and context when it is a site -- covered, R[f] C or G: what the extraction (pileup.hip pile_kind, pile_site) calls one.
__device__ __forceinline__ bool site_at(const SiteArgs& a, const uint32_t* s_start, const ChromTab& tab, WaveChrom& w, uint64_t wf,
                                        uint64_t wl, uint64_t f, uint32_t& m, uint32_t& u, uint8_t& strand, uint8_t& context) {
  if (wf < w.lo || wf >= w.hi) {
    chrom_bounds(s_start, a.start_index, tab, (uint32_t)wf, w.lo, w.hi);
    w.lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.lo);
    w.hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.hi);
  }
  if (f > wl) return false;
  m = a.plane[0][f]; u = a.plane[1][f];
  if (!(m | u)) return false;
  uint32_t c_lo = w.lo, c_hi = w.hi;
  if (wl >= w.hi) chrom_bounds(s_start, a.start_index, tab, (uint32_t)f, c_lo, c_hi);  // (uniform) the step holds a chromosome start
  return pile_site(meth_ref_ext(a.ref, (long long)f - 2, a.ref_last), (uint32_t)f, c_lo, c_hi, strand, context);
}

// The histogram: one streaming pass, a step of kBlock positions at a time, a wavefront on 64 neighbouring positions.
//   d <= kSiteLdsDepth   the block's LDS table (32-bit: a block holds fewer than 2^32 positions), flushed at the end with
//                        one 64-bit atomic per non-zero bin
//   d <= kSiteDepth      a 64-bit atomic straight into the caller's histogram
//   deeper               counted per wavefront by ballot, one atomic per wavefront and context at the end
__global__ __launch_bounds__(kBlock) void k_site_hist(const SiteArgs a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  __shared__ uint32_t s_hist[4 * kSiteLdsBins];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  for (uint32_t i = threadIdx.x; i < 4 * kSiteLdsBins; i += kBlock) s_hist[i] = 0u;
  __syncthreads();
  uint64_t lo, hi;
  site_block_range(a, lo, hi);
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  unsigned long long n_deep[4] = {0, 0, 0, 0};  // (uniform)
  WaveChrom w;
  for (uint64_t f0 = lo; f0 < hi; f0 += kBlock) {
    const uint64_t wf = f0 + 64u * wave;  // (uniform) the wavefront's first position of this step
    if (wf >= hi) continue;
    const uint64_t wl = wf + 63 < hi - 1 ? wf + 63 : hi - 1;
    uint32_t m = 0, u = 0;
    uint8_t strand = 0, context = 0;
    const bool site = site_at(a, s_start, tab, w, wf, wl, wf + lane, m, u, strand, context);
    const unsigned long long d = (unsigned long long)m + u;
    const bool is_deep = site && d > kSiteDepth;
    if (site && !is_deep) {
      const uint32_t bin = sitecall_bin((uint32_t)d, m);
      if (d <= kSiteLdsDepth) atomicAdd(&s_hist[context * kSiteLdsBins + bin], 1u);
      else atomicAdd(a.hist + (size_t)context * kSiteBins + bin, 1ull);
    }
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) n_deep[c] += (uint32_t)__popcll(__ballot(is_deep && context == c));
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c)
      if (n_deep[c]) atomicAdd(a.deep + c, n_deep[c]);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < 4 * kSiteLdsBins; i += kBlock) {
    const uint32_t v = s_hist[i];
    if (v) atomicAdd(a.hist + (size_t)(i / kSiteLdsBins) * kSiteBins + i % kSiteLdsBins, (unsigned long long)v);
  }
}

// the table of the extraction in LDS; the caller's barrier follows
__device__ __forceinline__ void site_table_stage(uint32_t* s_tab, const uint32_t* __restrict__ min_meth) {
  for (uint32_t i = threadIdx.x; i < kSiteTable; i += kBlock) s_tab[i] = min_meth[i];
}

// pass 1: records per block
__global__ __launch_bounds__(kBlock) void k_site_count(const SiteArgs a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  __shared__ uint32_t s_tab[kSiteTable];
  __shared__ unsigned long long s_red[kBlock / 64];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  site_table_stage(s_tab, a.min_meth);
  __syncthreads();
  uint64_t lo, hi;
  site_block_range(a, lo, hi);
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  unsigned long long n = 0;  // (uniform)
  WaveChrom w;
  for (uint64_t f0 = lo; f0 < hi; f0 += kBlock) {
    const uint64_t wf = f0 + 64u * wave;
    if (wf >= hi) continue;
    const uint64_t wl = wf + 63 < hi - 1 ? wf + 63 : hi - 1;
    uint32_t m = 0, u = 0;
    uint8_t strand = 0, context = 0;
    const bool site = site_at(a, s_start, tab, w, wf, wl, wf + lane, m, u, strand, context);
    n += (uint32_t)__popcll(__ballot(site && sitecall_verdict(s_tab, context, m, u) != kSiteNone));
  }
  if (lane == 0) s_red[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (uint32_t k = 0; k < kBlock / 64; ++k) t += s_red[k];
    a.table[blockIdx.x] = t;
  }
}

// pass 2 (behind the scan): the records, ascending by position, ranked as k_pile_write ranks the sites
__global__ __launch_bounds__(kBlock) void k_site_write(const SiteArgs a, uint32_t n_blocks) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  __shared__ uint32_t s_tab[kSiteTable];
  __shared__ uint32_t s_wave[kBlock / 64];
  if (a.table[n_blocks] > a.cap) return;  // (uniform) too many for the caller's array: nothing is written
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  site_table_stage(s_tab, a.min_meth);
  __syncthreads();
  uint64_t lo, hi;
  site_block_range(a, lo, hi);
  unsigned long long at = a.table[blockIdx.x];
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  WaveChrom w;
  for (uint64_t f0 = lo; f0 < hi; f0 += kBlock) {  // (uniform trip count)
    const uint64_t wf = f0 + 64u * wave, f = wf + lane;
    uint32_t m = 0, u = 0, verdict = kSiteNone;
    uint8_t strand = 0, context = 0;
    if (wf < hi) {  // (uniform)
      const uint64_t wl = wf + 63 < hi - 1 ? wf + 63 : hi - 1;
      if (site_at(a, s_start, tab, w, wf, wl, f, m, u, strand, context)) verdict = sitecall_verdict(s_tab, context, m, u);
    }
    const unsigned long long vote = __ballot(verdict != kSiteNone);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kBlock / 64; ++k) {
      before += k < wave ? s_wave[k] : 0u;
      total += s_wave[k];
    }
    if (verdict != kSiteNone) {
      const unsigned long long slot = at + before + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
      // one 16-byte store: pos, meth, unmeth, strand | context << 8 | reserved << 16 (1: a deep site)
      *reinterpret_cast<uint4*>(a.sites + slot) =
          make_uint4((uint32_t)f, m, u, (uint32_t)strand | ((uint32_t)context << 8) | (verdict == kSiteDeep ? 1u << 16 : 0u));
    }
    at += total;
    __syncthreads();  // s_wave is rewritten by the next step
  }
}

static SiteArgs site_args(const walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, uint32_t& n_blocks) {
  const walt_index* idx = p->idx;
  SiteArgs a;
  a.plane[0] = p->plane[0]; a.plane[1] = p->plane[1];
  a.ref = idx->ref[0];
  a.ref_last = (idx->head.genome_len + 15) / 16 + kRefPadWords - 1;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  a.pos_lo = pos_lo; a.pos_hi = pos_hi;
  n_blocks = extract_blocks(idx, (uint64_t)pos_hi - pos_lo, kPileTile, kPileMaxBlocks, &a.chunk);
  a.hist = nullptr; a.deep = nullptr; a.min_meth = nullptr;
  a.table = p->table;
  a.sites = nullptr; a.cap = 0;
  return a;
}

// the caller's arrays zeroed and the pass, on `stream`
static int site_hist_launch(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, void* d_hist, void* d_deep, hipStream_t stream) {
  uint32_t n_blocks;
  SiteArgs a = site_args(p, pos_lo, pos_hi, n_blocks);
  a.hist = static_cast<unsigned long long*>(d_hist);
  a.deep = static_cast<unsigned long long*>(d_deep);
  WALT_HIP(hipMemsetAsync(d_hist, 0, 4ull * kSiteBins * sizeof(unsigned long long), stream));
  WALT_HIP(hipMemsetAsync(d_deep, 0, 4 * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_site_hist, dim3(n_blocks), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_pileup_depth_hist_device(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, void* d_hist, void* d_deep, void* stream) {
  const char* who = "walt_pileup_depth_hist_device";
  const int rc = range_refusal(p, who, "pile-up", pos_lo, pos_hi);
  if (rc) return rc;
  if (!d_hist || !d_deep) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null hist or deep)");
  if (((uintptr_t)d_hist & 7u) || ((uintptr_t)d_deep & 7u)) return fail(WALT_EINVAL, std::string(who) + ": hist and deep must be 8-byte aligned");
  WALT_HIP(hipSetDevice(p->idx->device));
  return site_hist_launch(p, pos_lo, pos_hi, d_hist, d_deep, reinterpret_cast<hipStream_t>(stream));
}

int walt_pileup_depth_hist(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, uint64_t* hist, uint64_t* deep) {
  const char* who = "walt_pileup_depth_hist";
  int rc = range_refusal(p, who, "pile-up", pos_lo, pos_hi);
  if (rc) return rc;
  if (!hist || !deep) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null hist or deep)");
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the histogram is copied as it lies");
  const size_t words = 4 * (size_t)kSiteBins;
  DeviceTemp d;  // the histogram, the deep counts behind it
  if ((rc = d.get((words + 4) * 8, "depth histogram"))) return rc;
  unsigned long long* d_hist = static_cast<unsigned long long*>(d.p);
  if ((rc = site_hist_launch(p, pos_lo, pos_hi, d_hist, d_hist + words, nullptr))) return rc;
  WALT_HIP(hipMemcpy(hist, d_hist, words * 8, hipMemcpyDeviceToHost));
  WALT_HIP(hipMemcpy(deep, d_hist + words, 4 * 8, hipMemcpyDeviceToHost));
  return WALT_OK;
}

int walt_pileup_call_sites_device(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, const void* d_min_meth, void* d_out, uint64_t cap,
                                  void* d_n_out, void* stream) {
  const char* who = "walt_pileup_call_sites_device";
  int rc = range_refusal(p, who, "pile-up", pos_lo, pos_hi);
  if (rc) return rc;
  if (!d_min_meth || !d_n_out || (cap && !d_out)) return fail(WALT_EINVAL, std::string(who) + ": bad argument");
  if (((uintptr_t)d_min_meth & 3u) || ((uintptr_t)d_out & 15u) || ((uintptr_t)d_n_out & 7u))
    return fail(WALT_EINVAL, std::string(who) + ": min_meth must be 4-byte aligned, out 16-byte aligned, n_out 8-byte aligned");
  WALT_HIP(hipSetDevice(p->idx->device));
  uint32_t n_blocks;
  SiteArgs a = site_args(p, pos_lo, pos_hi, n_blocks);
  a.min_meth = static_cast<const uint32_t*>(d_min_meth);
  a.sites = static_cast<walt_meth_site*>(d_out);
  a.cap = cap;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_site_count, dim3(n_blocks), dim3(kBlock), 0, s, a);
  if ((rc = pile_scan_launch(a.table, n_blocks, static_cast<unsigned long long*>(d_n_out), nullptr, s))) return rc;
  if (cap) hipLaunchKernelGGL(k_site_write, dim3(n_blocks), dim3(kBlock), 0, s, a, n_blocks);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

int walt_pileup_call_sites(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, const uint32_t* min_meth, walt_meth_site* out, uint64_t cap,
                           uint64_t* n_out) {
  const char* who = "walt_pileup_call_sites";
  int rc = range_refusal(p, who, "pile-up", pos_lo, pos_hi);
  if (rc) return rc;
  if (!min_meth || !n_out || (cap && !out)) return fail(WALT_EINVAL, std::string(who) + ": bad argument");
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  DeviceTemp d_tab;
  if ((rc = d_tab.put(min_meth, kSiteTable * sizeof(uint32_t), "called sites"))) return rc;
  uint32_t n_blocks;
  SiteArgs a = site_args(p, pos_lo, pos_hi, n_blocks);
  a.min_meth = static_cast<const uint32_t*>(d_tab.p);
  hipLaunchKernelGGL(k_site_count, dim3(n_blocks), dim3(kBlock), 0, nullptr, a);
  if ((rc = pile_scan_launch(a.table, n_blocks, nullptr, nullptr, nullptr))) return rc;
  unsigned long long total = 0;
  WALT_HIP(hipMemcpy(&total, a.table + kPileTotals, sizeof total, hipMemcpyDeviceToHost));
  *n_out = total;
  if (total > cap)
    return fail(WALT_EINVAL, std::string(who) + ": the range holds " + std::to_string(total) + " called sites, the array has room for " +
                                 std::to_string(cap));
  if (!total) return WALT_OK;
  DeviceTemp d_out;
  if ((rc = d_out.get(total * sizeof(walt_meth_site), "called sites"))) return rc;
  a.sites = static_cast<walt_meth_site*>(d_out.p);
  a.cap = total;
  hipLaunchKernelGGL(k_site_write, dim3(n_blocks), dim3(kBlock), 0, nullptr, a, n_blocks);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(out, d_out.p, total * sizeof(walt_meth_site), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(WALT_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  return WALT_OK;
}

}  // extern "C"
