// variants.hip -- opposite-strand evidence (include/walt_amd.h, "opposite-strand evidence"): the kernel that counts, per
// forward position, the reads of the other strand that show the reference base and those that show another one, into a
// second walt_pileup; and the two passes over those counters at the end of a read file: the flagged positions as records
// (count / scan / write, the pile-up's compaction with another predicate) and the masking of a pile-up's counters there.
// The reference has no such mode; the contract is the header's.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "pile_device.h"
#include "variants_core.h"

namespace walt {

constexpr uint32_t kRefPadWords = 16;          // as meth.hip: zero words behind a packed reference
constexpr uint32_t kVarTotals = 5;             // judged, flagged, masked sites, methylated and unmethylated calls removed
static_assert(sizeof(walt_variant_site) == 24, "walt_variant_site is 24 bytes");
static_assert(kVarTotals <= 8, "the totals live in the last eight words of the table");

// ---------------------------------------------------------------------------
// the evidence kernel
// ---------------------------------------------------------------------------
struct EvArgs {
  const uint32_t* ref[2];      // '+' and '-' orientation
  uint32_t ref_last;
  uint32_t genome_len;
  const uint32_t* start_index;
  uint32_t n_chrom;
  const uint8_t* bases;
  const uint64_t* offsets;
  uint32_t n;
  const uint8_t* records;
  uint64_t rec_stride;
  const uint8_t* conv;         // null: `conversion` for every read
  uint64_t conv_stride;
  uint32_t conversion;
  const uint32_t* call_len;    // null: the whole read
  const uint8_t* skip;         // null: none
  uint64_t skip_stride;
  uint32_t* plane[2];          // match, other
  const uint8_t* quals;        // one byte per base (include/walt_amd.h, "minimum base quality"); read by the kQual instances alone
  uint32_t min_qual;
};

// Eight lanes per read, one 16-base slice per lane and trip, cut at the 16-byte boundaries of the bases array (a whole
// slice is one aligned 16-byte load); the first and last slice of a read are partial.  Nothing is written but the
// counters.  kRows: pile_rows instead of pile_slice (option pile_rows); every lane of a group then takes every trip.
// kQual: the batch comes with base qualities; a base below a.min_qual adds to neither counter (ev_read_slice_q).
// Instances of their own, as in meth.hip: a call without qualities launches the kernel it always launched.
template <bool kRows, bool kQual = false>
__device__ __forceinline__ void evidence_body(const EvArgs& a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  __syncthreads();
  const uint32_t sub = threadIdx.x & (kMethGroup - 1);
  const uint64_t groups = (uint64_t)gridDim.x * (kBlock / kMethGroup);
  const uint64_t batch_bytes = a.offsets[a.n];
  for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / kMethGroup) + threadIdx.x / kMethGroup; r < a.n; r += groups) {
    const uint64_t off = a.offsets[r], end = a.offsets[r + 1];
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.records + r * a.rec_stride);
    const uint32_t pos = rec[0], times = rec[1], strand = rec[2] & 0xFFu;
    const uint32_t cv = a.conv ? a.conv[r * a.conv_stride] : a.conversion;
    const uint32_t skip = a.skip ? a.skip[r * a.skip_stride] : 0u;
    // (the same for the eight lanes of the group)
    if (!ev_record_counts(times, skip, pos, a.genome_len, cv, end > off ? end - off : 0ull)) continue;
    const uint32_t len = (uint32_t)(end - off);
    uint32_t limit = a.call_len ? a.call_len[r] : len;
    limit = limit < len ? limit : len;
    if (!limit) continue;
    uint32_t c_lo, c_hi;
    chrom_bounds(s_start, a.start_index, tab, pos, c_lo, c_hi);
    const uint32_t ga = cv == 'A' ? 1u : 0u;
    const bool minus = strand == '-';
    const uint32_t* __restrict__ ref = a.ref[minus ? 1 : 0];
    const uint8_t* rb = a.bases + off;
    const uint8_t* qb = kQual ? a.quals + off : nullptr;
    const int head = (int)((uintptr_t)rb & 15u);
    if (kRows) {
      for (int base = -head; base < (int)limit; base += 16 * (int)kMethGroup) {
        const int i0 = base + 16 * (int)sub;
        EvSlice s = {0u, 0u};
        if (i0 < (int)limit)
          s = ev_read_slice_q<kQual>(rb, (int)len, limit, pos, c_lo, c_hi, ga, ref, a.ref_last, i0, off, batch_bytes - off, qb, a.min_qual);
        pile_rows(s.match, s.other, (long long)pos + base, sub, minus, c_lo, c_hi, a.plane);
      }
    } else {
      for (int i0 = -head + 16 * (int)sub; i0 < (int)limit; i0 += 16 * (int)kMethGroup) {
        const EvSlice s = ev_read_slice_q<kQual>(rb, (int)len, limit, pos, c_lo, c_hi, ga, ref, a.ref_last, i0, off, batch_bytes - off, qb, a.min_qual);
        pile_slice(s.match, s.other, (long long)pos + i0, minus, c_lo, c_hi,
                   [&](uint32_t f, bool m) { pile_add(a.plane[m ? 0 : 1], f); });
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_evidence(const EvArgs a) { evidence_body<false>(a); }
__global__ __launch_bounds__(kBlock) void k_evidence_rows(const EvArgs a) { evidence_body<true>(a); }
__global__ __launch_bounds__(kBlock) void k_evidence_qual(const EvArgs a) { evidence_body<false, true>(a); }
__global__ __launch_bounds__(kBlock) void k_evidence_rows_qual(const EvArgs a) { evidence_body<true, true>(a); }

int evidence_launch(walt_pileup* ev, const EvBatch& b, hipStream_t stream) {
  if (b.n == 0) return WALT_OK;
  const walt_index* idx = ev->idx;
  WALT_HIP(hipSetDevice(idx->device));
  EvArgs a;
  a.ref[0] = idx->ref[0]; a.ref[1] = idx->ref[1];
  a.ref_last = (idx->head.genome_len + 15) / 16 + kRefPadWords - 1;
  a.genome_len = idx->head.genome_len;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  a.bases = static_cast<const uint8_t*>(b.bases);
  a.offsets = static_cast<const uint64_t*>(b.offsets);
  a.n = b.n;
  a.records = static_cast<const uint8_t*>(b.records);
  a.rec_stride = b.rec_stride;
  a.conv = static_cast<const uint8_t*>(b.conv);
  a.conv_stride = b.conv_stride;
  a.conversion = (uint32_t)b.conversion;
  a.call_len = static_cast<const uint32_t*>(b.call_len);
  a.skip = static_cast<const uint8_t*>(b.skip);
  a.skip_stride = b.skip_stride;
  a.plane[0] = ev->plane[0]; a.plane[1] = ev->plane[1];
  a.quals = static_cast<const uint8_t*>(b.quals);
  a.min_qual = b.min_qual;
  const uint64_t want = ((uint64_t)b.n + kBlock / kMethGroup - 1) / (kBlock / kMethGroup);
  const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)idx->n_cu * 8);
  const auto kernel = a.quals ? (idx->opt.pile_rows ? k_evidence_rows_qual : k_evidence_qual)
                              : (idx->opt.pile_rows ? k_evidence_rows : k_evidence);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

// ---------------------------------------------------------------------------
// the passes over the counters
// ---------------------------------------------------------------------------
struct VarArgs {
  uint32_t* pile[2];           // the pile-up's counters: methylated, unmethylated
  const uint32_t* ev[2];       // the evidence: match, other
  const uint32_t* ref;         // the '+' reference
  uint32_t ref_last;
  const uint32_t* start_index;
  uint32_t n_chrom;
  uint32_t pos_lo, pos_hi;     // [pos_lo, pos_hi), pos_hi <= genome_len
  uint64_t chunk;              // positions per block
  uint32_t min_depth, max_percent;
  unsigned long long* table;   // the evidence object's
  walt_variant_site* out;
  unsigned long long cap;
};

__device__ __forceinline__ void var_block_range(const VarArgs& a, uint64_t& lo, uint64_t& hi) {
  lo = (uint64_t)a.pos_lo + (uint64_t)blockIdx.x * a.chunk;
  hi = lo + a.chunk;
  lo = lo < a.pos_hi ? lo : a.pos_hi;
  hi = hi < a.pos_hi ? hi : a.pos_hi;
}
// R[f] is C or G: the evidence at an A or T of R is never read
__device__ __forceinline__ bool var_is_site(const VarArgs& a, uint32_t f) {
  const uint32_t code = (a.ref[f >> 4] >> (2u * (f & 15u))) & 3u;
  return code == 1u || code == 2u;
}

// pass 1: flagged positions per block
__global__ __launch_bounds__(kBlock) void k_var_count(const VarArgs a) {
  __shared__ uint32_t s_red[kBlock / 64];
  uint64_t lo, hi;
  var_block_range(a, lo, hi);
  uint32_t v = 0;
  for (uint64_t f = lo + threadIdx.x; f < hi; f += kBlock)
    v += var_is_site(a, (uint32_t)f) && ev_flagged(a.ev[0][f], a.ev[1][f], a.min_depth, a.max_percent);
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_red[w];
    a.table[blockIdx.x] = t;
  }
}

// pass 2 (behind the scan): the records, ascending by position, ranked as k_pile_write ranks the sites
__global__ __launch_bounds__(kBlock) void k_var_write(const VarArgs a, uint32_t n_blocks) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  __shared__ uint32_t s_wave[kBlock / 64];
  if (a.table[n_blocks] > a.cap) return;  // (uniform) too many for the caller's array: nothing is written
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  __syncthreads();
  uint64_t lo, hi;
  var_block_range(a, lo, hi);
  unsigned long long at = a.table[blockIdx.x];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t f0 = lo; f0 < hi; f0 += kBlock) {  // (uniform trip count)
    const uint64_t f = f0 + threadIdx.x;
    uint32_t m = 0, o = 0;
    bool flag = false;
    if (f < hi) {
      m = a.ev[0][f]; o = a.ev[1][f];
      flag = var_is_site(a, (uint32_t)f) && ev_flagged(m, o, a.min_depth, a.max_percent);
    }
    const unsigned long long vote = __ballot(flag);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
      before += w < wave ? s_wave[w] : 0u;
      total += s_wave[w];
    }
    if (flag) {
      const unsigned long long slot = at + before + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
      uint32_t c_lo, c_hi;
      chrom_bounds(s_start, a.start_index, tab, (uint32_t)f, c_lo, c_hi);
      uint8_t strand = 0, context = 0;
      (void)pile_site(meth_ref_ext(a.ref, (long long)f - 2, a.ref_last), (uint32_t)f, c_lo, c_hi, strand, context);
      // three 8-byte stores: pos, meth | unmeth, strand | context << 8 | reserved 0 | match | other
      uint2* rec = reinterpret_cast<uint2*>(a.out + slot);
      rec[0] = make_uint2((uint32_t)f, a.pile[0][f]);
      rec[1] = make_uint2(a.pile[1][f], (uint32_t)strand | ((uint32_t)context << 8));
      rec[2] = make_uint2(m, o);
    }
    at += total;
    __syncthreads();  // s_wave is rewritten by the next step
  }
}

// The masking pass: R and the two evidence planes streamed, the pile-up's planes touched at flagged positions only.
// Sums per lane, then per wavefront, then per block, then one atomic per block and total.
__global__ __launch_bounds__(kBlock) void k_var_mask(const VarArgs a) {
  __shared__ unsigned long long s_red[kBlock / 64][kVarTotals];
  uint64_t lo, hi;
  var_block_range(a, lo, hi);
  unsigned long long v[kVarTotals] = {0, 0, 0, 0, 0};
  for (uint64_t f = lo + threadIdx.x; f < hi; f += kBlock) {
    const uint32_t m = a.ev[0][f], o = a.ev[1][f];
    if (!var_is_site(a, (uint32_t)f) || !ev_judged(m, o, a.min_depth)) continue;
    v[0] += 1;
    if (!ev_flagged(m, o, a.min_depth, a.max_percent)) continue;
    v[1] += 1;
    const uint32_t pm = a.pile[0][f], pu = a.pile[1][f];
    if (!(pm | pu)) continue;
    v[2] += 1; v[3] += pm; v[4] += pu;
    a.pile[0][f] = 0u; a.pile[1][f] = 0u;
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t i = 0; i < kVarTotals; ++i) {
    for (int d = 32; d > 0; d >>= 1) v[i] += __shfl_down(v[i], d);
    if (lane == 0) s_red[wave][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < kVarTotals) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_red[w][threadIdx.x];
    if (t) atomicAdd(&a.table[kPileTotals + threadIdx.x], t);
  }
}

// what both passes refuse, host and device form alike
static int var_check(const walt_pileup* p, const walt_pileup* ev, const char* who, uint32_t pos_lo, uint32_t pos_hi,
                     uint32_t min_depth, uint32_t max_percent) {
  if (const int rc = range_refusal(p, who, "pile-up", pos_lo, pos_hi)) return rc;
  if (!ev) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null evidence)");
  if (ev == p) return fail(WALT_EINVAL, std::string(who) + ": the evidence and the pile-up are one object");
  if (ev->idx != p->idx) return fail(WALT_EINVAL, std::string(who) + ": the evidence belongs to another index");
  if (min_depth == 0) return fail(WALT_EINVAL, std::string(who) + ": min_depth is 1 to 4294967295");
  if (max_percent > 99) return fail(WALT_EINVAL, std::string(who) + ": max_percent " + std::to_string(max_percent) + " is not 0 to 99");
  return WALT_OK;
}

static VarArgs var_args(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth, uint32_t max_percent,
                        uint32_t& n_blocks) {
  const walt_index* idx = p->idx;
  VarArgs a;
  a.pile[0] = p->plane[0]; a.pile[1] = p->plane[1];
  a.ev[0] = ev->plane[0]; a.ev[1] = ev->plane[1];
  a.ref = idx->ref[0];
  a.ref_last = (idx->head.genome_len + 15) / 16 + kRefPadWords - 1;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  a.pos_lo = pos_lo; a.pos_hi = pos_hi;
  n_blocks = extract_blocks(idx, (uint64_t)pos_hi - pos_lo, kPileTile, kPileMaxBlocks, &a.chunk);
  a.min_depth = min_depth; a.max_percent = max_percent;
  a.table = ev->table;
  a.out = nullptr; a.cap = 0;
  return a;
}

static int var_mask_launch(const VarArgs& a, uint32_t n_blocks, void* d_out, hipStream_t stream) {
  WALT_HIP(hipMemsetAsync(a.table + kPileTotals, 0, kVarTotals * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_var_mask, dim3(n_blocks), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  if (d_out) WALT_HIP(hipMemcpyAsync(d_out, a.table + kPileTotals, kVarTotals * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_pileup_variants_device(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth,
                                uint32_t max_percent, void* d_out, uint64_t cap, void* d_n_out, void* stream) {
  const char* who = "walt_pileup_variants_device";
  int rc = var_check(p, ev, who, pos_lo, pos_hi, min_depth, max_percent);
  if (rc) return rc;
  if (!d_n_out || (cap && !d_out)) return fail(WALT_EINVAL, std::string(who) + ": bad argument");
  if (((uintptr_t)d_out & 7u) || ((uintptr_t)d_n_out & 7u)) return fail(WALT_EINVAL, std::string(who) + ": out and n_out must be 8-byte aligned");
  WALT_HIP(hipSetDevice(p->idx->device));
  uint32_t n_blocks;
  VarArgs a = var_args(p, ev, pos_lo, pos_hi, min_depth, max_percent, n_blocks);
  a.out = static_cast<walt_variant_site*>(d_out);
  a.cap = cap;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_var_count, dim3(n_blocks), dim3(kBlock), 0, s, a);
  if ((rc = pile_scan_launch(a.table, n_blocks, static_cast<unsigned long long*>(d_n_out), nullptr, s))) return rc;
  if (cap) hipLaunchKernelGGL(k_var_write, dim3(n_blocks), dim3(kBlock), 0, s, a, n_blocks);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

int walt_pileup_variants(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth,
                         uint32_t max_percent, walt_variant_site* out, uint64_t cap, uint64_t* n_out) {
  const char* who = "walt_pileup_variants";
  int rc = var_check(p, ev, who, pos_lo, pos_hi, min_depth, max_percent);
  if (rc) return rc;
  if (!n_out || (cap && !out)) return fail(WALT_EINVAL, std::string(who) + ": bad argument");
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  uint32_t n_blocks;
  VarArgs a = var_args(p, ev, pos_lo, pos_hi, min_depth, max_percent, n_blocks);
  hipLaunchKernelGGL(k_var_count, dim3(n_blocks), dim3(kBlock), 0, nullptr, a);
  if ((rc = pile_scan_launch(a.table, n_blocks, nullptr, nullptr, nullptr))) return rc;
  unsigned long long total = 0;
  WALT_HIP(hipMemcpy(&total, a.table + kPileTotals, sizeof total, hipMemcpyDeviceToHost));
  *n_out = total;
  if (total > cap)
    return fail(WALT_EINVAL, std::string(who) + ": the range holds " + std::to_string(total) + " flagged positions, the array has room for " +
                                 std::to_string(cap));
  if (!total) return WALT_OK;
  DeviceTemp d_out;
  if ((rc = d_out.get(total * sizeof(walt_variant_site), "variants"))) return rc;
  a.out = static_cast<walt_variant_site*>(d_out.p);
  a.cap = total;
  hipLaunchKernelGGL(k_var_write, dim3(n_blocks), dim3(kBlock), 0, nullptr, a, n_blocks);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(out, d_out.p, total * sizeof(walt_variant_site), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(WALT_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  return WALT_OK;
}

int walt_pileup_mask_variants_device(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth,
                                     uint32_t max_percent, void* d_out, void* stream) {
  const char* who = "walt_pileup_mask_variants_device";
  const int rc = var_check(p, ev, who, pos_lo, pos_hi, min_depth, max_percent);
  if (rc) return rc;
  if (!d_out) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null out)");
  if ((uintptr_t)d_out & 7u) return fail(WALT_EINVAL, std::string(who) + ": out must be 8-byte aligned");
  WALT_HIP(hipSetDevice(p->idx->device));
  uint32_t n_blocks;
  const VarArgs a = var_args(p, ev, pos_lo, pos_hi, min_depth, max_percent, n_blocks);
  return var_mask_launch(a, n_blocks, d_out, reinterpret_cast<hipStream_t>(stream));
}

int walt_pileup_mask_variants(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth,
                              uint32_t max_percent, uint64_t* out) {
  const char* who = "walt_pileup_mask_variants";
  int rc = var_check(p, ev, who, pos_lo, pos_hi, min_depth, max_percent);
  if (rc) return rc;
  if (!out) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null out)");
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  uint32_t n_blocks;
  const VarArgs a = var_args(p, ev, pos_lo, pos_hi, min_depth, max_percent, n_blocks);
  if ((rc = var_mask_launch(a, n_blocks, nullptr, nullptr))) return rc;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the totals are copied as they lie");
  WALT_HIP(hipMemcpy(out, a.table + kPileTotals, kVarTotals * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return WALT_OK;
}

}  // extern "C"
