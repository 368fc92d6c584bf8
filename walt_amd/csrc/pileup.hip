// pileup.hip -- per-cytosine methylation pile-up (include/walt_amd.h, "methylation pile-up"): the counters, and the
// deterministic two-pass extraction of the covered positions as walt_meth_site records.  The adds are a variant of the
// calling kernel (meth.hip k_meth_pile).  The reference has no such mode; the contract is the header's.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "levels_core.h"
#include "pileup_core.h"
#include "regions_core.h"

namespace walt {

constexpr uint32_t kRefPadWords = 16;          // as meth.hip: zero words behind a packed reference
constexpr uint32_t kPileLevels = kPileTotals - 128;  // a summary's accumulator: walt_levels, kLevelWords words
constexpr uint32_t kLevelCols = 32;            // LDS columns of a histogram bin (k_pile_levels)
constexpr uint32_t kPileAddWindow = 1u << 22;  // positions walt_pileup_add stages on the device at a time
static_assert(kPileMaxBlocks + 1 <= kPileLevels && kPileLevels + kLevelWords <= kPileTotals,
              "the table holds the offsets in front of the summary's accumulator, and that in front of the totals");
static_assert(sizeof(walt_level_row) == 8 * kLevelRowWords && sizeof(walt_levels) == 8 * kLevelWords, "walt_levels is 656 bytes");
static_assert(kLevelWords <= kBlock && kLevelRows * kLevelBins <= kBlock, "one thread per word of a block's summary");
static_assert(sizeof(walt_meth_site) == 16, "walt_meth_site is 16 bytes");
static_assert(sizeof(walt_region) == 8 && sizeof(walt_region_row) == 32 && sizeof(walt_region_levels) == 32 * kLevelRows,
              "walt_region is 8 bytes, walt_region_levels 160");
static_assert(kRegionUnit == kPileTile, "a unit of a region is a tile of the extraction");
static_assert((WALT_REGIONS_MAX + kBlock - 1) / kBlock <= kPileMaxBlocks, "the table holds the sums of a regions call");

struct PileArgs {
  const uint32_t* plane[2];
  const uint32_t* ref;         // the '+' reference
  uint32_t ref_last;
  const uint32_t* start_index;
  uint32_t n_chrom;
  uint32_t pos_lo, pos_hi;     // [pos_lo, pos_hi), pos_hi <= genome_len
  uint64_t chunk;              // positions per block
  unsigned long long* table;
  walt_meth_site* sites;
  unsigned long long cap;
  unsigned long long* n_sites_out;  // device pointers of the device form (null: the host reads the table)
  unsigned long long* offref_out;
};

// block b's positions [lo, hi)
__device__ __forceinline__ void pile_block_range(const PileArgs& a, uint64_t& lo, uint64_t& hi) {
  lo = (uint64_t)a.pos_lo + (uint64_t)blockIdx.x * a.chunk;
  hi = lo + a.chunk;
  lo = lo < a.pos_hi ? lo : a.pos_hi;
  hi = hi < a.pos_hi ? hi : a.pos_hi;
}
// 0: uncovered, 1: a site, 2: covered but R[f] is A or T (only the base itself is looked at)
__device__ __forceinline__ uint32_t pile_kind(const PileArgs& a, uint32_t f, uint32_t m, uint32_t u) {
  if (!(m | u)) return 0u;
  const uint32_t code = (a.ref[f >> 4] >> (2u * (f & 15u))) & 3u;
  return code == 1u || code == 2u ? 1u : 2u;
}

// pass 1: sites per block; the off-reference calls summed per block, then one atomic per block and total
__global__ __launch_bounds__(kBlock) void k_pile_count(const PileArgs a) {
  __shared__ unsigned long long s_red[kBlock / 64][3];
  uint64_t lo, hi;
  pile_block_range(a, lo, hi);
  unsigned long long v[3] = {0, 0, 0};
  for (uint64_t f = lo + threadIdx.x; f < hi; f += kBlock) {
    const uint32_t m = a.plane[0][f], u = a.plane[1][f];
    const uint32_t kind = pile_kind(a, (uint32_t)f, m, u);
    v[0] += kind == 1u;
    v[1] += kind == 2u ? m : 0u;
    v[2] += kind == 2u ? u : 0u;
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t i = 0; i < 3; ++i) {
    for (int d = 32; d > 0; d >>= 1) v[i] += __shfl_down(v[i], d);
    if (lane == 0) s_red[wave][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_red[w][threadIdx.x];
    if (threadIdx.x == 0) a.table[blockIdx.x] = t;
    else if (t) atomicAdd(&a.table[kPileTotals + threadIdx.x], t);
  }
}

// exclusive scan of the block counts in place (one block); table[n_blocks] and the totals' first word = the sum
__global__ __launch_bounds__(1024) void k_pile_scan(const PileArgs a, uint32_t n_blocks) {
  __shared__ unsigned long long s_sum[1024];
  const uint32_t per = (n_blocks + 1023u) / 1024u;
  const uint32_t b0 = threadIdx.x * per, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
  unsigned long long mine = 0;
  for (uint32_t b = b0; b < b1; ++b) mine += a.table[b];
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (uint32_t t = 0; t < 1024; ++t) { const unsigned long long x = s_sum[t]; s_sum[t] = run; run += x; }
    a.table[n_blocks] = run;
    a.table[kPileTotals] = run;
    if (a.n_sites_out) *a.n_sites_out = run;
    if (a.offref_out) { a.offref_out[0] = a.table[kPileTotals + 1]; a.offref_out[1] = a.table[kPileTotals + 2]; }
  }
  __syncthreads();
  unsigned long long run = s_sum[threadIdx.x];
  for (uint32_t b = b0; b < b1; ++b) { const unsigned long long x = a.table[b]; a.table[b] = run; run += x; }
}

// pass 2: the records, ascending by position: a block walks its positions kBlock at a time and ranks the sites of a
// step by ballot within the wavefront and a prefix over the block's wavefronts
__global__ __launch_bounds__(kBlock) void k_pile_write(const PileArgs a, uint32_t n_blocks) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  __shared__ uint32_t s_wave[kBlock / 64];
  if (a.table[n_blocks] > a.cap) return;  // (uniform) too many for the caller's array: nothing is written
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  __syncthreads();
  uint64_t lo, hi;
  pile_block_range(a, lo, hi);
  unsigned long long at = a.table[blockIdx.x];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t f0 = lo; f0 < hi; f0 += kBlock) {  // (uniform trip count)
    const uint64_t f = f0 + threadIdx.x;
    uint32_t m = 0, u = 0, kind = 0;
    if (f < hi) {
      m = a.plane[0][f]; u = a.plane[1][f];
      kind = pile_kind(a, (uint32_t)f, m, u);
    }
    const unsigned long long vote = __ballot(kind == 1u);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
      before += w < wave ? s_wave[w] : 0u;
      total += s_wave[w];
    }
    if (kind == 1u) {
      const unsigned long long slot = at + before + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
      uint32_t c_lo, c_hi;
      chrom_bounds(s_start, a.start_index, tab, (uint32_t)f, c_lo, c_hi);
      uint8_t strand = 0, context = 0;
      (void)pile_site(meth_ref_ext(a.ref, (long long)f - 2, a.ref_last), (uint32_t)f, c_lo, c_hi, strand, context);
      // one 16-byte store: pos, meth, unmeth, strand | context << 8 | reserved 0
      *reinterpret_cast<uint4*>(a.sites + slot) = make_uint4((uint32_t)f, m, u, (uint32_t)strand | ((uint32_t)context << 8));
    }
    at += total;
    __syncthreads();  // s_wave is rewritten by the next step
  }
}

// The summary (include/walt_amd.h, "methylation levels"): one pass over the block's share, a step of kBlock positions at
// a time, a wavefront on 64 neighbouring positions.  Nothing global is touched per site:
//   sites, covered      ballots, counted per wavefront (uniform values)
//   sums, maxima        per-lane registers, one set per row, selected by the lane's class; folded once per block
//   histograms          an LDS table of the block, kLevelCols columns per bin: a lane adds in column lane % 32, so the
//                       adds of one LDS cycle (32 lanes) fall on 32 banks whatever their bins are
// and then one 64-bit atomic per non-zero word of the block's walt_levels.
// The chromosome of a step: a wavefront keeps the bounds of the chromosome it is in (uniform) and searches again only
// when its first position has left them; the lanes search for themselves only in a step that reaches beyond those
// bounds, i.e. one that holds a chromosome start.
// The G of a pair is the next lane's position: its counters come by a cross-lane move, and a lane loads them itself
// only where the next lane holds none -- the wavefront's last lane and the last position of the block's share.
__global__ __launch_bounds__(kBlock) void k_pile_levels(const PileArgs a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  __shared__ uint32_t s_hist[kLevelRows * kLevelBins][kLevelCols];
  __shared__ unsigned long long s_out[kLevelWords];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  for (uint32_t i = threadIdx.x; i < kLevelRows * kLevelBins * kLevelCols; i += kBlock) (&s_hist[0][0])[i] = 0u;
  if (threadIdx.x < kLevelWords) s_out[threadIdx.x] = 0ull;
  __syncthreads();
  uint64_t lo, hi;
  pile_block_range(a, lo, hi);
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  unsigned long long n_sites[kLevelRows], n_cov[kLevelRows];            // (uniform)
  unsigned long long sm[kLevelRows], su[kLevelRows], mx[kLevelRows], ls[kLevelRows], off_m = 0, off_u = 0;
#pragma unroll
  for (uint32_t r = 0; r < kLevelRows; ++r) n_sites[r] = n_cov[r] = sm[r] = su[r] = mx[r] = ls[r] = 0;
  uint32_t w_lo = 1, w_hi = 0;  // the chromosome the wavefront is in (none yet)
  for (uint64_t f0 = lo; f0 < hi; f0 += kBlock) {
    const uint64_t wf = f0 + 64u * wave;  // (uniform) the wavefront's first position of this step
    if (wf >= hi) continue;
    const uint64_t wl = wf + 63 < hi - 1 ? wf + 63 : hi - 1;
    if (wf < w_lo || wf >= w_hi) {
      chrom_bounds(s_start, a.start_index, tab, (uint32_t)wf, w_lo, w_hi);
      w_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_lo);
      w_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_hi);
    }
    const bool one_chrom = wl < w_hi;  // (uniform)
    const uint64_t f = wf + lane;
    uint32_t m = 0, u = 0, cls = kLevelNone, c_hi = w_hi;
    bool pair = false;
    if (f < hi) {
      m = a.plane[0][f]; u = a.plane[1][f];
      uint32_t c_lo = w_lo;
      if (!one_chrom) chrom_bounds(s_start, a.start_index, tab, (uint32_t)f, c_lo, c_hi);
      const unsigned long long ext = meth_ref_ext(a.ref, (long long)f - 2, a.ref_last);
      cls = levels_class(ext, (uint32_t)f, c_lo, c_hi);
      pair = levels_pair(ext, (uint32_t)f, c_hi);
    }
    uint32_t m1 = __shfl_down(m, 1), u1 = __shfl_down(u, 1);
    if (pair && (lane == 63 || f + 1 >= hi)) {  // (f + 1 < c_hi <= genome_len: inside the planes)
      m1 = a.plane[0][f + 1]; u1 = a.plane[1][f + 1];
    }
    const bool site = cls != kLevelNone;
    const unsigned long long d = (unsigned long long)m + u;
    const bool cov = site && d != 0;
    off_m += site ? 0u : m;
    off_u += site ? 0u : u;
    unsigned long long q = 0;
    if (cov) {
      q = level_q30(m, u);
      atomicAdd(&s_hist[cls * kLevelBins + level_bin_of(m, u, q)][lane & (kLevelCols - 1)], 1u);
    }
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const bool is = cls == r;
      n_sites[r] += (uint32_t)__popcll(__ballot(is));
      n_cov[r] += (uint32_t)__popcll(__ballot(is && cov));
      sm[r] += is ? m : 0u;
      su[r] += is ? u : 0u;
      const unsigned long long dr = is ? d : 0ull;
      mx[r] = mx[r] > dr ? mx[r] : dr;
      ls[r] += is ? q : 0ull;
    }
    const unsigned long long pm = pair ? (unsigned long long)m + m1 : 0ull, pu = pair ? (unsigned long long)u + u1 : 0ull;
    const unsigned long long pd = pm + pu;
    n_sites[kLevelPair] += (uint32_t)__popcll(__ballot(pair));
    n_cov[kLevelPair] += (uint32_t)__popcll(__ballot(pd != 0));
    if (pd != 0) {
      const unsigned long long pq = level_q30(pm, pu);
      atomicAdd(&s_hist[kLevelPair * kLevelBins + level_bin_of(pm, pu, pq)][lane & (kLevelCols - 1)], 1u);
      ls[kLevelPair] += pq;
    }
    sm[kLevelPair] += pm;
    su[kLevelPair] += pu;
    mx[kLevelPair] = mx[kLevelPair] > pd ? mx[kLevelPair] : pd;
  }
  // the block's walt_levels in LDS: a wavefront's sums by one lane, the histogram's columns by one thread per bin
#pragma unroll
  for (uint32_t r = 0; r < kLevelRows; ++r) {
    for (int s = 32; s > 0; s >>= 1) {
      sm[r] += __shfl_down(sm[r], s);
      su[r] += __shfl_down(su[r], s);
      ls[r] += __shfl_down(ls[r], s);
      const unsigned long long o = __shfl_down(mx[r], s);
      mx[r] = mx[r] > o ? mx[r] : o;
    }
    if (lane == 0) {
      unsigned long long* row = s_out + r * kLevelRowWords;
      atomicAdd(row + 0, n_sites[r]);
      atomicAdd(row + 1, n_cov[r]);
      atomicAdd(row + 2, sm[r]);
      atomicAdd(row + 3, su[r]);
      atomicMax(row + kLevelMaxWord, mx[r]);
      atomicAdd(row + 5, ls[r]);
    }
  }
  for (int s = 32; s > 0; s >>= 1) { off_m += __shfl_down(off_m, s); off_u += __shfl_down(off_u, s); }
  if (lane == 0) {
    atomicAdd(s_out + kLevelRows * kLevelRowWords, off_m);
    atomicAdd(s_out + kLevelRows * kLevelRowWords + 1, off_u);
  }
  __syncthreads();
  if (threadIdx.x < kLevelRows * kLevelBins) {
    unsigned long long t = 0;
    for (uint32_t c = 0; c < kLevelCols; ++c) t += s_hist[threadIdx.x][c];
    s_out[(threadIdx.x / kLevelBins) * kLevelRowWords + 6 + threadIdx.x % kLevelBins] = t;
  }
  __syncthreads();
  if (threadIdx.x < kLevelWords) {
    const unsigned long long v = s_out[threadIdx.x];
    unsigned long long* acc = a.table + kPileLevels + threadIdx.x;
    if (v) {
      if (threadIdx.x < kLevelRows * kLevelRowWords && threadIdx.x % kLevelRowWords == kLevelMaxWord) atomicMax(acc, v);
      else atomicAdd(acc, v);
    }
  }
}

// ---------------------------------------------------------------- levels per region (regions_core.h)
struct RegionArgs {
  const uint32_t* plane[2];
  const uint32_t* ref;
  uint32_t ref_last;
  const uint32_t* start_index;
  uint32_t n_chrom, genome_len;
  const walt_region* regions;  // n of them
  uint32_t n;
  unsigned long long* prefix;  // n + 1: the exclusive prefix of the regions' units, the total behind it
  unsigned long long* table;   // the pile-up's: sums of kBlock regions each, scanned by k_pile_scan
  walt_region_levels* out;
};

__device__ __forceinline__ unsigned long long region_units_at(const RegionArgs& a, uint64_t i) {
  if (i >= a.n) return 0ull;
  const uint2 r = reinterpret_cast<const uint2*>(a.regions)[i];
  return region_units(r.x, r.y, a.genome_len);
}

// scan, launch 1 of 3: units of kBlock neighbouring regions -> table[block]  (launch 2 is k_pile_scan over those sums)
__global__ __launch_bounds__(kBlock) void k_region_sums(const RegionArgs a) {
  __shared__ unsigned long long s_red[kBlock / 64];
  unsigned long long v = region_units_at(a, (uint64_t)blockIdx.x * kBlock + threadIdx.x);
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_red[w];
    a.table[blockIdx.x] = t;
  }
}

// scan, launch 3 of 3: prefix[i] = the block's scanned sum + the units of the block's regions in front of i
__global__ __launch_bounds__(kBlock) void k_region_apply(const RegionArgs a) {
  __shared__ unsigned long long s_wave[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long v = region_units_at(a, i);
  unsigned long long incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(incl, d);
    incl += lane >= (uint32_t)d ? o : 0ull;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned long long before = a.table[blockIdx.x];
  for (uint32_t w = 0; w < kBlock / 64; ++w) before += w < wave ? s_wave[w] : 0ull;
  if (i < a.n) {
    a.prefix[i] = before + incl - v;
    if (i + 1 == a.n) a.prefix[a.n] = before + incl;
  }
}

// One wavefront's sums of the units of one region: counts are uniform (ballots), sums per lane.
struct RegionAcc {
  uint32_t n_sites[kLevelRows], n_cov[kLevelRows];
  unsigned long long sm[kLevelRows], su[kLevelRows], ls[kLevelRows];
};
__device__ __forceinline__ void region_acc_clear(RegionAcc& c) {
#pragma unroll
  for (uint32_t r = 0; r < kLevelRows; ++r) { c.n_sites[r] = c.n_cov[r] = 0u; c.sm[r] = c.su[r] = c.ls[r] = 0ull; }
}
// folds the lanes' sums and adds the wavefront's non-zero words into the region's record; a row no lane has a call in
// is not folded at all (an uncovered row has only `sites`)
__device__ __forceinline__ void region_acc_flush(RegionAcc& c, walt_region_levels* rec, uint32_t lane) {
#pragma unroll
  for (uint32_t r = 0; r < kLevelRows; ++r) {
    walt_region_row* row = rec->row + r;
    if (c.n_cov[r]) {  // (uniform)
      for (int s = 32; s > 0; s >>= 1) {
        c.sm[r] += __shfl_down(c.sm[r], s);
        c.su[r] += __shfl_down(c.su[r], s);
        c.ls[r] += __shfl_down(c.ls[r], s);
      }
    }
    if (lane == 0) {
      if (c.n_sites[r]) atomicAdd(&row->sites, c.n_sites[r]);
      if (c.n_cov[r]) {
        atomicAdd(&row->covered, c.n_cov[r]);
        if (c.sm[r]) atomicAdd(reinterpret_cast<unsigned long long*>(&row->meth), c.sm[r]);
        if (c.su[r]) atomicAdd(reinterpret_cast<unsigned long long*>(&row->unmeth), c.su[r]);
        if (c.ls[r]) atomicAdd(reinterpret_cast<unsigned long long*>(&row->level_sum), c.ls[r]);
      }
    }
  }
  region_acc_clear(c);
}

// The regions' records (include/walt_amd.h, "methylation levels per region").  The call's units are numbered through
// all its regions (prefix); a wavefront takes runs of neighbouring units by stride over a fixed grid -- the total is
// read from device memory, no block waits for another -- and walks a unit as k_pile_levels walks a step: 64
// neighbouring positions, the partner's counters from the next lane, the chromosome bounds kept while the wavefront
// stays inside them.  A run finds its first region by one search and the following ones by looking at the next
// prefix; the sums of a run's units of one region stay in registers and reach the record once.
__global__ __launch_bounds__(kBlock) void k_pile_regions(const RegionArgs a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned long long total = a.prefix[a.n];
  const unsigned long long n_waves = (unsigned long long)gridDim.x * (kBlock / 64);
  const unsigned long long me = (unsigned long long)blockIdx.x * (kBlock / 64) + wave;
  unsigned long long run = total / n_waves;  // runs as long as every wavefront still gets one
  run = run < 1ull ? 1ull : run > kRegionRun ? (unsigned long long)kRegionRun : run;
  RegionAcc acc;
  region_acc_clear(acc);
  uint32_t w_lo = 1, w_hi = 0;  // the chromosome the wavefront is in (none yet)
  for (unsigned long long u0 = me * run; u0 < total; u0 += n_waves * run) {
    const unsigned long long u_end = u0 + run < total ? u0 + run : total;
    uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)region_of_unit(a.prefix, 0u, a.n, u0));
    for (unsigned long long unit = u0; unit < u_end; ++unit) {
      if (unit != u0) {
        const uint32_t r1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)region_next(a.prefix, a.n, r, unit));
        if (r1 != r) region_acc_flush(acc, a.out + r, lane);
        r = r1;
      }
      const uint2 reg = reinterpret_cast<const uint2*>(a.regions)[r];
      unsigned long long lo, hi;
      region_unit_range(reg.x, reg.y, (uint32_t)(unit - a.prefix[r]), lo, hi);
      for (unsigned long long wf = lo; wf < hi; wf += 64) {  // (uniform) the wavefront's first position of this step
        const unsigned long long wl = wf + 63 < hi - 1 ? wf + 63 : hi - 1;
        if (wf < w_lo || wf >= w_hi) {
          chrom_bounds(s_start, a.start_index, tab, (uint32_t)wf, w_lo, w_hi);
          w_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_lo);
          w_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_hi);
        }
        const bool one_chrom = wl < w_hi;  // (uniform)
        const unsigned long long f = wf + lane;
        uint32_t m = 0, u = 0, cls = kLevelNone, c_hi = w_hi;
        bool pair = false;
        if (f < hi) {
          m = a.plane[0][f]; u = a.plane[1][f];
          uint32_t c_lo = w_lo;
          if (!one_chrom) chrom_bounds(s_start, a.start_index, tab, (uint32_t)f, c_lo, c_hi);
          const unsigned long long ext = meth_ref_ext(a.ref, (long long)f - 2, a.ref_last);
          cls = levels_class(ext, (uint32_t)f, c_lo, c_hi);
          pair = levels_pair(ext, (uint32_t)f, c_hi);
        }
        uint32_t m1 = __shfl_down(m, 1), u1 = __shfl_down(u, 1);
        if (pair && (lane == 63 || f + 1 >= hi)) {  // (f + 1 < c_hi <= genome_len: inside the planes)
          m1 = a.plane[0][f + 1]; u1 = a.plane[1][f + 1];
        }
        const bool cov = cls != kLevelNone && (m | u) != 0u;
        const unsigned long long q = cov ? level_q30(m, u) : 0ull;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
          const bool is = cls == k;
          acc.n_sites[k] += (uint32_t)__popcll(__ballot(is));
          acc.n_cov[k] += (uint32_t)__popcll(__ballot(is && cov));
          acc.sm[k] += is ? m : 0u;
          acc.su[k] += is ? u : 0u;
          acc.ls[k] += is ? q : 0ull;
        }
        const unsigned long long pm = pair ? (unsigned long long)m + m1 : 0ull, pu = pair ? (unsigned long long)u + u1 : 0ull;
        acc.n_sites[kLevelPair] += (uint32_t)__popcll(__ballot(pair));
        acc.n_cov[kLevelPair] += (uint32_t)__popcll(__ballot((pm | pu) != 0ull));
        if (pm | pu) acc.ls[kLevelPair] += level_q30(pm, pu);
        acc.sm[kLevelPair] += pm;
        acc.su[kLevelPair] += pu;
      }
    }
    region_acc_flush(acc, a.out + r, lane);
  }
}

// counters of [lo, lo + n) += src[0 .. n) (walt_pileup_add; wraps as the counters do)
__global__ __launch_bounds__(kBlock) void k_pile_window_add(uint32_t* plane, uint64_t lo, uint64_t n, const uint32_t* src) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) plane[lo + i] += src[i];
}

static PileArgs pile_args(const walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, uint32_t& n_blocks) {
  const walt_index* idx = p->idx;
  PileArgs a;
  a.plane[0] = p->plane[0]; a.plane[1] = p->plane[1];
  a.ref = idx->ref[0];
  a.ref_last = (idx->head.genome_len + 15) / 16 + kRefPadWords - 1;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  a.pos_lo = pos_lo; a.pos_hi = pos_hi;
  n_blocks = extract_blocks(idx, (uint64_t)pos_hi - pos_lo, kPileTile, kPileMaxBlocks, &a.chunk);
  a.table = p->table;
  a.sites = nullptr; a.cap = 0; a.n_sites_out = nullptr; a.offref_out = nullptr;
  return a;
}

static int pile_range_check(const walt_pileup* p, const char* who, uint32_t pos_lo, uint32_t pos_hi) {
  return range_refusal(p, who, "pile-up", pos_lo, pos_hi);
}

// count and scan on `stream`
static int pile_count_launch(const PileArgs& a, uint32_t n_blocks, hipStream_t stream) {
  WALT_HIP(hipMemsetAsync(a.table + kPileTotals, 0, 3 * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_pile_count, dim3(n_blocks), dim3(kBlock), 0, stream, a);
  return pile_scan_launch(a.table, n_blocks, a.n_sites_out, a.offref_out, stream);
}

// the scan of n_blocks counts in `table`: the pile-up's extraction and the regions' sums here, the flagged positions in
// variants.hip
int pile_scan_launch(unsigned long long* table, uint32_t n_blocks, unsigned long long* d_total, unsigned long long* d_offref,
                     hipStream_t stream) {
  PileArgs scan;
  memset(&scan, 0, sizeof scan);
  scan.table = table;
  scan.n_sites_out = d_total;
  scan.offref_out = d_offref;
  hipLaunchKernelGGL(k_pile_scan, dim3(1), dim3(1024), 0, stream, scan, n_blocks);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_pileup_create(walt_index* idx, walt_pileup** out) {
  if (!idx || !out) return fail(WALT_EINVAL, "walt_pileup_create: bad argument");
  *out = nullptr;
  if (!idx->ref[0])
    return fail(WALT_EINVAL, "walt_pileup_create: the index holds no reference (open it with WALT_WITH_REFERENCE or call "
                             "walt_index_enable_reference)");
  WALT_HIP(hipSetDevice(idx->device));
  const uint64_t plane_bytes = 4ull * idx->head.genome_len, want = 2 * plane_bytes + kPileTableBytes;
  walt_pileup* p = new walt_pileup;
  p->idx = idx;
  void* got[3] = {nullptr, nullptr, nullptr};
  const uint64_t sizes[3] = {plane_bytes, plane_bytes, kPileTableBytes};
  for (int i = 0; i < 3; ++i) {
    const hipError_t e = hipMalloc(&got[i], sizes[i] ? sizes[i] : 4);
    if (e != hipSuccess || hipMemset(got[i], 0, sizes[i]) != hipSuccess) {  // the index stays as it was
      (void)hipGetLastError();
      for (void* q : got) if (q) (void)hipFree(q);
      delete p;
      return fail(WALT_ENOMEM, "walt_pileup_create: the pile-up wants " + std::to_string(want) + " bytes of device memory (8 x genome_len + " +
                                   std::to_string(kPileTableBytes) + "): " + hipGetErrorString(e));
    }
  }
  WALT_HIP(hipDeviceSynchronize());
  p->plane[0] = static_cast<uint32_t*>(got[0]);
  p->plane[1] = static_cast<uint32_t*>(got[1]);
  p->table = static_cast<unsigned long long*>(got[2]);
  p->device_bytes = want;
  *out = p;
  return WALT_OK;
}

void walt_pileup_destroy(walt_pileup* p) {
  if (!p) return;
  (void)hipSetDevice(p->idx->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(p->plane[0]);
  (void)hipFree(p->plane[1]);
  (void)hipFree(p->table);
  delete p;
}

int walt_pileup_clear(walt_pileup* p) {
  if (!p) return fail(WALT_EINVAL, "walt_pileup_clear: bad argument (null pile-up)");
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  for (int i = 0; i < 2; ++i) WALT_HIP(hipMemset(p->plane[i], 0, 4ull * p->idx->head.genome_len));
  WALT_HIP(hipDeviceSynchronize());
  return WALT_OK;
}

uint64_t walt_pileup_device_bytes(const walt_pileup* p) { return p ? p->device_bytes : 0; }

int walt_pileup_extract_device(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, void* d_sites, uint64_t cap, void* d_n_sites,
                               void* d_offref, void* stream) {
  int rc = pile_range_check(p, "walt_pileup_extract_device", pos_lo, pos_hi);
  if (rc) return rc;
  if (!d_n_sites || (cap && !d_sites)) return fail(WALT_EINVAL, "walt_pileup_extract_device: bad argument");
  if (((uintptr_t)d_sites & 15u) || ((uintptr_t)d_n_sites & 7u) || ((uintptr_t)d_offref & 7u))
    return fail(WALT_EINVAL, "walt_pileup_extract_device: sites must be 16-byte aligned, n_sites and offref 8-byte aligned");
  WALT_HIP(hipSetDevice(p->idx->device));
  uint32_t n_blocks;
  PileArgs a = pile_args(p, pos_lo, pos_hi, n_blocks);
  a.sites = static_cast<walt_meth_site*>(d_sites);
  a.cap = cap;
  a.n_sites_out = static_cast<unsigned long long*>(d_n_sites);
  a.offref_out = static_cast<unsigned long long*>(d_offref);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if ((rc = pile_count_launch(a, n_blocks, s))) return rc;
  if (cap) hipLaunchKernelGGL(k_pile_write, dim3(n_blocks), dim3(kBlock), 0, s, a, n_blocks);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

int walt_pileup_extract(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, walt_meth_site* sites, uint64_t cap,
                        uint64_t* n_sites, uint64_t* offref) {
  int rc = pile_range_check(p, "walt_pileup_extract", pos_lo, pos_hi);
  if (rc) return rc;
  if (!n_sites || (cap && !sites)) return fail(WALT_EINVAL, "walt_pileup_extract: bad argument");
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  uint32_t n_blocks;
  PileArgs a = pile_args(p, pos_lo, pos_hi, n_blocks);
  if ((rc = pile_count_launch(a, n_blocks, nullptr))) return rc;
  unsigned long long tot[3];
  WALT_HIP(hipMemcpy(tot, p->table + kPileTotals, sizeof tot, hipMemcpyDeviceToHost));
  *n_sites = tot[0];
  if (offref) { offref[0] = tot[1]; offref[1] = tot[2]; }
  if (tot[0] > cap)
    return fail(WALT_EINVAL, "walt_pileup_extract: the range holds " + std::to_string(tot[0]) + " sites, the array has room for " +
                                 std::to_string(cap));
  if (!tot[0]) return WALT_OK;
  DeviceTemp d_sites;
  if (hipMalloc(&d_sites.p, tot[0] * sizeof(walt_meth_site)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(WALT_ENOMEM, "walt_pileup_extract: hipMalloc of " + std::to_string(tot[0] * sizeof(walt_meth_site)) + " bytes failed");
  }
  a.sites = static_cast<walt_meth_site*>(d_sites.p);
  a.cap = tot[0];
  hipLaunchKernelGGL(k_pile_write, dim3(n_blocks), dim3(kBlock), 0, nullptr, a, n_blocks);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(sites, d_sites.p, tot[0] * sizeof(walt_meth_site), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(WALT_EHIP, std::string("walt_pileup_extract: ") + hipGetErrorString(e));
  return WALT_OK;
}

// the accumulator cleared, the pass, and the 656 bytes copied to `d_out` (null: they stay in the table), on `stream`
static int pile_levels_launch(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, void* d_out, hipStream_t stream) {
  uint32_t n_blocks;
  const PileArgs a = pile_args(p, pos_lo, pos_hi, n_blocks);
  WALT_HIP(hipMemsetAsync(a.table + kPileLevels, 0, sizeof(walt_levels), stream));
  hipLaunchKernelGGL(k_pile_levels, dim3(n_blocks), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  if (d_out) WALT_HIP(hipMemcpyAsync(d_out, a.table + kPileLevels, sizeof(walt_levels), hipMemcpyDeviceToDevice, stream));
  return WALT_OK;
}

int walt_pileup_levels_device(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, void* d_out, void* stream) {
  int rc = pile_range_check(p, "walt_pileup_levels_device", pos_lo, pos_hi);
  if (rc) return rc;
  if (!d_out) return fail(WALT_EINVAL, "walt_pileup_levels_device: bad argument (null out)");
  if ((uintptr_t)d_out & 7u) return fail(WALT_EINVAL, "walt_pileup_levels_device: out must be 8-byte aligned");
  WALT_HIP(hipSetDevice(p->idx->device));
  return pile_levels_launch(p, pos_lo, pos_hi, d_out, reinterpret_cast<hipStream_t>(stream));
}

int walt_pileup_levels(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, walt_levels* out) {
  int rc = pile_range_check(p, "walt_pileup_levels", pos_lo, pos_hi);
  if (rc) return rc;
  if (!out) return fail(WALT_EINVAL, "walt_pileup_levels: bad argument (null out)");
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  if ((rc = pile_levels_launch(p, pos_lo, pos_hi, nullptr, nullptr))) return rc;
  WALT_HIP(hipMemcpy(out, p->table + kPileLevels, sizeof(walt_levels), hipMemcpyDeviceToHost));
  return WALT_OK;
}

uint64_t walt_pileup_regions_workspace_bytes(uint32_t n) { return 8ull * ((uint64_t)n + 1); }

// the records zeroed, the three launches of the scan and the walk, on `stream`
static int pile_regions_launch(walt_pileup* p, const void* d_regions, uint32_t n, void* d_out, void* d_work, hipStream_t stream) {
  const walt_index* idx = p->idx;
  RegionArgs a;
  a.plane[0] = p->plane[0]; a.plane[1] = p->plane[1];
  a.ref = idx->ref[0];
  a.ref_last = (idx->head.genome_len + 15) / 16 + kRefPadWords - 1;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  a.genome_len = idx->head.genome_len;
  a.regions = static_cast<const walt_region*>(d_regions);
  a.n = n;
  a.prefix = static_cast<unsigned long long*>(d_work);
  a.table = p->table;
  a.out = static_cast<walt_region_levels*>(d_out);
  const uint32_t n_sums = (n + kBlock - 1) / kBlock;
  const uint64_t want = idx->opt.pile_extract_blocks ? (uint64_t)idx->opt.pile_extract_blocks : (uint64_t)idx->n_cu * 8;
  const uint32_t n_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, kPileMaxBlocks));
  WALT_HIP(hipMemsetAsync(d_out, 0, (uint64_t)n * sizeof(walt_region_levels), stream));
  hipLaunchKernelGGL(k_region_sums, dim3(n_sums), dim3(kBlock), 0, stream, a);
  if (const int rc = pile_scan_launch(p->table, n_sums, nullptr, nullptr, stream)) return rc;
  hipLaunchKernelGGL(k_region_apply, dim3(n_sums), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(k_pile_regions, dim3(n_blocks), dim3(kBlock), 0, stream, a);
  WALT_HIP(hipGetLastError());
  return WALT_OK;
}

int walt_pileup_regions_device(walt_pileup* p, const void* d_regions, uint32_t n, void* d_out, void* d_work, void* stream) {
  if (!p) return fail(WALT_EINVAL, "walt_pileup_regions_device: bad argument (null pile-up)");
  if (!n) return WALT_OK;
  if (n > WALT_REGIONS_MAX)
    return fail(WALT_EINVAL, "walt_pileup_regions_device: " + std::to_string(n) + " regions, a call takes " + std::to_string(WALT_REGIONS_MAX) +
                                 " at most");
  if (!d_regions || !d_out || !d_work) return fail(WALT_EINVAL, "walt_pileup_regions_device: bad argument (null regions, out or workspace)");
  if (((uintptr_t)d_regions & 7u) || ((uintptr_t)d_out & 7u) || ((uintptr_t)d_work & 7u))
    return fail(WALT_EINVAL, "walt_pileup_regions_device: regions, out and the workspace must be 8-byte aligned");
  WALT_HIP(hipSetDevice(p->idx->device));
  return pile_regions_launch(p, d_regions, n, d_out, d_work, reinterpret_cast<hipStream_t>(stream));
}

int walt_pileup_regions(walt_pileup* p, const walt_region* regions, uint64_t n, walt_region_levels* out) {
  if (!p) return fail(WALT_EINVAL, "walt_pileup_regions: bad argument (null pile-up)");
  if (!n) return WALT_OK;
  if (!regions || !out) return fail(WALT_EINVAL, "walt_pileup_regions: bad argument (null regions or out)");
  const uint32_t genome_len = p->idx->head.genome_len;
  for (uint64_t i = 0; i < n; ++i)
    if (regions[i].lo > regions[i].hi || regions[i].hi > genome_len)
      return fail(WALT_EINVAL, "walt_pileup_regions: region " + std::to_string(i) + " [" + std::to_string(regions[i].lo) + ", " +
                                   std::to_string(regions[i].hi) + ") is not inside the genome's " + std::to_string(genome_len) + " positions");
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  const uint32_t window = (uint32_t)std::min<uint64_t>(n, WALT_REGIONS_MAX);
  const uint64_t sizes[3] = {(uint64_t)window * sizeof(walt_region), (uint64_t)window * sizeof(walt_region_levels),
                             walt_pileup_regions_workspace_bytes(window)};
  void* got[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; ++i)
    if (hipMalloc(&got[i], sizes[i]) != hipSuccess) {
      (void)hipGetLastError();
      for (void* q : got) if (q) (void)hipFree(q);
      return fail(WALT_ENOMEM, "walt_pileup_regions: hipMalloc of " + std::to_string(sizes[i]) + " bytes failed");
    }
  hipError_t e = hipSuccess;
  int rc = WALT_OK;
  for (uint64_t at = 0; at < n && e == hipSuccess && rc == WALT_OK; at += window) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(window, n - at);
    e = hipMemcpy(got[0], regions + at, (uint64_t)m * sizeof(walt_region), hipMemcpyHostToDevice);
    if (e != hipSuccess) break;
    rc = pile_regions_launch(p, got[0], m, got[1], got[2], nullptr);
    if (rc == WALT_OK) e = hipMemcpy(out + at, got[1], (uint64_t)m * sizeof(walt_region_levels), hipMemcpyDeviceToHost);
  }
  for (void* q : got) (void)hipFree(q);
  if (rc != WALT_OK) return rc;
  if (e != hipSuccess) return fail(WALT_EHIP, std::string("walt_pileup_regions: ") + hipGetErrorString(e));
  return WALT_OK;
}

int walt_pileup_read(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, uint32_t* meth, uint32_t* unmeth) {
  const int rc = pile_range_check(p, "walt_pileup_read", pos_lo, pos_hi);
  if (rc) return rc;
  if (pos_lo == pos_hi) return WALT_OK;
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  uint32_t* const dst[2] = {meth, unmeth};
  for (int i = 0; i < 2; ++i)
    if (dst[i]) WALT_HIP(hipMemcpy(dst[i], p->plane[i] + pos_lo, 4ull * (pos_hi - pos_lo), hipMemcpyDeviceToHost));
  return WALT_OK;
}

int walt_pileup_add(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, const uint32_t* meth, const uint32_t* unmeth) {
  const int rc = pile_range_check(p, "walt_pileup_add", pos_lo, pos_hi);
  if (rc) return rc;
  if (pos_lo == pos_hi || (!meth && !unmeth)) return WALT_OK;
  WALT_HIP(hipSetDevice(p->idx->device));
  WALT_HIP(hipDeviceSynchronize());  // adds of any stream come first
  const uint64_t window = std::min<uint64_t>(kPileAddWindow, (uint64_t)pos_hi - pos_lo);
  void* d_src = nullptr;
  if (hipMalloc(&d_src, 4 * window) != hipSuccess) {
    (void)hipGetLastError();
    return fail(WALT_ENOMEM, "walt_pileup_add: hipMalloc of " + std::to_string(4 * window) + " bytes failed");
  }
  const uint32_t* const src[2] = {meth, unmeth};
  hipError_t e = hipSuccess;
  for (uint64_t lo = pos_lo; lo < pos_hi && e == hipSuccess; lo += window) {
    const uint64_t n = std::min<uint64_t>(window, (uint64_t)pos_hi - lo);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
      if (!src[i]) continue;
      e = hipMemcpy(d_src, src[i] + (lo - pos_lo), 4 * n, hipMemcpyHostToDevice);
      if (e != hipSuccess) break;
      hipLaunchKernelGGL(k_pile_window_add, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, p->plane[i], lo, n,
                         static_cast<const uint32_t*>(d_src));
      e = hipGetLastError();
      if (e == hipSuccess) e = hipDeviceSynchronize();  // the staging buffer is written again next
    }
  }
  (void)hipFree(d_src);
  if (e != hipSuccess) return fail(WALT_EHIP, std::string("walt_pileup_add: ") + hipGetErrorString(e));
  return WALT_OK;
}

}  // extern "C"
