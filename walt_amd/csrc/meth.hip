// meth.hip -- per-read methylation calling on the device (include/walt_amd.h, "methylation calls"): the unconverted
// reference rebuilt from the converted strand genomes, and the streaming kernel that classifies every base of every
// read of a mapped batch against it.  The reference has no such mode; the contract is the header's.
#include <fcntl.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "meth_core.h"
#include "pile_device.h"
#include "pileup_core.h"

namespace walt {

constexpr uint32_t kRefPadWords = 16;    // zero words behind a packed reference (meth_core.h meth_ref_ext reads three words)
constexpr uint32_t kMethShards = 64;     // shards of the batch totals (one 128-byte line each, like map_common.h kStatShards)
constexpr uint32_t kMethShardWords = 16;
constexpr uint32_t kMethTotals = 9;      // walt_meth_stats: reads, meth[4], unmeth[4]
constexpr uint64_t kMaxReadLenAny = 1024;  // walt_max_read_len() of the widest pattern: 16-bit counts hold a read's calls

// ---------------------------------------------------------------------------
// the unconverted reference: a position is C exactly where the G->A genome says C, else what the C->T genome says
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pack16(const uint8_t* __restrict__ bytes, uint64_t b0, uint32_t len) {
  uint32_t v = 0;
  if (b0 + 16 <= len) {
    const uint4 q = *reinterpret_cast<const uint4*>(bytes + b0);  // hipMalloc base is 256-B aligned
    const uint32_t qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) v |= (base_code((uint8_t)(qs[i] >> (8 * k))) & 3u) << (2 * (4 * i + k));
  } else {
    for (uint32_t k = 0; k < 16; ++k)
      if (b0 + k < len) v |= (base_code(bytes[b0 + k]) & 3u) << (2 * k);
  }
  return v;
}
// one packed word per thread; each side comes packed (a resident strand) or as the strand file's bytes
__global__ void k_ref_build(const uint32_t* __restrict__ ct_g2, const uint8_t* __restrict__ ct_bytes,
                            const uint32_t* __restrict__ ga_g2, const uint8_t* __restrict__ ga_bytes, uint32_t len,
                            uint32_t nwords, uint32_t* __restrict__ out) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwords) return;
  const uint32_t ct = ct_g2 ? ct_g2[w] : pack16(ct_bytes, (uint64_t)w * 16, len);
  const uint32_t ga = ga_g2 ? ga_g2[w] : pack16(ga_bytes, (uint64_t)w * 16, len);
  const uint32_t c = meth_eq2(ga, 1u);
  uint32_t v = (ct & ~(c * 3u)) | c;
  if ((uint64_t)w * 16 + 16 > len) v &= (1u << (2 * (len - w * 16))) - 1u;  // the last word: nothing beyond the genome
  out[w] = v;
}

static uint32_t ref_words(const walt_index* idx) { return (idx->head.genome_len + 15) / 16 + kRefPadWords; }

static int ref_alloc(walt_index* idx, void** p, uint64_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) return fail(WALT_ENOMEM, std::string("hipMalloc failed (reference): ") + hipGetErrorString(e));
  idx->allocs.push_back(*p);
  idx->device_bytes += bytes;
  return WALT_OK;
}

// genome section of a strand file (offset 1, genome_len bytes; reference.cpp:302-322) -> device bytes
static int read_genome_section(const std::string& path, uint32_t genome_len, uint8_t* d_bytes) {
  int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) return fail(WALT_EIO, "cannot open input file " + path);
  const size_t piece = 32u << 20;
  std::vector<char> buf(std::min<size_t>(piece, (size_t)genome_len + 1));
  int rc = WALT_OK;
  for (uint64_t at = 0; at < genome_len && !rc;) {
    const size_t want = (size_t)std::min<uint64_t>(piece, genome_len - at);
    size_t got = 0;
    while (got < want) {
      const ssize_t r = pread(fd, buf.data() + got, want - got, (off_t)(1 + at + got));
      if (r <= 0) break;
      got += (size_t)r;
    }
    if (got != want) rc = fail(WALT_EFORMAT, "read file error (strand index): file too short: " + path);
    else if (hipMemcpy(d_bytes + at, buf.data(), want, hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(WALT_EHIP, "upload of a strand genome failed");
    at += want;
  }
  ::close(fd);
  return rc;
}

// Builds both packed references.  A strand the index holds is taken from its packed genome; any other is read from
// <dbindex_path>_<strand> (its genome section alone), which needs dbindex_path.
int build_reference(walt_index* idx, const char* dbindex_path) {
  if (idx->ref[0]) return WALT_OK;
  static const char* sfx[4] = {"_CT00", "_CT01", "_GA10", "_GA11"};
  const uint32_t genome_len = idx->head.genome_len, nwords = (genome_len + 15) / 16, total = ref_words(idx);
  if (!dbindex_path && (idx->strand_mask & 15u) != 15u) {
    std::string missing;
    for (int s = 0; s < 4; ++s)
      if (!((idx->strand_mask >> s) & 1u)) missing += std::string(missing.empty() ? "" : ", ") + (sfx[s] + 1);
    return fail(WALT_EINVAL, "walt_index_enable_reference: the reference needs all four strands resident; missing: " +
                                 missing + " (open the index with WALT_WITH_REFERENCE instead)");
  }
  WALT_HIP(hipSetDevice(idx->device));
  const size_t allocs_before = idx->allocs.size();
  const uint64_t bytes_before = idx->device_bytes;
  uint32_t* ref[2] = {nullptr, nullptr};
  unsigned long long* shards = nullptr;
  int rc = WALT_OK;
  for (int o = 0; o < 2 && !rc; ++o) {
    DeviceTemp tmp[2];
    const uint32_t* g2[2] = {nullptr, nullptr};
    const uint8_t* bytes[2] = {nullptr, nullptr};
    for (int c = 0; c < 2 && !rc; ++c) {  // c = 0: the C->T strand of this orientation, 1: the G->A strand
      const int s = 2 * c + o;
      if ((idx->strand_mask >> s) & 1u) { g2[c] = idx->view.s[s].g2; continue; }
      if (hipMalloc(&tmp[c].p, (size_t)genome_len + 16) != hipSuccess) { rc = fail(WALT_ENOMEM, "hipMalloc failed (strand genome)"); break; }
      rc = read_genome_section(std::string(dbindex_path) + sfx[s], genome_len, static_cast<uint8_t*>(tmp[c].p));
      bytes[c] = static_cast<const uint8_t*>(tmp[c].p);
    }
    if (!rc) rc = ref_alloc(idx, reinterpret_cast<void**>(&ref[o]), (uint64_t)total * 4);
    if (!rc && hipMemset(ref[o] + nwords, 0, (size_t)kRefPadWords * 4) != hipSuccess) rc = fail(WALT_EHIP, "hipMemset failed (reference)");
    if (!rc && nwords) {
      hipLaunchKernelGGL(k_ref_build, dim3(grid_for(nwords)), dim3(kBlock), 0, nullptr, g2[0], bytes[0], g2[1], bytes[1],
                         genome_len, nwords, ref[o]);
      if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = fail(WALT_EHIP, "building the reference failed");
    }
  }
  if (!rc) rc = ref_alloc(idx, reinterpret_cast<void**>(&shards), (uint64_t)kMethShards * kMethShardWords * 8);
  if (!rc && hipMemset(shards, 0, (size_t)kMethShards * kMethShardWords * 8) != hipSuccess) rc = fail(WALT_EHIP, "hipMemset failed (reference)");
  if (rc) {  // the index stays as it was
    while (idx->allocs.size() > allocs_before) { (void)hipFree(idx->allocs.back()); idx->allocs.pop_back(); }
    idx->device_bytes = bytes_before;
    return rc;
  }
  idx->ref[0] = ref[0]; idx->ref[1] = ref[1];
  idx->meth_shards = shards;
  return WALT_OK;
}

// ---------------------------------------------------------------------------
// the calling kernel
// ---------------------------------------------------------------------------
struct MethArgs {
  const uint32_t* ref[2];      // '+' and '-' orientation
  uint32_t ref_last;           // last word index of a reference array
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
  uint8_t* calls;              // null: not wanted
  unsigned long long* counts;  // null: not wanted (two words per read: walt_meth_counts)
  unsigned long long* shards;  // null: no batch totals
  uint32_t* pile[2];           // the pile-up's counters by forward position: methylated, unmethylated (k_meth_pile* only)
  const uint8_t* skip;         // null: none; else a record with a non-zero byte at skip[r * skip_stride] is not counted
  uint64_t skip_stride;
  const uint32_t* excl;        // null: none; else excl[r] = ex_lo | ex_hi << 16, read positions of record r that get no call
  uint32_t trim5, trim3;       // the ignored read ends of the batch (include/walt_amd.h, "ignored read ends"); read by the kTrim instances alone
  const uint8_t* quals;        // one byte per base at the offsets of `bases` (include/walt_amd.h, "minimum base quality"); read by the kQual instances alone
  uint32_t min_qual;           // 0 .. 127
};

// Eight lanes per read, one 16-base slice per lane and trip.  Slices are cut at the 16-byte boundaries of the CALLS
// array, so a whole slice is one aligned 16-byte store and the eight lanes of a group write 128 contiguous bytes; the
// first and last slice of a read are partial (offsets are not multiples of 16) and touch only the read's own bytes.
//
// kPile: 0 the calling alone (k_meth_call), 1 / 2 the same with every call of a record with times == 1 added to the
// pile-up (include/walt_amd.h, "methylation pile-up"), the batch read once.  1: every lane adds its own slice's calls
// (pile_slice); 2: pile_rows.
// kExcl: the batch comes with excluded intervals (a.excl).  An instance of its own: the calls without them run the
// code they always ran (the word's load and the mask's arithmetic per slice cost the calling kernel 3 % when both
// lived in one instance).
// kTrim: the batch comes with ignored read ends (a.trim5, a.trim3: two scalars of the call, no load per record).  The 3'
// bound comes off `limit`, the 5' bound is the lower end of every slice's range; a slice wholly outside them returns
// inside meth_read_slice before it loads anything (all eight lanes of a group still take every trip: pile_rows).
// Instances of their own for the same reason as kExcl: a call without bounds runs the code it always ran.
// kQual: the batch comes with base qualities (a.quals, a.min_qual): every slice loads its 16 quality bytes beside its read
// bytes and the positions below the floor leave its flags (meth_read_slice_q).  Instances of their own once more: a call
// without qualities launches the kernels it always launched.  There are three of them, not twelve: a quality instance
// carries the interval word and the bounds unconditionally (kExcl and kTrim both set, a.excl tested for null per record,
// bounds of 0 without -I): DESIGN.md section 27 has the register figures the choice rests on.
template <int kPile, bool kExcl, bool kTrim, bool kQual = false>
__device__ __forceinline__ void meth_call_body(const MethArgs& a) {
  __shared__ uint32_t s_start[kLdsChroms + 1];
  __shared__ unsigned long long s_red[kBlock / 64][kMethTotals];
  const ChromTab tab = chrom_tab_of(a.n_chrom);
  chrom_tab_stage(s_start, a.start_index, tab);
  __syncthreads();
  const uint32_t sub = threadIdx.x & (kMethGroup - 1);
  const uint64_t groups = (uint64_t)gridDim.x * (kBlock / kMethGroup);
  const uint64_t batch_bytes = a.offsets[a.n];
  uint32_t tot[kMethTotals];  // this lane's share of the batch totals (group leaders only)
#pragma unroll
  for (uint32_t i = 0; i < kMethTotals; ++i) tot[i] = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / kMethGroup) + threadIdx.x / kMethGroup; r < a.n; r += groups) {
    const uint64_t off = a.offsets[r], end = a.offsets[r + 1];
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.records + r * a.rec_stride);
    const uint32_t pos = rec[0], times = rec[1], strand = rec[2] & 0xFFu;
    const uint32_t cv = a.conv ? a.conv[r * a.conv_stride] : a.conversion;
    const uint32_t len = end > off && end - off <= kMaxReadLenAny ? (uint32_t)(end - off) : 0u;
    uint32_t limit = a.call_len ? a.call_len[r] : len;
    limit = limit < len ? limit : len;
    if (kTrim) limit = meth_trim_limit(limit, a.trim3);
    const uint32_t trim5 = kTrim ? a.trim5 : 0u;
    // unmapped, made up (a position outside the genome, an unknown conversion) or empty: no call anywhere
    const bool valid = times != 0 && pos < a.genome_len && (cv == 'T' || cv == 'A');
    const bool mapped = valid && limit != 0;
    // counted: piled up and summed into the batch totals (a duplicate, include/walt_amd.h "duplicates", is called but not counted)
    const bool counted = times == 1 && !(a.skip && a.skip[r * a.skip_stride]);
    uint32_t c_lo = 0, c_hi = 0;
    if (mapped) chrom_bounds(s_start, a.start_index, tab, pos, c_lo, c_hi);
    // the other mate of the pair calls these read positions (include/walt_amd.h, "overlap of a pair"); 0: none
    const uint32_t ex = !kExcl || (kQual && !a.excl) ? 0u : a.excl[r];
    const uint32_t ex_lo = ex & 0xFFFFu, ex_hi = ex >> 16;
    const uint32_t ga = cv == 'A' ? 1u : 0u;
    const uint32_t* __restrict__ ref = a.ref[strand == '-' ? 1 : 0];
    unsigned long long meth = 0, unmeth = 0;
    if (kPile == 2 && end > off && (mapped || a.calls)) {  // as below, every lane of the group taking every trip
      const uint8_t* rb = a.bases + off;
      const uint8_t* qb = kQual ? a.quals + off : nullptr;
      uint8_t* cb = a.calls ? a.calls + off : nullptr;
      const int head = (int)((a.calls ? (uintptr_t)cb : (uintptr_t)rb) & 15u);
      for (uint64_t done = 0; done < end - off; done += 1u << 30) {
        const int total = (int)(end - off - done < (1u << 30) ? end - off - done : (1u << 30));
        const int h = done ? 0 : head;
        for (int base = -h; base < total; base += 16 * (int)kMethGroup) {
          const int i0 = base + 16 * (int)sub;
          uint32_t cm = 0, cu = 0;
          if (i0 < total) {
            uint32_t out[4];
            meth_read_slice_q<kQual>(rb + done, total, limit, mapped && !done, pos, c_lo, c_hi, ga, ref, a.ref_last, i0, off + done,
                                     batch_bytes - off - done, out, meth, unmeth, cm, cu, ex_lo, ex_hi, trim5,
                                     kQual ? qb + done : nullptr, a.min_qual);
            if (cb) meth_store_slice(cb + done, total, i0, out);
          }
          if (counted) pile_rows(cm, cu, (long long)pos + base, sub, strand == '-', c_lo, c_hi, a.pile);
        }
      }
    } else if (end > off && (mapped || a.calls)) {
      // (bytes of calls to write: the read's own; a read longer than any pattern allows is written in pieces of 2^30)
      const uint8_t* rb = a.bases + off;
      const uint8_t* qb = kQual ? a.quals + off : nullptr;
      uint8_t* cb = a.calls ? a.calls + off : nullptr;
      // slice grid: by the calls array's address (by the bases' when no calls are wanted)
      const int head = (int)((a.calls ? (uintptr_t)cb : (uintptr_t)rb) & 15u);
      for (uint64_t done = 0; done < end - off; done += 1u << 30) {  // (one trip unless the caller made the offsets up)
        const int total = (int)(end - off - done < (1u << 30) ? end - off - done : (1u << 30));
        const int h = done ? 0 : head;
        for (int i0 = -h + 16 * (int)sub; i0 < total; i0 += 16 * (int)kMethGroup) {
          uint32_t out[4], cm, cu;
          meth_read_slice_q<kQual>(rb + done, total, limit, mapped && !done, pos, c_lo, c_hi, ga, ref, a.ref_last, i0, off + done,
                                   batch_bytes - off - done, out, meth, unmeth, cm, cu, ex_lo, ex_hi, trim5,
                                   kQual ? qb + done : nullptr, a.min_qual);
          if (kPile == 1 && counted)  // (flags are set only where done == 0: slice position k is genome position pos + i0 + k)
            pile_slice(cm, cu, (long long)pos + i0, strand == '-', c_lo, c_hi,
                       [&](uint32_t f, bool m) { pile_add(a.pile[m ? 0 : 1], f); });
          if (cb) meth_store_slice(cb + done, total, i0, out);
        }
      }
    }
    // the group's eight partial counts (16-bit fields: a read holds at most 1024 bases)
#pragma unroll
    for (uint32_t d = 1; d < kMethGroup; d <<= 1) {
      meth += __shfl_xor(meth, d, kMethGroup);
      unmeth += __shfl_xor(unmeth, d, kMethGroup);
    }
    if (sub == 0) {
      if (a.counts) { a.counts[2 * r] = meth; a.counts[2 * r + 1] = unmeth; }
      if (counted && valid) {
        tot[0] += 1;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
          tot[1 + i] += (uint32_t)(meth >> (16 * i)) & 0xFFFFu;
          tot[5 + i] += (uint32_t)(unmeth >> (16 * i)) & 0xFFFFu;
        }
      }
    }
  }
  if (!a.shards) return;  // (uniform)
  // batch totals: wavefront, block, then one shard per block (one atomic per lane would serialise at a single line)
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t i = 0; i < kMethTotals; ++i) {
    unsigned long long v = tot[i];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) s_red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kMethTotals) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_red[w][threadIdx.x];
    if (t) atomicAdd(&a.shards[(uint64_t)(blockIdx.x % kMethShards) * kMethShardWords + threadIdx.x], t);
  }
}

__global__ __launch_bounds__(kBlock) void k_meth_call(const MethArgs a) { meth_call_body<0, false, false>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile(const MethArgs a) { meth_call_body<1, false, false>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_rows(const MethArgs a) { meth_call_body<2, false, false>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_call_excl(const MethArgs a) { meth_call_body<0, true, false>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_excl(const MethArgs a) { meth_call_body<1, true, false>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_rows_excl(const MethArgs a) { meth_call_body<2, true, false>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_call_trim(const MethArgs a) { meth_call_body<0, false, true>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_trim(const MethArgs a) { meth_call_body<1, false, true>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_rows_trim(const MethArgs a) { meth_call_body<2, false, true>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_call_excl_trim(const MethArgs a) { meth_call_body<0, true, true>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_excl_trim(const MethArgs a) { meth_call_body<1, true, true>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_rows_excl_trim(const MethArgs a) { meth_call_body<2, true, true>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_call_qual(const MethArgs a) { meth_call_body<0, true, true, true>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_qual(const MethArgs a) { meth_call_body<1, true, true, true>(a); }
__global__ __launch_bounds__(kBlock) void k_meth_pile_rows_qual(const MethArgs a) { meth_call_body<2, true, true, true>(a); }

// folds the shards into walt_meth_stats (accumulating) and clears them
__global__ void k_meth_reduce(unsigned long long* __restrict__ shards, unsigned long long* __restrict__ stats) {
  const uint32_t t = threadIdx.x;  // one thread per total
  unsigned long long sum = 0;
  for (uint32_t k = 0; k < kMethShards; ++k) {
    sum += shards[(uint64_t)k * kMethShardWords + t];
    shards[(uint64_t)k * kMethShardWords + t] = 0;
  }
  if (sum) atomicAdd(&stats[t], sum);
}

// One call of the calling kernel, through whichever of the twelve entry points it came: the index, the destinations and
// filters it may have, and the batch -- host arrays in a host form, device arrays in a device form and in meth_launch.
// What an entry point does not have stays null.  (Initialised by name: hipcc takes designated initialisers in C++17.)
struct MethCall {
  const char* who = nullptr;       // the entry point, as the refusals name it
  bool pile_required = false;      // the two oldest pile-up forms: a pile-up must be given (the newer ones: null is calls only)
  walt_index* idx = nullptr;
  walt_pileup* pile = nullptr;
  const void *bases = nullptr, *offsets = nullptr;
  uint32_t n = 0;
  const void* records = nullptr;
  size_t record_stride = 0;
  const void* conv = nullptr;      // null: `conversion` for every read
  size_t conv_stride = 0;
  int conversion = 0;
  const void* call_len = nullptr;
  void *calls = nullptr, *counts = nullptr, *stats = nullptr;
  const void* skip = nullptr;
  size_t skip_stride = 0;
  const void* excl = nullptr;
  walt_mbias* mb = nullptr;        // the bias set whose `table` takes the calls too
  uint32_t table = 0;
  uint32_t trim5 = 0, trim3 = 0;   // the ignored read ends (include/walt_amd.h, "ignored read ends"); both 0: none
  walt_cpgpairs* ap = nullptr;     // the pair table that takes the calls too (include/walt_amd.h, "adjacent CpG pairs")
  walt_epialleles* ep = nullptr;   // the window table that takes the calls too (include/walt_amd.h, "four-CpG epialleles")
  walt_pileup* ev = nullptr;       // the object that takes the batch's opposite-strand evidence (include/walt_amd.h, "opposite-strand evidence")
  bool ev_required = false;        // walt_meth_evidence_batch[_device]: it must be given
  const void* quals = nullptr;     // one byte per base (include/walt_amd.h, "minimum base quality"); null: the call as it was
  uint32_t min_qual = 0;
  // the rule that judges the calls too (include/walt_amd.h, "non-converted reads"; null: none), and where the verdicts go
  bool rule_form = false;          // walt_meth_nonconv_batch[_device]: a rule must be given
  const walt_nonconv_rule* rule = nullptr;
  void* filt = nullptr;
  size_t filt_stride = 0;
  void* tally = nullptr;
  void* stream = nullptr;          // device forms
};

// What a host form and a device form refuse alike, before they look at the batch.  has_calls: the bias table is counted
// from the calls on the device (a host form always has them there).
static int meth_call_check(const MethCall& c, bool has_calls) {
  const std::string who(c.who);
  if (!c.idx) return fail(WALT_EINVAL, who + ": bad argument");
  if (!c.pile && c.pile_required) return fail(WALT_EINVAL, who + ": bad argument (null pile-up)");
  if (c.pile && c.pile->idx != c.idx) return fail(WALT_EINVAL, who + ": the pile-up belongs to another index");
  if (!c.ev && c.ev_required) return fail(WALT_EINVAL, who + ": bad argument (null evidence)");
  if (c.ev && c.ev->idx != c.idx) return fail(WALT_EINVAL, who + ": the evidence belongs to another index");
  if (c.ev && c.ev == c.pile) return fail(WALT_EINVAL, who + ": the evidence and the pile-up are one object");
  if (!c.idx->ref[0])
    return fail(WALT_EINVAL, who + ": the index holds no reference (open it with WALT_WITH_REFERENCE or "
                                   "call walt_index_enable_reference)");
  if (c.min_qual > 127u)
    return fail(WALT_EINVAL, who + ": min_qual " + std::to_string(c.min_qual) + " (a quality byte is compared with 0 to 127)");
  if (!c.quals && c.min_qual)
    return fail(WALT_EINVAL, who + ": min_qual " + std::to_string(c.min_qual) + " without quals");
  std::string bad = record_stride_refusal(c.record_stride);
  if (bad.empty()) bad = conv_refusal(c.conv, c.conv_stride, c.conversion);
  if (!bad.empty()) return fail(WALT_EINVAL, who + ": " + bad);
  if (c.mb) {  // (include/walt_amd.h, "methylation bias by read position"): same device, a table it has, calls to count
    if (c.mb->device != c.idx->device)
      return fail(WALT_EINVAL, who + ": the bias set lives on device " + std::to_string(c.mb->device) +
                                   ", the index on device " + std::to_string(c.idx->device));
    if (c.table >= c.mb->n_tables)
      return fail(WALT_EINVAL, who + ": table " + std::to_string(c.table) + " of a bias set with " + std::to_string(c.mb->n_tables));
    if (!has_calls)
      return fail(WALT_EINVAL, who + ": the bias table is counted from the calls: d_calls must not be NULL when a bias set is given");
  }
  if (!(bad = skip_stride_refusal(c.skip, c.skip_stride)).empty()) return fail(WALT_EINVAL, who + ": " + bad);
  if (c.ap) {  // (include/walt_amd.h, "adjacent CpG pairs"): the same index, calls to fold
    if (c.ap->idx != c.idx) return fail(WALT_EINVAL, who + ": the pair table belongs to another index");
    if (!has_calls)
      return fail(WALT_EINVAL, who + ": the pair table is counted from the calls: d_calls must not be NULL when a pair table is given");
  }
  if (c.ep) {  // (include/walt_amd.h, "four-CpG epialleles"): the same index, calls to fold
    if (c.ep->idx != c.idx) return fail(WALT_EINVAL, who + ": the epiallele table belongs to another index");
    if (!has_calls)
      return fail(WALT_EINVAL, who + ": the epiallele table is counted from the calls: d_calls must not be NULL when an epiallele table is given");
  }
  return WALT_OK;
}

// walt_meth_nonconv_batch[_device] on top of that: the rule, somewhere for the verdicts, calls to judge
static int meth_nonconv_check(const MethCall& c, bool has_calls) {
  const std::string who(c.who);
  if (const int rc = meth_call_check(c, has_calls)) return rc;
  const std::string bad = nonconv_refusal(c.rule, c.filt, c.filt_stride);
  if (!bad.empty()) return fail(WALT_EINVAL, who + ": " + bad);
  if (c.n && !c.filt) return fail(WALT_EINVAL, who + ": bad argument (null filt)");
  if (!has_calls)
    return fail(WALT_EINVAL, who + ": the verdict is made from the calls: d_calls must not be NULL");
  return WALT_OK;
}

// c: a checked call whose arrays are on the device.  The calling kernel and, with a bias set (which comes with calls),
// the bias kernel from the calls just written: behind it on the same stream.  Likewise the pair kernel with a pair table,
// the window kernel with an epiallele table and the judging kernel with a rule.  With an evidence object the evidence
// kernel runs right behind the calling kernel, over the same device arrays; alone when nothing else is wanted.
static int meth_launch(const MethCall& c) {
  walt_index* const idx = c.idx;
  if (c.n == 0) return WALT_OK;
  const EvBatch evidence = {c.bases, c.offsets, c.n, c.records, c.record_stride, c.conv, c.conv_stride, c.conversion,
                            c.call_len, c.skip, c.skip_stride, c.quals, c.min_qual};
  if (!c.calls && !c.counts && !c.stats && !c.pile)
    return c.ev ? evidence_launch(c.ev, evidence, reinterpret_cast<hipStream_t>(c.stream)) : WALT_OK;
  WALT_HIP(hipSetDevice(idx->device));
  const hipStream_t stream = reinterpret_cast<hipStream_t>(c.stream);
  MethArgs a;
  a.ref[0] = idx->ref[0]; a.ref[1] = idx->ref[1];
  a.ref_last = ref_words(idx) - 1;
  a.genome_len = idx->head.genome_len;
  a.start_index = idx->view.start_index;
  a.n_chrom = idx->view.n_chrom;
  a.bases = static_cast<const uint8_t*>(c.bases);
  a.offsets = static_cast<const uint64_t*>(c.offsets);
  a.n = c.n;
  a.records = static_cast<const uint8_t*>(c.records);
  a.rec_stride = c.record_stride;
  a.conv = static_cast<const uint8_t*>(c.conv);
  a.conv_stride = c.conv_stride;
  a.conversion = (uint32_t)c.conversion;
  a.call_len = static_cast<const uint32_t*>(c.call_len);
  a.calls = static_cast<uint8_t*>(c.calls);
  a.counts = static_cast<unsigned long long*>(c.counts);
  a.shards = c.stats ? idx->meth_shards : nullptr;
  a.pile[0] = c.pile ? c.pile->plane[0] : nullptr;
  a.pile[1] = c.pile ? c.pile->plane[1] : nullptr;
  a.skip = static_cast<const uint8_t*>(c.skip);
  a.skip_stride = c.skip_stride;
  a.excl = static_cast<const uint32_t*>(c.excl);
  a.trim5 = c.trim5;
  a.trim3 = c.trim3;
  a.quals = static_cast<const uint8_t*>(c.quals);
  a.min_qual = c.min_qual;
  const uint64_t want = ((uint64_t)c.n + kBlock / kMethGroup - 1) / (kBlock / kMethGroup);
  const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)idx->n_cu * 8);
  // [bounds][excl][no pile-up, pile-up, pile_rows]: a call whose bounds are both 0 runs the instances it always ran
  static void (*const kernels[2][2][3])(const MethArgs) = {
      {{k_meth_call, k_meth_pile, k_meth_pile_rows}, {k_meth_call_excl, k_meth_pile_excl, k_meth_pile_rows_excl}},
      {{k_meth_call_trim, k_meth_pile_trim, k_meth_pile_rows_trim},
       {k_meth_call_excl_trim, k_meth_pile_excl_trim, k_meth_pile_rows_excl_trim}}};
  // with qualities: the three instances that carry the interval word and the bounds whether given or not
  static void (*const qual_kernels[3])(const MethArgs) = {k_meth_call_qual, k_meth_pile_qual, k_meth_pile_rows_qual};
  const int by_pile = !c.pile ? 0 : idx->opt.pile_rows ? 2 : 1;
  const auto kernel = a.quals ? qual_kernels[by_pile] : kernels[c.trim5 || c.trim3][a.excl != nullptr][by_pile];
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, a);
  if (c.stats)
    hipLaunchKernelGGL(k_meth_reduce, dim3(1), dim3(kMethTotals), 0, stream, idx->meth_shards,
                       static_cast<unsigned long long*>(c.stats));
  WALT_HIP(hipGetLastError());
  if (c.ev)
    if (const int rc = evidence_launch(c.ev, evidence, stream)) return rc;
  if (c.mb)
    if (const int rc = mbias_launch(c.mb, c.table, {c.calls, c.offsets, c.n, c.records, c.record_stride, c.skip, c.skip_stride}, stream))
      return rc;
  if (c.ap)
    if (const int rc = cpgpairs_launch(c.ap, {c.calls, c.offsets, c.n, c.records, c.record_stride, c.skip, c.skip_stride}, stream))
      return rc;
  if (c.ep)
    if (const int rc = epialleles_launch(c.ep, {c.calls, c.offsets, c.n, c.records, c.record_stride, c.skip, c.skip_stride}, stream))
      return rc;
  if (!c.rule) return WALT_OK;
  return nonconv_launch(idx, {c.calls, c.offsets, c.n, c.records, c.record_stride, *c.rule, c.filt, c.filt_stride, c.tally}, stream);
}

// the six device forms: asynchronous on the caller's stream
static int meth_batch_device(const MethCall& c) {
  const std::string who(c.who);
  if (const int rc = c.rule_form ? meth_nonconv_check(c, c.calls != nullptr) : meth_call_check(c, c.calls != nullptr)) return rc;
  if (c.n && (!c.offsets || !c.records)) return fail(WALT_EINVAL, who + ": bad argument");
  if (((uintptr_t)c.records & 3u) || ((uintptr_t)c.counts & 7u) || ((uintptr_t)c.call_len & 3u) || ((uintptr_t)c.stats & 7u))
    return fail(WALT_EINVAL, who + ": records and call_len must be 4-byte aligned, counts and stats 8-byte aligned");
  if ((uintptr_t)c.tally & 7u) return fail(WALT_EINVAL, who + ": tally must be 8-byte aligned");
  if ((uintptr_t)c.excl & 3u) return fail(WALT_EINVAL, who + ": excl must be 4-byte aligned");
  return meth_launch(c);
}

// The six host forms: the batch into device temporaries of this call (offsets relative to the first read, the
// caller's strided arrays packed: its strides stay on the host), the kernels on the null stream, the results back --
// calls at calls + offsets[0], stats accumulated into.
static int meth_batch_host(const MethCall& c) {
  const std::string who(c.who);
  int rc = c.rule_form ? meth_nonconv_check(c, true) : meth_call_check(c, true);
  if (rc) return rc;
  const uint32_t n = c.n;
  if (n == 0) return WALT_OK;
  const uint64_t* offsets = static_cast<const uint64_t*>(c.offsets);
  const char* bases = static_cast<const char*>(c.bases);
  if (!offsets || !c.records || (!bases && offsets[n] > offsets[0])) return fail(WALT_EINVAL, who + ": bad argument");
  const std::string bad = call_reads_refusal(c.who, offsets, n, static_cast<const uint8_t*>(c.conv), c.conv_stride);
  if (!bad.empty()) return fail(WALT_EINVAL, bad);
  walt_meth_stats* stats = static_cast<walt_meth_stats*>(c.stats);
  if (!c.calls && !c.counts && !stats && !c.pile && !c.mb && !c.rule && !c.ap && !c.ep && !c.ev) return WALT_OK;
  WALT_HIP(hipSetDevice(c.idx->device));
  const uint64_t nbytes = offsets[n] - offsets[0];
  const std::vector<walt_best_match> rec = pack_strided<walt_best_match>(c.records, c.record_stride, n);
  const std::vector<uint8_t> cv = pack_strided<uint8_t>(c.conv, c.conv_stride, c.conv ? n : 0);
  const std::vector<uint8_t> sk = pack_strided<uint8_t>(c.skip, c.skip_stride, c.skip ? n : 0);
  std::vector<uint64_t> rel;
  const uint64_t* off = rebase_offsets(offsets, n, rel);
  const char* const what = "methylation calls";
  DeviceTemp d_bases, d_off, d_rec, d_conv, d_len, d_calls, d_counts, d_stats, d_skip, d_excl, d_filt, d_tally, d_quals;
  if ((rc = d_bases.put(bases + offsets[0], nbytes, what, 16)) || (rc = d_off.put(off, ((size_t)n + 1) * 8, what)) ||
      (rc = d_rec.put(rec.data(), (size_t)n * 16, what)))
    return rc;
  if (c.conv && (rc = d_conv.put(cv.data(), n, what))) return rc;
  if (c.call_len && (rc = d_len.put(c.call_len, (size_t)n * 4, what))) return rc;
  if (c.skip && (rc = d_skip.put(sk.data(), n, what))) return rc;
  if (c.excl && (rc = d_excl.put(c.excl, (size_t)n * 4, what))) return rc;
  if (c.quals && (rc = d_quals.put(static_cast<const char*>(c.quals) + offsets[0], nbytes, what))) return rc;
  if ((c.calls || c.mb || c.rule || c.ap || c.ep) && (rc = d_calls.get(nbytes + 16, what))) return rc;  // (the bias, pair and window tables are counted, the verdict made, from the device copy)
  if (c.rule && (rc = d_filt.get(n, what))) return rc;
  if (c.rule && c.tally && (rc = d_tally.get((size_t)n * sizeof(walt_nonconv_tally), what))) return rc;
  if (c.counts && (rc = d_counts.get((size_t)n * sizeof(walt_meth_counts), what))) return rc;
  if (stats && (rc = d_stats.get(sizeof(walt_meth_stats), what))) return rc;
  if (stats) WALT_HIP(hipMemset(d_stats.p, 0, sizeof(walt_meth_stats)));
  MethCall d = c;  // the same call on the device copies
  d.bases = d_bases.p; d.offsets = d_off.p; d.records = d_rec.p; d.record_stride = 16;
  d.conv = d_conv.p; d.conv_stride = 1; d.call_len = d_len.p;
  d.calls = d_calls.p; d.counts = d_counts.p; d.stats = d_stats.p;
  d.skip = d_skip.p; d.skip_stride = 1; d.excl = d_excl.p; d.stream = nullptr;
  d.filt = d_filt.p; d.filt_stride = 1; d.tally = d_tally.p;
  d.quals = d_quals.p;
  if ((rc = meth_launch(d))) return rc;
  WALT_HIP(hipStreamSynchronize(nullptr));
  if (c.calls && nbytes) WALT_HIP(hipMemcpy(static_cast<char*>(c.calls) + offsets[0], d_calls.p, nbytes, hipMemcpyDeviceToHost));
  if (c.counts) WALT_HIP(hipMemcpy(c.counts, d_counts.p, (size_t)n * sizeof(walt_meth_counts), hipMemcpyDeviceToHost));
  if (c.rule && (rc = nonconv_results(d_filt.p, d_tally.p, n, static_cast<uint8_t*>(c.filt), c.filt_stride,
                                      static_cast<walt_nonconv_tally*>(c.tally))))
    return rc;
  if (stats) {
    walt_meth_stats st;
    WALT_HIP(hipMemcpy(&st, d_stats.p, sizeof(st), hipMemcpyDeviceToHost));
    stats->reads += st.reads;
    for (int i = 0; i < 4; ++i) { stats->meth[i] += st.meth[i]; stats->unmeth[i] += st.unmeth[i]; }
  }
  return WALT_OK;
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_index_enable_reference(walt_index* idx) {
  if (!idx) return fail(WALT_EINVAL, "walt_index_enable_reference: bad argument");
  return build_reference(idx, nullptr);
}

int walt_index_has_reference(const walt_index* idx) { return idx && idx->ref[0] ? 1 : 0; }

int walt_meth_call_batch_device(walt_index* idx, const void* d_bases, const void* d_offsets, uint32_t n,
                                const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                void* stream) {
  return meth_batch_device({.who = "walt_meth_call_batch_device", .idx = idx,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats, .stream = stream});
}

int walt_meth_call_batch(walt_index* idx, const char* bases, const uint64_t* offsets, uint32_t n, const void* records,
                         size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                         const uint32_t* call_len, char* calls, walt_meth_counts* counts, walt_meth_stats* stats) {
  return meth_batch_host({.who = "walt_meth_call_batch", .idx = idx,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats});
}

int walt_meth_pileup_batch_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                  const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                  int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                  void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_device", .pile_required = true, .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats, .stream = stream});
}

int walt_meth_pileup_batch(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                           const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                           const uint32_t* call_len, char* calls, walt_meth_counts* counts, walt_meth_stats* stats) {
  return meth_batch_host({.who = "walt_meth_pileup_batch", .pile_required = true, .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats});
}

// the pile-up forms plus skip (include/walt_amd.h, "duplicates"); here the pile-up may be null: calls only
int walt_meth_pileup_batch_skip_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                       const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                       int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                       const void* d_skip, size_t skip_stride, void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_skip_device", .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats,
                            .skip = d_skip, .skip_stride = skip_stride, .stream = stream});
}

int walt_meth_pileup_batch_skip(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride) {
  return meth_batch_host({.who = "walt_meth_pileup_batch_skip", .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats,
                          .skip = skip, .skip_stride = skip_stride});
}

// the skip forms plus excl (include/walt_amd.h, "overlap of a pair"); the pile-up and skip may be null
int walt_meth_pileup_batch_excl_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                       const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                       int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                       const void* d_skip, size_t skip_stride, const void* d_excl, void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_excl_device", .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats,
                            .skip = d_skip, .skip_stride = skip_stride, .excl = d_excl, .stream = stream});
}

int walt_meth_pileup_batch_excl(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl) {
  return meth_batch_host({.who = "walt_meth_pileup_batch_excl", .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats,
                          .skip = skip, .skip_stride = skip_stride, .excl = excl});
}

// the excl forms plus a bias set (include/walt_amd.h, "methylation bias by read position"); mb null: the excl form
int walt_meth_pileup_batch_mbias_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                        const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                        int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                        const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                        uint32_t table, void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_mbias_device", .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats,
                            .skip = d_skip, .skip_stride = skip_stride, .excl = d_excl, .mb = mb, .table = table, .stream = stream});
}

int walt_meth_pileup_batch_mbias(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                 const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                 int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                 walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                                 walt_mbias* mb, uint32_t table) {
  return meth_batch_host({.who = "walt_meth_pileup_batch_mbias", .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats,
                          .skip = skip, .skip_stride = skip_stride, .excl = excl, .mb = mb, .table = table});
}

// the bias forms plus the ignored read ends of the batch (include/walt_amd.h, "ignored read ends"); both 0: the bias form
int walt_meth_pileup_batch_trim_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                       const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                       int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                       const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                       uint32_t table, uint32_t trim5, uint32_t trim3, void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_trim_device", .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats,
                            .skip = d_skip, .skip_stride = skip_stride, .excl = d_excl, .mb = mb, .table = table,
                            .trim5 = trim5, .trim3 = trim3, .stream = stream});
}

int walt_meth_pileup_batch_trim(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                                walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3) {
  return meth_batch_host({.who = "walt_meth_pileup_batch_trim", .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats,
                          .skip = skip, .skip_stride = skip_stride, .excl = excl, .mb = mb, .table = table,
                          .trim5 = trim5, .trim3 = trim3});
}

// the trim forms plus a pair table (include/walt_amd.h, "adjacent CpG pairs"); ap null: the trim form
int walt_meth_pileup_batch_pairs_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                        const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                        int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                        const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                        uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_pairs_device", .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats,
                            .skip = d_skip, .skip_stride = skip_stride, .excl = d_excl, .mb = mb, .table = table,
                            .trim5 = trim5, .trim3 = trim3, .ap = ap, .stream = stream});
}

int walt_meth_pileup_batch_pairs(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                 const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                 int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                 walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                                 walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap) {
  return meth_batch_host({.who = "walt_meth_pileup_batch_pairs", .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats,
                          .skip = skip, .skip_stride = skip_stride, .excl = excl, .mb = mb, .table = table,
                          .trim5 = trim5, .trim3 = trim3, .ap = ap});
}

// the pairs forms plus an epiallele table (include/walt_amd.h, "four-CpG epialleles"); ep null: the pairs form
int walt_meth_pileup_batch_epi_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                      const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                      int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                      const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                      uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, walt_epialleles* ep,
                                      void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_epi_device", .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats,
                            .skip = d_skip, .skip_stride = skip_stride, .excl = d_excl, .mb = mb, .table = table,
                            .trim5 = trim5, .trim3 = trim3, .ap = ap, .ep = ep, .stream = stream});
}

int walt_meth_pileup_batch_epi(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                               const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                               int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                               walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                               walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap,
                               walt_epialleles* ep) {
  return meth_batch_host({.who = "walt_meth_pileup_batch_epi", .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats,
                          .skip = skip, .skip_stride = skip_stride, .excl = excl, .mb = mb, .table = table,
                          .trim5 = trim5, .trim3 = trim3, .ap = ap, .ep = ep});
}

// the epi forms plus an evidence object (include/walt_amd.h, "opposite-strand evidence"); ev null: the epi form
int walt_meth_pileup_batch_ev_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                     const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                     int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                     const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                     uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, walt_epialleles* ep,
                                     walt_pileup* ev, void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_ev_device", .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats,
                            .skip = d_skip, .skip_stride = skip_stride, .excl = d_excl, .mb = mb, .table = table,
                            .trim5 = trim5, .trim3 = trim3, .ap = ap, .ep = ep, .ev = ev, .stream = stream});
}

int walt_meth_pileup_batch_ev(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                              const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                              int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                              walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                              walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap,
                              walt_epialleles* ep, walt_pileup* ev) {
  return meth_batch_host({.who = "walt_meth_pileup_batch_ev", .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats,
                          .skip = skip, .skip_stride = skip_stride, .excl = excl, .mb = mb, .table = table,
                          .trim5 = trim5, .trim3 = trim3, .ap = ap, .ep = ep, .ev = ev});
}

// the ev forms plus the base qualities and their floor (include/walt_amd.h, "minimum base quality"); quals null: the ev form
int walt_meth_pileup_batch_qual_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                       const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                       int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                       const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                       uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, walt_epialleles* ep,
                                       walt_pileup* ev, const void* d_quals, uint32_t min_qual, void* stream) {
  return meth_batch_device({.who = "walt_meth_pileup_batch_qual_device", .idx = idx, .pile = p,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .counts = d_counts, .stats = d_stats,
                            .skip = d_skip, .skip_stride = skip_stride, .excl = d_excl, .mb = mb, .table = table,
                            .trim5 = trim5, .trim3 = trim3, .ap = ap, .ep = ep, .ev = ev,
                            .quals = d_quals, .min_qual = min_qual, .stream = stream});
}

int walt_meth_pileup_batch_qual(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                                const uint32_t* call_len, char* calls, walt_meth_counts* counts, walt_meth_stats* stats,
                                const uint8_t* skip, size_t skip_stride, const uint32_t* excl, walt_mbias* mb, uint32_t table,
                                uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, walt_epialleles* ep, walt_pileup* ev,
                                const uint8_t* quals, uint32_t min_qual) {
  return meth_batch_host({.who = "walt_meth_pileup_batch_qual", .idx = idx, .pile = p,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .counts = counts, .stats = stats,
                          .skip = skip, .skip_stride = skip_stride, .excl = excl, .mb = mb, .table = table,
                          .trim5 = trim5, .trim3 = trim3, .ap = ap, .ep = ep, .ev = ev,
                          .quals = quals, .min_qual = min_qual});
}

// the evidence kernel alone: the batch as the calling call takes it, nothing written but the evidence
int walt_meth_evidence_batch_device(walt_index* idx, walt_pileup* ev, const void* d_bases, const void* d_offsets, uint32_t n,
                                    const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                    int conversion, const void* d_call_len, const void* d_skip, size_t skip_stride,
                                    void* stream) {
  return meth_batch_device({.who = "walt_meth_evidence_batch_device", .idx = idx,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .skip = d_skip, .skip_stride = skip_stride, .ev = ev, .ev_required = true, .stream = stream});
}

int walt_meth_evidence_batch(walt_index* idx, walt_pileup* ev, const char* bases, const uint64_t* offsets, uint32_t n,
                             const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                             int conversion, const uint32_t* call_len, const uint8_t* skip, size_t skip_stride) {
  return meth_batch_host({.who = "walt_meth_evidence_batch", .idx = idx,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .skip = skip, .skip_stride = skip_stride, .ev = ev, .ev_required = true});
}

// the calling call plus the verdict on its calls (include/walt_amd.h, "non-converted reads"): no pile-up, no statistics
int walt_meth_nonconv_batch_device(walt_index* idx, const void* d_bases, const void* d_offsets, uint32_t n,
                                   const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                   int conversion, const void* d_call_len, void* d_calls, const walt_nonconv_rule* rule,
                                   void* d_filt, size_t filt_stride, void* d_tally, void* stream) {
  return meth_batch_device({.who = "walt_meth_nonconv_batch_device", .idx = idx,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls,
                            .rule_form = true, .rule = rule, .filt = d_filt, .filt_stride = filt_stride, .tally = d_tally,
                            .stream = stream});
}

int walt_meth_nonconv_batch(walt_index* idx, const char* bases, const uint64_t* offsets, uint32_t n, const void* records,
                            size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                            const uint32_t* call_len, char* calls, const walt_nonconv_rule* rule, uint8_t* filt,
                            size_t filt_stride, walt_nonconv_tally* tally) {
  return meth_batch_host({.who = "walt_meth_nonconv_batch", .idx = idx,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls,
                          .rule_form = true, .rule = rule, .filt = filt, .filt_stride = filt_stride, .tally = tally});
}

// walt_meth_nonconv_batch[_device] plus the base qualities and their floor: the verdict is made from the masked calls
int walt_meth_nonconv_batch_qual_device(walt_index* idx, const void* d_bases, const void* d_offsets, uint32_t n,
                                        const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                        int conversion, const void* d_call_len, void* d_calls, const walt_nonconv_rule* rule,
                                        void* d_filt, size_t filt_stride, void* d_tally, const void* d_quals, uint32_t min_qual,
                                        void* stream) {
  return meth_batch_device({.who = "walt_meth_nonconv_batch_qual_device", .idx = idx,
                            .bases = d_bases, .offsets = d_offsets, .n = n, .records = d_records, .record_stride = record_stride,
                            .conv = d_conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = d_call_len,
                            .calls = d_calls, .quals = d_quals, .min_qual = min_qual,
                            .rule_form = true, .rule = rule, .filt = d_filt, .filt_stride = filt_stride, .tally = d_tally,
                            .stream = stream});
}

int walt_meth_nonconv_batch_qual(walt_index* idx, const char* bases, const uint64_t* offsets, uint32_t n, const void* records,
                                 size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                                 const uint32_t* call_len, char* calls, const walt_nonconv_rule* rule, uint8_t* filt,
                                 size_t filt_stride, walt_nonconv_tally* tally, const uint8_t* quals, uint32_t min_qual) {
  return meth_batch_host({.who = "walt_meth_nonconv_batch_qual", .idx = idx,
                          .bases = bases, .offsets = offsets, .n = n, .records = records, .record_stride = record_stride,
                          .conv = conv, .conv_stride = conv_stride, .conversion = conversion, .call_len = call_len,
                          .calls = calls, .quals = quals, .min_qual = min_qual,
                          .rule_form = true, .rule = rule, .filt = filt, .filt_stride = filt_stride, .tally = tally});
}

}  // extern "C"
