// device_common.h -- the walt_index handle and HIP helpers shared by the .hip
// translation units.
#ifndef WALT_AMD_DEVICE_COMMON_H_
#define WALT_AMD_DEVICE_COMMON_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/walt_amd.h"
#include "batch_host.h"
#include "host_common.h"
#include "index_core.h"

#define WALT_HIP(expr)                                                                       \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return walt::fail(WALT_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

// WALT_HIP once work may be queued on the index's own streams: `unwind` -- a callable in scope that waits for those
// streams -- runs before the error return, so that nothing still uses the caller's workspace when the call is back
#define WALT_HIP_FORKED(expr)                                                                \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      unwind();                                                                              \
      return walt::fail(WALT_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    }                                                                                        \
  } while (0)

// Tuning values and test hooks of the mapping calls (walt_index_set_option; the names: kOptions in device_index.hip, described in include/walt_amd.h).  The mapping calls
// read NO environment variable: an index maps the same way whatever the process environment holds.  None of these
// values can make a call need MORE workspace than walt_se_workspace_bytes / walt_pe_workspace_bytes promise.
struct walt_options {
  // single-end
  int se_pipe = 1;            // the staged heavy pass in two halves on two streams
  long long se_heavy_chunk = 0;  // reads per chunk of the heavy list (0: the default; test hook: several chunks on a small batch)
  int se_lit_side = 1;        // the literal pass on a side stream beside the end of the heavy pass (0: on the call's stream, after it)
  long long se_defer_min = -1;   // long seeds: key-equal ranges of more slots go to the verifier (-1: default, 0: never)
  int se_stage_occ = 0;       // wavefronts per SIMD the stage kernel is built for (0: default)
  int se_carry = 1;           // pass 1 hands its state to the staged rounds (0: they start over at seed 0)
  int se_heavy_mono = 0;      // the one-kernel heavy pass instead of the staged rounds (comparison)
  int se_verify_share = 1;    // dense items of reads up to 128 bases grouped by region, a region streamed once per group (0: once per item)
  int se_share_r = 0;         // se_verify_share = 2 (measurement: groups counted, items verified one by one): items per group at most (0: 4, the verifier's)
  long long se_share_cap = 0; // items of a launch that are grouped (0: all; test hook: the others are verified one by one)
  long long grid = 0;         // blocks of the persistent mapping kernels (0: 8 per compute unit)
  // paired-end
  int pe_mode = 0;            // 0: staged path, 1: list kernels only
  long long pe_chunk = 0;     // pairs per pass (0: default; test hook)
  long long pe_rounds = 0;    // rounds a staged list is taken in (0: default)
  long long pe_stage_cap = 0; // reads of a staged round (0: default; test hook)
  int pe_small_heaps = 0;     // force the 8-slot heaps + overflow list of long literal lists
  int pe_serial = 0;          // mates and pipeline slots one after the other (profiling)
  int pe_push_wide = 0;       // 4-byte heap entries in the push kernel whatever -m is (A/B; 0: 2-byte entries when -m <= 15)
  long long pe_defer_min = -1;
  int pe_lit_fuse = 1;        // the literal round's three seed shifts in one launch when its list is short (0: seed by seed; A/B)
  int pe_roomy = -1;          // -1: decided once per index from the device's free memory
  // methylation pile-up
  int pile_rows = 0;          // the adds with neighbouring lanes on neighbouring positions (meth.hip pile_rows; A/B) instead of lane by slice
  long long pile_extract_blocks = 0;  // blocks of the extraction kernels (0: by the range; test hook: the table does not depend on it)
};

struct walt_index {
  int device = 0;
  int n_cu = 256;              // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  walt_options opt;
  walt::IndexHead head;
  std::vector<uint32_t> start_index;  // n_chrom + 1
  walt::IndexView view;               // device pointers
  std::vector<void*> allocs;          // everything to hipFree
  uint32_t* d_mask_table = nullptr;   // compare_mask_table() on the device
  uint64_t device_bytes = 0;
  uint64_t bad_buckets[4] = {0, 0, 0, 0};
  uint64_t outliers[4] = {0, 0, 0, 0};
  uint32_t* brk[4] = {nullptr, nullptr, nullptr, nullptr};  // index slots of the chromosome-end entries (k_make_ent), for build_windows
  uint32_t n_brk[4] = {0, 0, 0, 0};
  uint32_t window_records[4] = {0, 0, 0, 0};  // index slots with a dense candidate window (core.h StrandView::win)
  uint64_t window_eligible[4] = {0, 0, 0, 0};  // index slots in runs that qualify for one (more than the records when the budget ended first)
  unsigned strand_mask = 0;
  // methylation calling (meth.hip): the unconverted reference, 2 bits per base, per orientation ('+', '-'); null until
  // walt_index_open(WALT_WITH_REFERENCE) / walt_index_enable_reference builds it.  meth_shards: the batch totals' shards
  uint32_t* ref[2] = {nullptr, nullptr};
  unsigned long long* meth_shards = nullptr;
  // measurement hooks (walt_profile_enable / walt_profile_last)
  bool profile = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // before pack, before map, after map
  bool ev_valid = false;
  // walt_profile_detail: events at the boundaries between the kernel groups of the last single-end call (at most
  // kDetailEvents - 1 intervals; kind of the interval that ENDS at event i: 0 pass 1, 1 heavy stages, 2 verifier,
  // 3 literal pass incl. its sort)
  static constexpr int kDetailEvents = 96;
  hipEvent_t ev_detail[kDetailEvents] = {};
  unsigned char ev_kind[kDetailEvents] = {};
  int n_detail = 0;
  std::mutex se_busy;  // one single-end call at a time per index (the streams and events below are the call's)
  hipStream_t se_side = nullptr;  // the literal pass beside the end of the heavy pass (created on first use)
  hipEvent_t se_fork = nullptr, se_join = nullptr;
  // single-end staged heavy pass in two halves (map_se.hip launch_map_se): the second half's stream and the events
  // that order the halves: [0] pass 1 done, [1] the first half's last look-up stage done, [2] second half done
  hipStream_t se_pipe = nullptr;
  hipEvent_t se_pipe_ev[3] = {nullptr, nullptr, nullptr};
  // paired-end (created on first use): two pipeline slots, each with a stream for mate 1 + merge (A, unused in
  // slot 0 of a single-pass call: the caller's stream plays that role) and one for mate 2 (B)
  std::mutex pe_busy;  // one paired-end call at a time per index
  hipStream_t pe_stream[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  hipEvent_t pe_fork[2] = {nullptr, nullptr}, pe_join[2] = {nullptr, nullptr}, pe_done[2] = {nullptr, nullptr};
  hipEvent_t pe_start = nullptr;
  // device buffers of the host-buffer entry points (walt_map_se_batch / walt_map_pe_batch), kept between calls and
  // grown on demand: the reference's driver calls once per -N batch (mapping.cpp:479-517), and a hipMalloc /
  // hipFree pair per buffer and call costs milliseconds each.  One call at a time per index.
  void* host_api_buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t host_api_cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// Per-cytosine pile-up (pileup.hip): two planes of 32-bit counters indexed by forward position -- methylated,
// unmethylated -- and the extraction's table (block offsets, then the totals in its last words).
struct walt_pileup {
  walt_index* idx = nullptr;
  uint32_t* plane[2] = {nullptr, nullptr};
  unsigned long long* table = nullptr;
  uint64_t device_bytes = 0;
};
namespace walt {
constexpr uint32_t kPileMaxBlocks = 65536;     // blocks of an extraction at most
constexpr uint64_t kPileTableBytes = 1u << 20; // block offsets [kPileMaxBlocks + 1], the totals in the last words
constexpr uint32_t kPileTotals = (uint32_t)(kPileTableBytes / 8) - 8;  // n_sites, off-reference meth, unmeth
constexpr uint32_t kPileTile = 4096;           // positions per block the default grid aims at
}  // namespace walt

// Methylation bias by read position (mbias.hip): n_tables x kMbiasReplicas replica tables of 64-bit counters,
// count[4][2][1024] each; a block of the bias kernel flushes into replica blockIdx % kMbiasReplicas of its table.
struct walt_mbias {
  int device = 0;
  int n_cu = 256;
  uint32_t n_tables = 0;
  unsigned long long* tabs = nullptr;
};

// A table keyed by CpG pair number (cpgpairs.hip): one bit per forward position that starts a pair (n_words words, the
// zero padding included), the pairs in front of every block of 128 positions, the table count[n_pairs][columns] and the
// extraction's block offsets.  The two public tables are this with 4 columns (adjacent CpG pairs) and with 16 (four-CpG
// epialleles); each has its own bitmap and directory.
namespace walt {
struct CpgTable {
  walt_index* idx = nullptr;
  uint32_t* bits = nullptr;
  uint32_t* dir = nullptr;
  uint32_t* table = nullptr;
  unsigned long long* scan = nullptr;
  uint64_t n_words = 0;
  uint32_t n_pairs = 0;
  uint64_t device_bytes = 0;
};
}  // namespace walt
struct walt_cpgpairs : walt::CpgTable {};
struct walt_epialleles : walt::CpgTable {};

namespace walt {
// One batch of calls as the kernels that consume calls read it (k_mbias, k_cpg_fold, k_nonconv without the skip bytes):
// device arrays in a launch, the caller's host arrays in calls_host_batch.
struct CallsBatch {
  const void *calls, *offsets;
  uint32_t n;
  const void* records;
  size_t rec_stride;
  const void* skip;  // null: none
  size_t skip_stride;
};
// the same as a kernel takes it: the first member of its argument struct
struct CallsView {
  const uint8_t* calls;
  const uint64_t* offsets;
  uint32_t n;
  const uint8_t* records;
  uint64_t rec_stride;
  const uint8_t* skip;         // null: none
  uint64_t skip_stride;
};
inline CallsView calls_view(const CallsBatch& b) {
  return {static_cast<const uint8_t*>(b.calls), static_cast<const uint64_t*>(b.offsets), b.n, static_cast<const uint8_t*>(b.records),
          b.rec_stride, static_cast<const uint8_t*>(b.skip), b.skip_stride};
}
// mbias.hip: the bias kernel over a batch on `stream`
int mbias_launch(walt_mbias* mb, uint32_t table, const CallsBatch& b, hipStream_t stream);
// cpgpairs.hip: the fold kernel of either table over the same batch on `stream` of the table's index's device
int cpgpairs_launch(walt_cpgpairs* ap, const CallsBatch& b, hipStream_t stream);
int epialleles_launch(walt_epialleles* ep, const CallsBatch& b, hipStream_t stream);

// pileup.hip: k_pile_scan over n_blocks counts at the front of `table` (a pile-up's): the exclusive scan in place, the
// total behind it, in table[kPileTotals] and, when given, at d_total; d_offref (when given): table[kPileTotals + 1 .. 2]
int pile_scan_launch(unsigned long long* table, uint32_t n_blocks, unsigned long long* d_total, unsigned long long* d_offref,
                     hipStream_t stream);

// variants.hip: one batch of reads as the evidence kernel reads it (device arrays; the calling kernel's), and the kernel
// on `stream` of ev's index's device
struct EvBatch {
  const void *bases, *offsets;
  uint32_t n;
  const void* records;
  size_t rec_stride;
  const void* conv;      // null: `conversion` for every read
  size_t conv_stride;
  int conversion;
  const void* call_len;  // null: the whole read
  const void* skip;      // null: none
  size_t skip_stride;
  const void* quals = nullptr;  // null: none; else one byte per base (include/walt_amd.h, "minimum base quality")
  uint32_t min_qual = 0;
};
int evidence_launch(walt_pileup* ev, const EvBatch& b, hipStream_t stream);

// nonconv.hip: one batch of calls as the judging kernel reads it (device arrays; tally null: not wanted), the kernel on
// `stream` of idx's device, what every form refuses of a rule and a filt array (empty: nothing), and the end of a host
// form: the packed device verdicts into the caller's strided bytes, the tallies as they are
struct NonconvBatch {
  const void *calls, *offsets;
  uint32_t n;
  const void* records;
  size_t rec_stride;
  walt_nonconv_rule rule;
  void* filt;
  size_t filt_stride;
  void* tally;
};
int nonconv_launch(const walt_index* idx, const NonconvBatch& b, hipStream_t stream);
std::string nonconv_refusal(const walt_nonconv_rule* rule, const void* filt, size_t filt_stride);
int nonconv_results(const void* d_filt, const void* d_tally, uint32_t n, uint8_t* filt, size_t filt_stride, walt_nonconv_tally* tally);

// A device temporary of one call, freed on every return path.  `what` names the call in the out-of-memory message
// ("methylation calls", "duplicates", ...).  The host forms of the methylation-side calls allocate theirs per call.
struct DeviceTemp {
  void* p = nullptr;
  DeviceTemp() = default;
  DeviceTemp(const DeviceTemp&) = delete;
  DeviceTemp& operator=(const DeviceTemp&) = delete;
  ~DeviceTemp() { if (p) (void)hipFree(p); }
  int get(size_t bytes, const char* what) {  // (a zero-byte request still allocates a byte: p is a device address afterwards)
    return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess ? WALT_OK : fail(WALT_ENOMEM, std::string("hipMalloc failed (") + what + ")");
  }
  // get(bytes + room) and the host array's `bytes` copied in (pageable host memory: done when it returns)
  int put(const void* host, size_t bytes, const char* what, size_t room = 0) {
    if (const int rc = get(bytes + room, what)) return rc;
    if (bytes) WALT_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    return WALT_OK;
  }
};

// What the device forms of the calls consumers refuse of a batch's arrays (`who`: the call).  out: null, or the two
// arrays walt_nonconv_batch_device writes besides, {filt, tally}.
inline int calls_device_check(const std::string& who, const CallsBatch& b, const void* const* out = nullptr) {
  if (b.n && (!b.calls || !b.offsets || !b.records || (out && !out[0])))
    return fail(WALT_EINVAL, who + ": bad argument (null calls, offsets" + (out ? ", records or filt)" : " or records)"));
  if (((uintptr_t)b.records & 3u) || ((uintptr_t)b.offsets & 7u) || (out && ((uintptr_t)out[1] & 7u)))
    return fail(WALT_EINVAL, who + ": records must be 4-byte aligned, offsets " + (out ? "and tally " : "") + "8-byte aligned");
  return WALT_OK;
}

// The host form of a calls consumer after its own refusals: h holds the caller's host arrays (no alignment is asked of
// them; the device copies are aligned).  The calls from the first read's on, the offsets relative to it, the records
// and skip bytes packed as the kernels read them (the caller's strides stay on the host) go to temporaries on `device`;
// launch(device batch) queues the work on the null stream, which is waited for.  any_length: offsets need only be
// non-decreasing (walt_nonconv_batch, which also wants `filt`); else scan_offsets's rule, no read above 1024 calls.
template <class Launch>
inline int calls_host_batch(const std::string& who, const char* what, const CallsBatch& h, bool any_length, const void* filt,
                            int device, Launch&& launch) {
  if (h.n == 0) return WALT_OK;
  const uint64_t* offsets = static_cast<const uint64_t*>(h.offsets);
  const uint32_t n = h.n;
  if (!offsets || !h.records || (any_length && !filt) || (!h.calls && offsets[n] > offsets[0]))
    return fail(WALT_EINVAL, who + ": bad argument (null calls, offsets" + (any_length ? ", records or filt)" : " or records)"));
  if (any_length) {
    for (uint32_t i = 0; i < n; ++i)
      if (offsets[i + 1] < offsets[i]) return fail(WALT_EINVAL, who + ": offsets not non-decreasing");
  } else {
    uint32_t max_len = 0;
    if (const char* bad = scan_offsets(offsets, n, &max_len)) return fail(WALT_EINVAL, who + ": " + bad);
  }
  WALT_HIP(hipSetDevice(device));
  const uint64_t nbytes = offsets[n] - offsets[0];
  const std::vector<walt_best_match> rec = pack_strided<walt_best_match>(h.records, h.rec_stride, n);
  const std::vector<uint8_t> sk = pack_strided<uint8_t>(h.skip, h.skip_stride, h.skip ? n : 0);
  std::vector<uint64_t> rel;
  const uint64_t* off = rebase_offsets(offsets, n, rel);
  DeviceTemp d_calls, d_off, d_rec, d_skip;
  int rc;
  if ((rc = d_calls.put(nbytes ? static_cast<const char*>(h.calls) + offsets[0] : nullptr, nbytes, what)) ||
      (rc = d_off.put(off, ((size_t)n + 1) * 8, what)) || (rc = d_rec.put(rec.data(), (size_t)n * 16, what)) ||
      (h.skip && (rc = d_skip.put(sk.data(), n, what))))
    return rc;
  if ((rc = launch(CallsBatch{d_calls.p, d_off.p, n, d_rec.p, 16, d_skip.p, 1}))) return rc;
  WALT_HIP(hipStreamSynchronize(nullptr));
  return WALT_OK;
}

// what every call over a range of forward positions refuses of its object (a pile-up, a CpgTable: `noun`) and the range
template <class T>
inline int range_refusal(const T* obj, const char* who, const char* noun, uint32_t pos_lo, uint32_t pos_hi) {
  if (!obj) return fail(WALT_EINVAL, std::string(who) + ": bad argument (null " + noun + ")");
  const uint32_t genome_len = obj->idx->head.genome_len;
  if (pos_lo <= pos_hi && pos_hi <= genome_len) return WALT_OK;
  return fail(WALT_EINVAL, std::string(who) + ": range [" + std::to_string(pos_lo) + ", " + std::to_string(pos_hi) +
                               ") is not inside the genome's " + std::to_string(genome_len) + " positions");
}

// The blocks of an extraction over `range` units (positions, bitmap words): option pile_extract_blocks, else one per
// `tile` units up to eight per CU; at least one, at most max_blocks and one per unit.  *chunk: units per block.
inline uint32_t extract_blocks(const walt_index* idx, uint64_t range, uint32_t tile, uint32_t max_blocks, uint64_t* chunk) {
  uint64_t want = idx->opt.pile_extract_blocks ? (uint64_t)idx->opt.pile_extract_blocks
                                               : std::min<uint64_t>((range + tile - 1) / tile, (uint64_t)idx->n_cu * 8);
  want = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(want, max_blocks), std::max<uint64_t>(range, 1)));
  *chunk = (range + want - 1) / want;
  return (uint32_t)want;
}

// grow-only device buffer `slot` of idx (freed by walt_index_close)
inline hipError_t host_api_buffer(walt_index* idx, int slot, size_t bytes, void** out) {
  if (idx->host_api_cap[slot] < bytes) {
    if (idx->host_api_buf[slot]) (void)hipFree(idx->host_api_buf[slot]);
    idx->host_api_buf[slot] = nullptr;
    idx->host_api_cap[slot] = 0;
    const size_t want = bytes + bytes / 8 + 256;
    const hipError_t e = hipMalloc(&idx->host_api_buf[slot], want);
    if (e != hipSuccess) return e;
    idx->host_api_cap[slot] = want;
  }
  *out = idx->host_api_buf[slot];
  return hipSuccess;
}

// One call of a kind (single-end: se_busy, paired-end: pe_busy) at a time per index: its streams, events and host-call
// buffers are the call's.  A second one is refused, never queued (include/walt_amd.h).  A host form takes the lock
// after its argument checks and before its first host_api_buffer, and tells the device implementation it calls that
// the lock is held; a public device form takes it itself.
inline int take_busy(std::unique_lock<std::mutex>& busy, std::mutex& m, const char* entry, const char* kind) {
  busy = std::unique_lock<std::mutex>(m, std::try_to_lock);
  if (busy.owns_lock()) return WALT_OK;
  return fail(WALT_EINVAL, std::string(entry) + ": another " + kind + " call is running on this index (an index is not re-entrant)");
}

// The device side of a host form's arguments: buffers from idx's grow-only slots and the copies into them (pageable
// host memory: the copy is done when hipMemcpy returns).  The first failure sticks in `e` (alloc: it was an
// allocation) and what follows does nothing, so a host form checks once, after its last upload.
struct HostUpload {
  walt_index* idx;
  hipError_t e = hipSuccess;
  bool alloc = false;
  void* buffer(int slot, size_t bytes) {
    void* p = nullptr;
    if (e == hipSuccess && (e = host_api_buffer(idx, slot, bytes, &p)) != hipSuccess) alloc = true;
    return p;
  }
  void* zeroed(int slot, size_t bytes) {
    void* p = buffer(slot, bytes);
    if (e == hipSuccess) e = hipMemset(p, 0, bytes);
    return p;
  }
  // one read set into the slots slot_bases / slot_off: its bases from the first read's on, its offsets relative to that read
  void reads(int slot_bases, int slot_off, const char* bases, const uint64_t* offsets, uint32_t n, void** d_bases, void** d_off) {
    const uint64_t nbytes = offsets[n] - offsets[0];
    const size_t off_bytes = ((size_t)n + 1) * sizeof(uint64_t);
    std::vector<uint64_t> rel;
    const uint64_t* off_src = rebase_offsets(offsets, n, rel);
    *d_bases = buffer(slot_bases, nbytes + 16);
    *d_off = buffer(slot_off, off_bytes);
    if (e == hipSuccess) e = hipMemcpy(*d_bases, bases + offsets[0], nbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(*d_off, off_src, off_bytes, hipMemcpyHostToDevice);
  }
};

// map_se.hip: err[0] / err[1] / err[2] (non-ACGT words / over-long reads / dropped work items) at the start of a workspace
int check_read_errors(const void* d_workspace, hipStream_t stream);

// The end of a host form: what the kernels refused in the reads (check_read_errors waits for the null stream's work),
// then the results -- records, conversion bytes, statistics; one whose host pointer is null is not asked for.
struct HostDownload {
  void* host;
  const void* dev;
  size_t bytes;
};
inline int host_api_finish(const void* d_workspace, std::initializer_list<HostDownload> results) {
  if (const int rc = check_read_errors(d_workspace, nullptr)) return rc;
  for (const HostDownload& r : results) {
    if (!r.host) continue;
    const hipError_t e = hipMemcpy(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(WALT_EHIP, std::string("download failed: ") + hipGetErrorString(e));
  }
  return WALT_OK;
}

// A stream (non-blocking; *priority when given) and its events (timing disabled) for the index: made into locals,
// destroyed again when one of them fails, and handed over only when all exist -- a member that is set says the whole
// set is.
inline hipError_t create_stream_set(hipStream_t* stream, const int* priority, std::initializer_list<hipEvent_t*> events) {
  hipStream_t s = nullptr;
  hipError_t e = priority ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, *priority)
                          : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e != hipSuccess) return e;
  std::vector<hipEvent_t> made;
  while (made.size() < events.size()) {
    hipEvent_t ev = nullptr;
    if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) break;
    made.push_back(ev);
  }
  if (e != hipSuccess) {
    for (hipEvent_t ev : made) (void)hipEventDestroy(ev);
    (void)hipStreamDestroy(s);
    return e;
  }
  *stream = s;
  size_t i = 0;
  for (hipEvent_t* p : events) *p = made[i++];
  return hipSuccess;
}
}  // namespace walt

namespace walt {

constexpr int kBlock = 256;
constexpr uint32_t kG2PadWords = 96;  // slack behind the packed genome for window loads

inline unsigned grid_for(uint64_t n, int block = kBlock) { return (unsigned)((n + block - 1) / block); }
unsigned persistent_grid(const walt_index* idx);  // blocks of the persistent mapping kernels: 8 per compute unit (option grid)

// words per packed read for a maximum read length (template instances 7/8/10/16/32/64)
inline int nw_for_len(uint32_t max_len) {
  if (max_len <= 112) return 7;  // 100 bp reads: 7 words, genome window of exactly two 16-byte loads
  if (max_len <= 128) return 8;
  if (max_len <= 160) return 10;  // 150 bp reads: 10 words instead of 16 keeps three waves per SIMD
  if (max_len <= 256) return 16;
  if (max_len <= 512) return 32;
  if (max_len <= 1024) return 64;
  return 0;
}

// The kernel instance of a word count nw (nw_for_len): f(std::integral_constant<int, NW>()) with NW the instance, so
// that f names it as a template argument.  Patterns 5 / 7 stop at kMaxReadLen = 148 / 152 bases: instances 7, 8, 10.
// WALT_ONLY_NW (development: tools/kernel_resources.sh) builds that one instance only, for quick resource checks.
template <class F>
inline int dispatch_nw(int nw, F&& f) {
#if defined(WALT_ONLY_NW)
  (void)nw;
  return f(std::integral_constant<int, WALT_ONLY_NW>());
#else
  switch (nw) {
    case 7: return f(std::integral_constant<int, 7>());
    case 8: return f(std::integral_constant<int, 8>());
#if WALT_SEEDPATTERN == 3
    case 10: return f(std::integral_constant<int, 10>());
    case 16: return f(std::integral_constant<int, 16>());
    case 32: return f(std::integral_constant<int, 32>());
    default: return f(std::integral_constant<int, 64>());
#else
    default: return f(std::integral_constant<int, 10>());
#endif
  }
#endif
}

constexpr uint32_t kHashSpan = care_pos(kKeyWeight - 1) - care_pos(0);
constexpr int kHashWin = (int)(kHashSpan / 16) + 2;
// the 12 hashed characters (indexed positions keep them inside the genome, reference.cpp:202-203), MSB first
__device__ __forceinline__ uint32_t hash_at_dev(const uint32_t* __restrict__ g2, uint32_t pos) {
  const uint64_t first = (uint64_t)pos + care_pos(0);
  const uint32_t* w = g2 + (first >> 4);
  const uint32_t sh = 2 * (uint32_t)(first & 15);
  uint32_t raw[kHashWin + 1];
#pragma unroll
  for (int i = 0; i <= kHashWin; ++i) raw[i] = w[i];
  uint32_t h = 0;
#pragma unroll
  for (uint32_t p = 0; p < kKeyWeight; ++p) {
    const uint32_t off = care_pos(p) - care_pos(0);
    const uint32_t word = funnel_r(raw[off >> 4], raw[(off >> 4) + 1], sh);
    h = (h << 2) | ((word >> (2 * (off & 15))) & 3u);
  }
  return h;
}

// Care characters [P0, P1) (at most 32) behind genome position pos as makedb's comparator ranks them
// (reference.cpp:271-288): 0 when the character lies at or beyond `room` = chromosome end - pos, else 1 / 2 / 3
// for the strand's three letters in order; one window of genome words, characters at compile-time offsets.
template <uint32_t P0, uint32_t P1>
__device__ __forceinline__ unsigned long long marked_chars_dev(const uint32_t* __restrict__ g2, uint32_t pos,
                                                               uint32_t room) {
  static_assert(P1 > P0 && P1 - P0 <= 32, "at most 32 characters");
  constexpr uint32_t span = care_pos(P1 - 1) - care_pos(P0);
  constexpr int kWin = (int)(span / 16) + 2;
  const uint64_t first = (uint64_t)pos + care_pos(P0);
  const uint32_t* w = g2 + (first >> 4);  // g2 carries kG2PadWords of slack behind the genome
  const uint32_t sh = 2 * (uint32_t)(first & 15);
  uint32_t raw[kWin + 1];
#pragma unroll
  for (int i = 0; i <= kWin; ++i) raw[i] = w[i];
  unsigned long long k = 0;
#pragma unroll
  for (uint32_t p = P0; p < P1; ++p) {
    const uint32_t off = care_pos(p) - care_pos(P0);
    const uint32_t word = funnel_r(raw[off >> 4], raw[(off >> 4) + 1], sh);
    const uint32_t c = (word >> (2 * (off & 15))) & 3u;
    const uint32_t v = care_pos(p) >= room ? 0u : (c == 0 ? 1u : (c == 3 ? 3u : 2u));
    k = (k << 2) | v;
  }
  return k;
}

// Upload + derived-structure build for one strand from DEVICE-resident raw
// arrays (genome bytes, counter, index).  Takes ownership of nothing; the raw
// index/bytes may be freed by the caller afterwards; counter is copied.
int build_strand_device(walt_index* idx, int strand, const uint8_t* d_bytes, const uint32_t* d_counter,
                        const uint32_t* d_index, uint32_t index_size, hipStream_t stream);
int alloc_strand_g2(walt_index* idx, uint32_t** g2_out, hipStream_t stream);
int finish_strand_device(walt_index* idx, int strand, uint32_t* g2, const uint32_t* d_counter,
                         const uint32_t* d_index, uint32_t index_size, hipStream_t stream);
int new_index(int device, const IndexHead& head, int dir_bits, int n_strands, walt_index** out);
int finish_index_device(walt_index* idx);  // start_index, mask table
int choose_dir_bits(uint64_t max_index_size, int requested, int n_strands, uint64_t device_bytes);
// meth.hip: both packed references from the resident strands, the others' genome sections read from
// <dbindex_path>_<strand> (null: all four strands must be resident)
int build_reference(walt_index* idx, const char* dbindex_path);

}  // namespace walt
#endif
