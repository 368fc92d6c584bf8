// epialleles.hip -- four-CpG epialleles on the device (include/walt_amd.h, "four-CpG epialleles"): a table of sixteen
// counters per pair number -- the patterns the four neighbouring CpGs from that pair on showed on one read -- and the
// extraction of the entries with enough reads.  The implementation is cpg_device.h's, the one the pair table has
// (cpgpairs.hip): the fold kernel with EpiFold (epialleles_core.h), a fold with a depth of three calls instead of one,
// and the count / write passes with EpiTab below.  The reference has no such mode; the contract is the header's.
#include <string.h>

#include <hip/hip_runtime.h>

#include "map_common.h"
#include "epialleles_core.h"
#include "cpg_device.h"

namespace walt {

static_assert(sizeof(walt_epiallele_site) == 72, "walt_epiallele_site is 72 bytes");
static_assert(kEpiColumns == 16, "an entry is four 16-byte loads");

struct EpiTab {
  using Handle = walt_epialleles;
  using Fold = EpiFold;
  using Site = walt_epiallele_site;
  static constexpr const char* kNoun = "epiallele table";
  static constexpr const char* kWhat = "four-CpG epialleles";
  struct Entry { uint4 q[4]; };
  // entry j (64 bytes at a 64-byte aligned place); kept: its counters sum to min_total or more
  static __device__ __forceinline__ bool load(const CpgExtract& a, uint32_t j, Entry& e) {
    const uint4* p = reinterpret_cast<const uint4*>(a.table) + 4ull * j;
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e.q[k] = p[k];
      sum += (unsigned long long)e.q[k].x + e.q[k].y + e.q[k].z + e.q[k].w;
    }
    return sum >= a.min_total;
  }
  // c_{j+3} from c_j: three steps along the bitmap (kCpgNoNext when one finds nothing: no entry that a read added to)
  static __device__ __forceinline__ uint32_t window_last(const CpgExtract& a, uint32_t pos) {
#pragma unroll 1
    for (uint32_t k = 0; k < kEpiWindow - 1 && pos != kCpgNoNext; ++k) pos = cpg_next(a.bits, pos, a.n_words);
    return pos;
  }
  static __device__ __forceinline__ void store(const CpgExtract& a, unsigned long long slot, uint32_t pos, const Entry& e) {
    uint2* rec = reinterpret_cast<uint2*>(static_cast<Site*>(a.out) + slot);  // (72-byte records at an 8-byte aligned base)
    rec[0] = make_uint2(pos, window_last(a, pos));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      rec[1 + 2 * k] = make_uint2(e.q[k].x, e.q[k].y);
      rec[2 + 2 * k] = make_uint2(e.q[k].z, e.q[k].w);
    }
  }
};
// (named here so that the instances are this file's whatever calls them)
template __global__ void k_cpg_fold<EpiFold>(const CpgFoldArgs);
template __global__ void k_cpg_count<EpiTab>(const CpgExtract);
template __global__ void k_cpg_write<EpiTab>(const CpgExtract, uint32_t);

int epialleles_launch(walt_epialleles* ep, const CallsBatch& b, hipStream_t stream) { return cpg_fold_launch<EpiFold>(ep, b, stream); }

static int epi_range_check(const walt_epialleles* ep, const char* who, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total) {
  if (const int rc = range_refusal(ep, who, EpiTab::kNoun, pos_lo, pos_hi)) return rc;
  return min_total ? WALT_OK : fail(WALT_EINVAL, std::string(who) + ": min_total must be at least 1");
}

}  // namespace walt

using namespace walt;

extern "C" {

int walt_epialleles_create(walt_index* idx, walt_epialleles** out) { return cpg_table_create<EpiTab>("walt_epialleles_create", idx, out); }
void walt_epialleles_destroy(walt_epialleles* ep) { cpg_table_destroy<EpiTab>(ep); }
int walt_epialleles_clear(walt_epialleles* ep) { return cpg_table_clear<EpiTab>("walt_epialleles_clear", ep); }
uint64_t walt_epialleles_device_bytes(const walt_epialleles* ep) { return ep ? ep->device_bytes : 0; }
uint64_t walt_epialleles_n_pairs(const walt_epialleles* ep) { return ep ? ep->n_pairs : 0; }

int walt_epialleles_batch_device(walt_epialleles* ep, const void* d_calls, const void* d_offsets, uint32_t n, const void* d_records,
                                 size_t record_stride, const void* d_skip, size_t skip_stride, void* stream) {
  return cpg_table_batch_device<EpiTab>("walt_epialleles_batch_device", ep, {d_calls, d_offsets, n, d_records, record_stride, d_skip, skip_stride},
                                        stream);
}

int walt_epialleles_batch(walt_epialleles* ep, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                          size_t record_stride, const uint8_t* skip, size_t skip_stride) {
  return cpg_table_batch<EpiTab>("walt_epialleles_batch", ep, {calls, offsets, n, records, record_stride, skip, skip_stride});
}

int walt_epialleles_extract_device(walt_epialleles* ep, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, void* d_out,
                                   uint64_t cap, void* d_n_out, void* stream) {
  const char* who = "walt_epialleles_extract_device";
  if (const int rc = epi_range_check(ep, who, pos_lo, pos_hi, min_total)) return rc;
  return cpg_table_extract_device<EpiTab>(who, ep, pos_lo, pos_hi, min_total, d_out, cap, d_n_out, stream);
}

int walt_epialleles_extract(walt_epialleles* ep, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, walt_epiallele_site* out,
                            uint64_t cap, uint64_t* n_out) {
  const char* who = "walt_epialleles_extract";
  if (const int rc = epi_range_check(ep, who, pos_lo, pos_hi, min_total)) return rc;
  return cpg_table_extract<EpiTab>(who, ep, pos_lo, pos_hi, min_total, out, cap, n_out);
}

}  // extern "C"
