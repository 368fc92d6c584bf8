// group_core.h -- grouping the dense work items of a verifier launch by the region they name (map_se.hip, the
// launches between a round's stage kernel and its dense verifier).  An item is one (read, probe) pair and names a
// region by (strand, first dense record, size) (map_items.h, quad 0); reads whose seeds have the same key name the
// same region.  The items are binned by a hash of (strand, record) and every bin is cut into UNITS: items of equal
// key AND equal size, at most R of them, which one wavefront may evaluate together against records streamed once.
// Pure inline functions shared by the HIP kernels and a g++ unit test (tests/test_group_cpu.py compiles
// tests/group_harness.cpp): the key, the bucket, which lanes join a leader, and where a lane of a set of equal
// items goes.  In bucket order equal keys lie next to each other; a wavefront cuts 64 places of that order (one SLICE)
// at a time, whatever buckets they belong to: the lanes that equal the first lane not yet placed are found by one
// ballot, placed behind what has been placed, and cut into units by their rank; a run that crosses a slice border is
// cut there.  group_cut_slice below is that loop lane by lane, for the host.
#ifndef WALT_AMD_GROUP_CORE_H_
#define WALT_AMD_GROUP_CORE_H_

#include <stdint.h>

#if !defined(WALT_HD)
#if defined(__HIPCC__)
#define WALT_HD __host__ __device__ __forceinline__
#else
#define WALT_HD inline
#endif
#endif

namespace walt {

constexpr uint32_t kGroupBucketBits = 16;
constexpr uint32_t kGroupBuckets = 1u << kGroupBucketBits;
constexpr uint32_t kGroupSlice = 64;  // items cut at a time: one per lane
constexpr uint32_t kGroupRMax = kGroupSlice;

// strand(id) << 32 | rec0 (id: chunk position | strand << 31, map_se.hip SummarySink)
WALT_HD uint64_t group_key(uint32_t id, uint32_t rec0) { return ((uint64_t)(id >> 31) << 32) | rec0; }

WALT_HD uint32_t group_bucket(uint64_t key) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - kGroupBucketBits));
}

// does an item join the unit run of a leader?  Equal key and equal size, and neither is a tail item (tail != 0:
// the region is a key-equal range the verifier tests and counts per read -- always a unit of one)
WALT_HD bool group_joins(uint64_t key, uint32_t size, uint32_t tail, uint64_t lead_key, uint32_t lead_size, uint32_t lead_tail) {
  return tail == 0 && lead_tail == 0 && key == lead_key && size == lead_size;
}

struct GroupPlace {
  uint32_t pos;         // the item's new place in its slice
  uint32_t unit_first;  // place of its unit's first item
  uint32_t unit_n;      // items of its unit
  bool leads;           // the item is its unit's first
};
WALT_HD uint32_t group_popc(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(m);
#else
  return (uint32_t)__builtin_popcountll(m);
#endif
}
// lane `lane` of the set `m` (lanes of one slice that hold equal items), `placed` items of the slice placed before
// the set, units of at most r items (1 <= r)
WALT_HD GroupPlace group_place(unsigned long long m, uint32_t lane, uint32_t placed, uint32_t r) {
  const uint32_t rank = group_popc(m & ((1ull << lane) - 1ull)), n = group_popc(m);
  const uint32_t first = rank / r * r;
  GroupPlace p;
  p.pos = placed + rank;
  p.unit_first = placed + first;
  p.unit_n = n - first < r ? n - first : r;
  p.leads = rank == first;
  return p;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One slice of n <= kGroupSlice items as a wavefront cuts it (map_se.hip k_se_share_cut), lane by lane: place[t] for
// the item in lane t.
inline void group_cut_slice(const uint64_t* key, const uint32_t* size, const uint32_t* tail, uint32_t n, uint32_t r, GroupPlace* place) {
  unsigned long long rem = n >= 64 ? ~0ull : (1ull << n) - 1ull;
  uint32_t placed = 0;
  while (rem) {
    const uint32_t ld = (uint32_t)__builtin_ctzll(rem);
    unsigned long long m = 0;
    for (uint32_t t = 0; t < n; ++t)
      if (t == ld || group_joins(key[t], size[t], tail[t], key[ld], size[ld], tail[ld])) m |= 1ull << t;
    m &= rem;
    for (uint32_t t = 0; t < n; ++t)
      if ((m >> t) & 1ull) place[t] = group_place(m, t, placed, r);
    placed += group_popc(m);
    rem &= ~m;
  }
}
#endif

}  // namespace walt
#endif  // WALT_AMD_GROUP_CORE_H_
