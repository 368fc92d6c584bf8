// regions_core.h -- methylation levels per region (include/walt_amd.h, "methylation levels per region"): how a call's
// regions are cut into units of even work and how a unit finds its region again.  Pure inline functions shared by the
// HIP kernels (pileup.hip k_region_sums, k_region_apply, k_pile_regions) and a g++ unit test (tests/test_regions_cpu.py
// compiles tests/regions_harness.cpp).  What a unit does per position is levels_core.h's.
#ifndef WALT_AMD_REGIONS_CORE_H_
#define WALT_AMD_REGIONS_CORE_H_

#include "levels_core.h"

namespace walt {

constexpr uint32_t kRegionUnit = 4096;  // positions of a unit at most (pileup.hip kPileTile)
constexpr uint32_t kRegionRun = 16;     // neighbouring units a wavefront takes at a time at most

// Units of the region [lo, hi): ceil((hi - lo) / kRegionUnit); none for an empty region, and none for one that is not
// inside the genome (lo > hi or hi > genome_len) -- such a region is never walked, and its record stays zero.
WALT_HD uint32_t region_units(uint32_t lo, uint32_t hi, uint32_t genome_len) {
  if (lo > hi || hi > genome_len) return 0u;
  return (uint32_t)(((unsigned long long)(hi - lo) + kRegionUnit - 1ull) / kRegionUnit);
}

// Region of `unit`: the LAST r in [first, n) with prefix[r] <= unit, where prefix[0 .. n] is the exclusive prefix of the
// regions' units (prefix[n] the total) and prefix[first] <= unit < prefix[n].  A region without units shares its
// prefix with its successor; "the last" steps over it, so it is never the answer.
WALT_HD uint32_t region_of_unit(const unsigned long long* prefix, uint32_t first, uint32_t n, unsigned long long unit) {
  uint32_t lo = first, hi = n;  // prefix[lo] <= unit < prefix[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (prefix[mid] <= unit) lo = mid; else hi = mid;
  }
  return lo;
}

// Region of `unit` given the region r of an earlier unit (prefix[r] <= unit < prefix[n]): r itself, the next region,
// or a search behind that one.
WALT_HD uint32_t region_next(const unsigned long long* prefix, uint32_t n, uint32_t r, unsigned long long unit) {
  if (unit < prefix[r + 1u]) return r;
  if (unit < prefix[r + 2u]) return r + 1u;  // (r + 2 <= n: prefix[r + 1] <= unit < prefix[n])
  return region_of_unit(prefix, r + 2u, n, unit);
}

// Positions [u_lo, u_hi) of unit k (0 .. region_units - 1) of the region [lo, hi); the sums stay below 2^32 + 4096.
WALT_HD void region_unit_range(uint32_t lo, uint32_t hi, uint32_t k, unsigned long long& u_lo, unsigned long long& u_hi) {
  u_lo = (unsigned long long)lo + (unsigned long long)k * kRegionUnit;
  u_hi = u_lo + kRegionUnit < hi ? u_lo + kRegionUnit : hi;
}

}  // namespace walt
#endif  // WALT_AMD_REGIONS_CORE_H_
