// sitecall_core.h -- called sites (include/walt_amd.h, "called sites").  Two halves:
//   per lane (HIP kernels of sitecall.hip and the g++ harness): the bin of a (depth, meth) pair and the verdict of a site
//     against the table "smallest significant meth per depth" -- integers only;
//   host only (bin/walt, the harness): the binomial tail, Benjamini-Hochberg over the occupied bins weighted by their
//     counts, and the table a cutoff turns into.
// tests/test_sitecall_cpu.py compiles tests/sitecall_harness.cpp.
#ifndef WALT_AMD_SITECALL_CORE_H_
#define WALT_AMD_SITECALL_CORE_H_

#include <stdint.h>

#if !defined(WALT_HD)  // (core.h's, for a host program that takes this header alone: bin/walt)
#if defined(__HIPCC__)
#define WALT_HD __host__ __device__ __forceinline__
#else
#define WALT_HD inline
#endif
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>

#include <algorithm>
#include <vector>
#endif

namespace walt {

constexpr uint32_t kSiteDepth = 127;                               // WALT_SITECALL_DEPTH
constexpr uint32_t kSiteBins = kSiteDepth * (kSiteDepth + 3) / 2;  // WALT_SITECALL_BINS: 8255
constexpr uint32_t kSiteTable = 4 * (kSiteDepth + 1);              // words of min_meth[4][128]
constexpr uint32_t kSiteLdsDepth = 31;                             // depths a block histograms in LDS (sitecall.hip)
constexpr uint32_t kSiteLdsBins = kSiteLdsDepth * (kSiteLdsDepth + 3) / 2;  // 527: bin(31, 31) + 1
static_assert(kSiteBins == 8255 && kSiteLdsBins == 527, "bin(d, d) + 1 = d * (d + 3) / 2");

// bin(d, m) for 1 <= d <= kSiteDepth, 0 <= m <= d: the bins of depth d follow those of depth d - 1
WALT_HD uint32_t sitecall_bin(uint32_t d, uint32_t m) { return (d - 1u) * (d + 2u) / 2u + m; }

// A site's verdict against min_meth[4][128]: 0 not called, 1 called (reserved 0), 2 deep (reserved 1).  The depth is
// taken in 64 bits: two full counters give 2^33 - 2, which is deep and does not wrap.
enum : uint32_t { kSiteNone = 0, kSiteCalled = 1, kSiteDeep = 2 };
WALT_HD uint32_t sitecall_verdict(const uint32_t* min_meth, uint32_t context, uint32_t m, uint32_t u) {
  const unsigned long long d = (unsigned long long)m + u;
  if (d > kSiteDepth) return kSiteDeep;
  return m >= min_meth[context * (kSiteDepth + 1u) + (uint32_t)d] ? kSiteCalled : kSiteNone;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---------------------------------------------------------------- host only
// log of the binomial probability of k successes out of d at rate r, 0 < r < 1 (lr = log r, l1 = log1p(-r))
inline double sitecall_log_term(double ld1, uint64_t d, uint64_t k, double lr, double l1) {
  return ld1 - lgamma((double)k + 1.0) - lgamma((double)(d - k) + 1.0) + (double)k * lr + (double)(d - k) * l1;
}

// The upper binomial tail P(X >= m | d, r): 1 for m == 0; 0 for r == 0 and m >= 1 (and for m > d); else the sum of the
// terms k = m .. d, clamped to 1.  The terms rise up to the mode and fall behind it, so the sum starts at the larger of
// m and the mode and runs outwards on either side until a term no longer changes it: a deep site costs the width of
// its distribution, not its depth.
inline double sitecall_pval(uint64_t d, uint64_t m, double r) {
  if (m == 0) return 1.0;
  if (m > d || r <= 0.0) return 0.0;
  if (r >= 1.0) return 1.0;
  const double lr = log(r), l1 = log1p(-r), ld1 = lgamma((double)d + 1.0);
  uint64_t mode = (uint64_t)(((double)d + 1.0) * r);
  if (mode > d) mode = d;
  const uint64_t k0 = m > mode ? m : mode;
  double sum = 0.0;
  for (uint64_t k = k0;; ++k) {  // falling terms
    const double before = sum;
    sum += exp(sitecall_log_term(ld1, d, k, lr, l1));
    if (k == d || (sum == before && k > k0)) break;
  }
  for (uint64_t k = k0; k > m;) {  // below the mode, falling towards m
    --k;
    const double before = sum;
    sum += exp(sitecall_log_term(ld1, d, k, lr, l1));
    if (sum == before) break;
  }
  return sum < 1.0 ? sum : 1.0;
}

// Benjamini-Hochberg over groups of tested sites: (p, how many sites have it), in any order; equal p-values are one
// group.  With K_j the cumulative count through group j of the ascending order and n the number tested, group j passes
// when p_j <= K_j * alpha / n; the cutoff is the largest passing p_j.  -> false when no group passes.
struct SitecallGroup {
  double p;
  uint64_t n;
};
inline bool sitecall_bh_cutoff(std::vector<SitecallGroup>& groups, double alpha, uint64_t* tested, double* cutoff) {
  std::sort(groups.begin(), groups.end(), [](const SitecallGroup& a, const SitecallGroup& b) { return a.p < b.p; });
  uint64_t n = 0;
  for (const SitecallGroup& g : groups) n += g.n;
  *tested = n;
  bool any = false;
  uint64_t K = 0;
  for (size_t j = 0; j < groups.size();) {
    size_t e = j;
    while (e < groups.size() && groups[e].p == groups[j].p) K += groups[e++].n;
    if (groups[j].p <= (double)K * alpha / (double)n) { any = true; *cutoff = groups[j].p; }
    j = e;
  }
  return any;
}

// One context.  hist: its kSiteBins counts (the control left out); deep: its deep sites as (d, m) and how many sites have
// that pair (a caller that keeps them one by one sets n = 1).
// Tested: the sites with d >= min_depth.  min_meth[d] (128 words, index 0 unused): the smallest m in 1 .. d with
// pval(d, m, r) <= cutoff, d + 1 where there is none, for d < min_depth and when nothing passes.
struct SitecallDeep {
  uint64_t d, m, n;
};
struct SitecallContext {
  uint64_t tested = 0, called = 0;
  bool has_cutoff = false;
  double cutoff = 0.0;
};
inline SitecallContext sitecall_context(const uint64_t* hist, const SitecallDeep* deep, size_t n_deep, double r, double alpha,
                                        uint32_t min_depth, uint32_t* min_meth) {
  SitecallContext c;
  std::vector<double> pv(kSiteBins, 1.0);  // of every bin at or above min_depth
  std::vector<SitecallGroup> groups;
  for (uint32_t d = min_depth; d <= kSiteDepth; ++d)
    for (uint32_t m = 0; m <= d; ++m) {
      const uint32_t b = sitecall_bin(d, m);
      pv[b] = sitecall_pval(d, m, r);
      if (hist[b]) groups.push_back({pv[b], hist[b]});
    }
  for (size_t i = 0; i < n_deep; ++i) groups.push_back({sitecall_pval(deep[i].d, deep[i].m, r), deep[i].n});  // (deeper than any min_depth)
  if (!groups.empty()) c.has_cutoff = sitecall_bh_cutoff(groups, alpha, &c.tested, &c.cutoff);
  for (uint32_t d = 0; d <= kSiteDepth; ++d) {
    min_meth[d] = d + 1u;
    if (!c.has_cutoff || d < min_depth || d == 0) continue;
    for (uint32_t m = 1; m <= d; ++m)
      if (pv[sitecall_bin(d, m)] <= c.cutoff) { min_meth[d] = m; break; }
    for (uint32_t m = min_meth[d]; m <= d; ++m) c.called += hist[sitecall_bin(d, m)];
  }
  if (c.has_cutoff)
    for (size_t i = 0; i < n_deep; ++i) c.called += sitecall_pval(deep[i].d, deep[i].m, r) <= c.cutoff ? deep[i].n : 0u;
  return c;
}
#endif  // host only

}  // namespace walt
#endif  // WALT_AMD_SITECALL_CORE_H_
