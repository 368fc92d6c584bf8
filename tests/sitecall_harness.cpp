// sitecall_harness.cpp -- CPU build of walt_amd/csrc/sitecall_core.h: the bin and the verdict the kernels of sitecall.hip
// run per lane, driven over a range of forward positions the way the kernels drive them (counters, the packed reference,
// the chromosome's bounds, pile_site's context), and the host's half: the binomial tail, Benjamini-Hochberg and the table.
// Also the pieces of bin/walt -MS that live in host/hostio.h: the value parsers and the two writers.
// Compiled by tests/test_sitecall_cpu.py:  g++ -O2 -fopenmp -shared -fPIC -I walt_amd/csrc tests/sitecall_harness.cpp
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "host/hostio.h"
#include "pileup_core.h"
#include "sitecall_core.h"

extern "C" {

uint32_t sitecall_harness_bin(uint32_t d, uint32_t m) { return walt::sitecall_bin(d, m); }

double sitecall_harness_pval(uint64_t d, uint64_t m, double r) { return walt::sitecall_pval(d, m, r); }

uint32_t sitecall_harness_verdict(const uint32_t* min_meth, uint32_t context, uint32_t m, uint32_t u) {
  return walt::sitecall_verdict(min_meth, context, m, u);
}

// One context: hist its WALT_SITECALL_BINS counts, deep_d / deep_m its n_deep deep sites.  min_meth: 128 words.
// out: tested, called.  -> 1 and *cutoff when a group passed
int sitecall_harness_context(const uint64_t* hist, const uint64_t* deep_d, const uint64_t* deep_m, uint64_t n_deep, double r, double alpha,
                             uint32_t min_depth, uint32_t* min_meth, uint64_t* out, double* cutoff) {
  std::vector<walt::SitecallDeep> deep((size_t)n_deep);
  for (uint64_t i = 0; i < n_deep; ++i) deep[i] = {deep_d[i], deep_m[i], 1};
  const walt::SitecallContext c = walt::sitecall_context(hist, deep.data(), deep.size(), r, alpha, min_depth, min_meth);
  out[0] = c.tested;
  out[1] = c.called;
  *cutoff = c.cutoff;
  return c.has_cutoff ? 1 : 0;
}

// The two passes over the forward positions [lo, hi).  ref: the packed '+' reference, ref_last its last word index; start:
// the n_chrom + 1 chromosome starts; meth / unmeth: the counters, genome_len of each.
//   hist (4 x WALT_SITECALL_BINS) and deep (4), when hist is given: += as walt_pileup_depth_hist counts
//   min_meth (4 x 128) and sites, when min_meth is given: the records of walt_pileup_call_sites, cap of them at most
// -> the records the table gives (written or not)
uint64_t sitecall_harness_walk(const uint32_t* ref, uint32_t ref_last, const uint32_t* start, uint32_t n_chrom, const uint32_t* meth,
                               const uint32_t* unmeth, uint32_t lo, uint32_t hi, uint64_t* hist, uint64_t* deep, const uint32_t* min_meth,
                               walt_meth_site* sites, uint64_t cap) {
  uint64_t n = 0;
  uint32_t chr = 0;
  for (uint32_t f = lo; f < hi; ++f) {
    const uint32_t m = meth[f], u = unmeth[f];
    if (!(m | u)) continue;
    while (chr + 1 < n_chrom && f >= start[chr + 1]) ++chr;
    uint8_t strand = 0, context = 0;
    if (!walt::pile_site(walt::meth_ref_ext(ref, (long long)f - 2, ref_last), f, start[chr], start[chr + 1], strand, context)) continue;
    const unsigned long long d = (unsigned long long)m + u;
    if (hist) {
      if (d <= walt::kSiteDepth) hist[(size_t)context * walt::kSiteBins + walt::sitecall_bin((uint32_t)d, m)] += 1;
      else deep[context] += 1;
    }
    if (min_meth) {
      const uint32_t v = walt::sitecall_verdict(min_meth, context, m, u);
      if (v == walt::kSiteNone) continue;
      if (n < cap) sites[n] = {f, m, u, strand, context, (uint16_t)(v == walt::kSiteDeep ? 1 : 0)};
      ++n;
    }
  }
  return n;
}

// -> 1 and *out when `text` is a value of -MSR (zero_allowed) or -MSA
int sitecall_harness_parse_fraction(const char* text, int zero_allowed, double* out) {
  return hostio::parse_site_fraction(std::string(text), zero_allowed != 0, *out) ? 1 : 0;
}
int sitecall_harness_parse_depth(const char* text, uint32_t* out) { return hostio::parse_site_depth(std::string(text), *out) ? 1 : 0; }

// one line of <out>.methsites; site: a walt_meth_site.  -> its length (copied when it fits)
uint32_t sitecall_harness_line(const char* chrom, uint32_t chrom_start, const void* site, double pval, char* out, uint32_t cap) {
  hostio::Sink s;
  hostio::put_site_line(s, std::string(chrom), chrom_start, *static_cast<const walt_meth_site*>(site), pval);
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}

// one block of <out>.sitestats.  counts: null under -MSR; tested, called, has_cutoff, cutoff: four of each
uint32_t sitecall_harness_block(const char* control, const uint64_t* counts, int has_rate, double rate, double alpha, uint32_t min_depth,
                                const uint64_t* tested, const uint64_t* called, const int* has_cutoff, const double* cutoff, char* out,
                                uint32_t cap) {
  hostio::SiteStatsRow row[4];
  for (int c = 0; c < 4; ++c) row[c] = {tested[c], called[c], has_cutoff[c] != 0, cutoff[c]};
  hostio::Sink s;
  hostio::put_sitestats_block(s, std::string(control), counts, has_rate != 0, rate, alpha, min_depth, row);
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}

}  // extern "C"
