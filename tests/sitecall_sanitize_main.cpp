// sitecall_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/sitecall_harness.cpp, and
// through it walt_amd/csrc/sitecall_core.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -I walt_amd/csrc
//       tests/sitecall_sanitize_main.cpp tests/sitecall_harness.cpp -o sitecall_sanitize && ./sitecall_sanitize
// Random genomes (chromosomes of 1, 2 and 17 bases among them) with counters of every interesting depth (1, 31, 32, 127,
// 128, both counters full); the packed reference, the two planes, the histogram, the table and the records each fill a
// heap block of exactly their size, so a load or an add outside them ends the program.  The histogram and the records of
// random ranges are compared with a plain walk over the genome's text; then the host half: p-values at the edges and at
// large depths, and Benjamini-Hochberg with its table on the histograms just made.  Prints "ok <records>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/walt_amd.h"

extern "C" {
uint32_t sitecall_harness_bin(uint32_t d, uint32_t m);
double sitecall_harness_pval(uint64_t d, uint64_t m, double r);
int sitecall_harness_context(const uint64_t* hist, const uint64_t* deep_d, const uint64_t* deep_m, uint64_t n_deep, double r, double alpha,
                             uint32_t min_depth, uint32_t* min_meth, uint64_t* out, double* cutoff);
uint64_t sitecall_harness_walk(const uint32_t* ref, uint32_t ref_last, const uint32_t* start, uint32_t n_chrom, const uint32_t* meth,
                               const uint32_t* unmeth, uint32_t lo, uint32_t hi, uint64_t* hist, uint64_t* deep, const uint32_t* min_meth,
                               walt_meth_site* sites, uint64_t cap);
}

static uint32_t code_of(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }

// context of forward position f of `text` inside [lo, hi), as include/walt_amd.h words it; -1: no site
static int context_of(const std::vector<char>& text, uint32_t f, uint32_t lo, uint32_t hi) {
  const char b = text[f];
  if (b != 'C' && b != 'G') return -1;
  const long long step = b == 'C' ? 1 : -1;
  const char key = b == 'C' ? 'G' : 'C';
  const long long q1 = (long long)f + step, q2 = (long long)f + 2 * step;
  if (q1 < (long long)lo || q1 >= (long long)hi) return 3;
  if (text[q1] == key) return 0;
  if (q2 < (long long)lo || q2 >= (long long)hi) return 3;
  return text[q2] == key ? 1 : 2;
}

int main() {
  srand(11);
  static const uint32_t chrom_len[] = {700, 1, 2, 17, 1300, 64};
  static const uint32_t pick[] = {0, 0, 0, 1, 1, 2, 15, 16, 30, 31, 32, 63, 64, 126, 127, 128, 1000, 0xFFFFFFFFu};
  uint32_t start[7] = {0};
  for (int c = 0; c < 6; ++c) start[c + 1] = start[c] + chrom_len[c];
  const uint32_t glen = start[6];
  unsigned long long total_records = 0;
  for (int trial = 0; trial < 300; ++trial) {
    std::vector<char> text(glen);
    for (uint32_t i = 0; i < glen; ++i) text[i] = "ACGTCG"[rand() % 6];
    const uint32_t nwords = (glen + 15) / 16, pad = 16;
    uint32_t* ref = static_cast<uint32_t*>(calloc(nwords + pad, 4));  // exactly the words the library keeps
    for (uint32_t i = 0; i < glen; ++i) ref[i >> 4] |= code_of(text[i]) << (2 * (i & 15));
    uint32_t* meth = static_cast<uint32_t*>(calloc(glen, 4));
    uint32_t* unmeth = static_cast<uint32_t*>(calloc(glen, 4));
    for (uint32_t i = 0; i < glen; ++i) { meth[i] = pick[rand() % 18]; unmeth[i] = pick[rand() % 18]; }
    uint64_t* hist = static_cast<uint64_t*>(calloc(4 * (size_t)WALT_SITECALL_BINS, 8));
    uint64_t* deep = static_cast<uint64_t*>(calloc(4, 8));
    uint32_t* table = static_cast<uint32_t*>(malloc(4 * 128 * 4));
    for (uint32_t i = 0; i < 512; ++i) {
      const uint32_t d = i & 127u;
      table[i] = trial % 3 == 0 ? d + 1 : trial % 3 == 1 ? 1u : (uint32_t)(rand() % (d + 2));
    }
    uint32_t lo = (uint32_t)(rand() % (glen + 1)), hi = (uint32_t)(rand() % (glen + 1));
    if (trial % 4 == 0) { lo = 0; hi = glen; }
    if (lo > hi) { const uint32_t t = lo; lo = hi; hi = t; }
    // the count first (no array), then an array of exactly that many records
    const uint64_t n = sitecall_harness_walk(ref, nwords + pad - 1, start, 6, meth, unmeth, lo, hi, hist, deep, table, nullptr, 0);
    walt_meth_site* sites = static_cast<walt_meth_site*>(malloc(n ? n * sizeof(walt_meth_site) : 1));
    const uint64_t n2 = sitecall_harness_walk(ref, nwords + pad - 1, start, 6, meth, unmeth, lo, hi, nullptr, nullptr, table, sites, n);
    // the plain walk
    std::vector<uint64_t> want_hist(4 * (size_t)WALT_SITECALL_BINS, 0), want_deep(4, 0);
    uint64_t k = 0;
    bool same = n2 == n;
    for (uint32_t f = lo; f < hi && same; ++f) {
      if (!(meth[f] | unmeth[f])) continue;
      int c = 0;
      while (f >= start[c + 1]) ++c;
      const int ctx = context_of(text, f, start[c], start[c + 1]);
      if (ctx < 0) continue;
      const uint64_t d = (uint64_t)meth[f] + unmeth[f];
      bool rec = false, is_deep = false;
      if (d <= WALT_SITECALL_DEPTH) {
        want_hist[(size_t)ctx * WALT_SITECALL_BINS + (d - 1) * (d + 2) / 2 + meth[f]] += 1;
        rec = meth[f] >= table[ctx * 128 + d];
      } else {
        want_deep[ctx] += 1;
        rec = is_deep = true;
      }
      if (!rec) continue;
      if (k >= n) { same = false; break; }
      const walt_meth_site& s = sites[k++];
      same = s.pos == f && s.meth == meth[f] && s.unmeth == unmeth[f] && s.strand == (text[f] == 'C' ? '+' : '-') && s.context == ctx &&
             s.reserved == (is_deep ? 1 : 0);
    }
    same = same && k == n && memcmp(hist, want_hist.data(), want_hist.size() * 8) == 0 && memcmp(deep, want_deep.data(), 32) == 0;
    // the host half on this histogram: the table is consistent with the p-values and the cutoff
    for (int c = 0; c < 4 && same && trial % 8 == 0; ++c) {
      const double r = trial % 40 == 0 ? 0.0 : 0.004 * (1 + trial % 7);
      const uint32_t min_depth = trial % 16 ? 1u : 5u;
      std::vector<uint64_t> dd, dm;
      for (uint32_t f = 0; f < glen && dd.size() < 40; ++f)
        if ((uint64_t)meth[f] + unmeth[f] > WALT_SITECALL_DEPTH) { dd.push_back((uint64_t)meth[f] + unmeth[f]); dm.push_back(meth[f]); }
      uint32_t* mm = static_cast<uint32_t*>(malloc(128 * 4));
      uint64_t out[2] = {0, 0};
      double cutoff = 0.0;
      const int has = sitecall_harness_context(hist + (size_t)c * WALT_SITECALL_BINS, dd.data(), dm.data(), dd.size(), r, 0.05, min_depth, mm, out, &cutoff);
      for (uint32_t d = 1; d <= 127 && same; ++d) {
        const uint32_t t = mm[d];
        if (!has || d < min_depth) { same = t == d + 1; continue; }
        same = t >= 1 && t <= d + 1;
        if (same && t <= d) same = sitecall_harness_pval(d, t, r) <= cutoff;
        if (same && t > 1) same = sitecall_harness_pval(d, t - 1, r) > cutoff;
      }
      same = same && out[1] <= out[0];
      free(mm);
    }
    free(ref); free(meth); free(unmeth); free(hist); free(deep); free(table); free(sites);
    if (!same) {
      printf("trial %d: range [%u, %u), %llu records: the walk differs\n", trial, lo, hi, (unsigned long long)n);
      return 1;
    }
    total_records += n;
  }
  // p-values: the edges, and depths a loop over every term would take long for
  bool ok = sitecall_harness_pval(10, 0, 0.01) == 1.0 && sitecall_harness_pval(10, 3, 0.0) == 0.0 && sitecall_harness_pval(1, 1, 0.25) > 0.2499 &&
            sitecall_harness_pval(1, 1, 0.25) < 0.2501 && sitecall_harness_bin(127, 127) == WALT_SITECALL_BINS - 1;
  for (uint64_t d = 1000; d <= 8589934590ull && ok; d *= 97) {
    double last = 1.0;
    for (uint64_t m = 0; m <= d && ok; m += d / 7 + 1) {
      const double p = sitecall_harness_pval(d, m, 0.005);
      ok = p >= 0.0 && p <= last;
      last = p;
    }
  }
  if (!ok) { printf("p-values: an edge value or the order in meth is off\n"); return 1; }
  printf("ok %llu records\n", total_records);
  return 0;
}
