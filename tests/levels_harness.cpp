// levels_harness.cpp -- CPU build of what the summary kernel runs per lane (walt_amd/csrc/levels_core.h on top of
// pileup_core.h) and of the <out>.levels writer (walt_amd/csrc/host/hostio.h put_levels_block).
// Compiled by tests/test_levels_cpu.py:  g++ -O2 -I walt_amd/csrc tests/levels_harness.cpp, as a shared object, and as
// a stand-alone program (-DLEVELS_HARNESS_MAIN, with host sanitizers) that walks a small genome by itself.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define HOSTIO_ALLOC(bytes, out) ((*(out) = malloc(bytes)) ? 0 : -5)
#define HOSTIO_FREE(p) free(p)
#define HOSTIO_ALLOC_ERROR() "malloc failed"
#include "host/hostio.h"
#include "levels_core.h"

extern "C" {

// Class (0..3, 4: no site) and pair flag of every forward position of the genome; ref: the packed '+' reference,
// start: the n_chrom + 1 chromosome starts.
void levels_harness_classes(const uint32_t* ref, uint32_t ref_last, const uint32_t* start, uint32_t n_chrom, uint8_t* cls,
                            uint8_t* pair) {
  for (uint32_t c = 0; c < n_chrom; ++c)
    for (uint32_t f = start[c]; f < start[c + 1]; ++f) {
      const unsigned long long ext = walt::meth_ref_ext(ref, (long long)f - 2, ref_last);
      cls[f] = (uint8_t)walt::levels_class(ext, f, start[c], start[c + 1]);
      pair[f] = walt::levels_pair(ext, f, start[c + 1]) ? 1 : 0;
    }
}

uint64_t levels_harness_q30(uint64_t m, uint64_t u) { return walt::level_q30(m, u); }
uint32_t levels_harness_bin(uint64_t m, uint64_t u) { return walt::level_bin(m, u); }

// The whole summary of [pos_lo, pos_hi) the way the kernel composes it, one position at a time.
void levels_harness_summary(const uint32_t* ref, uint32_t ref_last, const uint32_t* start, uint32_t n_chrom, const uint32_t* meth,
                            const uint32_t* unmeth, uint32_t pos_lo, uint32_t pos_hi, walt_levels* out) {
  memset(out, 0, sizeof *out);
  auto take = [&](walt_level_row& row, unsigned long long m, unsigned long long u) {
    row.sites += 1;
    if (!(m + u)) return;
    row.covered += 1;
    row.meth += m; row.unmeth += u;
    row.max_depth = row.max_depth > m + u ? row.max_depth : m + u;
    const unsigned long long q = walt::level_q30(m, u);
    row.level_sum += q;
    row.hist[walt::level_bin_of(m, u, q)] += 1;
  };
  for (uint32_t c = 0; c < n_chrom; ++c)
    for (uint32_t f = start[c]; f < start[c + 1]; ++f) {
      if (f < pos_lo || f >= pos_hi) continue;
      const unsigned long long ext = walt::meth_ref_ext(ref, (long long)f - 2, ref_last);
      const uint32_t cls = walt::levels_class(ext, f, start[c], start[c + 1]);
      if (cls == walt::kLevelNone) { out->offref[0] += meth[f]; out->offref[1] += unmeth[f]; }
      else take(out->row[cls], meth[f], unmeth[f]);
      if (walt::levels_pair(ext, f, start[c + 1]))
        take(out->row[walt::kLevelPair], (unsigned long long)meth[f] + meth[f + 1], (unsigned long long)unmeth[f] + unmeth[f + 1]);
    }
}

// <out>.levels' block of one walt_levels -> buf (cap bytes); returns its length, or -1 when it does not fit
int levels_harness_text(const walt_levels* lv, char* buf, int cap) {
  hostio::Sink s;
  hostio::put_levels_block(s, *lv);
  if ((int)s.n > cap) return -1;
  memcpy(buf, s.p, s.n);
  return (int)s.n;
}

}  // extern "C"

#ifdef LEVELS_HARNESS_MAIN
// A fixed pseudo-random genome with chromosomes of 1, 2, 3 and 17 bases among longer ones and counters at 0, 1 and
// 0xFFFFFFFF: every function above runs over it once; the sums are printed for the test to compare.
int main() {
  const uint32_t lengths[] = {1, 2, 3, 17, 300, 1, 64, 257};
  const uint32_t n_chrom = sizeof lengths / sizeof lengths[0];
  uint32_t start[n_chrom + 1];
  start[0] = 0;
  for (uint32_t c = 0; c < n_chrom; ++c) start[c + 1] = start[c] + lengths[c];
  const uint32_t glen = start[n_chrom], words = (glen + 15) / 16 + 16;
  uint32_t* ref = (uint32_t*)calloc(words, 4);
  uint32_t* meth = (uint32_t*)calloc(glen, 4);
  uint32_t* unmeth = (uint32_t*)calloc(glen, 4);
  uint8_t* cls = (uint8_t*)malloc(glen);
  uint8_t* pair = (uint8_t*)malloc(glen);
  uint64_t x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  static const uint32_t pick[3] = {0u, 1u, 0xFFFFFFFFu};
  for (uint32_t f = 0; f < glen; ++f) {
    const uint32_t code = (uint32_t)(rnd() % 6);  // C / G rich: A C G T C G
    ref[f >> 4] |= (code < 4 ? code : code - 3) << (2 * (f & 15));
    meth[f] = pick[rnd() % 3];
    unmeth[f] = pick[rnd() % 3];
  }
  levels_harness_classes(ref, words - 1, start, n_chrom, cls, pair);
  walt_levels whole, a, b;
  levels_harness_summary(ref, words - 1, start, n_chrom, meth, unmeth, 0, glen, &whole);
  levels_harness_summary(ref, words - 1, start, n_chrom, meth, unmeth, 0, glen / 2, &a);
  levels_harness_summary(ref, words - 1, start, n_chrom, meth, unmeth, glen / 2, glen, &b);
  int bad = 0;
  for (int r = 0; r < 5; ++r) {
    bad += whole.row[r].sites != a.row[r].sites + b.row[r].sites;
    bad += whole.row[r].level_sum != a.row[r].level_sum + b.row[r].level_sum;
    bad += whole.row[r].max_depth != (a.row[r].max_depth > b.row[r].max_depth ? a.row[r].max_depth : b.row[r].max_depth);
  }
  char text[4096];
  const int n = levels_harness_text(&whole, text, (int)sizeof text);
  uint32_t n_pair = 0;
  for (uint32_t f = 0; f < glen; ++f) n_pair += pair[f];
  bad += n < 0 || n_pair != whole.row[4].sites;
  printf("positions %u pairs %u bytes %d bad %d\n", glen, n_pair, n, bad);
  free(ref); free(meth); free(unmeth); free(cls); free(pair);
  return bad ? 1 : 0;
}
#endif
