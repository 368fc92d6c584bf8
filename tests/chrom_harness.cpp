// chrom_harness.cpp -- CPU build of the chromosome look-up the kernels run per position (walt_amd/csrc/chrom_core.h),
// driven the way the HIP kernels drive it: the table of sampled starts staged word by word (chrom_tab_word), then
// chrom_find over the staged words and the full array.  Both arrays are heap blocks of EXACTLY the words the contract
// names (m + 1 staged words, n_chrom + 1 starts), so that a build with -fsanitize=address,undefined reports any word
// read beyond them.  A program rather than a shared library: the sanitizer's runtime has to be the process's own.
// Compiled by tests/test_chrom_cpu.py:  g++ -O1 -g [-fsanitize=address,undefined] -I walt_amd/csrc tests/chrom_harness.cpp
//
//   chrom_harness IN OUT
//   IN   uint32 n_chrom, n_query; uint32 start[n_chrom + 1]; uint32 pos[n_query]
//   OUT  uint32 shift, m, top; then per query uint32 chr, c_lo, c_hi
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "chrom_core.h"

static bool read_words(FILE* f, uint32_t* p, size_t n) { return fread(p, 4, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  uint32_t head[2];
  if (!read_words(in, head, 2) || !head[0]) return 2;
  const uint32_t n_chrom = head[0], n_query = head[1];
  uint32_t* start = (uint32_t*)malloc(4 * ((size_t)n_chrom + 1));
  uint32_t* pos = (uint32_t*)malloc(4 * ((size_t)n_query + 1));
  if (!start || !pos || !read_words(in, start, (size_t)n_chrom + 1) || !read_words(in, pos, n_query)) return 2;
  fclose(in);

  const walt::ChromTab t = walt::chrom_tab_of(n_chrom);
  if (t.m > walt::kLdsChroms) return 3;  // (the kernels' LDS array has kLdsChroms + 1 words)
  uint32_t* lds = (uint32_t*)malloc(4 * ((size_t)t.m + 1));
  if (!lds) return 2;
  for (uint32_t i = 0; i <= t.m; ++i) lds[i] = start[walt::chrom_tab_word(t, i)];

  uint32_t* out = (uint32_t*)malloc(4 * (3 * (size_t)n_query + 3));
  if (!out) return 2;
  out[0] = t.shift; out[1] = t.m; out[2] = t.top;
  for (uint32_t q = 0; q < n_query; ++q) {
    uint32_t chr = 0xFFFFFFFFu, c_lo = 0xFFFFFFFFu, c_hi = 0xFFFFFFFFu;
    walt::chrom_find(lds, start, t, pos[q], chr, c_lo, c_hi);
    out[3 + 3 * q] = chr; out[4 + 3 * q] = c_lo; out[5 + 3 * q] = c_hi;
    // chrom_bounds is the same look-up without the id
    uint32_t b_lo = 0, b_hi = 0;
    walt::chrom_bounds(lds, start, t, pos[q], b_lo, b_hi);
    if (b_lo != c_lo || b_hi != c_hi) return 4;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(out, 4, 3 * (size_t)n_query + 3, o) != 3 * (size_t)n_query + 3 || fclose(o)) return 2;
  free(out); free(lds); free(pos); free(start);
  return 0;
}
