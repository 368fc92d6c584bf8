// batch_host_harness.cpp -- CPU build of what the host-buffer mapping calls do with a caller's offsets array
// (walt_amd/csrc/batch_host.h: scan_offsets, rebase_offsets), driven the way a call drives it: the read sets of one
// call (one for a single-end call, two mates for a paired one) are scanned in order into ONE running maximum, the
// first refusal ends the call, and every accepted set is rebased.  Each offsets array is a heap block of EXACTLY
// n + 1 words, so that a build with -fsanitize=address,undefined reports any word read beyond it.  A program rather
// than a shared library: the sanitizer's runtime has to be the process's own.
// Compiled by tests/test_batch_host_cpu.py:  g++ -O1 -g [-fsanitize=address,undefined] -I walt_amd/csrc tests/batch_host_harness.cpp
//
//   batch_host_harness IN OUT
//   IN   uint64 n_sets; per set: uint64 n, uint64 offsets[n + 1]
//   OUT  per set, one text line:  <message, or "ok">\t<running max_len>\t<1: the caller's own array came back, else 0>\t<n + 1 rebased offsets>
//        (no line after a refused set; a refused set has no third and fourth field)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "batch_host.h"

static bool read_words(FILE* f, uint64_t* p, size_t n) { return fread(p, 8, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 2;
  uint64_t n_sets = 0;
  if (!read_words(in, &n_sets, 1)) return 2;
  uint32_t max_len = 0;
  for (uint64_t s = 0; s < n_sets; ++s) {
    uint64_t n64 = 0;
    if (!read_words(in, &n64, 1) || n64 > 0xFFFFFFFFull) return 2;
    const uint32_t n = (uint32_t)n64;
    uint64_t* offsets = (uint64_t*)malloc(8 * ((size_t)n + 1));
    if (!offsets || !read_words(in, offsets, (size_t)n + 1)) return 2;
    const char* bad = walt::scan_offsets(offsets, n, &max_len);
    if (bad) {
      fprintf(out, "%s\t%u\n", bad, max_len);
      free(offsets);
      break;
    }
    std::vector<uint64_t> rel;
    const uint64_t* r = walt::rebase_offsets(offsets, n, rel);
    if (r != offsets && (r != rel.data() || rel.size() != (size_t)n + 1)) return 3;
    fprintf(out, "ok\t%u\t%d\t", max_len, r == offsets ? 1 : 0);
    for (uint32_t i = 0; i <= n; ++i) fprintf(out, "%s%llu", i ? " " : "", (unsigned long long)r[i]);
    fprintf(out, "\n");
    free(offsets);
  }
  fclose(in);
  return fclose(out) ? 2 : 0;
}
