// hostio_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives hio_merge_rows of
// tests/hostio_harness.cpp, and through it hostio::merge_rows of walt_amd/csrc/host/hostio.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/hostio_sanitize_main.cpp tests/hostio_harness.cpp -o hostio_sanitize && ./hostio_sanitize <cases>
// <cases> is the file tests/test_hostio_cpu.py writes from the cases it runs itself, whitespace-separated numbers: the
// number of cases, then per case `kind n_dev`, per device its number of rows and the rows (pos and the kind's counters),
// and the merged rows in the same form.  Every array is a heap block of exactly its entries, so a row read or written
// outside them is reported.  Prints "ok <rows>" and returns 0 when every case gives the merged rows of the file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" int hio_merge_counters(int kind);
extern "C" uint64_t hio_merge_rows(int kind, int n_dev, const uint64_t* n_rows, const uint32_t* pos, const uint64_t* counters,
                                   uint32_t* out_pos, uint64_t* out_counters);

static unsigned long long next(FILE* f) {
  unsigned long long v = 0;
  if (fscanf(f, "%llu", &v) != 1) { printf("the case file ends early\n"); exit(2); }
  return v;
}
template <class T>
static T* block(size_t n) { return static_cast<T*>(malloc(n ? n * sizeof(T) : 1)); }
// `n` rows appended to pos / counters, which are grown to exactly what they hold
static void read_rows(FILE* f, int width, size_t n, size_t& total, uint32_t*& pos, uint64_t*& counters) {
  pos = static_cast<uint32_t*>(realloc(pos, (total + n) ? (total + n) * sizeof(uint32_t) : 1));
  counters = static_cast<uint64_t*>(realloc(counters, (total + n) ? (total + n) * width * sizeof(uint64_t) : 1));
  for (size_t i = total; i < total + n; ++i) {
    pos[i] = (uint32_t)next(f);
    for (int k = 0; k < width; ++k) counters[i * width + k] = next(f);
  }
  total += n;
}

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
  if (!f) { printf("usage: hostio_sanitize <cases>\n"); return 2; }
  const size_t n_cases = next(f);
  unsigned long long rows = 0;
  for (size_t c = 0; c < n_cases; ++c) {
    const int kind = (int)next(f), n_dev = (int)next(f), width = hio_merge_counters(kind);
    uint64_t* n_rows = block<uint64_t>(n_dev);
    uint32_t* pos = nullptr;
    uint64_t* counters = nullptr;
    size_t total = 0;
    for (int d = 0; d < n_dev; ++d) {
      n_rows[d] = next(f);
      read_rows(f, width, n_rows[d], total, pos, counters);
    }
    uint32_t* want_pos = nullptr;
    uint64_t* want_counters = nullptr;
    size_t n_want = 0;
    read_rows(f, width, next(f), n_want, want_pos, want_counters);
    uint32_t* got_pos = block<uint32_t>(total);
    uint64_t* got_counters = block<uint64_t>(total * width);
    const uint64_t n_got = hio_merge_rows(kind, n_dev, n_rows, pos, counters, got_pos, got_counters);
    bool ok = n_got == n_want;
    for (size_t i = 0; ok && i < n_want; ++i) {
      ok = got_pos[i] == want_pos[i];
      for (int k = 0; ok && k < width; ++k) ok = got_counters[i * width + k] == want_counters[i * width + k];
    }
    free(n_rows); free(pos); free(counters); free(want_pos); free(want_counters); free(got_pos); free(got_counters);
    if (!ok) { printf("case %zu (kind %d, %d devices): the merged rows differ\n", c, kind, n_dev); return 1; }
    rows += n_got;
  }
  fclose(f);
  printf("ok %llu rows\n", rows);
  return 0;
}
