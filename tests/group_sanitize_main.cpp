// group_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/group_harness.cpp, and
// through it walt_amd/csrc/group_core.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I walt_amd/csrc \
//       tests/group_sanitize_main.cpp tests/group_harness.cpp -o group_sanitize && ./group_sanitize
// Random launches of 0 .. 700 items over few or many regions; every array is a heap block of exactly n entries, so a
// place or a unit written outside them is reported.  Every result is checked: each item in exactly one unit, no unit
// of more than r items, of mixed keys or sizes, or with a tail item beside another.  Prints "ok <units>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" uint32_t group_harness_cut(const uint32_t* id, const uint32_t* size, const uint32_t* rec0, const uint32_t* tail, uint32_t n,
                                      uint32_t r, uint32_t big_first, uint32_t* order, uint32_t* unit_first, uint32_t* unit_n,
                                      uint8_t* unit_big);

int main() {
  srand(11);
  static const uint32_t ns[] = {0, 1, 2, 63, 64, 65, 130, 700}, rs[] = {1, 2, 4, 8, 64};
  long long total = 0;
  for (int trial = 0; trial < 3000; ++trial) {
    const uint32_t n = ns[rand() % 8], r = rs[rand() % 5], n_regions = 1 + rand() % (trial % 3 ? 4 : 200);
    std::vector<uint32_t> rrec(n_regions), rsize(n_regions);
    for (uint32_t k = 0; k < n_regions; ++k) {
      rrec[k] = trial % 5 ? (uint32_t)rand() : 0xFFFFFFFFu - (uint32_t)(rand() % 3);  // also the largest record numbers
      rsize[k] = 17 + rand() % 5000;
    }
    uint32_t* id = static_cast<uint32_t*>(malloc(n ? n * 4 : 1));
    uint32_t* size = static_cast<uint32_t*>(malloc(n ? n * 4 : 1));
    uint32_t* rec0 = static_cast<uint32_t*>(malloc(n ? n * 4 : 1));
    uint32_t* tail = static_cast<uint32_t*>(malloc(n ? n * 4 : 1));
    uint32_t* order = static_cast<uint32_t*>(malloc(n ? n * 4 : 1));
    uint32_t* ufirst = static_cast<uint32_t*>(malloc(n ? n * 4 : 1));
    uint32_t* un = static_cast<uint32_t*>(malloc(n ? n * 4 : 1));
    uint8_t* ubig = static_cast<uint8_t*>(malloc(n ? n : 1));
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t k = rand() % n_regions;
      id[i] = (uint32_t)(rand() & 0xFFFFF) | ((uint32_t)(rand() & 1) << 31);
      rec0[i] = rrec[k];
      size[i] = rsize[k] + (rand() % 10 == 0);
      tail[i] = rand() % 20 == 0 ? 1 + rand() % 2 : 0;
    }
    const uint32_t units = group_harness_cut(id, size, rec0, tail, n, r, 1024, order, ufirst, un, ubig);
    std::vector<uint32_t> seen(n, 0), item_seen(n, 0);
    bool ok = units <= n;
    for (uint32_t i = 0; ok && i < n; ++i) {
      ok = order[i] < n;
      if (ok) ++item_seen[order[i]];
    }
    for (uint32_t u = 0; ok && u < units; ++u) {
      ok = un[u] >= 1 && un[u] <= r && ufirst[u] < n && un[u] <= n - ufirst[u];
      if (!ok) break;
      const uint32_t a = order[ufirst[u]];
      for (uint32_t p = ufirst[u]; p < ufirst[u] + un[u]; ++p) {
        const uint32_t b = order[p];
        ++seen[p];
        ok = ok && (id[a] >> 31) == (id[b] >> 31) && rec0[a] == rec0[b] && size[a] == size[b] && (un[u] == 1 || tail[b] == 0);
      }
      ok = ok && ubig[u] == (size[a] > 1024 ? 1 : 0);
    }
    for (uint32_t i = 0; ok && i < n; ++i) ok = seen[i] == 1 && item_seen[i] == 1;
    free(id); free(size); free(rec0); free(tail); free(order); free(ufirst); free(un); free(ubig);
    if (!ok) {
      printf("trial %d (n = %u, r = %u): the units are no partition of the items into runs of equal key and size\n", trial, n, r);
      return 1;
    }
    total += units;
  }
  printf("ok %lld units\n", total);
  return 0;
}
