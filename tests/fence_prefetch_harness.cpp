// fence_prefetch_harness.cpp -- CPU build of the long-slot search whose first fence round takes the keys of its A pivots
// from core.h fence_first_keys (slot_fence_bounds_first below: what the heavy kernels do with the keys that
// map_common.h probe_entries_first fetched beside the directory pair), checked against slot_fence_search and
// std::equal_range.  A program rather than a shared library, so that a build with -fsanitize=address,undefined has the
// sanitizer's runtime as its own; every array is a heap block of EXACTLY its words, so that build reports any key read
// beyond one.  Compiled by tests/test_fence_prefetch_cpu.py:
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I walt_amd/csrc tests/fence_prefetch_harness.cpp
//
//   fence_prefetch_harness SEED   -> exit 0 and one line of counts per class on stdout, or a message and exit 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "core.h"

using namespace walt;

namespace {

struct Arrays {
  uint32_t n = 0;
  Ent* ent = nullptr;
  uint32_t* fen[kFenceLevels] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t fen_keys[kFenceLevels] = {0, 0, 0, 0};
  std::vector<uint64_t> key;  // the same keys, for std::equal_range
};

// sorted keys in runs of equal keys (1 .. 5,000 entries, and one run longer than the longest slot); the steps between
// runs are 2^0 .. 2^44, so keys that differ in their last characters agree in their first ones: every prefix mask sees
// equal runs of its own, from a few entries to whole slots.  The first character of every key is 1, so that an all-zero
// target lies below every key and an all-one target above.
void make_keys(Arrays& A, std::mt19937_64& rng, uint32_t n, uint32_t long_run) {
  A.n = n;
  A.key.resize(n);
  static const uint32_t kRun[] = {1, 1, 1, 1, 2, 3, 5, 20, 300, 5000};
  uint64_t k = 0x4000000000000000ull;
  uint32_t i = 0;
  const uint32_t long_at = n / 3;
  bool long_done = false;
  while (i < n) {
    uint32_t run = kRun[rng() % 10];
    if (!long_done && i >= long_at) { run = long_run; long_done = true; }
    for (uint32_t t = 0; t < run && i < n; ++t) A.key[i++] = k;
    k += 1ull << (rng() % 45);
  }
  A.ent = (Ent*)malloc(sizeof(Ent) * (size_t)n);
  for (uint32_t j = 0; j < n; ++j) { A.ent[j].key_hi = (uint32_t)(A.key[j] >> 32); A.ent[j].key_lo = (uint32_t)A.key[j]; A.ent[j].pos = j; }
  for (uint32_t lv = 0; lv < kFenceLevels; ++lv) {  // device_index.hip k_make_fences: the key of every 16^(lv+1)-th entry
    const uint32_t sh = 4 * (lv + 1), n_k = ((n - 1) >> sh) + 1;
    A.fen_keys[lv] = n_k;
    A.fen[lv] = (uint32_t*)malloc(8 * (size_t)n_k);
    for (uint32_t f = 0; f < n_k; ++f) { A.fen[lv][2 * f] = A.ent[(size_t)f << sh].key_hi; A.fen[lv][2 * f + 1] = A.ent[(size_t)f << sh].key_lo; }
  }
}

// core.h slot_fence_bounds whose first round does not load its A pivots: their keys are first_a[0..3], fetched beforehand
// from the addresses fence_first_keys names.  In that round the two searches share their range, so the four keys serve
// both.  A one-lane model of what the heavy kernels do (map_common.h fence_round_dual<true>, which only the GPU tests
// run): it shows that a search may start from those keys, and the address checks below show which keys they are.
void slot_fence_bounds_first(const StrandView& sv, uint32_t lo, uint32_t hi, uint64_t T, uint64_t M, const uint64_t* first_a,
                                     uint32_t& o1, uint32_t& o2) {
  uint32_t x1 = lo, y1 = hi, x2 = lo, y2 = hi;
  bool first = true;
  while (y1 > x1 || y2 > x2) {
    const FencePlan p1 = fence_plan(sv, x1, y1), p2 = fence_plan(sv, x2, y2);
    uint64_t a1[4], a2[4], b1[4], b2[4];
    for (uint32_t j = 0; j < 4; ++j) {
      a1[j] = first ? first_a[j] : fence_load(fence_ptr(sv, p1, 4 * j + 3, lo));
      a2[j] = first ? first_a[j] : fence_load(fence_ptr(sv, p2, 4 * j + 3, lo));
    }
    first = false;
    const uint32_t q1 = fence_count4(p1, a1, 3, 4, 4, T, M, true), q2 = fence_count4(p2, a2, 3, 4, 4, T, M, false);
    for (uint32_t j = 0; j < 3; ++j) {
      b1[j] = fence_load(fence_ptr(sv, p1, 4 * q1 + j, lo));
      b2[j] = fence_load(fence_ptr(sv, p2, 4 * q2 + j, lo));
    }
    b1[3] = b2[3] = 0;
    fence_narrow(p1, 4 * q1 + fence_count4(p1, b1, 4 * q1, 1, 3, T, M, true), x1, y1);
    fence_narrow(p2, 4 * q2 + fence_count4(p2, b2, 4 * q2, 1, 3, T, M, false), x2, y2);
  }
  o1 = x1; o2 = x2;
}

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  std::mt19937_64 rng(seed);
  Arrays A;
  const uint32_t kHuge = 70003;
  make_keys(A, rng, 260000, 82000);
  StrandView sv{};
  sv.ent = A.ent;
  sv.index_size = A.n;
  for (uint32_t lv = 0; lv < kFenceLevels; ++lv) sv.fen[lv] = A.fen[lv];

  static const uint32_t kSizes[] = {5, 16, 17, 31, 32, 255, 256, 257, 4095, 4097, 8200, kHuge};
  const uint32_t n_sizes = sizeof(kSizes) / sizeof(kSizes[0]);
  // counts per class, printed at the end: the test asserts that none is empty
  uint64_t by_size[2][16] = {}, by_nk[33] = {}, by_target[5] = {}, by_sh[5] = {}, few_pivots = 0, found_n = 0, cases = 0;
  for (uint32_t si = 0; si < n_sizes; ++si) {
    const uint32_t ne = kSizes[si];
    for (uint32_t aligned = 0; aligned < 2; ++aligned) {
      for (uint32_t rep = 0; rep < 3; ++rep) {
        // (rep 2: a slot inside the long equal run -- the equal run that is the whole slot, under every mask)
        uint32_t lo = rep == 2 ? A.n / 3 + 5100 : (uint32_t)(rng() % (A.n - ne));
        lo = aligned ? (lo & ~15u) : (lo | (1u + (uint32_t)(rng() % 7) * 2u));
        if (lo + ne > A.n) lo = aligned ? ((A.n - ne) & ~15u) : (((A.n - ne) & ~15u) - 15u);
        if ((aligned != 0) != ((lo & 15u) == 0)) FAIL("slot alignment: lo %u", lo);
        const uint32_t hi = lo + ne;
        // ---- the addresses: those of the first round of slot_fence_bounds, inside their arrays
        const FencePlan plan = fence_plan(sv, lo, hi);
        const uint32_t* at[4];
        const FencePlan got_plan = fence_first_keys(sv, lo, ne, at);
        if (got_plan.sh != plan.sh || got_plan.first != plan.first || got_plan.m != plan.m) FAIL("plan differs: lo %u ne %u", lo, ne);
        if (plan.m == 0 || plan.m > 16 || (plan.sh & 3u) || plan.sh > 16) FAIL("plan of a slot: lo %u ne %u sh %u m %u", lo, ne, plan.sh, plan.m);
        uint64_t first_a[4];
        for (uint32_t j = 0; j < 4; ++j) {
          if (at[j] != fence_ptr(sv, plan, 4 * j + 3, lo)) FAIL("pivot %u: not the address slot_fence_bounds reads (lo %u ne %u)", j, lo, ne);
          const uint32_t* base = plan.sh ? A.fen[plan.sh / 4 - 1] : reinterpret_cast<const uint32_t*>(A.ent);
          const size_t words = plan.sh ? 2 * (size_t)A.fen_keys[plan.sh / 4 - 1] : 3 * (size_t)A.n;
          if (at[j] < base || at[j] + 2 > base + words) FAIL("pivot %u: key outside its array (lo %u ne %u sh %u)", j, lo, ne, plan.sh);
          // the kernels read 12 bytes there: an entry, or a fence key and the word behind it, which the slack of 32
          // words behind every fence array (device_index.hip) covers
          if (at[j] + 3 > base + words + (plan.sh ? 32 : 0)) FAIL("pivot %u: 12 bytes beyond the array (lo %u ne %u)", j, lo, ne);
          // its pivot is entry (first + min(4j+3, m-1)) << sh, inside the slot
          const uint32_t i = 4 * j + 3 < plan.m ? 4 * j + 3 : plan.m - 1;
          const uint64_t e = ((uint64_t)plan.first + i) << plan.sh;
          if (e < lo || e >= hi) FAIL("pivot %u: entry %llu outside the slot [%u, %u)", j, (unsigned long long)e, lo, hi);
          first_a[j] = fence_load(at[j]);
          if (first_a[j] != A.key[e]) FAIL("pivot %u: key differs from entry %llu's", j, (unsigned long long)e);
        }
        by_sh[plan.sh / 4]++;
        if (plan.sh == 0 && plan.m < 16) ++few_pivots;
        by_size[aligned][si]++;
        // ---- the searches
        for (uint32_t nk = 1; nk <= 32; ++nk) {
          const uint64_t M = key_mask(nk);
          const uint64_t unit = M & (~M + 1);  // lowest bit of the mask
          uint64_t T[6];
          uint32_t cls[6], nt = 0;
          T[nt] = 0; cls[nt++] = 1;                                  // below every key
          T[nt] = M; cls[nt++] = 2;                                  // above every key
          T[nt] = A.key[(uint64_t)(plan.first + (plan.m > 3 ? 3 : plan.m - 1)) << plan.sh] & M; cls[nt++] = 3;  // an A pivot's key
          T[nt] = A.key[lo + rng() % ne] & M; cls[nt++] = 3;         // some entry's key
          T[nt] = A.key[lo] & M; cls[nt++] = 3;                      // the first entry's key (the whole slot when all are equal)
          T[nt] = (A.key[lo + rng() % ne] & M) + unit; cls[nt++] = 0;  // just above an entry's key: absent unless a neighbour holds it
          for (uint32_t t = 0; t < nt; ++t) {
            std::vector<uint64_t>::const_iterator b = A.key.begin() + lo, e = A.key.begin() + hi;
            const uint64_t Tq = T[t];
            const uint32_t r1 = (uint32_t)(std::lower_bound(b, e, Tq, [M](uint64_t k, uint64_t v) { return (k & M) < v; }) - A.key.begin());
            const uint32_t r2 = (uint32_t)(std::upper_bound(b, e, Tq, [M](uint64_t v, uint64_t k) { return v < (k & M); }) - A.key.begin());
            const bool want_found = r2 > r1;
            uint32_t a0 = 0, u0 = 0;
            const bool f0 = slot_fence_search(sv, lo, hi, Tq, M, a0, u0);
            uint32_t x1 = 0, x2 = 0;
            slot_fence_bounds_first(sv, lo, hi, Tq, M, first_a, x1, x2);
            const bool f1 = x2 > x1;
            if (f0 != want_found || f1 != want_found) FAIL("found differs: lo %u ne %u nk %u T %016llx: equal_range %d fence %d prefetched %d", lo, ne, nk, (unsigned long long)Tq, (int)want_found, (int)f0, (int)f1);
            if (x1 != r1 || x2 != r2) FAIL("bounds differ: lo %u ne %u nk %u T %016llx: equal_range [%u, %u) prefetched [%u, %u)", lo, ne, nk, (unsigned long long)Tq, r1, r2, x1, x2);
            if (want_found && (a0 != r1 || u0 != r2 - 1)) FAIL("slot_fence_search differs: lo %u ne %u nk %u", lo, ne, nk);
            ++cases;
            by_nk[nk]++;
            found_n += want_found ? 1 : 0;
            if (cls[t] == 1 && (want_found || r1 != lo)) FAIL("a target below every key was found");
            if (cls[t] == 2 && (want_found || r1 != hi)) FAIL("a target above every key was found");
            if (cls[t] == 1 || cls[t] == 2) by_target[cls[t]]++;
            if (!want_found && r1 > lo && r1 < hi) by_target[0]++;  // absent, inside the slot
            if (want_found) {
              bool spans = false;  // the equal run holds a pivot of the first round and an entry beside it
              for (uint32_t i = 0; i < plan.m; ++i) {
                const uint64_t pe = ((uint64_t)plan.first + i) << plan.sh;
                spans = spans || (pe >= r1 && pe < r2 && r2 - r1 > 1);
              }
              if (spans) by_target[3]++;
              if (r1 == lo && r2 == hi) by_target[4]++;  // the equal run is the whole slot
            }
          }
        }
      }
    }
  }
  printf("cases %llu found %llu few_pivots %llu", (unsigned long long)cases, (unsigned long long)found_n, (unsigned long long)few_pivots);
  for (uint32_t a = 0; a < 2; ++a)
    for (uint32_t si = 0; si < n_sizes; ++si) printf(" size_%u_%s %llu", kSizes[si], a ? "aligned" : "unaligned", (unsigned long long)by_size[a][si]);
  for (uint32_t nk = 1; nk <= 32; ++nk) printf(" nk_%u %llu", nk, (unsigned long long)by_nk[nk]);
  static const char* kTarget[5] = {"absent", "below", "above", "run_over_pivot", "run_is_slot"};
  for (uint32_t t = 0; t < 5; ++t) printf(" target_%s %llu", kTarget[t], (unsigned long long)by_target[t]);
  for (uint32_t s = 0; s < 5; ++s) printf(" sh_%u %llu", 4 * s, (unsigned long long)by_sh[s]);
  printf("\n");
  for (uint32_t lv = 0; lv < kFenceLevels; ++lv) free(A.fen[lv]);
  free(A.ent);
  return 0;
}
