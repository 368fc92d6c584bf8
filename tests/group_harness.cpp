// group_harness.cpp -- C entry points (TEST INFRASTRUCTURE) over walt_amd/csrc/group_core.h, what the grouping kernels
// of map_se.hip run: key and bucket of an item header, and the whole grouping of a launch's items on the host -- count
// per bucket, exclusive scan, scatter in item order, then the bucket order cut in slices of 64 places with the
// wavefront's own steps (group_cut_slice).  Compiled with g++ by tests/test_group_cpu.py (no device) and, under the host's sanitizers,
// with tests/group_sanitize_main.cpp.
#include <stdint.h>

#include <vector>

#include "group_core.h"

using namespace walt;

extern "C" {

uint32_t group_harness_buckets() { return kGroupBuckets; }
uint32_t group_harness_slice() { return kGroupSlice; }
uint64_t group_harness_key(uint32_t id, uint32_t rec0) { return group_key(id, rec0); }
uint32_t group_harness_bucket(uint64_t key) { return group_bucket(key); }

// Items 0 .. n-1 by their header words (id, size, rec0) and tail word; units of at most r items.
//   order[n]        the item numbers in bucket order, every slice regrouped
//   unit_first[n], unit_n[n]   the units in the order they are emitted: first place in `order`, items
//   big_first       units whose region exceeds this many candidates are flagged in unit_big[n]
// -> the number of units
uint32_t group_harness_cut(const uint32_t* id, const uint32_t* size, const uint32_t* rec0, const uint32_t* tail, uint32_t n, uint32_t r,
                           uint32_t big_first, uint32_t* order, uint32_t* unit_first, uint32_t* unit_n, uint8_t* unit_big) {
  std::vector<uint32_t> count(kGroupBuckets, 0), cursor(kGroupBuckets, 0);
  for (uint32_t i = 0; i < n; ++i) ++count[group_bucket(group_key(id[i], rec0[i]))];
  uint32_t run = 0;
  for (uint32_t b = 0; b < kGroupBuckets; ++b) {
    cursor[b] = run;
    run += count[b];
  }
  for (uint32_t i = 0; i < n; ++i) order[cursor[group_bucket(group_key(id[i], rec0[i]))]++] = i;
  uint32_t n_units = 0;
  for (uint32_t s = 0; s < n; s += kGroupSlice) {
    const uint32_t m = n - s < kGroupSlice ? n - s : kGroupSlice;
    uint64_t key[kGroupSlice];
    uint32_t sz[kGroupSlice], tl[kGroupSlice], item[kGroupSlice];
    GroupPlace place[kGroupSlice];
    for (uint32_t t = 0; t < m; ++t) {
      item[t] = order[s + t];
      key[t] = group_key(id[item[t]], rec0[item[t]]);
      sz[t] = size[item[t]];
      tl[t] = tail[item[t]];
    }
    group_cut_slice(key, sz, tl, m, r, place);
    for (uint32_t t = 0; t < m; ++t) order[s + place[t].pos] = item[t];
    for (uint32_t t = 0; t < m; ++t)
      if (place[t].leads) {
        unit_first[n_units] = s + place[t].unit_first;
        unit_n[n_units] = place[t].unit_n;
        unit_big[n_units] = sz[t] > big_first ? 1 : 0;
        ++n_units;
      }
  }
  return n_units;
}

}  // extern "C"
