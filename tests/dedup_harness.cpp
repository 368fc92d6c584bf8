// dedup_harness.cpp -- CPU build of what the duplicate kernels run per lane (walt_amd/csrc/dedup_core.h): the keys, and
// a sequential table driven the way dedup.hip drives the device's -- per call an insert pass over all records, then a
// mark pass; the load kept at 1/2 by doubling and moving every slot -- with plain memory operations (DedupSeqOps).
// Compiled by tests/test_dedup_cpu.py:  g++ -O2 -shared -fPIC -I walt_amd/csrc tests/dedup_harness.cpp
#include <stdint.h>
#include <string.h>

#include <vector>

#include "dedup_core.h"

using namespace walt;

namespace {
struct SeqTable {
  std::vector<uint64_t> key, first;
  uint64_t occupied = 0, fed = 0, grown = 0;
  explicit SeqTable(uint64_t slots) : key(dedup_round_slots(slots), kDedupEmpty), first(key.size(), kDedupEmpty) {}
  bool reserve(uint64_t n_more) {
    const uint64_t want = dedup_slots_for(key.size(), occupied + n_more);
    if (want == key.size()) return true;
    std::vector<uint64_t> k2(want, kDedupEmpty), f2(want, kDedupEmpty);
    for (size_t s = 0; s < key.size(); ++s)
      if (key[s] != kDedupEmpty && !dedup_move<DedupSeqOps>(k2.data(), f2.data(), want - 1, key[s], first[s])) return false;
    key.swap(k2);
    first.swap(f2);
    ++grown;
    return true;
  }
};
}  // namespace

extern "C" {

uint64_t dedup_harness_key(uint32_t kind, uint32_t conv, uint32_t strand, uint32_t aux, uint32_t pos) {
  return dedup_key(kind, conv, strand, aux, pos);
}
uint64_t dedup_harness_empty() { return kDedupEmpty; }
uint64_t dedup_harness_hash(uint64_t x) { return dedup_hash(x); }
uint64_t dedup_harness_round_slots(uint64_t want) { return dedup_round_slots(want); }

// -> 1 and *key when the record has a key
int dedup_harness_single(uint32_t pos, uint32_t times, uint32_t strand, uint32_t conv, uint32_t kind, uint64_t* key) {
  return dedup_single_key(pos, times, strand, conv, kind, *key) ? 1 : 0;
}
// keys[2], has[2] of one pair
void dedup_harness_pair(uint32_t pos1, uint32_t times1, uint32_t strand1, uint32_t pos2, uint32_t times2, uint32_t strand2,
                        uint32_t best_times, int32_t frag_len, uint32_t conv1, uint32_t conv2, uint64_t* keys, uint8_t* has) {
  const DedupPairKeys k = dedup_pair_keys(pos1, times1, strand1, pos2, times2, strand2, best_times, frag_len, conv1, conv2);
  keys[0] = k.key[0]; keys[1] = k.key[1];
  has[0] = k.has[0]; has[1] = k.has[1];
}

void* dedup_harness_new(uint64_t slots) { return new SeqTable(slots); }
void dedup_harness_free(void* t) { delete static_cast<SeqTable*>(t); }
uint64_t dedup_harness_slots(void* t) { return static_cast<SeqTable*>(t)->key.size(); }
uint64_t dedup_harness_occupied(void* t) { return static_cast<SeqTable*>(t)->occupied; }
uint64_t dedup_harness_grown(void* t) { return static_cast<SeqTable*>(t)->grown; }

// One call over n records, each with up to two keys (keys[2i], keys[2i + 1]; has[...] says which exist; a pair's two
// mates share one ordinal): insert pass, then mark pass.  dup[2i + k].  -> 0, or -1 when a probe ran through the table.
int dedup_harness_call(void* tv, const uint64_t* keys, const uint8_t* has, uint32_t n, uint8_t* dup) {
  SeqTable& t = *static_cast<SeqTable*>(tv);
  if (!t.reserve(2ull * n)) return -1;
  const uint64_t mask = t.key.size() - 1;
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < 2; ++k) {
      if (!has[2 * i + k] || (k == 1 && has[2 * i] && keys[2 * i] == keys[2 * i + 1])) continue;
      uint32_t fresh = 0;
      if (!dedup_insert<DedupSeqOps>(t.key.data(), t.first.data(), mask, keys[2 * i + k], t.fed + i, fresh)) return -1;
      t.occupied += fresh;
    }
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < 2; ++k)
      dup[2 * i + k] = has[2 * i + k] && dedup_is_dup<DedupSeqOps>(t.key.data(), t.first.data(), mask, keys[2 * i + k], t.fed + i) ? 1 : 0;
  t.fed += n;
  return 0;
}

}  // extern "C"
