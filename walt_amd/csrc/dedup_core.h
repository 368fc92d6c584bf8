// dedup_core.h -- PCR-duplicate marking (include/walt_amd.h, "duplicates"): the 64-bit key of a record, which records
// have one, the hash, and the probe sequences of the open-addressing table.  Pure inline functions shared by the HIP
// kernels (dedup.hip) and a g++ unit test (tests/test_dedup_cpu.py compiles tests/dedup_harness.cpp).  The table's
// memory operations come from an Ops policy: atomics on the device (dedup.hip DevOps), plain loads and stores in the
// sequential table of the harness (SeqOps below) -- the probe order and every decision are the same code.
#ifndef WALT_AMD_DEDUP_CORE_H_
#define WALT_AMD_DEDUP_CORE_H_

#include <stdint.h>

#if !defined(WALT_HD)
#if defined(__HIPCC__)
#define WALT_HD __host__ __device__ __forceinline__
#else
#define WALT_HD inline
#endif
#endif

namespace walt {

constexpr uint64_t kDedupEmpty = ~0ull;        // an empty slot of the key plane; also "no ordinal yet" in the first plane
constexpr uint64_t kDedupNoSlot = ~0ull;       // a probe sequence that ran through the whole table
constexpr uint64_t kDedupMinSlots = 64;
constexpr uint32_t kDedupNoPos = 0xFFFFFFFFu;  // a genome_pos that makes a record ineligible (so no key is all ones)
constexpr uint32_t kDedupAuxMask = 0x0FFFFFFFu;
constexpr uint32_t kDedupKindPair = 3;

// bit 63 conv == 'A', 62 strand == '-', 61:60 kind, 59:32 aux (28 bits), 31:0 genome_pos
WALT_HD uint64_t dedup_key(uint32_t kind, uint32_t conv, uint32_t strand, uint32_t aux, uint32_t pos) {
  return ((uint64_t)(conv == 'A') << 63) | ((uint64_t)(strand == '-') << 62) | ((uint64_t)(kind & 3u) << 60) |
         ((uint64_t)(aux & kDedupAuxMask) << 32) | (uint64_t)pos;
}

// 64-bit finaliser (the mixing steps of splitmix64): every input bit reaches every output bit, so keys that differ
// in the position alone -- neighbours on the genome -- spread over the whole table
WALT_HD uint64_t dedup_hash(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// a walt_best_match as a single record of `kind` (0: a single-end read, 1 / 2: a lone mate 1 / mate 2)
WALT_HD bool dedup_single_key(uint32_t pos, uint32_t times, uint32_t strand, uint32_t conv, uint32_t kind, uint64_t& key) {
  const bool ok = times == 1 && pos != kDedupNoPos && (conv == 'T' || conv == 'A');
  key = ok ? dedup_key(kind, conv, strand, 0u, pos) : kDedupEmpty;
  return ok;
}

// The keys of one walt_pair_result: a unique pair has ONE key (kind 3, mate 1's position, strand and conversion, the
// fragment length in aux) that both mates share -- key[0] == key[1], has[0] == has[1] == true; otherwise each mate
// with times == 1 is a single record of kind 1 / 2 under its own conversion.
struct DedupPairKeys {
  uint64_t key[2];
  bool has[2];
};
WALT_HD DedupPairKeys dedup_pair_keys(uint32_t pos1, uint32_t times1, uint32_t strand1, uint32_t pos2, uint32_t times2,
                                      uint32_t strand2, uint32_t best_times, int32_t frag_len, uint32_t conv1, uint32_t conv2) {
  DedupPairKeys k;
  if (best_times == 1) {
    const bool ok = pos1 != kDedupNoPos && (conv1 == 'T' || conv1 == 'A');
    k.key[0] = k.key[1] = ok ? dedup_key(kDedupKindPair, conv1, strand1, (uint32_t)frag_len & kDedupAuxMask, pos1) : kDedupEmpty;
    k.has[0] = k.has[1] = ok;
  } else {
    k.has[0] = dedup_single_key(pos1, times1, strand1, conv1, 1u, k.key[0]);
    k.has[1] = dedup_single_key(pos2, times2, strand2, conv2, 2u, k.key[1]);
  }
  return k;
}
// mate 2's conversion when the caller gives one for mate 1 alone
WALT_HD uint32_t dedup_conv_complement(uint32_t conv) { return conv == 'T' ? 'A' : conv == 'A' ? 'T' : conv; }

// Linear probing from dedup_hash(key) & mask, at most `slots` steps.  Insert: stop at a slot that already holds the key,
// or at an empty one this call took (CAS of the empty word -> key; a lost race is looked at again: the winner may have
// written this very key).  Nobody waits for anybody.  fresh: this call occupied the slot.
template <class Ops>
WALT_HD uint64_t dedup_probe_insert(uint64_t* keys, uint64_t mask, uint64_t key, bool& fresh) {
  fresh = false;
  uint64_t s = dedup_hash(key) & mask;
  for (uint64_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {
    uint64_t cur = Ops::load(keys + s);
    if (cur == kDedupEmpty) {
      cur = Ops::cas(keys + s, kDedupEmpty, key);  // -> what the slot held
      if (cur == kDedupEmpty) { fresh = true; return s; }
    }
    if (cur == key) return s;
  }
  return kDedupNoSlot;
}
// the slot that holds the key; kDedupNoSlot when an empty slot or the whole table came first (the key was never inserted)
template <class Ops>
WALT_HD uint64_t dedup_probe_find(const uint64_t* keys, uint64_t mask, uint64_t key) {
  uint64_t s = dedup_hash(key) & mask;
  for (uint64_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {
    const uint64_t cur = Ops::load(keys + s);
    if (cur == key) return s;
    if (cur == kDedupEmpty) return kDedupNoSlot;
  }
  return kDedupNoSlot;
}
// insert + the ordinal of the first record that produced the key (a minimum: whoever comes first in the schedule, the
// smallest ordinal stays).  -> false: the table is full (the host keeps the load at 1/2: a malformed table)
template <class Ops>
WALT_HD bool dedup_insert(uint64_t* keys, uint64_t* first, uint64_t mask, uint64_t key, uint64_t ordinal, uint32_t& fresh_count) {
  bool fresh;
  const uint64_t s = dedup_probe_insert<Ops>(keys, mask, key, fresh);
  if (s == kDedupNoSlot) return false;
  fresh_count += fresh ? 1u : 0u;
  Ops::min(first + s, ordinal);
  return true;
}
// after the inserts of the call: a duplicate exactly when a smaller ordinal produced the key
template <class Ops>
WALT_HD bool dedup_is_dup(const uint64_t* keys, const uint64_t* first, uint64_t mask, uint64_t key, uint64_t ordinal) {
  const uint64_t s = dedup_probe_find<Ops>(keys, mask, key);
  return s != kDedupNoSlot && Ops::load(first + s) != ordinal;
}
// one old slot into a larger table (keys of the old table are distinct: nobody else writes this key's slot)
template <class Ops>
WALT_HD bool dedup_move(uint64_t* keys, uint64_t* first, uint64_t mask, uint64_t key, uint64_t ordinal) {
  uint32_t fresh = 0;
  return dedup_insert<Ops>(keys, first, mask, key, ordinal, fresh);
}

WALT_HD uint64_t dedup_round_slots(uint64_t want) {
  uint64_t s = kDedupMinSlots;
  while (s < want && s < (1ull << 62)) s <<= 1;
  return s;
}
// the smallest doubling of `slots` that keeps `keys` at a load of at most 1/2
WALT_HD uint64_t dedup_slots_for(uint64_t slots, uint64_t keys) {
  while (keys > slots / 2 && slots < (1ull << 62)) slots <<= 1;
  return slots;
}

// the table's memory operations without concurrency (the g++ harness; the host never touches the device's table)
struct DedupSeqOps {
  static inline uint64_t load(const uint64_t* p) { return *p; }
  static inline uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
    const uint64_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  static inline void min(uint64_t* p, uint64_t v) { if (v < *p) *p = v; }
};

}  // namespace walt
#endif  // WALT_AMD_DEDUP_CORE_H_
