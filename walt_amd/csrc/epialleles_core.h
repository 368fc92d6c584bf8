// epialleles_core.h -- four-CpG epialleles (include/walt_amd.h, "four-CpG epialleles"): the chain of neighbouring calls
// that ends a stretch of a read, how two stretches meet, the fold of one 16-byte slice of calls and the windows that
// straddle a slice's left boundary.  Pure inline functions shared by the HIP kernel (epialleles.hip) and a g++ unit test
// (tests/test_epialleles_cpu.py compiles tests/epialleles_harness.cpp).  Pairs, ranks, slices and trips are
// cpgpairs_core.h's.
#ifndef WALT_AMD_EPIALLELES_CORE_H_
#define WALT_AMD_EPIALLELES_CORE_H_

#include "cpgpairs_core.h"

namespace walt {

constexpr uint32_t kEpiWindow = 4;     // calls per window
constexpr uint32_t kEpiColumns = 16;   // patterns of a window: 8 u0 + 4 u1 + 2 u2 + u3, u = 1 unmethylated
constexpr uint32_t kEpiChain = kEpiWindow - 1;  // calls of a chain that are kept: what a window needs in front of its last

// A chain: calls that follow each other among the calls of a read that have a pair, with pair numbers j, j + s, j + 2 s ..
// for one s in {+1, -1} ('+' records walk the pairs upwards, '-' records downwards).  chain(S) of a stretch S of calls is
// the longest such suffix of S, cut to its last kEpiChain calls.  It packs into one word, 0 = the stretch has no call:
//   bits 0..1  the calls kept, 1 .. 3
//   bit  2     "whole": S is nothing but these calls (so S has at most 3)
//   bit  3     s == -1 (meaningful from 2 calls on; 0 for 1 call)
//   bits 4..6  the states, u = 1 unmethylated: bit 4 the last call's, bit 5 the one in front of it, bit 6 the third from the end
//   bits 8..39 the pair number of the last call
WALT_HD unsigned long long epi_pack(uint32_t j, uint32_t len, uint32_t down, uint32_t states, uint32_t whole) {
  return ((unsigned long long)j << 8) | (unsigned long long)((states & 7u) << 4 | down << 3 | whole << 2 | len);
}
WALT_HD uint32_t epi_len(unsigned long long c) { return (uint32_t)c & 3u; }
WALT_HD uint32_t epi_whole(unsigned long long c) { return ((uint32_t)c >> 2) & 1u; }
WALT_HD uint32_t epi_down(unsigned long long c) { return ((uint32_t)c >> 3) & 1u; }
WALT_HD uint32_t epi_states(unsigned long long c) { return ((uint32_t)c >> 4) & 7u; }
WALT_HD uint32_t epi_last(unsigned long long c) { return (uint32_t)(c >> 8); }
WALT_HD unsigned long long epi_set_whole(unsigned long long c, bool whole) {
  return c ? (c & ~4ull) | (whole ? 4ull : 0ull) : 0ull;
}
// the pair number of call k of a chain, k = 0 the first kept; its state
WALT_HD uint32_t epi_pair_of(unsigned long long c, uint32_t k) {
  const uint32_t back = epi_len(c) - 1u - k;
  return epi_down(c) ? epi_last(c) + back : epi_last(c) - back;
}
WALT_HD uint32_t epi_state_of(unsigned long long c, uint32_t k) { return (epi_states(c) >> (epi_len(c) - 1u - k)) & 1u; }

// The call (j, u) behind chain c: the chain that ends on it (the whole bit left 0).  Where the call is the fourth of a
// chain, add(entry, column) gets its window: entry = the lowest pair's number, column from the four states in forward
// order, the lowest position first.
template <class Add>
WALT_HD unsigned long long epi_push(unsigned long long c, uint32_t j, uint32_t u, Add&& add) {
  if (!c) return epi_pack(j, 1u, 0u, u, 0u);
  const unsigned long long jl = epi_last(c);
  const bool up = (unsigned long long)j == jl + 1ull, down = (unsigned long long)j + 1ull == jl;
  if (!up && !down) return epi_pack(j, 1u, 0u, u, 0u);  // no neighbour (the same pair twice included): a new chain
  const uint32_t len = epi_len(c), st = epi_states(c);
  if (len >= 2u && epi_down(c) != (down ? 1u : 0u)) return epi_pack(j, 2u, down ? 1u : 0u, (st << 1 | u) & 3u, 0u);  // it turns round
  if (len == kEpiChain) {
    // read order: bit 2 of st, bit 1, bit 0, u
    const uint32_t fwd = st << 1 | u;  // the first call read in bit 3
    const uint32_t rev = (u << 3) | ((st & 1u) << 2) | (st & 2u) | (st >> 2 & 1u);
    if (down) add(j, rev);
    else add(j - 3u, fwd);
  }
  return epi_pack(j, len < kEpiChain ? len + 1u : kEpiChain, down ? 1u : 0u, st << 1 | u, 0u);
}

// The calls of chain h, in read order, behind chain c (whole bit left 0); add as in epi_push.
template <class Add>
WALT_HD unsigned long long epi_replay(unsigned long long c, unsigned long long h, Add&& add) {
  const uint32_t n = epi_len(h);
  for (uint32_t k = 0; k < n; ++k) c = epi_push(c, epi_pair_of(h, k), epi_state_of(h, k), add);
  return c;
}

// chain(A ++ B) from chain(A) and chain(B).  A stretch that is not whole keeps its chain whatever stands in front of it:
// the chain stopped at a break inside the stretch, or was cut at three calls.  A whole one is taken call by call behind
// the left chain.  Associative; 0 is the identity.
WALT_HD unsigned long long epi_combine(unsigned long long a, unsigned long long b) {
  if (!b) return a;
  if (!a || !epi_whole(b)) return b;
  const uint32_t calls = epi_len(a) + epi_len(b);
  const unsigned long long c = epi_replay(a, b, [](uint32_t, uint32_t) {});
  return epi_set_whole(c, epi_whole(a) && calls <= kEpiChain && epi_len(c) == calls);
}

// One slice as mbias_load_slice returns it, in slice order: the windows that lie wholly inside it are added; head = the
// chain its first calls make (at most three: the calls a window that straddles the slice's left boundary can end on),
// tail = chain(slice) with its whole bit.  0, 0: the slice has no call with a pair.  number(i): as in cpg_slice, asked
// once per call.
template <class Number, class Add>
WALT_HD void epi_slice(const uint32_t w[4], int i0, Number&& number, Add&& add, unsigned long long& head, unsigned long long& tail) {
  head = tail = 0ull;
  uint32_t calls = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 4; ++j) {
    uint32_t bits = mbias_not_dot(w[j]);
    while (bits) {
      const int k = __builtin_ctz(bits) >> 3;
      bits &= bits - 1u;
      const uint32_t b = (w[j] >> (8 * k)) & 0xFFu;
      if ((b | 0x20u) != 'z') continue;
      const long long n = number(i0 + 4 * j + k);
      if (n < 0) continue;
      tail = epi_push(tail, (uint32_t)n, (b >> 5) & 1u, add);
      ++calls;
      if (epi_len(tail) == calls) head = tail;  // still one chain from the slice's first call on
    }
  }
  tail = epi_set_whole(tail, epi_len(tail) == calls);
}

// The windows that end inside a slice and begin in front of it: the slice's head behind the chain that reaches it.
template <class Add>
WALT_HD void epi_straddle(unsigned long long in, unsigned long long head, Add&& add) {
  if (in && head) (void)epi_replay(in, head, add);
}

// The epiallele table's fold (cpgpairs_core.h CpgPairFold has the shape; cpg_fold_read<EpiFold> is the one-thread model
// of the kernel).  A slice without a call with a pair ends no window: its straddle costs no combine.
struct EpiFold {
  static constexpr uint32_t kColumns = kEpiColumns;
  template <class Number, class Add>
  static WALT_HD void slice(const uint32_t w[4], int i0, Number&& number, Add&& add, unsigned long long& head, unsigned long long& tail) {
    epi_slice(w, i0, number, add, head, tail);
  }
  static WALT_HD unsigned long long combine(unsigned long long a, unsigned long long b) { return epi_combine(a, b); }
  template <class Add>
  static WALT_HD void straddle(unsigned long long carry, unsigned long long left, unsigned long long head, Add&& add) {
    if (head) epi_straddle(epi_combine(carry, left), head, add);
  }
};
// the epiallele table's model under the name its CPU harness (tests/epialleles_harness.cpp) calls
template <class Number, class Add>
WALT_HD void epi_read(const uint8_t* __restrict__ rb, int len, uint64_t before, uint64_t after, Number&& number, Add&& add) {
  cpg_fold_read<EpiFold>(rb, len, before, after, number, add);
}

}  // namespace walt
#endif  // WALT_AMD_EPIALLELES_CORE_H_
