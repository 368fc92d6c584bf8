// cpgpairs_core.h -- adjacent CpG pairs (include/walt_amd.h, "adjacent CpG pairs"): the pair bitmap of the forward
// reference and its rank directory, the pair of a call, the fold of one 16-byte slice of calls and how the last call of
// one stretch meets the first of the next.  Pure inline functions shared by the HIP kernels (cpgpairs.hip) and a g++
// unit test (tests/test_cpgpairs_cpu.py compiles tests/cpgpairs_harness.cpp).  The slices are mbias_core.h's: same
// cut, same loads, same masks; the trips are nonconv_core.h's.
#ifndef WALT_AMD_CPGPAIRS_CORE_H_
#define WALT_AMD_CPGPAIRS_CORE_H_

#include "nonconv_core.h"

namespace walt {

constexpr uint32_t kCpgGroup = kNonconvGroup;  // lanes that share a read
constexpr uint32_t kCpgMaxCalls = 1024;        // walt_max_read_len() of the widest pattern: a longer read adds nothing
constexpr uint32_t kCpgBlockWords = 4;         // bitmap words per directory entry: one 16-byte load
constexpr uint32_t kCpgBlockBits = 32u * kCpgBlockWords;
constexpr uint32_t kCpgPadWords = 8;           // zero words behind the bitmap (cpg_next and the last block read into them)
constexpr uint32_t kCpgNextWords = 34;         // cpg_next looks this far: a read of 1024 calls spans at most 1025 positions
constexpr uint32_t kCpgNoNext = 0xFFFFFFFFu;

// The bitmap: bit f & 31 of word f >> 5 is set where forward position f starts a pair.  Words of the bitmap for a genome
// of genome_len positions, a multiple of kCpgBlockWords, the padding not included; and its directory entries.
WALT_HD uint64_t cpg_bit_words(uint64_t genome_len) {
  const uint64_t w = (genome_len + 31u) / 32u;
  return (w + kCpgBlockWords - 1u) / kCpgBlockWords * kCpgBlockWords;
}
WALT_HD uint64_t cpg_dir_entries(uint64_t genome_len) { return cpg_bit_words(genome_len) / kCpgBlockWords; }

// Word w of the bitmap from the packed '+' reference (2 bits per base, A 0, C 1, G 2, T 3; sixteen bases per word):
// r0, r1 = reference words 2 w and 2 w + 1, r2 = word 2 w + 2 (its first base alone is looked at).  Bit k: R[32 w + k]
// is C and R[32 w + k + 1] is G.  The chromosome rule is not applied here (cpg_end_word / cpg_end_mask).
WALT_HD uint32_t cpg_pair_word(uint32_t r0, uint32_t r1, uint32_t r2) {
  const uint64_t k = 0x5555555555555555ull;
  const uint64_t x = (uint64_t)r0 | ((uint64_t)r1 << 32);
  const uint64_t y = (x >> 2) | ((uint64_t)(r2 & 3u) << 62);  // the base behind each
  const uint64_t c = x & ~(x >> 1) & k;                       // fields equal to 1
  const uint64_t g = (y >> 1) & ~y & k;                       // fields equal to 2
  uint64_t p = c & g;                                         // bit 2 k: position k starts a pair
  p = (p | (p >> 1)) & 0x3333333333333333ull;
  p = (p | (p >> 2)) & 0x0F0F0F0F0F0F0F0Full;
  p = (p | (p >> 4)) & 0x00FF00FF00FF00FFull;
  p = (p | (p >> 8)) & 0x0000FFFF0000FFFFull;
  p = (p | (p >> 16)) & 0x00000000FFFFFFFFull;
  return (uint32_t)p;
}
// The chromosome rule: c + 1 must lie in c's chromosome, so the last position of a chromosome -- `end` is the first of
// the next, or the genome's length -- starts no pair: its word and the mask that clears its bit (end >= 1).
WALT_HD uint64_t cpg_end_word(uint32_t end) { return (uint64_t)(end - 1u) >> 5; }
WALT_HD uint32_t cpg_end_mask(uint32_t end) { return ~(1u << ((end - 1u) & 31u)); }

WALT_HD uint32_t cpg_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
WALT_HD uint32_t cpg_block_count(const uint32_t* __restrict__ bits, uint64_t blk) {
  const uint32_t* b = bits + kCpgBlockWords * blk;
  return cpg_popc(b[0]) + cpg_popc(b[1]) + cpg_popc(b[2]) + cpg_popc(b[3]);
}

WALT_HD bool cpg_bit(const uint32_t* __restrict__ bits, uint32_t f) { return ((bits[f >> 5] >> (f & 31u)) & 1u) != 0u; }

// The pairs in front of forward position p: dir[b] = the pairs in front of block b, plus the popcounts inside the block.
// For a p that starts a pair this is its number j.
WALT_HD uint32_t cpg_rank(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ dir, uint32_t p) {
  const uint32_t blk = p >> 7, wi = (p >> 5) & 3u;
  uint32_t b[4];
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 q = *reinterpret_cast<const uint4*>(bits + (uint64_t)kCpgBlockWords * blk);  // (the bitmap's base is 256-byte aligned)
  b[0] = q.x; b[1] = q.y; b[2] = q.z; b[3] = q.w;
#else
  memcpy(b, bits + (uint64_t)kCpgBlockWords * blk, 16);
#endif
  uint32_t r = dir[blk];
  r += wi > 0u ? cpg_popc(b[0]) : 0u;
  r += wi > 1u ? cpg_popc(b[1]) : 0u;
  r += wi > 2u ? cpg_popc(b[2]) : 0u;
  const uint32_t cur = wi == 0u ? b[0] : wi == 1u ? b[1] : wi == 2u ? b[2] : b[3];
  return r + cpg_popc(cur & ((1u << (p & 31u)) - 1u));
}

// The pair of a call at forward position f (inside the genome): f where f starts a pair (the call sits on the C), else
// f - 1 where that starts one (the call sits on the G), else none (-1).  The reference alone decides.
WALT_HD long long cpg_pair_at(const uint32_t* __restrict__ bits, uint32_t f) {
  if (cpg_bit(bits, f)) return (long long)f;
  if (f > 0u && cpg_bit(bits, f - 1u)) return (long long)f - 1;
  return -1;
}

// The first pair behind position c, kCpgNoNext when none starts within kCpgNextWords words (n_words: the bitmap's words
// with its padding).
WALT_HD uint32_t cpg_next(const uint32_t* __restrict__ bits, uint32_t c, uint64_t n_words) {
  uint64_t w = c >> 5;
  uint32_t cur = (c & 31u) == 31u ? 0u : bits[w] & (~0u << ((c & 31u) + 1u));
  for (uint32_t k = 0; k < kCpgNextWords; ++k) {
    if (cur) return (uint32_t)(32u * w + (uint32_t)__builtin_ctz(cur));
    if (++w >= n_words) break;
    cur = bits[w];
  }
  return kCpgNoNext;
}

// the bits of bitmap word w whose positions lie in [pos_lo, pos_hi)
WALT_HD uint32_t cpg_range_mask(uint64_t w, uint32_t pos_lo, uint32_t pos_hi) {
  const uint64_t first = 32u * w;
  uint32_t m = ~0u;
  if ((uint64_t)pos_lo > first) m &= (uint64_t)pos_lo - first >= 32u ? 0u : ~0u << (pos_lo - (uint32_t)first);
  if ((uint64_t)pos_hi < first + 32u) m &= (uint64_t)pos_hi <= first ? 0u : (1u << (pos_hi - (uint32_t)first)) - 1u;
  return m;
}

// A record adds when it is unique, not skipped, its read has 1 to 1024 calls and its position lies inside the genome;
// tested before any index is formed.
WALT_HD bool cpg_counted(uint32_t times, uint32_t skip_byte, uint64_t off, uint64_t end, uint32_t pos, uint32_t genome_len) {
  return times == 1u && skip_byte == 0u && end > off && end - off <= (uint64_t)kCpgMaxCalls && pos < genome_len;
}

// The pair of the call at read position i of a record at `pos` of its strand genome, inside the chromosome [lo, hi): -1
// when the position lies at or beyond the chromosome's end or on no pair.
WALT_HD long long cpg_call_pair(const uint32_t* __restrict__ bits, uint32_t pos, int i, bool minus, uint32_t lo, uint32_t hi) {
  const long long q = (long long)pos + i;
  if (q >= (long long)hi) return -1;
  const long long f = minus ? (long long)lo + (long long)hi - 1 - q : q;
  if (f < (long long)lo) return -1;  // (a position the record's own start rules out: pos >= lo)
  return cpg_pair_at(bits, (uint32_t)f);
}

// A call that has a pair, as the fold moves it: (j << 1 | u) + 1 with u = 1 for an unmethylated call; 0: none.
WALT_HD unsigned long long cpg_call(uint32_t j, uint32_t u) { return (((unsigned long long)j << 1) | u) + 1ull; }

// Two calls that follow each other in a read: a couple when their pairs are neighbours.  add(entry, column): entry =
// the lower pair's number, column = 2 * u_lo + u_hi (0 MM, 1 MU, 2 UM, 3 UU).  Every other couple, and an absent call
// on either side, adds nothing.
template <class Add>
WALT_HD void cpg_couple(unsigned long long a, unsigned long long b, Add&& add) {
  if (!a || !b) return;
  const unsigned long long ja = (a - 1ull) >> 1, jb = (b - 1ull) >> 1;
  const uint32_t ua = (uint32_t)(a - 1ull) & 1u, ub = (uint32_t)(b - 1ull) & 1u;
  if (jb == ja + 1ull) add((uint32_t)ja, 2u * ua + ub);
  else if (ja == jb + 1ull) add((uint32_t)jb, 2u * ub + ua);
}

// The last call of stretch A followed by stretch B: the rightmost that exists.  Associative; 0 is the identity.
WALT_HD unsigned long long cpg_combine(unsigned long long a, unsigned long long b) { return b ? b : a; }

// One slice as mbias_load_slice returns it, in slice order: the couples that lie wholly inside it are added, and its
// first and last call with a pair come back (0: it has none).  number(i) = the pair NUMBER of the z / Z at read position
// i, -1 when that call has none.  Every byte other than z / Z is skipped.
template <class Number, class Add>
WALT_HD void cpg_slice(const uint32_t w[4], int i0, Number&& number, Add&& add, unsigned long long& first, unsigned long long& last) {
  first = last = 0ull;
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
      const unsigned long long e = cpg_call((uint32_t)n, (b >> 5) & 1u);
      if (!first) first = e;
      cpg_couple(last, e, add);
      last = e;
    }
  }
}

// The pair table's fold, as k_cpg_fold, the extraction and cpg_fold_read take a fold: the columns of an entry, the fold of
// a slice, how two stretches meet, and what the call(s) in front of a slice -- `carry` from earlier trips, then `left`
// from the lanes in front of it -- add with the slice's first call.  (epialleles_core.h has the other one, EpiFold.)
struct CpgPairFold {
  static constexpr uint32_t kColumns = 4;
  template <class Number, class Add>
  static WALT_HD void slice(const uint32_t w[4], int i0, Number&& number, Add&& add, unsigned long long& first, unsigned long long& last) {
    cpg_slice(w, i0, number, add, first, last);
  }
  static WALT_HD unsigned long long combine(unsigned long long a, unsigned long long b) { return cpg_combine(a, b); }
  template <class Add>
  static WALT_HD void straddle(unsigned long long carry, unsigned long long left, unsigned long long first, Add&& add) {
    cpg_couple(cpg_combine(carry, left), first, add);
  }
};

// One read as a group of the kernel takes it, on one thread: per trip the eight lanes' slices, each lane's incoming call
// (chain) by the scan the three cross-lane steps make (lane s after step d holds the fold of slices s - 2 d + 1 .. s),
// the trip's fold carried to the next.  before / after: as in mbias_load_slice.
template <class Fold, class Number, class Add>
WALT_HD void cpg_fold_read(const uint8_t* __restrict__ rb, int len, uint64_t before, uint64_t after, Number&& number, Add&& add) {
  const int head = (int)((uintptr_t)rb & 15u);
  const int trips = nonconv_trips(len, head);
  unsigned long long carry = 0ull;
  for (int t = 0; t < trips; ++t) {
    unsigned long long first[kCpgGroup], incl[kCpgGroup];
    for (int sub = 0; sub < (int)kCpgGroup; ++sub) {
      const int i0 = -head + 16 * ((int)kCpgGroup * t + sub);
      first[sub] = incl[sub] = 0ull;
      if (i0 < len) {
        uint32_t w[4];
        mbias_load_slice(rb, len, i0, before, after, w);
        Fold::slice(w, i0, number, add, first[sub], incl[sub]);
      }
    }
    for (int d = 1; d < (int)kCpgGroup; d <<= 1)
      for (int sub = (int)kCpgGroup - 1; sub >= d; --sub) incl[sub] = Fold::combine(incl[sub - d], incl[sub]);
    for (int sub = 0; sub < (int)kCpgGroup; ++sub) Fold::straddle(carry, sub ? incl[sub - 1] : 0ull, first[sub], add);
    carry = Fold::combine(carry, incl[kCpgGroup - 1]);
  }
}
// the pair table's model under the name its CPU harness (tests/cpgpairs_harness.cpp) calls
template <class Number, class Add>
WALT_HD void cpg_read(const uint8_t* __restrict__ rb, int len, uint64_t before, uint64_t after, Number&& number, Add&& add) {
  cpg_fold_read<CpgPairFold>(rb, len, before, after, number, add);
}

}  // namespace walt
#endif  // WALT_AMD_CPGPAIRS_CORE_H_
