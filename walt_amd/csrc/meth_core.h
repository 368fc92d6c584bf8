// meth_core.h -- per-read methylation calling (include/walt_amd.h, "methylation calls"): the classification of one
// 16-base slice of a read against the unconverted reference, bit-parallel on 2-bit fields.  Pure inline functions
// shared by the HIP kernel (meth.hip) and a g++ unit test (tests/test_meth_cpu.py compiles tests/meth_harness.cpp).
#ifndef WALT_AMD_METH_CORE_H_
#define WALT_AMD_METH_CORE_H_

#include "core.h"

namespace walt {

// A "field mask" holds one flag per base of a slice in bit 2k (k = 0..15), the position of the low bit of base k's
// 2-bit field in a packed word (core.h g2_code: base k of a word in bits 2k+1..2k).
constexpr uint32_t kFieldLow = 0x55555555u;

// flag k set where the 2-bit field k of x equals code
WALT_HD uint32_t meth_eq2(uint32_t x, uint32_t code) {
  const uint32_t lo = (code & 1u) ? x : ~x, hi = (code & 2u) ? (x >> 1) : ~(x >> 1);
  return lo & hi & kFieldLow;
}
// flags of the slice positions [a, b), both clamped to [0, 16]
WALT_HD uint32_t meth_range(long long a, long long b) {
  const uint32_t ua = a < 0 ? 0u : a > 16 ? 16u : (uint32_t)a, ub = b < 0 ? 0u : b > 16 ? 16u : (uint32_t)b;
  const uint32_t below_b = ub >= 16 ? ~0u : (1u << (2 * ub)) - 1u, below_a = ua >= 16 ? ~0u : (1u << (2 * ua)) - 1u;
  return ua < ub ? (below_b & ~below_a & kFieldLow) : 0u;
}
// 16 sanitised read bytes (A C G T, four per word, first base in the low byte) -> 2-bit fields A 0, C 1, T 2, G 3:
// bits 2..1 of the ASCII codes 0x41 0x43 0x47 0x54.  Any other byte aliases to the letter whose bits 2..1 it shares.
WALT_HD uint32_t meth_read_fields(const uint32_t rd[4]) {
  uint32_t r = 0;
  for (int j = 0; j < 4; ++j) {
    uint32_t t = (rd[j] >> 1) & 0x03030303u;
    t = (t | (t >> 6) | (t >> 12) | (t >> 18)) & 0xFFu;
    r |= t << (8 * j);
  }
  return r;
}
// flags of four bases (bits 0, 2, 4, 6 of m) -> bit 0 of the four bytes of a word
WALT_HD uint32_t meth_spread(uint32_t m) {
  return (m | (m << 6) | (m << 12) | (m << 18)) & 0x01010101u;
}

// 16 quality bytes (four per word, first base in the low byte) -> the field mask of the positions whose byte is at
// least min_qual (include/walt_amd.h, "minimum base quality"); min_qual <= 127, the compare unsigned.  Per word: the low
// seven bits of every byte with bit 7 set on top, minus min_qual in every byte, keeps bit 7 exactly where the seven
// bits reach min_qual (0x80 + b - t lies in 1 .. 0xFF: no borrow leaves a byte); a byte of 128 or more passes by its own
// bit 7, which the subtraction alone would get wrong.  The four bit 7s then move to bits 0, 2, 4, 6 of the word's byte.
WALT_HD uint32_t meth_qual_mask(const uint32_t qd[4], uint32_t min_qual) {
  const uint32_t t4 = min_qual * 0x01010101u;
  uint32_t r = 0;
  for (int j = 0; j < 4; ++j) {
    const uint32_t w = qd[j];
    const uint32_t ge = ((((w & 0x7F7F7F7Fu) | 0x80808080u) - t4) | w) & 0x80808080u;
    const uint32_t x = ge >> 7;
    r |= ((x | (x >> 6) | (x >> 12) | (x >> 18)) & 0x55u) << (8 * j);
  }
  return r;
}

struct MethSlice {
  uint32_t out[4];             // the 16 call characters
  unsigned long long meth, unmeth;  // four 16-bit counts each: CpG, CHG, CHH, unknown (the layout of walt_meth_counts)
  uint32_t cm, cu;             // field masks of the positions called methylated / unmethylated (the pile-up's input)
};

// One slice: slice position k is read position i0 + k and genome position q0 + k.
//   rd       the 16 read bytes (anything at positions that cannot be called)
//   ext      reference codes (A 0, C 1, G 2, T 3) of genome positions q0 - 2 .. q0 + 29, two bits each, lowest first
//   ga       0: conversion 'T' (calls at reference C, context ahead); 1: 'A' (calls at reference G, context behind)
//   call     flags of the positions that may get a call (inside the read, below call_len, inside the chromosome)
//   v1, v2   flags of the positions whose first / second context base lies inside the chromosome
WALT_HD MethSlice meth_slice(const uint32_t rd[4], unsigned long long ext, uint32_t ga, uint32_t call, uint32_t v1,
                             uint32_t v2) {
  const uint32_t cur = (uint32_t)(ext >> 4);
  const uint32_t n1 = ga ? (uint32_t)(ext >> 2) : (uint32_t)(ext >> 6);
  const uint32_t n2 = ga ? (uint32_t)ext : (uint32_t)(ext >> 8);
  const uint32_t rf = meth_read_fields(rd);
  const uint32_t key = ga ? 1u : 2u;  // the context key: G ahead of a C, C behind a G
  const uint32_t m = meth_eq2(rf, ga ? 3u : 1u);  // read G / C: methylated
  const uint32_t u = meth_eq2(rf, ga ? 0u : 2u);  // read A / T: unmethylated
  const uint32_t c = meth_eq2(cur, ga ? 2u : 1u) & (m | u) & call;
  const uint32_t k1 = meth_eq2(n1, key), k2 = meth_eq2(n2, key);
  const uint32_t z = c & v1 & k1;
  const uint32_t rest = c & v1 & ~k1;
  const uint32_t x = rest & v2 & k2;
  const uint32_t h = rest & v2 & ~k2;
  const uint32_t un = (c & ~v1) | (rest & ~v2);
  const uint32_t cm = c & m;
  MethSlice s;
  for (int j = 0; j < 4; ++j) {
    const uint32_t sh = 8 * j;
    // '.' 0x2E; z 0x7A, x 0x78, h 0x68, u 0x75; upper case = lower case ^ 0x20
    s.out[j] = 0x2E2E2E2Eu ^ (meth_spread((z >> sh) & 0xFFu) * 0x54u) ^ (meth_spread((x >> sh) & 0xFFu) * 0x56u) ^
               (meth_spread((h >> sh) & 0xFFu) * 0x46u) ^ (meth_spread((un >> sh) & 0xFFu) * 0x5Bu) ^
               (meth_spread((cm >> sh) & 0xFFu) * 0x20u);
  }
#if defined(__HIP_DEVICE_COMPILE__)
#define WALT_METH_POPC(v) ((unsigned long long)__popc(v))
#else
#define WALT_METH_POPC(v) ((unsigned long long)__builtin_popcount(v))
#endif
  s.meth = WALT_METH_POPC(z & m) | (WALT_METH_POPC(x & m) << 16) | (WALT_METH_POPC(h & m) << 32) | (WALT_METH_POPC(un & m) << 48);
  s.unmeth = WALT_METH_POPC(z & u) | (WALT_METH_POPC(x & u) << 16) | (WALT_METH_POPC(h & u) << 32) | (WALT_METH_POPC(un & u) << 48);
#undef WALT_METH_POPC
  s.cm = cm;
  s.cu = c & u;
  return s;
}

// The three flag sets of meth_slice for a slice that starts at read position i0 (negative in a read's first slice),
// of a read at genome position p in the chromosome [lo, hi), with `limit` = min(read length, call_len).
// [ex_lo, ex_hi): read positions that get no call although they could (include/walt_amd.h, "overlap of a pair": the
// other mate of the pair calls them); empty when ex_lo >= ex_hi.
// trim5 >= 0: the read positions below it get no call (include/walt_amd.h, "ignored read ends").  The read's start and
// the 5' bound are two lower ends of one range, the larger wins: the bound is the range's lower end, 0 without one.
// (The 3' bound has no term here: the caller takes it off `limit`, meth_trim_limit.)
WALT_HD void meth_slice_flags(long long i0, long long p, long long lo, long long hi, long long limit, uint32_t ga,
                              uint32_t& call, uint32_t& v1, uint32_t& v2, long long ex_lo, long long ex_hi, long long trim5) {
  const long long room = hi - p;  // read positions below it lie inside the chromosome
  call = meth_range(trim5 - i0, (limit < room ? limit : room) - i0) & ~meth_range(ex_lo - i0, ex_hi - i0);
  if (ga) {  // context at q - 1, q - 2 >= lo  <=>  k >= lo + 1 - p - i0, lo + 2 - p - i0
    v1 = meth_range(lo + 1 - p - i0, 16);
    v2 = meth_range(lo + 2 - p - i0, 16);
  } else {   // context at q + 1, q + 2 < hi  <=>  k < room - i0 - 1, room - i0 - 2
    v1 = meth_range(0, room - i0 - 1);
    v2 = meth_range(0, room - i0 - 2);
  }
}
WALT_HD void meth_slice_flags(long long i0, long long p, long long lo, long long hi, long long limit, uint32_t ga,
                              uint32_t& call, uint32_t& v1, uint32_t& v2, long long ex_lo, long long ex_hi) {
  meth_slice_flags(i0, p, lo, hi, limit, ga, call, v1, v2, ex_lo, ex_hi, 0);
}
WALT_HD void meth_slice_flags(long long i0, long long p, long long lo, long long hi, long long limit, uint32_t ga,
                              uint32_t& call, uint32_t& v1, uint32_t& v2) {
  meth_slice_flags(i0, p, lo, hi, limit, ga, call, v1, v2, 0, 0, 0);
}
// limit = min(read length, call_len) with the last trim3 positions before it taken off, saturating at 0: the 3' bound
// counts back from the clip point (include/walt_amd.h, "ignored read ends")
WALT_HD uint32_t meth_trim_limit(uint32_t limit, uint32_t trim3) { return limit > trim3 ? limit - trim3 : 0u; }

// ext of meth_slice from the packed reference: positions qs = q0 - 2 .. qs + 31 (qs may be negative at the genome's
// start: the fields below position 0 read as 0 and are never used, their positions lie outside every chromosome).
// `last` = the last word index the array holds: a slice beyond the genome (a read that runs over its chromosome's
// end gets no call there) reads the array's zero padding instead.
WALT_HD unsigned long long meth_ref_ext(const uint32_t* ref, long long qs, uint32_t last) {
  const long long q = qs < 0 ? 0 : qs;
  uint32_t w = (uint32_t)(q >> 4);
  w = w + 2 > last ? last - 2 : w;
  const uint32_t sh = 2 * (uint32_t)(q & 15);
  const uint32_t a = ref[w], b = ref[w + 1], c = ref[w + 2];
  const unsigned long long ab = ((unsigned long long)b << 32) | a, bc = ((unsigned long long)c << 32) | b;
  const unsigned long long e = ((unsigned long long)(uint32_t)(bc >> sh) << 32) | (uint32_t)(ab >> sh);
  return qs < 0 ? e << (2 * (uint32_t)(-qs)) : e;
}

// The slice of a read that starts at read position i0 (a multiple of 16 apart from the head: -15 .. len - 1):
// out = its 16 call characters, meth / unmeth += its counts.  rb: the read's first base, total: its length,
// limit = min(length, call_len); mapped: the record can be called at all.  before / after: the bytes of the batch's
// bases in front of rb and from rb on: a partial slice (a read's head or tail) is loaded whole where the 16 bytes lie
// inside the batch (the neighbouring read's bases are masked out by the flags), byte by byte at the batch's two ends.
// cm / cu = the slice's positions called methylated / unmethylated (field masks; 0 where nothing is called): what a
// per-cytosine pile-up adds (pileup_core.h).  [ex_lo, ex_hi): the read positions excluded from calling (meth_slice_flags).
// trim5: the read positions below it get no call; `limit` comes with the 3' bound taken off (meth_trim_limit).  A slice
// that lies wholly below trim5 returns like one at or beyond `limit`: before any read byte or reference word is loaded.
// kQual: qb = the read's first quality byte, at the offsets of rb in an array as long as the bases (include/walt_amd.h,
// "minimum base quality"); the slice's quality bytes are loaded beside its read bytes, in the same way and under the
// same bounds, and the positions below min_qual leave `call`; a slice they leave nothing of returns before the reference
// words are loaded.  Without kQual neither argument is read and the code is what it was.
template <bool kQual>
WALT_HD void meth_read_slice_q(const uint8_t* rb, int total, uint32_t limit, bool mapped, uint32_t pos, uint32_t lo,
                               uint32_t hi, uint32_t ga, const uint32_t* ref, uint32_t ref_last, int i0,
                               unsigned long long before, unsigned long long after, uint32_t out[4],
                               unsigned long long& meth, unsigned long long& unmeth, uint32_t& cm, uint32_t& cu,
                               uint32_t ex_lo, uint32_t ex_hi, uint32_t trim5, const uint8_t* qb, uint32_t min_qual) {
  out[0] = out[1] = out[2] = out[3] = 0x2E2E2E2Eu;
  cm = cu = 0;
  if (!mapped || i0 >= (int)limit || (long long)i0 + 16 <= (long long)trim5) return;
  uint32_t call, v1, v2;
  meth_slice_flags(i0, pos, lo, hi, limit, ga, call, v1, v2, ex_lo, ex_hi, trim5);
  if (!call) return;
  uint32_t rd[4] = {0, 0, 0, 0}, qd[4] = {0, 0, 0, 0};
  if ((i0 >= 0 || (unsigned long long)(-i0) <= before) && (unsigned long long)(i0 + 16) <= after) {
    __builtin_memcpy(rd, rb + i0, 16);  // (bases and calls may differ in alignment)
    if (kQual) __builtin_memcpy(qd, qb + i0, 16);  // (and so may the qualities)
  } else {
    for (int k = 0; k < 16; ++k) {
      const int i = i0 + k;
      if (i >= 0 && i < total) rd[k >> 2] |= (uint32_t)rb[i] << (8 * (k & 3));
      if (kQual && i >= 0 && i < total) qd[k >> 2] |= (uint32_t)qb[i] << (8 * (k & 3));
    }
  }
  if (kQual) {
    call &= meth_qual_mask(qd, min_qual);
    if (!call) return;
  }
  const MethSlice s = meth_slice(rd, meth_ref_ext(ref, (long long)pos + i0 - 2, ref_last), ga, call, v1, v2);
  out[0] = s.out[0]; out[1] = s.out[1]; out[2] = s.out[2]; out[3] = s.out[3];
  meth += s.meth; unmeth += s.unmeth;
  cm = s.cm; cu = s.cu;
}
WALT_HD void meth_read_slice(const uint8_t* rb, int total, uint32_t limit, bool mapped, uint32_t pos, uint32_t lo,
                             uint32_t hi, uint32_t ga, const uint32_t* ref, uint32_t ref_last, int i0,
                             unsigned long long before, unsigned long long after, uint32_t out[4],
                             unsigned long long& meth, unsigned long long& unmeth, uint32_t& cm, uint32_t& cu,
                             uint32_t ex_lo, uint32_t ex_hi, uint32_t trim5) {
  meth_read_slice_q<false>(rb, total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, before, after, out, meth, unmeth, cm, cu,
                           ex_lo, ex_hi, trim5, nullptr, 0u);
}
// the form without ignored ends, and the forms without an excluded interval: what they always gave
WALT_HD void meth_read_slice(const uint8_t* rb, int total, uint32_t limit, bool mapped, uint32_t pos, uint32_t lo,
                             uint32_t hi, uint32_t ga, const uint32_t* ref, uint32_t ref_last, int i0,
                             unsigned long long before, unsigned long long after, uint32_t out[4],
                             unsigned long long& meth, unsigned long long& unmeth, uint32_t& cm, uint32_t& cu,
                             uint32_t ex_lo, uint32_t ex_hi) {
  meth_read_slice(rb, total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, before, after, out, meth, unmeth, cm, cu, ex_lo, ex_hi, 0u);
}
WALT_HD void meth_read_slice(const uint8_t* rb, int total, uint32_t limit, bool mapped, uint32_t pos, uint32_t lo,
                             uint32_t hi, uint32_t ga, const uint32_t* ref, uint32_t ref_last, int i0,
                             unsigned long long before, unsigned long long after, uint32_t out[4],
                             unsigned long long& meth, unsigned long long& unmeth, uint32_t& cm, uint32_t& cu) {
  meth_read_slice(rb, total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, before, after, out, meth, unmeth, cm, cu, 0u, 0u);
}
WALT_HD void meth_read_slice(const uint8_t* rb, int total, uint32_t limit, bool mapped, uint32_t pos, uint32_t lo,
                             uint32_t hi, uint32_t ga, const uint32_t* ref, uint32_t ref_last, int i0,
                             unsigned long long before, unsigned long long after, uint32_t out[4],
                             unsigned long long& meth, unsigned long long& unmeth) {
  uint32_t cm, cu;
  meth_read_slice(rb, total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, before, after, out, meth, unmeth, cm, cu, 0u, 0u);
}
// Stores the slice's characters that belong to the read; cb + i0 is 16-byte aligned.  A whole slice is one 16-byte
// store.  A read's tail [0, kb) goes out as naturally aligned pieces of 8, 4, 2 and 1 bytes by the bits of kb, its
// head [ka, 16) the same way from the slice's end: four stores at most instead of fifteen; a read that lies inside
// one slice (both ends cut) goes byte by byte.
WALT_HD void meth_store_slice(uint8_t* cb, int total, int i0, const uint32_t out[4]) {
  uint8_t* p = cb + i0;
  const int ka = i0 < 0 ? -i0 : 0, kb = total - i0 < 16 ? total - i0 : 16;
  if (ka == 0 && kb == 16) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4*>(p) = make_uint4(out[0], out[1], out[2], out[3]);
#else
    __builtin_memcpy(p, out, 16);
#endif
    return;
  }
  const unsigned long long lo64 = ((unsigned long long)out[1] << 32) | out[0], hi64 = ((unsigned long long)out[3] << 32) | out[2];
  if (ka == 0) {  // tail: pieces at 0, kb & 8, kb & 12, kb & 14
    const uint32_t n = (uint32_t)kb;
    if (n & 8u) *reinterpret_cast<unsigned long long*>(p) = lo64;
    const unsigned long long half = (n & 8u) ? hi64 : lo64;           // the 8 bytes that hold the rest
    const uint32_t word = (n & 4u) ? (uint32_t)(half >> 32) : (uint32_t)half;  // the 4 bytes behind an 4-byte piece
    if (n & 4u) *reinterpret_cast<uint32_t*>(p + (n & 8u)) = (uint32_t)half;
    if (n & 2u) *reinterpret_cast<uint16_t*>(p + (n & 12u)) = (uint16_t)word;
    if (n & 1u) p[n & 14u] = (uint8_t)(word >> ((n & 2u) ? 16 : 0));
  } else if (kb == 16) {  // head: pieces that end at 16, 16 - (n & 8), 16 - (n & 12), 16 - (n & 14)
    const uint32_t n = (uint32_t)(16 - ka);
    if (n & 8u) *reinterpret_cast<unsigned long long*>(p + 8) = hi64;
    const unsigned long long half = (n & 8u) ? lo64 : hi64;
    const uint32_t word = (n & 4u) ? (uint32_t)half : (uint32_t)(half >> 32);
    if (n & 4u) *reinterpret_cast<uint32_t*>(p + 12 - (n & 8u)) = (uint32_t)(half >> 32);
    if (n & 2u) *reinterpret_cast<uint16_t*>(p + 14 - (n & 12u)) = (uint16_t)(word >> 16);
    if (n & 1u) p[15 - (n & 14u)] = (uint8_t)(word >> ((n & 2u) ? 8 : 24));
  } else {
    for (int k = ka; k < kb; ++k) p[k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
  }
}

}  // namespace walt
#endif  // WALT_AMD_METH_CORE_H_
