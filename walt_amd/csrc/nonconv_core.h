// nonconv_core.h -- non-converted reads (include/walt_amd.h, "non-converted reads"): which call letters count, the
// summary of a stretch of calls and how two neighbouring stretches combine, which records are judged, the rule, and the
// pair rule.  Pure inline functions shared by the HIP kernels (nonconv.hip) and a g++ unit test (tests/test_nonconv_cpu.py
// compiles tests/nonconv_harness.cpp).  The slices are mbias_core.h's: same cut, same loads, same masks.
#ifndef WALT_AMD_NONCONV_CORE_H_
#define WALT_AMD_NONCONV_CORE_H_

#include "../../include/walt_amd.h"
#include "mbias_core.h"

namespace walt {

constexpr uint32_t kNonconvMaxCalls = 1024;  // walt_max_read_len() of the widest pattern: a longer read is not judged
constexpr uint32_t kNonconvGroup = 8;        // lanes that share a read: a trip of a group is 8 slices, 128 bytes

// 1: a methylated non-CpG call (H, X); 2: an unmethylated one (h, x); 0: every other byte of the 256.  b | 0x20 is 'h'
// or 'x' for exactly the four letters; bit 5 tells the case.
WALT_HD uint32_t nonconv_class(uint32_t b) {
  const uint32_t low = b | 0x20u;
  return (low == 'h' || low == 'x') ? 1u + ((b >> 5) & 1u) : 0u;
}

// A stretch of calls in read order: methylated and all non-CpG calls, the run of H / X it begins with, the run it ends
// with, its longest run, and whether it holds no h / x at all (then the three runs are equal to meth).
struct NonconvSum {
  uint32_t meth, total, pre, suf, best, full;
};
WALT_HD NonconvSum nonconv_identity() { return NonconvSum{0u, 0u, 0u, 0u, 0u, 1u}; }

// A followed by B.  Associative, not commutative; nonconv_identity() on either side changes nothing.
WALT_HD NonconvSum nonconv_combine(const NonconvSum& A, const NonconvSum& B) {
  NonconvSum r;
  r.meth = A.meth + B.meth;
  r.total = A.total + B.total;
  const uint32_t mid = A.suf + B.pre;
  r.best = A.best > B.best ? A.best : B.best;
  r.best = r.best > mid ? r.best : mid;
  r.pre = A.full ? A.pre + B.pre : A.pre;
  r.suf = B.full ? A.suf + B.suf : B.suf;
  r.full = A.full & B.full;
  return r;
}

// S followed by one byte of class c: nonconv_combine(S, the summary of that byte) written out
WALT_HD void nonconv_push(NonconvSum& s, uint32_t c) {
  if (c == 1u) {
    ++s.meth; ++s.total; ++s.suf;
    s.pre += s.full;
    s.best = s.best > s.suf ? s.best : s.suf;
  } else if (c == 2u) {
    ++s.total;
    s.suf = 0u;
    s.full = 0u;
  }
}

// one slice as mbias_load_slice returns it (bytes outside the read are 0: no letter), in slice order
WALT_HD NonconvSum nonconv_slice(const uint32_t w[4]) {
  NonconvSum s = nonconv_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 4; ++j) {
    uint32_t bits = mbias_not_dot(w[j]);
    while (bits) {
      const int k = __builtin_ctz(bits) >> 3;
      bits &= bits - 1u;
      nonconv_push(s, nonconv_class((w[j] >> (8 * k)) & 0xFFu));
    }
  }
  return s;
}

// What a cross-lane step moves: two words.  A step only ever moves summaries of at most one trip of a group (128 bytes;
// the lanes whose result nobody reads stay below 2^3 slices as well), so a field is at most 128 here and takes 8 bits;
// the read's running summary, whose fields reach 1024, never crosses lanes.
static_assert(kNonconvGroup * 16u <= 255u, "a trip's fields fit in 8 bits");
WALT_HD void nonconv_pack(const NonconvSum& s, uint32_t& w0, uint32_t& w1) {
  w0 = s.meth | s.total << 8 | s.best << 16 | s.full << 24;
  w1 = s.pre | s.suf << 8;
}
WALT_HD NonconvSum nonconv_unpack(uint32_t w0, uint32_t w1) {
  return NonconvSum{w0 & 0xFFu, (w0 >> 8) & 0xFFu, w1 & 0xFFu, (w1 >> 8) & 0xFFu, (w0 >> 16) & 0xFFu, (w0 >> 24) & 1u};
}

// The trips a group takes over a read of len calls whose first call sits `head` bytes behind a 16-byte boundary: the
// same for its eight lanes (a lane whose slice starts at or beyond len contributes the identity).
WALT_HD int nonconv_trips(int len, int head) { return (head + len + 16 * (int)kNonconvGroup - 1) / (16 * (int)kNonconvGroup); }

// One read as a group of the kernel takes it, on one thread: per trip the eight lanes' slices, folded pairwise in lane
// order as the three cross-lane steps fold them (through the packed words), then onto the running summary.
// before / after: as in mbias_load_slice.
WALT_HD NonconvSum nonconv_read(const uint8_t* __restrict__ rb, int len, uint64_t before, uint64_t after) {
  const int head = (int)((uintptr_t)rb & 15u);
  NonconvSum run = nonconv_identity();
  const int trips = nonconv_trips(len, head);
  for (int t = 0; t < trips; ++t) {
    NonconvSum lane[kNonconvGroup];
    for (int sub = 0; sub < (int)kNonconvGroup; ++sub) {
      const int i0 = -head + 16 * ((int)kNonconvGroup * t + sub);
      lane[sub] = nonconv_identity();
      if (i0 < len) {
        uint32_t w[4];
        mbias_load_slice(rb, len, i0, before, after, w);
        lane[sub] = nonconv_slice(w);
      }
    }
    for (int d = 1; d < (int)kNonconvGroup; d <<= 1)
      for (int sub = 0; sub + d < (int)kNonconvGroup; sub += 2 * d) {
        uint32_t w0, w1;
        nonconv_pack(lane[sub + d], w0, w1);
        lane[sub] = nonconv_combine(lane[sub], nonconv_unpack(w0, w1));
      }
    run = nonconv_combine(run, lane[0]);
  }
  return run;
}

// A record is judged when it is unique and its read has 1 to 1024 calls; tested before any address is formed.
WALT_HD bool nonconv_judged(uint32_t times, uint64_t off, uint64_t end) {
  return times == 1u && end > off && end - off <= (uint64_t)kNonconvMaxCalls;
}

WALT_HD walt_nonconv_tally nonconv_tally_of(const NonconvSum& s) {
  return walt_nonconv_tally{(uint16_t)s.meth, (uint16_t)s.total, (uint16_t)s.best, 0};
}

// the rule: any enabled test fires (a field of 0 switches its test off); integer arithmetic
WALT_HD uint32_t nonconv_fails(uint32_t meth, uint32_t total, uint32_t run, const walt_nonconv_rule& r) {
  if (r.min_meth > 0u && meth >= r.min_meth) return 1u;
  if (r.min_run > 0u && run >= r.min_run) return 1u;
  const uint32_t floor_total = r.min_total > 1u ? r.min_total : 1u;
  if (r.min_percent > 0u && total >= floor_total && 100ull * meth >= (unsigned long long)r.min_percent * total) return 1u;
  return 0u;
}
inline bool nonconv_rule_ok(const walt_nonconv_rule& r) { return r.min_percent <= 100u; }

// the pair rule, in place on the two mates' bytes: a pair that mapped as one goes when either mate fails
WALT_HD void nonconv_pair(uint32_t best_times, uint8_t& f1, uint8_t& f2) {
  if (best_times == 1u) f1 = f2 = (uint8_t)(f1 | f2);
}

}  // namespace walt
#endif  // WALT_AMD_NONCONV_CORE_H_
