// align_harness.cpp -- C entry points (TEST INFRASTRUCTURE) over the aligned mismatch count of walt_amd/csrc/core.h
// (align_word, align_read, count_mismatch_aligned, aligned_header_word) and the count it replaces in the dense
// verifiers (count_mismatch_regs).  Compiled with g++ -DWALT_SEEDPATTERN=3 / 5 / 7 by tests/test_align_cpu.py (no
// device) and, under the host's sanitizers, with tests/align_sanitize_main.cpp.  nw is 7 or 8.
#include <stdint.h>

#include "core.h"

using namespace walt;

namespace {
template <int NW>
uint32_t aligned(const uint32_t* g, uint32_t sh, const uint32_t* rd, const uint32_t* mk, uint32_t* rd_a, uint32_t* mk_a, uint32_t* top) {
  align_read<NW>(rd, mk, sh, rd_a, mk_a);
  *top = mk_a[NW] != 0u ? 1u : 0u;
  return count_mismatch_aligned<NW>(g, rd_a, mk_a, mk_a[NW] != 0u);
}
template <int NW>
void header(const uint32_t* in, uint32_t sh, uint32_t* out) {
  for (uint32_t i = 0; i < 32; ++i) out[i] = in[i];
  for (uint32_t i = 0; i < 8 + 2 * NW; ++i) out[i] = aligned_header_word<NW>(i, in[i], i ? in[i - 1] : 0u, sh);
  out[8 + 2 * NW] = aligned_header_top(in[8 + NW - 1], sh);
  out[8 + 2 * NW + 1] = aligned_header_top(in[8 + 2 * NW - 1], sh);
}
}  // namespace

extern "C" {

uint32_t align_harness_pat() { return kPat; }
uint32_t align_harness_lead() { return kWinLead; }
uint32_t align_harness_max_len1() { return kWinMaxLen1; }
uint32_t align_harness_tail_mask(uint32_t w, uint32_t lo, uint32_t hi) { return tail_mask_word(w, lo, hi); }

// count_mismatch_regs<nw>(g[nw + 1], sh, rd[nw], mk[nw])
uint32_t align_harness_regs(uint32_t nw, const uint32_t* g, uint32_t sh, const uint32_t* rd, const uint32_t* mk) {
  return nw == 7 ? count_mismatch_regs<7>(g, sh, rd, mk) : count_mismatch_regs<8>(g, sh, rd, mk);
}
// align_read<nw> into rd_a[nw + 1], mk_a[nw + 1], then count_mismatch_aligned<nw> with top = (mk_a[nw] != 0), also
// written to *top
uint32_t align_harness_aligned(uint32_t nw, const uint32_t* g, uint32_t sh, const uint32_t* rd, const uint32_t* mk, uint32_t* rd_a,
                               uint32_t* mk_a, uint32_t* top) {
  return nw == 7 ? aligned<7>(g, sh, rd, mk, rd_a, mk_a, top) : aligned<8>(g, sh, rd, mk, rd_a, mk_a, top);
}
// the same count with `top` given (what a build that drops the top word computes: top = 0)
uint32_t align_harness_count(uint32_t nw, const uint32_t* g, const uint32_t* rd_a, const uint32_t* mk_a, uint32_t top) {
  return nw == 7 ? count_mismatch_aligned<7>(g, rd_a, mk_a, top != 0u) : count_mismatch_aligned<8>(g, rd_a, mk_a, top != 0u);
}
// the 32 words the lanes of one read hold (k_se_verify_shared: lane 8 r + q, component c is word 4 q + c), aligned in place
void align_harness_header(uint32_t nw, const uint32_t* in, uint32_t sh, uint32_t* out) {
  if (nw == 7) header<7>(in, sh, out); else header<8>(in, sh, out);
}

}
