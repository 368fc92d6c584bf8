// pileup_core.h -- per-cytosine methylation pile-up (include/walt_amd.h, "methylation pile-up"): where a slice's calls
// land on the forward strand, and the strand and context of a covered position.  Pure inline functions shared by the
// HIP kernels (pileup.hip, meth.hip) and a g++ unit test (tests/test_pileup_cpu.py compiles tests/pileup_harness.cpp).
#ifndef WALT_AMD_PILEUP_CORE_H_
#define WALT_AMD_PILEUP_CORE_H_

#include "meth_core.h"

namespace walt {

// Forward position of position q of a record's strand genome, q inside the chromosome [lo, hi): the '-' genomes are
// reverse-complemented chromosome by chromosome, so both strands share the chromosome starts.
WALT_HD uint32_t pile_forward(long long q, bool minus, uint32_t lo, uint32_t hi) {
  return minus ? (uint32_t)((long long)lo + (long long)hi - 1 - q) : (uint32_t)q;
}

// The calls of one slice (meth_read_slice's cm / cu; slice position k is genome position q0 + k of the record's
// strand): add(f, methylated) once per call, in slice order -- descending f on the '-' strand.
template <class Add>
WALT_HD void pile_slice(uint32_t cm, uint32_t cu, long long q0, bool minus, uint32_t lo, uint32_t hi, Add&& add) {
  uint32_t bits = cm | cu;  // (disjoint: a base is called one way)
  while (bits) {
    const uint32_t b = (uint32_t)__builtin_ctz(bits);
    bits &= bits - 1u;
    add(pile_forward(q0 + (long long)(b >> 1), minus, lo, hi), ((cm >> b) & 1u) != 0u);
  }
}

// Strand and context of forward position f inside the chromosome [lo, hi), from the '+' reference alone.
//   ext   meth_ref_ext(R, f - 2, last): the codes (A 0, C 1, G 2, T 3) of positions f - 2 .. f + 29
// false: R[f] is A or T (calls there were made on an independent fill of the '-' files: off-reference, no site).
// C: strand '+', context ahead, key G.  G: strand '-', context behind, key C.  Context 0 CpG, 1 CHG, 2 CHH, 3 unknown.
WALT_HD bool pile_site(unsigned long long ext, uint32_t f, uint32_t lo, uint32_t hi, uint8_t& strand, uint8_t& context) {
  const uint32_t cur = (uint32_t)(ext >> 4) & 3u;
  if (cur != 1u && cur != 2u) return false;
  const bool g = cur == 2u;
  const uint32_t n1 = (uint32_t)(g ? ext >> 2 : ext >> 6) & 3u, n2 = (uint32_t)(g ? ext : ext >> 8) & 3u;
  const uint32_t key = g ? 1u : 2u;
  const long long q = f;
  const bool in1 = g ? q - 1 >= (long long)lo : q + 1 < (long long)hi;
  const bool in2 = g ? q - 2 >= (long long)lo : q + 2 < (long long)hi;
  strand = g ? (uint8_t)'-' : (uint8_t)'+';
  context = !in1 ? 3u : n1 == key ? 0u : !in2 ? 3u : n2 == key ? 1u : 2u;
  return true;
}

}  // namespace walt
#endif  // WALT_AMD_PILEUP_CORE_H_
