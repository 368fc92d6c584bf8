// align_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/align_harness.cpp, and through
// it the aligned mismatch count of walt_amd/csrc/core.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DWALT_SEEDPATTERN=3 -I walt_amd/csrc \
//       tests/align_sanitize_main.cpp tests/align_harness.cpp -o align_sanitize && ./align_sanitize
// For 7 and 8 words, every seed shift and every length 16 NW - kWinLead - 3 .. 16 NW: random windows, reads and
// even-bit masks in heap blocks of exactly NW + 1, NW and NW words, so a word read or written outside them is reported,
// as is a shift by more than the operand's width.  Every count is compared with count_mismatch_regs, the top flag with
// its rule, the header form with align_read.  Prints "ok <cases>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" {
uint32_t align_harness_pat();
uint32_t align_harness_lead();
uint32_t align_harness_tail_mask(uint32_t w, uint32_t lo, uint32_t hi);
uint32_t align_harness_regs(uint32_t nw, const uint32_t* g, uint32_t sh, const uint32_t* rd, const uint32_t* mk);
uint32_t align_harness_aligned(uint32_t nw, const uint32_t* g, uint32_t sh, const uint32_t* rd, const uint32_t* mk, uint32_t* rd_a,
                               uint32_t* mk_a, uint32_t* top);
void align_harness_header(uint32_t nw, const uint32_t* in, uint32_t sh, uint32_t* out);
}

static uint32_t rnd32() { return ((uint32_t)rand() << 17) ^ ((uint32_t)rand() << 5) ^ (uint32_t)rand(); }

int main() {
  srand(17);
  const uint32_t pat = align_harness_pat(), lead = align_harness_lead();
  long long cases = 0;
  for (uint32_t nw = 7; nw <= 8; ++nw)
    for (uint32_t seed_i = 0; seed_i < pat; ++seed_i)
      for (uint32_t len = 16 * nw - lead - 3; len <= 16 * nw; ++len)
        for (int trial = 0; trial < 40; ++trial) {
          const uint32_t sh = 2 * (lead - seed_i);
          uint32_t* g = static_cast<uint32_t*>(malloc((nw + 1) * 4));
          uint32_t* rd = static_cast<uint32_t*>(malloc(nw * 4));
          uint32_t* mk = static_cast<uint32_t*>(malloc(nw * 4));
          uint32_t* rd_a = static_cast<uint32_t*>(malloc((nw + 1) * 4));
          uint32_t* mk_a = static_cast<uint32_t*>(malloc((nw + 1) * 4));
          uint32_t* hdr = static_cast<uint32_t*>(malloc(32 * 4));
          uint32_t* out = static_cast<uint32_t*>(malloc(32 * 4));
          for (uint32_t w = 0; w <= nw; ++w) g[w] = rnd32();
          for (uint32_t w = 0; w < nw; ++w) {
            rd[w] = rnd32();
            mk[w] = align_harness_tail_mask(w, 0, len) & (trial % 2 ? 0xFFFFFFFFu : rnd32() | (w + 1 == nw ? 0xFFFFF000u : 0u));  // (the last base, at 16 NW - 10 or above, is always compared)
          }
          uint32_t top = 7;
          const uint32_t want = align_harness_regs(nw, g, sh, rd, mk);
          const uint32_t got = align_harness_aligned(nw, g, sh, rd, mk, rd_a, mk_a, &top);
          bool ok = want == got && top == (len + lead - seed_i > 16 * nw ? 1u : 0u);
          for (uint32_t i = 0; i < 32; ++i) hdr[i] = rnd32();
          for (uint32_t w = 0; w < nw; ++w) { hdr[8 + w] = rd[w]; hdr[8 + nw + w] = mk[w]; }
          align_harness_header(nw, hdr, sh, out);
          for (uint32_t i = 0; i < 32; ++i) {
            uint32_t v = hdr[i];
            if (i >= 8 && i < 8 + nw) v = rd_a[i - 8];
            else if (i >= 8 + nw && i < 8 + 2 * nw) v = mk_a[i - 8 - nw];
            else if (i == 8 + 2 * nw) v = rd_a[nw];
            else if (i == 8 + 2 * nw + 1) v = mk_a[nw];
            ok = ok && out[i] == v;
          }
          free(g); free(rd); free(mk); free(rd_a); free(mk_a); free(hdr); free(out);
          if (!ok) {
            printf("nw %u seed_i %u len %u trial %d: count %u against %u, top %u\n", nw, seed_i, len, trial, got, want, top);
            return 1;
          }
          ++cases;
        }
  printf("ok %lld cases\n", cases);
  return 0;
}
