// qual_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/qual_harness.cpp, and through it
// the quality-aware slice readers of walt_amd/csrc/meth_core.h and variants_core.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -I walt_amd/csrc \
//       tests/qual_sanitize_main.cpp tests/qual_harness.cpp -o qual_sanitize && ./qual_sanitize
// Random batches of three reads of every interesting length; the quality array is a heap block of exactly offsets[n]
// bytes, and so are the bases, so a load in front of or behind either ends the program (the first and the last read of a
// batch take the byte-by-byte path, the middle one the 16-byte loads).  Every read's calls are compared with the plain
// reader's calls with '.' where the quality byte is below the floor, its evidence with the plain walk.  Prints
// "ok <letters kept> <letters masked> <evidence adds>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" void qual_harness_read(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, const uint8_t* quals, uint8_t* calls,
                                  uint64_t off, uint64_t total, uint64_t batch_bytes, uint32_t limit, uint32_t pos, uint32_t lo,
                                  uint32_t hi, uint32_t ga, uint32_t ex_lo, uint32_t ex_hi, uint32_t trim5, uint32_t trim3,
                                  uint32_t min_qual, uint16_t* counts8, uint8_t* cmu);
extern "C" long long qual_harness_evidence(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, const uint8_t* quals,
                                           uint64_t off, uint64_t total, uint64_t batch_bytes, uint32_t limit, uint32_t pos,
                                           uint32_t lo, uint32_t hi, uint32_t ga, int minus, uint32_t min_qual, uint32_t* match,
                                           uint32_t* other);

static uint32_t code_of(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }

int main() {
  srand(11);
  static const int lens[] = {1, 15, 16, 17, 33, 100, 128, 1024};
  static const uint32_t floors[] = {0, 1, 2, 33, 35, 53, 64, 74, 126, 127};
  const uint32_t glen = 2400, lo = 0, hi = glen;
  long long kept = 0, masked = 0, ev_adds = 0;
  for (int trial = 0; trial < 3000; ++trial) {
    std::vector<char> text(glen);
    for (uint32_t i = 0; i < glen; ++i) text[i] = "ACGTCG"[rand() % 6];
    const uint32_t nwords = (glen + 15) / 16, pad = 16;
    uint32_t* ref = static_cast<uint32_t*>(calloc(nwords + pad, 4));
    for (uint32_t i = 0; i < glen; ++i) ref[i >> 4] |= code_of(text[i]) << (2 * (i & 15));
    const uint32_t t = floors[rand() % 10];
    const uint8_t pool[7] = {0, (uint8_t)(t ? t - 1 : 0), (uint8_t)t, (uint8_t)(t + 1), 127, 128, 255};
    uint64_t offsets[4] = {0, 0, 0, 0};
    for (int r = 0; r < 3; ++r) offsets[r + 1] = offsets[r] + (uint64_t)lens[rand() % 8];
    const uint64_t bytes = offsets[3];
    uint8_t* bases = static_cast<uint8_t*>(malloc(bytes));
    uint8_t* quals = static_cast<uint8_t*>(malloc(bytes));  // exactly offsets[n] bytes
    const int shift = rand() % 16;
    uint8_t* block = static_cast<uint8_t*>(malloc(bytes + shift + 16));
    uint8_t* plain_block = static_cast<uint8_t*>(malloc(bytes + shift + 16));
    for (uint64_t i = 0; i < bytes; ++i) { bases[i] = (uint8_t)"ACGT"[rand() % 4]; quals[i] = pool[rand() % 7]; }
    for (int r = 0; r < 3; ++r) {
      const uint64_t off = offsets[r], n = offsets[r + 1] - off;
      const uint32_t pos = (uint32_t)(rand() % (glen - 8)), ga = rand() & 1, minus = rand() & 1;
      const uint32_t limit = rand() % 3 ? (uint32_t)n : (uint32_t)(rand() % (n + 1));
      const uint32_t ex_lo = rand() % 4 ? 0 : (uint32_t)(rand() % (n + 1)), ex_hi = ex_lo ? ex_lo + (uint32_t)(rand() % 20) : 0;
      const uint32_t trim5 = rand() % 3 ? 0 : (uint32_t)(rand() % 20), trim3 = rand() % 3 ? 0 : (uint32_t)(rand() % 20);
      uint16_t c_plain[8], c_got[8];
      memset(block, '#', bytes + shift + 16);
      memset(plain_block, '#', bytes + shift + 16);
      qual_harness_read(ref, nwords + pad - 1, bases, nullptr, plain_block + shift, off, n, bytes, limit, pos, lo, hi, ga, ex_lo, ex_hi,
                        trim5, trim3, 0, c_plain, nullptr);
      qual_harness_read(ref, nwords + pad - 1, bases, quals, block + shift, off, n, bytes, limit, pos, lo, hi, ga, ex_lo, ex_hi, trim5,
                        trim3, t, c_got, nullptr);
      uint32_t want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (uint64_t i = 0; i < n; ++i) {
        const uint8_t plain = plain_block[shift + off + i], got = block[shift + off + i];
        const uint8_t w = quals[off + i] >= t ? plain : (uint8_t)'.';
        if (got != w) { printf("trial %d read %d position %llu: '%c', want '%c'\n", trial, r, (unsigned long long)i, got, w); return 1; }
        if (plain != '.') (w == '.' ? masked : kept) += 1;
        const int ctx = (w | 0x20) == 'z' ? 0 : (w | 0x20) == 'x' ? 1 : (w | 0x20) == 'h' ? 2 : (w | 0x20) == 'u' ? 3 : -1;
        if (ctx >= 0) want[(w & 0x20 ? 4 : 0) + ctx] += 1;
      }
      for (int k = 0; k < 8; ++k)
        if (c_got[k] != want[k]) { printf("trial %d read %d: count %d is %u, the letters have %u\n", trial, r, k, c_got[k], want[k]); return 1; }
      for (uint64_t i = 0; i < bytes + shift + 16; ++i)
        if ((i < shift + off || i >= shift + off + n) && block[i] != '#') { printf("trial %d read %d: wrote outside the read\n", trial, r); return 1; }
      // the evidence of the same read, as a counted record
      uint32_t* match = static_cast<uint32_t*>(calloc(glen, 4));
      uint32_t* other = static_cast<uint32_t*>(calloc(glen, 4));
      const long long adds = qual_harness_evidence(ref, nwords + pad - 1, bases, quals, off, n, bytes, limit, pos, lo, hi, ga, (int)minus,
                                                   t, match, other);
      long long want_adds = 0;
      bool same = adds >= 0;
      for (uint32_t i = 0; i < limit && pos + i < hi; ++i) {
        const uint32_t q = pos + i, f = minus ? lo + hi - 1 - q : q;
        if (text[q] != (ga ? 'C' : 'G') || quals[off + i] < t) continue;
        const uint32_t field = (bases[off + i] >> 1) & 3u;  // A 0, C 1, T 2, G 3
        uint32_t* plane = field == (ga ? 1u : 3u) ? match : other;
        if (!plane[f]) same = false; else plane[f] -= 1;
        ++want_adds;
      }
      for (uint32_t f = 0; f < glen; ++f) same = same && !match[f] && !other[f];
      free(match); free(other);
      if (!same || adds != want_adds) { printf("trial %d read %d: %lld evidence adds, the walk has %lld\n", trial, r, adds, want_adds); return 1; }
      ev_adds += adds;
    }
    free(bases); free(quals); free(block); free(plain_block); free(ref);
  }
  printf("ok %lld %lld %lld\n", kept, masked, ev_adds);
  return 0;
}
