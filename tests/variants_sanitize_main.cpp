// variants_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/variants_harness.cpp, and
// through it walt_amd/csrc/variants_core.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -I walt_amd/csrc \
//       tests/variants_sanitize_main.cpp tests/variants_harness.cpp -o variants_sanitize && ./variants_sanitize
// Random genomes (chromosomes of 1, 2 and 17 bases among them) and reads of every interesting length at every alignment;
// the batch's bases, the packed reference and the two counter planes each fill a heap block of exactly their size, the
// bases ending with their block (odd trials) or starting with it (even trials), so a load or an add outside them ends the
// program.  Every read's adds are compared with a plain walk.  Prints "ok <adds>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" long long variants_harness_read(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, uint32_t head, uint64_t off,
                                           uint64_t total, uint64_t batch_bytes, uint32_t limit, uint32_t pos, uint32_t lo,
                                           uint32_t hi, uint32_t ga, int minus, uint32_t* match, uint32_t* other);

static uint32_t code_of(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }

int main() {
  srand(7);
  static const uint32_t chrom_len[] = {700, 1, 2, 17, 1300, 64};
  static const int lens[] = {1, 15, 16, 17, 31, 100, 127, 128, 129, 1023, 1024, 40};
  uint32_t start[7] = {0};
  for (int c = 0; c < 6; ++c) start[c + 1] = start[c] + chrom_len[c];
  const uint32_t glen = start[6];
  long long total_adds = 0;
  for (int trial = 0; trial < 4000; ++trial) {
    std::vector<char> text(glen);
    for (uint32_t i = 0; i < glen; ++i) text[i] = "ACGTCG"[rand() % 6];
    const uint32_t nwords = (glen + 15) / 16, pad = 16;
    uint32_t* ref = static_cast<uint32_t*>(calloc(nwords + pad, 4));  // exactly the words the library keeps
    for (uint32_t i = 0; i < glen; ++i) ref[i >> 4] |= code_of(text[i]) << (2 * (i & 15));
    const int c = rand() % 6;
    const uint32_t lo = start[c], hi = start[c + 1];
    const uint32_t pos = lo + rand() % (hi - lo);
    const uint32_t n = (uint32_t)lens[rand() % 12];
    const uint32_t limit = rand() % 3 ? n : (uint32_t)(rand() % (n + 1));
    const uint32_t ga = rand() & 1, minus = rand() & 1;
    const uint64_t off = trial % 5 ? (uint64_t)(rand() % 40) : 0, behind = trial % 3 ? (uint64_t)(rand() % 40) : 0;
    const uint64_t bytes = off + n + behind;
    const int shift = trial & 1 ? rand() % 16 : 0;
    uint8_t* block = static_cast<uint8_t*>(malloc(bytes + shift));
    uint8_t* bases = block + shift;
    for (uint64_t i = 0; i < bytes; ++i) bases[i] = rand() % 20 ? (uint8_t)"ACGT"[rand() % 4] : (uint8_t)(rand() % 256);
    uint32_t* match = static_cast<uint32_t*>(calloc(glen, 4));
    uint32_t* other = static_cast<uint32_t*>(calloc(glen, 4));
    const uint32_t head = (uint32_t)((uintptr_t)(bases + off) & 15u);
    const long long adds = variants_harness_read(ref, nwords + pad - 1, bases, head, off, n, bytes, limit, pos, lo, hi, ga, (int)minus,
                                                 match, other);
    // the plain walk; the reference of a '-' record is R itself here: the kernel's arithmetic is the same for R and R'
    long long want = 0;
    bool same = adds >= 0;
    for (uint32_t i = 0; i < limit && pos + i < hi; ++i) {
      const uint32_t q = pos + i, f = minus ? lo + hi - 1 - q : q;
      if (text[q] != (ga ? 'C' : 'G')) continue;
      const uint32_t field = (bases[off + i] >> 1) & 3u;  // A 0, C 1, T 2, G 3
      uint32_t* plane = field == (ga ? 1u : 3u) ? match : other;
      if (!plane[f]) same = false; else plane[f] -= 1;
      ++want;
    }
    for (uint32_t f = 0; f < glen; ++f) same = same && !match[f] && !other[f];
    free(block); free(ref); free(match); free(other);
    if (!same || adds != want) {
      printf("trial %d: %lld adds, the walk has %lld%s\n", trial, adds, want, same ? "" : ", at other positions");
      return 1;
    }
    total_adds += adds;
  }
  printf("ok %lld adds\n", total_adds);
  return 0;
}
