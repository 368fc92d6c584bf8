// trim_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/trim_harness.cpp, and through it
// the overloads of walt_amd/csrc/meth_core.h and overlap_core.h with ignored read ends, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -I walt_amd/csrc \
//       tests/trim_sanitize_main.cpp tests/trim_harness.cpp -o trim_sanitize && ./trim_sanitize
// Random batches of reads of every interesting length on a random chromosome, with random bounds (0, small, around the
// read length, far beyond it), clip points and excluded intervals.  A batch's bases and its calls each fill a heap block
// that starts with the batch (even trials) or ends with it (odd trials: the batch at one of the 16 alignments), so a
// slice that reads or writes in front of the first base or behind the last one is reported.  Every call is also compared
// with the call without bounds, blanked outside [trim5, limit - trim3).  Prints "ok <calls>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" {
unsigned long long trim_harness_batch(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, uint8_t* calls,
                                      const uint64_t* offsets, uint32_t n, const uint32_t* recs, uint32_t lo, uint32_t hi,
                                      uint32_t trim5, uint32_t trim3);
uint32_t trim_harness_pair(const uint32_t* start, uint32_t n_chrom, uint32_t genome_len, uint32_t p1, uint32_t times1,
                           uint32_t strand1, uint32_t p2, uint32_t times2, uint32_t strand2, uint32_t best_times, uint64_t len1,
                           uint64_t len2, int has_cl1, uint32_t cl1, int has_cl2, uint32_t cl2, const uint32_t* trim, uint32_t* bases);
}

static uint32_t bound(uint32_t len) {
  switch (rand() % 8) {
    case 0: case 1: return 0;
    case 2: return 1 + rand() % 17;
    case 3: return len ? len - 1 : 0;
    case 4: return len;
    case 5: return len + 1;
    case 6: return 5000;
    default: return 0xFFFFFFFFu - (uint32_t)(rand() % 3);
  }
}

int main() {
  srand(5);
  static const int lens[] = {0, 1, 15, 16, 17, 31, 100, 127, 128, 129, 1024, 40};
  const uint32_t glen = 3000, lo = 200, hi = 2800;  // one chromosome inside a packed genome
  std::vector<uint32_t> ref((glen + 15) / 16 + 16, 0);
  for (uint32_t w = 0; w < (glen + 15) / 16; ++w) ref[w] = (uint32_t)rand() * 65536u + (uint32_t)rand();
  unsigned long long total = 0;
  for (int trial = 0; trial < 4000; ++trial) {
    const uint32_t n = 1 + rand() % 5;
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[rand() % 12];
    const size_t bytes = off[n];
    const int shift = trial & 1 ? rand() % 16 : 0;
    uint8_t* bblock = static_cast<uint8_t*>(malloc(bytes + shift ? bytes + shift : 1));
    uint8_t* cblock = static_cast<uint8_t*>(malloc(bytes + shift ? bytes + shift : 1));
    uint8_t* pblock = static_cast<uint8_t*>(malloc(bytes + shift ? bytes + shift : 1));
    uint8_t *bases = bblock + shift, *calls = cblock + shift, *plain = pblock + shift;
    for (size_t i = 0; i < bytes; ++i) bases[i] = (uint8_t)"ACGT"[rand() % 4];
    std::vector<uint32_t> recs(4 * (size_t)n);
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
      longest = len > longest ? len : longest;
      recs[4 * i] = rand() % 4 == 0 ? hi - 1 - rand() % 40 : lo + rand() % (hi - lo);  // (some run over the chromosome's end)
      recs[4 * i + 1] = rand() % 3 == 0 ? (uint32_t)(rand() % (len + 4)) : 0xFFFFFFFFu;
      recs[4 * i + 2] = (uint32_t)rand() & 1u;
      const uint32_t e_lo = len ? rand() % len : 0, e_hi = len ? e_lo + rand() % (len - e_lo + 1) : 0;
      recs[4 * i + 3] = rand() % 2 ? e_lo | (e_hi << 16) : 0u;
    }
    const uint32_t trim5 = bound(longest), trim3 = bound(longest);
    const unsigned long long got = trim_harness_batch(ref.data(), (uint32_t)ref.size() - 1, bases, calls, off.data(), n, recs.data(), lo, hi, trim5, trim3);
    trim_harness_batch(ref.data(), (uint32_t)ref.size() - 1, bases, plain, off.data(), n, recs.data(), lo, hi, 0, 0);
    unsigned long long letters = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
      const uint32_t limit = recs[4 * i + 1] < len ? recs[4 * i + 1] : len;
      for (uint32_t k = 0; k < len; ++k) {
        const bool inside = trim5 <= k && (unsigned long long)k + trim3 < limit;
        const uint8_t want = inside ? plain[off[i] + k] : (uint8_t)'.';
        if (calls[off[i] + k] != want) {
          printf("trial %d read %u position %u: got %c want %c (trim5 %u trim3 %u limit %u)\n", trial, i, k, calls[off[i] + k], want, trim5, trim3, limit);
          return 1;
        }
        letters += want != '.';
      }
    }
    if (letters != got) {
      printf("trial %d: %llu letters, counts sum to %llu\n", trial, letters, got);
      return 1;
    }
    total += got;
    free(bblock); free(cblock); free(pblock);
    // one pair with bounds of the same kinds: any value is legal, the word stays inside mate 2
    const uint32_t start[2] = {0, glen};
    const uint32_t len1 = 1 + rand() % 150, len2 = 1 + rand() % 150;
    const uint32_t t[4] = {bound(len1), bound(len1), bound(len2), bound(len2)};
    uint32_t b = 0;
    const uint32_t w = trim_harness_pair(start, 1, glen, rand() % glen, 1, rand() % 2 ? '-' : '+', rand() % glen, 1, rand() % 2 ? '-' : '+', 1,
                                         len1, len2, rand() % 2, rand() % (len1 + 2), rand() % 2, rand() % (len2 + 2), t, &b);
    if ((w >> 16) > len2 || (w && (w & 0xFFFFu) >= (w >> 16)) || b > (w >> 16) - (w & 0xFFFFu)) {
      printf("trial %d: interval word %08x with %u bases of a mate of %u\n", trial, w, b, len2);
      return 1;
    }
  }
  printf("ok %llu calls\n", total);
  return 0;
}
