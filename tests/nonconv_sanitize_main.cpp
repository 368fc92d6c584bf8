// nonconv_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/nonconv_harness.cpp, and
// through it walt_amd/csrc/nonconv_core.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/nonconv_sanitize_main.cpp tests/nonconv_harness.cpp -o nonconv_sanitize && ./nonconv_sanitize
// Random batches of reads of every interesting length; a batch's calls fill a heap block exactly: the block starts with
// the batch's first call (even trials) or ends with its last (odd trials: the batch sits at one of the 16 alignments), so
// a slice that reads in front of the first call or behind the last one is reported.  Every tally is compared with a plain
// loop over the read's bytes, every verdict with the rule written out.  Prints "ok <judged reads>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

struct Tally {
  uint16_t meth, total, run, reserved;
};
extern "C" long long nonconv_harness_batch(const uint8_t* calls, const uint64_t* offsets, uint32_t n, const uint8_t* records,
                                           uint64_t rec_stride, const uint32_t* rule4, uint8_t* filt, Tally* tally);

int main() {
  srand(5);
  static const char dense[] = "HHHHXXXXhxHXHXHH", sparse[] = "zZxXhHuU....ACGT";
  static const int lens[] = {0, 1, 15, 16, 17, 31, 127, 128, 129, 1024, 1025, 40};
  long long total = 0;
  for (int trial = 0; trial < 6000; ++trial) {
    const uint32_t n = 1 + rand() % 6;
    const char* al = trial % 3 ? sparse : dense;
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[rand() % 12];
    const size_t bytes = off[n];
    const int shift = trial & 1 ? rand() % 16 : 0;
    uint8_t* block = static_cast<uint8_t*>(malloc(bytes + shift ? bytes + shift : 1));
    uint8_t* calls = block + shift;  // [calls, calls + bytes) ends with the block; it starts with it when shift is 0
    for (size_t i = 0; i < bytes; ++i) calls[i] = (uint8_t)al[rand() % 16];
    std::vector<uint8_t> rec(n * 16, 0);
    std::vector<uint32_t> times(n);
    for (uint32_t i = 0; i < n; ++i) {
      times[i] = rand() % 4 ? 1 : rand() % 3;
      memcpy(&rec[i * 16 + 4], &times[i], 4);
    }
    const uint32_t rule[4] = {(uint32_t)(rand() % 3 ? rand() % 40 : 0), (uint32_t)(rand() % 3 ? rand() % 12 : 0),
                              (uint32_t)(rand() % 3 ? rand() % 101 : 0), (uint32_t)(rand() % 20)};
    std::vector<uint8_t> filt(n, 9);
    std::vector<Tally> tally(n);
    const long long judged = nonconv_harness_batch(calls, off.data(), n, rec.data(), 16, rule, filt.data(), tally.data());
    long long want_judged = 0;
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t meth = 0, tot = 0, run = 0, cur = 0, fails = 0;
      const uint64_t len = off[i + 1] - off[i];
      if (times[i] == 1 && len >= 1 && len <= 1024) {
        ++want_judged;
        for (uint64_t k = off[i]; k < off[i + 1]; ++k) {
          const uint8_t b = calls[k];
          if (b == 'H' || b == 'X') { ++meth; ++tot; ++cur; if (cur > run) run = cur; }
          else if (b == 'h' || b == 'x') { ++tot; cur = 0; }
        }
        fails = (rule[0] > 0 && meth >= rule[0]) || (rule[1] > 0 && run >= rule[1]) ||
                (rule[2] > 0 && tot >= (rule[3] > 1 ? rule[3] : 1) && 100ull * meth >= (unsigned long long)rule[2] * tot);
      }
      if (tally[i].meth != meth || tally[i].total != tot || tally[i].run != run || tally[i].reserved != 0 || filt[i] != fails) {
        printf("trial %d read %u: tally (%u, %u, %u) verdict %u, the plain loop (%u, %u, %u) verdict %u\n", trial, i, tally[i].meth,
               tally[i].total, tally[i].run, filt[i], meth, tot, run, fails);
        free(block);
        return 1;
      }
    }
    free(block);
    if (judged != want_judged) {
      printf("trial %d: %lld reads judged, %lld expected\n", trial, judged, want_judged);
      return 1;
    }
    total += judged;
  }
  printf("ok %lld judged reads\n", total);
  return 0;
}
