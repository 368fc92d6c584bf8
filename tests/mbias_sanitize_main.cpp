// mbias_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/mbias_harness.cpp, and through
// it walt_amd/csrc/mbias_core.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/mbias_sanitize_main.cpp tests/mbias_harness.cpp -o mbias_sanitize && ./mbias_sanitize
// Random batches of reads of every interesting length; a batch's calls fill a heap block exactly when the block starts
// at the batch (even trials) or end with it (odd trials: the batch sits at one of the 16 alignments), so a slice that
// reads in front of the first call or behind the last one is reported.  Prints "ok <adds>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" long long mbias_harness_batch(const uint8_t* calls, const uint64_t* offsets, uint32_t n, const uint8_t* records,
                                         uint64_t rec_stride, const uint8_t* skip, uint64_t skip_stride, uint64_t* count);

int main() {
  srand(3);
  static const char al[] = "zZxXhHuU....ACGT";
  static const int lens[] = {0, 1, 15, 16, 17, 31, 127, 128, 129, 1024, 1025, 40};
  long long total = 0;
  for (int trial = 0; trial < 6000; ++trial) {
    const uint32_t n = 1 + rand() % 6;
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[rand() % 12];
    const size_t bytes = off[n];
    const int shift = trial & 1 ? rand() % 16 : 0;
    uint8_t* block = static_cast<uint8_t*>(malloc(bytes + shift ? bytes + shift : 1));
    uint8_t* calls = block + shift;  // [calls, calls + bytes) ends with the block; it starts with it when shift is 0
    for (size_t i = 0; i < bytes; ++i) calls[i] = (uint8_t)al[rand() % 16];
    std::vector<uint8_t> rec(n * 16, 0);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t t = rand() % 3;
      memcpy(&rec[i * 16 + 4], &t, 4);
    }
    std::vector<uint64_t> count(8192, 0);
    const long long adds = mbias_harness_batch(calls, off.data(), n, rec.data(), 16, nullptr, 1, count.data());
    free(block);
    if (adds < 0) {
      printf("an add outside the table or the read, trial %d\n", trial);
      return 1;
    }
    total += adds;
  }
  printf("ok %lld adds\n", total);
  return 0;
}
