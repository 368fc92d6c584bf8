// epialleles_sanitize_main.cpp -- stand-alone program (TEST INFRASTRUCTURE) that drives tests/epialleles_harness.cpp, and
// through it walt_amd/csrc/epialleles_core.h, under the host's sanitizers:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -I walt_amd/csrc \
//       tests/epialleles_sanitize_main.cpp tests/epialleles_harness.cpp tests/cpgpairs_harness.cpp -o epialleles_sanitize
// Random CpG-rich genomes of one to five chromosomes -- bitmap, directory and table in heap blocks of exactly their size --
// and random batches of reads of every interesting length on both strands; a batch's calls fill a heap block exactly: the
// block starts with the batch's first call (even trials) or ends with its last (odd trials: the batch sits at one of the
// 16 alignments), so a slice that reads in front of the first call or behind the last one is reported, and so is a bitmap,
// directory or table index outside its array.  Every table is compared with a plain walk over the genome's text and the
// reads' bytes: every four calls that follow each other on neighbouring pairs.  Prints "ok <windows>" and returns 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" {
uint64_t cpgpairs_harness_bit_words(uint64_t genome_len);
uint64_t cpgpairs_harness_dir_entries(uint64_t genome_len);
uint32_t cpgpairs_harness_build(const char* text, uint32_t genome_len, const uint32_t* start_index, uint32_t n_chrom, uint32_t* bits,
                                uint32_t* dir);
long long epi_harness_batch(const uint32_t* bits, const uint32_t* dir, uint32_t genome_len, const uint32_t* start_index,
                            uint32_t n_chrom, const uint8_t* calls, const uint64_t* offsets, uint32_t n, const uint8_t* records,
                            uint64_t rec_stride, const uint8_t* skip, uint64_t skip_stride, uint32_t* table);
}

int main() {
  srand(11);
  static const char dense[] = "zZzZzZzZzZzZzZ.x", sparse[] = "zZzZzZ....xHA#zZ";
  static const int lens[] = {0, 1, 15, 16, 17, 31, 127, 128, 129, 1024, 1025, 300};
  long long total = 0;
  for (int trial = 0; trial < 1500; ++trial) {
    const uint32_t n_chrom = 1 + rand() % 5;
    std::vector<uint32_t> start(n_chrom + 1, 0);
    for (uint32_t c = 0; c < n_chrom; ++c) start[c + 1] = start[c] + 1 + rand() % (trial % 4 ? 900 : 40);
    const uint32_t glen = start[n_chrom];
    std::string text(glen, 'A');
    const char* gal = trial % 5 == 0 ? "CG" : trial % 5 == 1 ? "AT" : trial % 5 == 2 ? "ACGT" : "ACGCGT";
    for (uint32_t i = 0; i < glen; ++i) text[i] = gal[rand() % strlen(gal)];
    std::vector<long long> number(glen, -1);  // the plain scan: the number of the pair that starts at c
    uint32_t n_pairs = 0;
    for (uint32_t c = 0; c < n_chrom; ++c)
      for (uint32_t f = start[c]; f + 1 < start[c + 1]; ++f)
        if (text[f] == 'C' && text[f + 1] == 'G') number[f] = n_pairs++;
    uint32_t* bits = static_cast<uint32_t*>(malloc(4 * cpgpairs_harness_bit_words(glen)));
    uint32_t* dir = static_cast<uint32_t*>(malloc(4 * cpgpairs_harness_dir_entries(glen)));
    if (cpgpairs_harness_build(text.data(), glen, start.data(), n_chrom, bits, dir) != n_pairs) {
      printf("trial %d: the bitmap holds another number of pairs than the scan's %u\n", trial, n_pairs);
      return 1;
    }
    uint32_t* table = static_cast<uint32_t*>(calloc(n_pairs ? 16 * (size_t)n_pairs : 1, 4));
    std::vector<uint32_t> want(16 * (size_t)n_pairs + 1, 0);
    const uint32_t n = 1 + rand() % 6;
    const char* al = trial % 3 ? dense : sparse;
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[rand() % 12];
    const size_t bytes = off[n];
    const int shift = trial & 1 ? rand() % 16 : 0;
    uint8_t* block = static_cast<uint8_t*>(malloc(bytes + shift ? bytes + shift : 1));
    uint8_t* calls = block + shift;  // [calls, calls + bytes) ends with the block; it starts with it when shift is 0
    for (size_t i = 0; i < bytes; ++i) calls[i] = (uint8_t)al[rand() % 16];
    std::vector<uint8_t> rec(n * 16, 0), skip(n, 0);
    long long want_counted = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t times = rand() % 5 ? 1 : rand() % 3, pos = rand() % 9 ? rand() % glen : glen + rand() % 3;
      const bool minus = rand() % 2;
      const uint32_t strand = minus ? '-' : '+';
      skip[i] = rand() % 6 ? 0 : 1 + rand() % 200;
      memcpy(&rec[i * 16], &pos, 4);
      memcpy(&rec[i * 16 + 4], &times, 4);
      memcpy(&rec[i * 16 + 8], &strand, 4);
      const uint64_t len = off[i + 1] - off[i];
      if (times != 1 || skip[i] || len < 1 || len > 1024 || pos >= glen) continue;
      ++want_counted;
      uint32_t c = 0;
      while (start[c + 1] <= pos) ++c;
      const long long lo = start[c], hi = start[c + 1];
      std::vector<long long> js, us;  // the calls that have a pair, in read order
      for (uint64_t k = 0; k < len; ++k) {
        const uint8_t b = calls[off[i] + k];
        const long long q = (long long)pos + (long long)k;
        if ((b != 'z' && b != 'Z') || q >= hi) continue;
        const long long f = minus ? lo + hi - 1 - q : q;
        const long long j = number[f] >= 0 ? number[f] : f > 0 ? number[f - 1] : -1;
        if (j < 0) continue;
        js.push_back(j);
        us.push_back(b == 'z');
      }
      for (size_t t = 0; t + 3 < js.size(); ++t) {
        const long long s = js[t + 1] - js[t];
        if ((s != 1 && s != -1) || js[t + 2] != js[t] + 2 * s || js[t + 3] != js[t] + 3 * s) continue;
        if (s == 1) want[16 * js[t] + 8 * us[t] + 4 * us[t + 1] + 2 * us[t + 2] + us[t + 3]] += 1;
        else want[16 * js[t + 3] + 8 * us[t + 3] + 4 * us[t + 2] + 2 * us[t + 1] + us[t]] += 1;
      }
    }
    const long long counted = epi_harness_batch(bits, dir, glen, start.data(), n_chrom, calls, off.data(), n, rec.data(), 16,
                                                skip.data(), 1, table);
    bool same = counted == want_counted;
    for (size_t w = 0; same && w < 16 * (size_t)n_pairs; ++w) {
      same = table[w] == want[w];
      total += table[w];
    }
    free(block); free(table); free(dir); free(bits);
    if (!same) {
      printf("trial %d: the table or the number of counted records (%lld, %lld expected) differs from the plain walk\n", trial, counted,
             want_counted);
      return 1;
    }
  }
  if (total < 1000) {
    printf("only %lld windows: the trials do not reach the fold\n", total);
    return 1;
  }
  printf("ok %lld windows\n", total);
  return 0;
}
