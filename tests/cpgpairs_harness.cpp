// cpgpairs_harness.cpp -- C entry points (TEST INFRASTRUCTURE) over walt_amd/csrc/cpgpairs_core.h, what the kernels of
// cpgpairs.hip run per lane, and over the Fisher test and the <out>.allelic writer of walt_amd/csrc/host/hostio.h.
// Compiled with g++ by tests/test_cpgpairs_cpu.py (no device) and, under the host's sanitizers, with
// tests/cpgpairs_sanitize_main.cpp.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "host/hostio.h"
#include "chrom_core.h"
#include "cpgpairs_core.h"

using namespace walt;

// the chromosome table as a block stages it (map_common.h chrom_tab_stage)
static std::vector<uint32_t> staged(const uint32_t* start_index, const ChromTab& tab) {
  std::vector<uint32_t> lds(kLdsChroms + 1, 0u);
  for (uint32_t i = 0; i <= tab.m; ++i) lds[i] = start_index[chrom_tab_word(tab, i)];
  return lds;
}

extern "C" {

uint64_t cpgpairs_harness_bit_words(uint64_t genome_len) { return cpg_bit_words(genome_len) + kCpgPadWords; }
uint64_t cpgpairs_harness_dir_entries(uint64_t genome_len) { return cpg_dir_entries(genome_len); }

// The bitmap and the directory of a genome given as text (ACGT), as walt_cpgpairs_create builds them: the '+' reference
// packed 2 bits per base behind 16 zero words, one bitmap word from three reference words, the last position of every
// chromosome cleared, an exclusive prefix over the blocks.  bits: cpgpairs_harness_bit_words words, dir:
// cpgpairs_harness_dir_entries.  -> the number of pairs
uint32_t cpgpairs_harness_build(const char* text, uint32_t genome_len, const uint32_t* start_index, uint32_t n_chrom,
                                uint32_t* bits, uint32_t* dir) {
  const uint64_t ref_words = ((uint64_t)genome_len + 15) / 16 + 16;
  std::vector<uint32_t> ref(ref_words, 0u);
  for (uint32_t i = 0; i < genome_len; ++i) {
    const uint32_t code = text[i] == 'C' ? 1u : text[i] == 'G' ? 2u : text[i] == 'T' ? 3u : 0u;
    ref[i >> 4] |= code << (2 * (i & 15));
  }
  const uint64_t n_words = cpg_bit_words(genome_len), ref_last = ref_words - 1;
  memset(bits, 0, 4 * (n_words + kCpgPadWords));
  for (uint64_t w = 0; w < ((uint64_t)genome_len + 31) / 32; ++w) {
    uint32_t r[3];
    for (uint32_t k = 0; k < 3; ++k) r[k] = 2 * w + k <= ref_last ? ref[2 * w + k] : 0u;
    bits[w] = cpg_pair_word(r[0], r[1], r[2]);
  }
  for (uint32_t c = 0; c < n_chrom; ++c)
    if (start_index[c + 1]) bits[cpg_end_word(start_index[c + 1])] &= cpg_end_mask(start_index[c + 1]);
  uint32_t run = 0;
  for (uint64_t b = 0; b < cpg_dir_entries(genome_len); ++b) {
    dir[b] = run;
    run += cpg_block_count(bits, b);
  }
  return run;
}

uint32_t cpgpairs_harness_rank(const uint32_t* bits, const uint32_t* dir, uint32_t p) { return cpg_rank(bits, dir, p); }
long long cpgpairs_harness_pair_at(const uint32_t* bits, uint32_t f) { return cpg_pair_at(bits, f); }
uint32_t cpgpairs_harness_next(const uint32_t* bits, uint32_t c, uint64_t n_words) { return cpg_next(bits, c, n_words); }
uint32_t cpgpairs_harness_range_mask(uint64_t w, uint32_t pos_lo, uint32_t pos_hi) { return cpg_range_mask(w, pos_lo, pos_hi); }
int cpgpairs_harness_counted(uint32_t times, uint32_t skip, uint64_t off, uint64_t end, uint32_t pos, uint32_t genome_len) {
  return cpg_counted(times, skip, off, end, pos, genome_len) ? 1 : 0;
}

// calls as the fold moves them, the combine, and one couple: out[0] = 1 when it adds, out[1] = entry, out[2] = column
uint64_t cpgpairs_harness_call(uint32_t j, uint32_t u) { return cpg_call(j, u); }
uint64_t cpgpairs_harness_combine(uint64_t a, uint64_t b) { return cpg_combine(a, b); }
void cpgpairs_harness_couple(uint64_t a, uint64_t b, uint32_t* out) {
  out[0] = out[1] = out[2] = 0;
  cpg_couple(a, b, [&](uint32_t entry, uint32_t column) { out[0] += 1; out[1] = entry; out[2] = column; });
}

// One read through the kernel's own slices, trips and scan, the pair numbers given per read position (numbers[i], -1:
// none): every add as (entry, column) into adds[2 * cap] -> how many there were.  before / after: the batch's bytes
// around rb.
uint32_t cpgpairs_harness_read(const uint8_t* rb, uint32_t len, uint64_t before, uint64_t after, const long long* numbers,
                               uint32_t* adds, uint32_t cap) {
  uint32_t n = 0;
  cpg_read(rb, (int)len, before, after, [&](int i) { return numbers[i]; },
           [&](uint32_t entry, uint32_t column) {
             if (n < cap) { adds[2 * n] = entry; adds[2 * n + 1] = column; }
             ++n;
           });
  return n;
}

// A batch as k_cpg_pairs takes it, read by read: table[n_pairs][4] += its couples; -> the number of records that counted
long long cpgpairs_harness_batch(const uint32_t* bits, const uint32_t* dir, uint32_t genome_len, const uint32_t* start_index,
                                 uint32_t n_chrom, const uint8_t* calls, const uint64_t* offsets, uint32_t n, const uint8_t* records,
                                 uint64_t rec_stride, const uint8_t* skip, uint64_t skip_stride, uint32_t* table) {
  const ChromTab tab = chrom_tab_of(n_chrom);
  const std::vector<uint32_t> lds = staged(start_index, tab);
  const uint64_t batch_lo = offsets[0], batch_hi = offsets[n];
  long long counted = 0;
  for (uint32_t r = 0; r < n; ++r) {
    const uint64_t off = offsets[r], end = offsets[r + 1];
    uint32_t rec[3];
    memcpy(rec, records + r * rec_stride, 12);
    const uint32_t pos = rec[0], times = rec[1];
    const bool minus = (rec[2] & 0xFFu) == '-';
    const uint32_t sk = skip ? skip[r * skip_stride] : 0u;
    if (!cpg_counted(times, sk, off, end, pos, genome_len) || off < batch_lo || end > batch_hi) continue;
    ++counted;
    uint32_t c_lo = 0, c_hi = 0;
    chrom_bounds(lds.data(), start_index, tab, pos, c_lo, c_hi);
    cpg_read(calls + off, (int)(end - off), off - batch_lo, batch_hi - off,
             [&](int i) -> long long {
               const long long c = cpg_call_pair(bits, pos, i, minus, c_lo, c_hi);
               return c < 0 ? -1ll : (long long)cpg_rank(bits, dir, (uint32_t)c);
             },
             [&](uint32_t entry, uint32_t column) { table[4ull * entry + column] += 1u; });
  }
  return counted;
}

double cpgpairs_harness_fisher(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return hostio::fisher_exact_two_sided(a, b, c, d); }

// one line of <out>.allelic -> its length (the text in `out`, cap bytes)
uint32_t cpgpairs_harness_allelic_line(const char* chrom, uint32_t pos, uint32_t next, const uint64_t* n, char* out, uint32_t cap) {
  hostio::Sink s;
  hostio::put_allelic_line(s, std::string(chrom), pos, next, n);
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}

}  // extern "C"
