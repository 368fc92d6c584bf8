// epialleles_harness.cpp -- C entry points (TEST INFRASTRUCTURE) over walt_amd/csrc/epialleles_core.h, what the kernel of
// epialleles.hip runs per lane, and over the statistics, the <out>.epialleles writer and the merge of
// walt_amd/csrc/host/hostio.h.  Compiled with g++ together with tests/cpgpairs_harness.cpp (the bitmap and its directory)
// by tests/test_epialleles_cpu.py (no device) and, under the host's sanitizers, with tests/epialleles_sanitize_main.cpp.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "host/hostio.h"
#include "chrom_core.h"
#include "epialleles_core.h"

using namespace walt;

static std::vector<uint32_t> staged(const uint32_t* start_index, const ChromTab& tab) {
  std::vector<uint32_t> lds(kLdsChroms + 1, 0u);
  for (uint32_t i = 0; i <= tab.m; ++i) lds[i] = start_index[chrom_tab_word(tab, i)];
  return lds;
}

extern "C" {

// chain(S) of a stretch of n calls (js: pair numbers, us: states), built call by call as a slice is walked
uint64_t epi_harness_chain(const uint32_t* js, const uint32_t* us, uint32_t n) {
  unsigned long long c = 0;
  for (uint32_t k = 0; k < n; ++k) c = epi_push(c, js[k], us[k], [](uint32_t, uint32_t) {});
  return epi_set_whole(c, epi_len(c) == n);
}
uint64_t epi_harness_pack(uint32_t j, uint32_t len, uint32_t down, uint32_t states, uint32_t whole) {
  return epi_pack(j, len, down, states, whole);
}

// Every stretch of up to max_calls calls on `numbers` pair numbers, a call a digit j * 2 + u of base 2 * numbers, the
// stretches of one length side by side behind those of the shorter ones (the first call the lowest digit).  ref[code(S)]:
// the chain the test worked out.  Checked: the walk gives ref[S]; combine(ref[A], ref[B]) == ref[A ++ B] for every split;
// combine is associative over every split in three; 0 is the identity.  -> how many of these fail (first_bad: one of them)
uint64_t epi_harness_check_all(const uint64_t* ref, uint32_t numbers, uint32_t max_calls, uint64_t* first_bad) {
  const uint64_t base = 2ull * numbers;
  std::vector<uint64_t> first(max_calls + 2, 0), pw(max_calls + 2, 1);
  for (uint32_t n = 0; n <= max_calls; ++n) {
    pw[n + 1] = pw[n] * base;
    first[n + 1] = first[n] + pw[n];
  }
  uint64_t bad = 0;
  const auto fail = [&](uint64_t code) { if (!bad++) *first_bad = code; };
  for (uint32_t n = 0; n <= max_calls; ++n)
    for (uint64_t s = 0; s < pw[n]; ++s) {
      const uint64_t code = first[n] + s;
      uint32_t js[16], us[16];
      for (uint32_t k = 0; k < n; ++k) {
        const uint64_t digit = s / pw[k] % base;
        js[k] = (uint32_t)(digit >> 1);
        us[k] = (uint32_t)(digit & 1u);
      }
      if (epi_harness_chain(js, us, n) != ref[code]) fail(code);
      if (epi_combine(ref[code], 0) != ref[code] || epi_combine(0, ref[code]) != ref[code]) fail(code);
      // S = A ++ B ++ C with A the first x calls, B the next y - x
      for (uint32_t x = 0; x <= n; ++x)
        for (uint32_t y = x; y <= n; ++y) {
          const uint64_t a = ref[first[x] + s % pw[x]];
          const uint64_t b = ref[first[y - x] + s / pw[x] % pw[y - x]];
          const uint64_t c = ref[first[n - y] + s / pw[y]];
          const uint64_t bc = ref[first[n - x] + s / pw[x]];
          if (epi_combine(b, c) != bc || epi_combine(a, bc) != ref[code]) fail(code);
          if (epi_combine(epi_combine(a, b), c) != ref[code]) fail(code);
        }
    }
  return bad;
}

// One read through the kernel's own slices, trips and scan, the pair numbers given per read position (numbers[i], -1:
// none): every add as (entry, column) into adds[2 * cap] -> how many there were; asked[i] += 1 per rank gathered.
uint32_t epi_harness_read(const uint8_t* rb, uint32_t len, uint64_t before, uint64_t after, const long long* numbers,
                          uint32_t* adds, uint32_t cap, uint32_t* asked) {
  uint32_t n = 0;
  epi_read(rb, (int)len, before, after,
           [&](int i) {
             if (asked) asked[i] += 1;
             return numbers[i];
           },
           [&](uint32_t entry, uint32_t column) {
             if (n < cap) { adds[2 * n] = entry; adds[2 * n + 1] = column; }
             ++n;
           });
  return n;
}

// A batch as k_epialleles takes it, read by read: table[n_pairs][16] += its windows; -> the number of records that counted
long long epi_harness_batch(const uint32_t* bits, const uint32_t* dir, uint32_t genome_len, const uint32_t* start_index,
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
    epi_read(calls + off, (int)(end - off), off - batch_lo, batch_hi - off,
             [&](int i) -> long long {
               const long long c = cpg_call_pair(bits, pos, i, minus, c_lo, c_hi);
               return c < 0 ? -1ll : (long long)cpg_rank(bits, dir, (uint32_t)c);
             },
             [&](uint32_t entry, uint32_t column) { table[(uint64_t)kEpiColumns * entry + column] += 1u; });
  }
  return counted;
}

// the four statistics of a window: out[0 .. 3] = meth, epipoly, entropy, discordant -> total
uint64_t epi_harness_stats(const uint64_t* n, double* out) {
  const hostio::EpialleleStats s = hostio::epiallele_stats(n);
  out[0] = s.meth; out[1] = s.epipoly; out[2] = s.entropy; out[3] = s.discordant;
  return s.total;
}

// one line of <out>.epialleles -> its length (the text in `out`, cap bytes)
uint32_t epi_harness_line(const char* chrom, uint32_t pos, uint32_t end, const uint64_t* n, char* out, uint32_t cap) {
  hostio::Sink s;
  hostio::put_epiallele_line(s, std::string(chrom), pos, end, n);
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}

// The merge of the windows of several devices as bin/walt -ME -g does it: rows of 18 words (pos, last, n[16]), n_rows[d]
// of them per device one after the other, each device's ascending -> the merged rows in out (cap rows), how many
uint32_t epi_harness_merge(const uint64_t* rows, const uint32_t* n_rows, uint32_t n_dev, uint64_t* out, uint32_t cap) {
  std::vector<hostio::EpialleleRow> acc, add, other;
  for (uint32_t d = 0; d < n_dev; ++d) {
    add.resize(n_rows[d]);
    for (uint32_t i = 0; i < n_rows[d]; ++i, rows += 18) {
      add[i].pos = (uint32_t)rows[0];
      add[i].last = (uint32_t)rows[1];
      for (int k = 0; k < 16; ++k) add[i].n[k] = rows[2 + k];
    }
    hostio::merge_epiallele_rows(acc, add.data(), add.size(), other);
  }
  for (size_t i = 0; i < acc.size() && i < cap; ++i) {
    out[18 * i] = acc[i].pos;
    out[18 * i + 1] = acc[i].last;
    for (int k = 0; k < 16; ++k) out[18 * i + 2 + k] = acc[i].n[k];
  }
  return (uint32_t)acc.size();
}

}  // extern "C"
