// regions_harness.cpp -- CPU build of how the regions kernel cuts a call into units and finds a unit's region again
// (walt_amd/csrc/regions_core.h on top of levels_core.h), and of the BED reader and the <out>.regions writer
// (walt_amd/csrc/host/hostio.h parse_bed_text, resolve_bed, put_regions_block).
// Compiled by tests/test_regions_cpu.py:  g++ -O2 -I walt_amd/csrc tests/regions_harness.cpp, as a shared object, and as
// a stand-alone program (-DREGIONS_HARNESS_MAIN, with host sanitizers) that runs a small call by itself.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#define HOSTIO_ALLOC(bytes, out) ((*(out) = malloc(bytes)) ? 0 : -5)
#define HOSTIO_FREE(p) free(p)
#define HOSTIO_ALLOC_ERROR() "malloc failed"
#include "host/hostio.h"
#include "regions_core.h"

static int copy_out(const std::string& s, char* buf, int cap) {
  if ((int)s.size() > cap) return -1;
  memcpy(buf, s.data(), s.size());
  return (int)s.size();
}
// names: the chromosome names joined by '\n'
static std::vector<std::string> split_names(const char* names) {
  std::vector<std::string> out;
  for (const char* p = names; *p;) {
    const char* e = strchr(p, '\n');
    if (!e) { out.push_back(p); break; }
    out.push_back(std::string(p, e - p));
    p = e + 1;
  }
  return out;
}

extern "C" {

uint32_t regions_harness_unit() { return walt::kRegionUnit; }
uint32_t regions_harness_units(uint32_t lo, uint32_t hi, uint32_t genome_len) { return walt::region_units(lo, hi, genome_len); }

// the exclusive prefix the three launches of the scan leave: prefix[0 .. n]
void regions_harness_prefix(const walt_region* regions, uint32_t n, uint32_t genome_len, uint64_t* prefix) {
  uint64_t run = 0;
  for (uint32_t i = 0; i < n; ++i) { prefix[i] = run; run += walt::region_units(regions[i].lo, regions[i].hi, genome_len); }
  prefix[n] = run;
}
uint32_t regions_harness_region_of_unit(const uint64_t* prefix, uint32_t n, uint64_t unit) {
  return walt::region_of_unit(reinterpret_cast<const unsigned long long*>(prefix), 0u, n, unit);
}
uint32_t regions_harness_region_next(const uint64_t* prefix, uint32_t n, uint32_t r, uint64_t unit) {
  return walt::region_next(reinterpret_cast<const unsigned long long*>(prefix), n, r, unit);
}
void regions_harness_unit_range(uint32_t lo, uint32_t hi, uint32_t k, uint64_t* u_lo, uint64_t* u_hi) {
  unsigned long long a, b;
  walt::region_unit_range(lo, hi, k, a, b);
  *u_lo = a; *u_hi = b;
}

// A whole call the way the kernel composes it for a grid of n_waves wavefronts: runs of units by stride, the first
// region of a run by search and the next ones by region_next, a unit's positions one at a time.  `taken` (one byte per
// unit) counts how often a unit was walked.
void regions_harness_call(const uint32_t* ref, uint32_t ref_last, const uint32_t* start, uint32_t n_chrom, const uint32_t* meth,
                          const uint32_t* unmeth, const walt_region* regions, uint32_t n, uint64_t n_waves, walt_region_levels* out,
                          uint8_t* taken) {
  const uint32_t genome_len = start[n_chrom];
  std::vector<unsigned long long> prefix(n + 1);
  regions_harness_prefix(regions, n, genome_len, reinterpret_cast<uint64_t*>(prefix.data()));
  memset(out, 0, sizeof(walt_region_levels) * (size_t)n);
  const unsigned long long total = prefix[n];
  unsigned long long run = total / n_waves;
  run = run < 1ull ? 1ull : run > walt::kRegionRun ? (unsigned long long)walt::kRegionRun : run;
  auto take = [&](walt_region_row& row, unsigned long long m, unsigned long long u) {
    row.sites += 1;
    if (!(m + u)) return;
    row.covered += 1;
    row.meth += m; row.unmeth += u;
    row.level_sum += walt::level_q30(m, u);
  };
  for (unsigned long long me = 0; me < n_waves; ++me)
    for (unsigned long long u0 = me * run; u0 < total; u0 += n_waves * run) {
      const unsigned long long u_end = u0 + run < total ? u0 + run : total;
      uint32_t r = walt::region_of_unit(prefix.data(), 0u, n, u0);
      for (unsigned long long unit = u0; unit < u_end; ++unit) {
        if (unit != u0) r = walt::region_next(prefix.data(), n, r, unit);
        if (taken) taken[unit] += 1;
        unsigned long long lo, hi;
        walt::region_unit_range(regions[r].lo, regions[r].hi, (uint32_t)(unit - prefix[r]), lo, hi);
        for (unsigned long long f = lo; f < hi; ++f) {
          uint32_t c = 0;
          while (start[c + 1] <= f) ++c;
          const unsigned long long ext = walt::meth_ref_ext(ref, (long long)f - 2, ref_last);
          const uint32_t cls = walt::levels_class(ext, (uint32_t)f, start[c], start[c + 1]);
          if (cls != walt::kLevelNone) take(out[r].row[cls], meth[f], unmeth[f]);
          if (walt::levels_pair(ext, (uint32_t)f, start[c + 1]))
            take(out[r].row[walt::kLevelPair], (unsigned long long)meth[f] + meth[f + 1], (unsigned long long)unmeth[f] + unmeth[f + 1]);
        }
      }
    }
}

// The BED text parsed: one line "chrom <TAB> start <TAB> end <TAB> name <TAB> line" per region, or "ERR <message>".
int regions_harness_parse(const char* text, uint32_t len, const char* file, char* buf, int cap) {
  std::vector<hostio::BedRegion> bed;
  std::string err, s;
  if (!hostio::parse_bed_text(text, len, file, bed, err)) return copy_out("ERR " + err, buf, cap);
  for (const hostio::BedRegion& r : bed)
    s += r.chrom + "\t" + std::to_string(r.start) + "\t" + std::to_string(r.end) + "\t" + r.name + "\t" + std::to_string(r.line) + "\n";
  return copy_out(s, buf, cap);
}

// ... and resolved against a genome: one line "lo <TAB> hi" per region and a last line "unknown <n>", or
// "ERR <message>".
int regions_harness_resolve(const char* text, uint32_t len, const char* file, const char* names, const uint32_t* start, char* buf,
                            int cap) {
  std::vector<hostio::BedRegion> bed;
  std::string err, s;
  if (!hostio::parse_bed_text(text, len, file, bed, err)) return copy_out("ERR " + err, buf, cap);
  const std::vector<std::string> name = split_names(names);
  const std::vector<uint32_t> st(start, start + name.size() + 1);
  std::vector<walt_region> regions;
  uint64_t n_unknown = 0;
  if (!hostio::resolve_bed(bed, name, st, file, regions, n_unknown, err)) return copy_out("ERR " + err, buf, cap);
  for (size_t i = 0; i < regions.size(); ++i)
    s += std::to_string(regions[i].lo) + "\t" + std::to_string(regions[i].hi) + "\n";
  s += "unknown " + std::to_string(n_unknown) + "\n";
  return copy_out(s, buf, cap);
}

// <out>.regions' block of the BED text's regions with the records lv[0 .. n): its length, -1 when it does not fit, -2
// when the text does not parse into n regions
int regions_harness_text(const char* text, uint32_t len, const walt_region_levels* lv, uint32_t n, char* buf, int cap) {
  std::vector<hostio::BedRegion> bed;
  std::string err;
  if (!hostio::parse_bed_text(text, len, "bed", bed, err) || bed.size() != n) return -2;
  hostio::Sink s;
  hostio::put_regions_block(s, bed, lv);
  if ((int)s.n > cap) return -1;
  memcpy(buf, s.p, s.n);
  return (int)s.n;
}

}  // extern "C"

#ifdef REGIONS_HARNESS_MAIN
// A fixed pseudo-random genome of 3 * kRegionUnit + 71 bases in chromosomes of 1, 2 and many bases; a call with empty
// regions in front, between and behind, regions of U - 1, U, U + 1 and 2U + 1 positions, an invalid one and the whole
// genome: run for several grids, every unit must be walked once, every grid must give the same records, and the
// partition must fold to the whole genome.  The BED reader and the writer run once over a text with every form.
int main() {
  const uint32_t U = walt::kRegionUnit;
  const uint32_t lengths[] = {1, 2, U + 7, 61, 2 * U};
  const uint32_t n_chrom = sizeof lengths / sizeof lengths[0];
  uint32_t start[n_chrom + 1];
  start[0] = 0;
  for (uint32_t c = 0; c < n_chrom; ++c) start[c + 1] = start[c] + lengths[c];
  const uint32_t glen = start[n_chrom], words = (glen + 15) / 16 + 16;
  uint32_t* ref = (uint32_t*)calloc(words, 4);
  uint32_t* meth = (uint32_t*)calloc(glen, 4);
  uint32_t* unmeth = (uint32_t*)calloc(glen, 4);
  uint64_t x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  static const uint32_t pick[4] = {0u, 1u, 7u, 0xFFFFFFFFu};
  for (uint32_t f = 0; f < glen; ++f) {
    const uint32_t code = (uint32_t)(rnd() % 6);  // C / G rich: A C G T C G
    ref[f >> 4] |= (code < 4 ? code : code - 3) << (2 * (f & 15));
    meth[f] = pick[rnd() % 4];
    unmeth[f] = pick[rnd() % 4];
  }
  const walt_region regions[] = {{0, 0}, {5, 5}, {0, glen}, {glen, glen}, {3, 3 + U - 1}, {3, 3 + U}, {7, 7}, {9, 9}, {3, 3 + U + 1},
                                 {100, 100 + 2 * U + 1}, {0, 1000}, {1000, glen}, {4, 3}, {0, glen + 1}, {glen, glen}, {0, 0}};
  const uint32_t n = sizeof regions / sizeof regions[0];
  std::vector<uint64_t> prefix(n + 1);
  regions_harness_prefix(regions, n, glen, prefix.data());
  const uint64_t total = prefix[n];
  int bad = 0;
  std::vector<walt_region_levels> first(n), got(n);
  const uint64_t grids[] = {1, 3, 4, 7, total, total + 5, 4000};
  for (size_t gi = 0; gi < sizeof grids / sizeof grids[0]; ++gi) {
    std::vector<uint8_t> taken(total, 0);
    regions_harness_call(ref, words - 1, start, n_chrom, meth, unmeth, regions, n, grids[gi], gi ? got.data() : first.data(), taken.data());
    for (uint64_t u = 0; u < total; ++u) bad += taken[u] != 1;
    if (gi) bad += memcmp(first.data(), got.data(), sizeof(walt_region_levels) * n) != 0;
  }
  for (int r = 0; r < 5; ++r) {
    bad += first[2].row[r].sites != first[10].row[r].sites + first[11].row[r].sites;
    bad += first[2].row[r].level_sum != first[10].row[r].level_sum + first[11].row[r].level_sum;
    bad += first[12].row[r].sites != 0 || first[13].row[r].sites != 0 || first[0].row[r].sites != 0;
  }
  const char* text = "# a comment\ntrack name=x\nbrowser position c0:1-2\n\nc0 0 1\r\nc2\t3\t4099\tisland  +\n  c9 5 9 far\nc4 0 8192";
  char buf[8192];
  int len = regions_harness_parse(text, (uint32_t)strlen(text), "x.bed", buf, (int)sizeof buf);
  bad += len <= 0 || !memcmp(buf, "ERR", 3);
  const char* names = "c0\nc1\nc2\nc3\nc4";
  len = regions_harness_resolve(text, (uint32_t)strlen(text), "x.bed", names, start, buf, (int)sizeof buf);
  bad += len <= 0 || !memcmp(buf, "ERR", 3);
  len = regions_harness_text(text, (uint32_t)strlen(text), first.data(), 4, buf, (int)sizeof buf);
  bad += len <= 0;
  const char* wrong = "c0 0 1\nc0 2 x\n";
  len = regions_harness_parse(wrong, (uint32_t)strlen(wrong), "x.bed", buf, (int)sizeof buf);
  bad += len < 12 || memcmp(buf, "ERR x.bed:2:", 12) != 0;
  printf("positions %u regions %u units %llu bad %d\n", glen, n, (unsigned long long)total, bad);
  free(ref); free(meth); free(unmeth);
  return bad ? 1 : 0;
}
#endif
