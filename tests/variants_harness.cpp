// variants_harness.cpp -- CPU build of what the evidence kernel runs per lane (walt_amd/csrc/variants_core.h on top of
// meth_core.h and pileup_core.h), driven the way the HIP kernel drives it: slices cut at 16-byte boundaries of the bases,
// eight "lanes" per read, every slice's evidence added at its forward positions; and the rule predicate.
// Also the pieces of bin/walt -MV that live in host/hostio.h: the value parser and the two writers.
// Compiled by tests/test_variants_cpu.py:  g++ -O2 -fopenmp -shared -fPIC -I walt_amd/csrc tests/variants_harness.cpp
#include <stdint.h>
#include <string.h>

#include <string>

#include "host/hostio.h"
#include "variants_core.h"

extern "C" {

// ev_slice as it is: out = {match, other}
void variants_harness_slice(const uint32_t* rd, uint64_t ext, uint32_t ga, uint32_t call, uint32_t* out) {
  const walt::EvSlice s = walt::ev_slice(rd, ext, ga, call);
  out[0] = s.match;
  out[1] = s.other;
}

int variants_harness_counts(uint32_t times, uint32_t skip, uint32_t pos, uint32_t genome_len, uint32_t cv, uint64_t len) {
  return walt::ev_record_counts(times, skip, pos, genome_len, cv, len) ? 1 : 0;
}

// bit 0: judged, bit 1: flagged
int variants_harness_rule(uint32_t match, uint32_t other, uint32_t min_depth, uint32_t max_percent) {
  return (walt::ev_judged(match, other, min_depth) ? 1 : 0) | (walt::ev_flagged(match, other, min_depth, max_percent) ? 2 : 0);
}

// One counted read.  ref: the packed reference of the record's strand (R or R'), ref_last its last word index; bases: the
// batch's bases (batch_bytes of them), the read at [off, off + total); head: the read's first byte modulo 16; minus: the
// record lies on the '-' strand.  match / other: counters by forward position, genome_len of each.
// -> the adds made, or -1 when one fell outside the read's chromosome [lo, hi) (nothing is added there)
long long variants_harness_read(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, uint32_t head, uint64_t off,
                                uint64_t total, uint64_t batch_bytes, uint32_t limit, uint32_t pos, uint32_t lo, uint32_t hi,
                                uint32_t ga, int minus, uint32_t* match, uint32_t* other) {
  const uint8_t* rb = bases + off;
  long long adds = 0;
  bool bad = false;
  for (uint32_t sub = 0; sub < 8; ++sub)
    for (int i0 = -(int)head + 16 * (int)sub; i0 < (int)limit; i0 += 16 * 8) {
      const walt::EvSlice s = walt::ev_read_slice(rb, (int)total, limit, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off);
      walt::pile_slice(s.match, s.other, (long long)pos + i0, minus != 0, lo, hi, [&](uint32_t f, bool m) {
        if (f < lo || f >= hi) { bad = true; return; }
        (m ? match : other)[f] += 1;
        ++adds;
      });
    }
  return bad ? -1 : adds;
}

// -> 1 and *out when `text` is a value of -MVD / -MVP between lo and hi
int variants_harness_parse(const char* text, uint32_t lo, uint32_t hi, uint32_t* out) {
  return hostio::parse_variant_value(std::string(text), lo, hi, *out) ? 1 : 0;
}

// one line of <out>.variants; site: a walt_variant_site.  -> its length (copied when it fits)
uint32_t variants_harness_line(const char* chrom, uint32_t chrom_start, const void* site, char* out, uint32_t cap) {
  hostio::Sink s;
  hostio::put_variant_line(s, std::string(chrom), chrom_start, *static_cast<const walt_variant_site*>(site));
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}

// one block of <out>.variantstats
uint32_t variants_harness_block(const uint64_t* tot, uint32_t min_depth, uint32_t max_percent, char* out, uint32_t cap) {
  hostio::Sink s;
  hostio::put_variant_block(s, tot, min_depth, max_percent);
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}

}  // extern "C"
