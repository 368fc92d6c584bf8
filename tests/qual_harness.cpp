// qual_harness.cpp -- CPU build of what the quality-aware kernels run per lane (include/walt_amd.h, "minimum base
// quality"): the mask function of walt_amd/csrc/meth_core.h, meth_read_slice_q driven the way meth.hip drives it (slices
// cut at the 16-byte boundaries of the calls array, eight "lanes" per read) and ev_read_slice_q the way variants.hip does
// (slices cut at the boundaries of the bases).  Also the pieces of bin/walt -MQ that live in host/hostio.h: the value
// parsers, the settings line and the quality packer of the FASTQ loader (on malloc, as tests/hostio_harness.cpp has it).
// Compiled by tests/test_qual_cpu.py:  g++ -O2 -fopenmp -shared -fPIC -I walt_amd/csrc tests/qual_harness.cpp
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

static int qh_alloc(size_t bytes, void** out) { *out = malloc(bytes ? bytes : 1); return *out ? 0 : -5; }
#define HOSTIO_ALLOC(bytes, out) qh_alloc((bytes), (out))
#define HOSTIO_FREE(p) free(p)
#define HOSTIO_ALLOC_ERROR() "out of memory"
#include "host/hostio.h"
#include "variants_core.h"

extern "C" {

// meth_qual_mask as it is
uint32_t qual_harness_mask(const uint32_t* qd, uint32_t min_qual) { return walt::meth_qual_mask(qd, min_qual); }

// One read as a group of eight lanes takes it in a quality instance of the calling kernel: the interval word and the
// bounds always there.  quals: the batch's quality bytes (batch_bytes of them, at the offsets of bases); null: the plain
// instance (meth_read_slice with the bounds).  cmu: the slices' cm and cu flags by read position (bit 0 / bit 1).
void qual_harness_read(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, const uint8_t* quals, uint8_t* calls,
                       uint64_t off, uint64_t total, uint64_t batch_bytes, uint32_t limit, uint32_t pos, uint32_t lo, uint32_t hi,
                       uint32_t ga, uint32_t ex_lo, uint32_t ex_hi, uint32_t trim5, uint32_t trim3, uint32_t min_qual,
                       uint16_t* counts8, uint8_t* cmu) {
  unsigned long long meth = 0, unmeth = 0;
  const uint8_t* rb = bases + off;
  const uint8_t* qb = quals ? quals + off : nullptr;
  uint8_t* cb = calls + off;
  const long long head = (long long)((uintptr_t)cb & 15u);
  limit = walt::meth_trim_limit(limit, trim3);
  const bool mapped = limit != 0;
  for (uint32_t sub = 0; sub < 8; ++sub)
    for (int i0 = -(int)head + 16 * (int)sub; i0 < (int)total; i0 += 16 * 8) {
      uint32_t out[4], cm = 0, cu = 0;
      if (qb)
        walt::meth_read_slice_q<true>(rb, (int)total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out,
                                      meth, unmeth, cm, cu, ex_lo, ex_hi, trim5, qb, min_qual);
      else
        walt::meth_read_slice(rb, (int)total, limit, mapped, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off, out, meth,
                              unmeth, cm, cu, ex_lo, ex_hi, trim5);
      walt::meth_store_slice(cb, (int)total, i0, out);
      for (int k = 0; k < 16; ++k) {
        const int i = i0 + k;
        if (cmu && i >= 0 && i < (int)total) cmu[i] |= (uint8_t)(((cm >> (2 * k)) & 1u) | (((cu >> (2 * k)) & 1u) << 1));
      }
    }
  memcpy(counts8, &meth, 8);
  memcpy(counts8 + 4, &unmeth, 8);
}

// One counted read as the evidence kernel's quality instance takes it (tests/variants_harness.cpp, variants_harness_read,
// plus the qualities).  -> the adds made, or -1 when one fell outside the read's chromosome
long long qual_harness_evidence(const uint32_t* ref, uint32_t ref_last, const uint8_t* bases, const uint8_t* quals, uint64_t off,
                                uint64_t total, uint64_t batch_bytes, uint32_t limit, uint32_t pos, uint32_t lo, uint32_t hi,
                                uint32_t ga, int minus, uint32_t min_qual, uint32_t* match, uint32_t* other) {
  const uint8_t* rb = bases + off;
  const uint32_t head = (uint32_t)((uintptr_t)rb & 15u);
  long long adds = 0;
  bool bad = false;
  for (uint32_t sub = 0; sub < 8; ++sub)
    for (int i0 = -(int)head + 16 * (int)sub; i0 < (int)limit; i0 += 16 * 8) {
      const walt::EvSlice s = quals ? walt::ev_read_slice_q<true>(rb, (int)total, limit, pos, lo, hi, ga, ref, ref_last, i0, off,
                                                                   batch_bytes - off, quals + off, min_qual)
                                    : walt::ev_read_slice(rb, (int)total, limit, pos, lo, hi, ga, ref, ref_last, i0, off, batch_bytes - off);
      walt::pile_slice(s.match, s.other, (long long)pos + i0, minus != 0, lo, hi, [&](uint32_t f, bool m) {
        if (f < lo || f >= hi) { bad = true; return; }
        (m ? match : other)[f] += 1;
        ++adds;
      });
    }
  return bad ? -1 : adds;
}

// -> 1 and *out when `text` is a value of -MQ (which = 0) or -MQO (which = 1)
int qual_harness_parse(const char* text, int which, uint32_t* out) {
  return (which ? hostio::parse_qual_offset(std::string(text), *out) : hostio::parse_min_qual(std::string(text), *out)) ? 1 : 0;
}
// -> 1 and *out = the byte the library compares with, 0 when the sum exceeds 127
int qual_harness_floor(uint32_t min_qual, uint32_t offset, uint32_t* out) { return hostio::quality_floor(min_qual, offset, *out) ? 1 : 0; }

// the settings line of <out>.methstats -> its length (the text in `out`, cap bytes)
uint32_t qual_harness_line(uint32_t min_qual, uint32_t offset, char* out, uint32_t cap) {
  hostio::Sink s;
  hostio::put_minqual_line(s, min_qual, offset);
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}

// The loader with want_quals: the first batch of `fastq`.  -> the number of reads, bases / quals / offsets copied out
// (cap bytes, cap_reads + 1 offsets); -1 with the loader's message in `err` when it throws; -2: too small a buffer.
// want_quals = 0: -> 1000000 + n when the batch got no quality buffer at all.
long long qual_harness_load(const char* fastq, const char* adaptor, int threads, int want_quals, uint8_t* bases, uint8_t* quals,
                            uint64_t cap, uint64_t* offsets, uint32_t cap_reads, char* err, uint32_t err_cap) {
  try {
    hostio::FastqReader rd;
    rd.want_quals = want_quals != 0;
    rd.open(fastq, threads);
    hostio::Batch bt;
    rd.load(cap_reads, adaptor ? adaptor : "", bt);
    rd.close();
    if (bt.n > cap_reads || bt.offsets[bt.n] > cap) return -2;
    memcpy(offsets, bt.offsets, ((size_t)bt.n + 1) * 8);
    memcpy(bases, bt.bases, bt.offsets[bt.n]);
    if (!want_quals) return bt.quals ? (long long)bt.n : 1000000ll + bt.n;
    memcpy(quals, bt.quals, bt.offsets[bt.n]);
    return bt.n;
  } catch (const std::exception& e) {
    snprintf(err, err_cap, "%s", e.what());
    return -1;
  }
}

}  // extern "C"
