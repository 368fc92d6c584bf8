// nonconv_harness.cpp -- C entry points (TEST INFRASTRUCTURE) over walt_amd/csrc/nonconv_core.h, what the kernels of
// nonconv.hip run per lane, and over the <out>.filterstats writer and option parser of walt_amd/csrc/host/hostio.h.
// Compiled with g++ by tests/test_nonconv_cpu.py (no device) and, under the host's sanitizers, with
// tests/nonconv_sanitize_main.cpp.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "host/hostio.h"
#include "nonconv_core.h"

using namespace walt;

static NonconvSum sum_of(const uint32_t* v) { return NonconvSum{v[0], v[1], v[2], v[3], v[4], v[5]}; }
static void sum_to(const NonconvSum& s, uint32_t* v) {
  v[0] = s.meth; v[1] = s.total; v[2] = s.pre; v[3] = s.suf; v[4] = s.best; v[5] = s.full;
}

extern "C" {

// the class of every byte value: out[256]
void nonconv_harness_classes(uint8_t* out) {
  for (uint32_t b = 0; b < 256; ++b) out[b] = (uint8_t)nonconv_class(b);
}

// summaries as six words: meth, total, pre, suf, best, full
void nonconv_harness_identity(uint32_t* out) { sum_to(nonconv_identity(), out); }
void nonconv_harness_combine(const uint32_t* a, const uint32_t* b, uint32_t* out) { sum_to(nonconv_combine(sum_of(a), sum_of(b)), out); }
void nonconv_harness_pack(const uint32_t* a, uint32_t* out) {
  uint32_t w0, w1;
  nonconv_pack(sum_of(a), w0, w1);
  sum_to(nonconv_unpack(w0, w1), out);
}
// the summary of a stretch scanned byte by byte (nonconv_push)
void nonconv_harness_scan(const uint8_t* p, uint32_t n, uint32_t* out) {
  NonconvSum s = nonconv_identity();
  for (uint32_t i = 0; i < n; ++i) nonconv_push(s, nonconv_class(p[i]));
  sum_to(s, out);
}

// one read through the kernel's own slices, trips and fold order; before / after: the batch's bytes around rb
void nonconv_harness_read(const uint8_t* rb, uint32_t len, uint64_t before, uint64_t after, uint32_t* out) {
  sum_to(nonconv_read(rb, (int)len, before, after), out);
}
uint32_t nonconv_harness_trips(int len, int head) { return (uint32_t)nonconv_trips(len, head); }

uint32_t nonconv_harness_fails(uint32_t meth, uint32_t total, uint32_t run, const uint32_t* rule) {
  return nonconv_fails(meth, total, run, walt_nonconv_rule{rule[0], rule[1], rule[2], rule[3]});
}
int nonconv_harness_judged(uint32_t times, uint64_t off, uint64_t end) { return nonconv_judged(times, off, end) ? 1 : 0; }
int nonconv_harness_rule_ok(const uint32_t* rule) { return nonconv_rule_ok(walt_nonconv_rule{rule[0], rule[1], rule[2], rule[3]}) ? 1 : 0; }

// a batch as k_nonconv takes it, read by read: filt[n], tally[n]; -> the number of judged reads
long long nonconv_harness_batch(const uint8_t* calls, const uint64_t* offsets, uint32_t n, const uint8_t* records, uint64_t rec_stride,
                                const uint32_t* rule4, uint8_t* filt, walt_nonconv_tally* tally) {
  const walt_nonconv_rule rule = {rule4[0], rule4[1], rule4[2], rule4[3]};
  const uint64_t batch_lo = offsets[0], batch_hi = offsets[n];
  long long judged = 0;
  for (uint32_t r = 0; r < n; ++r) {
    const uint64_t off = offsets[r], end = offsets[r + 1];
    uint32_t times;
    memcpy(&times, records + r * rec_stride + 4, 4);
    NonconvSum run = nonconv_identity();
    uint32_t fails = 0;
    if (nonconv_judged(times, off, end) && off >= batch_lo && end <= batch_hi) {
      run = nonconv_read(calls + off, (int)(end - off), off - batch_lo, batch_hi - off);
      fails = nonconv_fails(run.meth, run.total, run.best, rule);
      ++judged;
    }
    tally[r] = nonconv_tally_of(run);
    filt[r] = (uint8_t)fails;
  }
  return judged;
}

// the pair rule in place on f[2]
void nonconv_harness_pair(uint32_t best_times, uint8_t* f) { nonconv_pair(best_times, f[0], f[1]); }

// one block of <out>.filterstats -> its length (the text in `out`, cap bytes)
uint32_t nonconv_harness_filter_block(uint64_t records, uint64_t filtered, const uint32_t* rule, char* out, uint32_t cap) {
  hostio::Sink s;
  hostio::put_filter_block(s, records, filtered, rule);
  const uint32_t len = (uint32_t)s.n;
  if (len <= cap) memcpy(out, s.p, len);
  return len;
}
int nonconv_harness_parse(const char* text, uint32_t lo, uint32_t hi, uint32_t* out) {
  return hostio::parse_filter_value(text, lo, hi, *out) ? 1 : 0;
}

}  // extern "C"
