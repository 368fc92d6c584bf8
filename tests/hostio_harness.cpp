// hostio_harness.cpp -- CPU test harness for walt_amd/csrc/host/hostio.h (TEST
// INFRASTRUCTURE): runs the driver's FASTQ loader without a GPU (malloc instead
// of the page-locked allocator) and dumps every batch as text so that the tests
// can compare the multi-threaded scanner, its serial restatement and the Python
// restatement of LoadReadsFromFastqFile (tests/refio.py) on awkward inputs.
#include <stdlib.h>
static int hh_alloc(size_t bytes, void** out) { *out = malloc(bytes ? bytes : 1); return *out ? 0 : -5; }
#define HOSTIO_ALLOC(bytes, out) hh_alloc((bytes), (out))
#define HOSTIO_FREE(p) free(p)
#define HOSTIO_ALLOC_ERROR() "out of memory"
#include "../walt_amd/csrc/host/hostio.h"

// dump format: one line "#batch <n>" per batch, then "<name>\t<seq>\t<score>" per read
extern "C" int hio_dump(const char* fastq, uint32_t n_per_batch, const char* adaptor, int threads, int force_serial,
                        const char* out_path, int* used_serial) {
  try {
    hostio::FastqReader rd;
    if (force_serial) setenv("WALT_AMD_SERIAL_IO", "1", 1); else unsetenv("WALT_AMD_SERIAL_IO");
    rd.open(fastq, threads);
    hostio::Batch bt;
    hostio::Sink s;
    for (;;) {
      rd.load(n_per_batch, adaptor ? adaptor : "", bt);
      if (bt.n == 0) break;
      s.lit("#batch "); s.u32(bt.n); s.ch('\n');
      for (uint32_t j = 0; j < bt.n; ++j) {
        s.put(bt.name(j)); s.ch('\t'); s.put(bt.seq(j)); s.ch('\t'); s.put(bt.score(j)); s.ch('\n');
      }
      if (bt.n < n_per_batch) break;
    }
    if (used_serial) *used_serial = rd.serial ? 1 : 0;
    rd.close();
    hostio::OutFile f;
    if (!f.open_trunc(out_path)) return -2;
    f.write(s.p, s.n);
    f.close();
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "hio_dump: %s\n", e.what());
    return -1;
  }
}

// Sink number formatting and reverse complement against printf / a plain loop
extern "C" int hio_format_check(void) {
  hostio::Sink s;
  const uint32_t us[] = {0u, 7u, 10u, 99u, 100u, 4294967295u, 123456789u};
  const int is[] = {0, -1, 17, -2147483647 - 1, 2147483647, -500};
  std::string want;
  char tmp[64];
  for (uint32_t v : us) { s.u32(v); s.ch(' '); snprintf(tmp, sizeof tmp, "%u ", v); want += tmp; }
  for (int v : is) { s.i32(v); s.ch(' '); snprintf(tmp, sizeof tmp, "%d ", v); want += tmp; }
  const char* q = "ACGTNacgt";
  hostio::View v{q, 9};
  s.revcomp(v); s.ch(' '); s.rev(v);
  want += "tgcaNACGT tgcaNTGCA";
  return std::string(s.p, s.n) == want ? 0 : 1;
}

// hostio::merge_rows as the driver's three tables instantiate it.  kind 0: sites of -MC (2 counters, added in 32 bits),
// 1: entries of -MA (4 counters of 64 bits), 2: windows of -ME (16 counters of 64 bits).  The devices' rows, each device
// ascending by position, lie one after the other in pos / counters (hio_merge_counters(kind) counters per row) and are
// folded into an empty accumulator in that order; every array handed to the merge is a heap block of exactly its rows.
// Returns the number of merged rows, written to out_pos / out_counters (room for all rows of all devices).
static walt_meth_site row_of(const walt_meth_site*, uint32_t pos, const uint64_t* c) { return walt_meth_site{pos, (uint32_t)c[0], (uint32_t)c[1], '+', 0, 0}; }
static hostio::AllelicRow row_of(const hostio::AllelicRow*, uint32_t pos, const uint64_t* c) { return hostio::AllelicRow{pos, pos + 2, {c[0], c[1], c[2], c[3]}}; }
static hostio::EpialleleRow row_of(const hostio::EpialleleRow*, uint32_t pos, const uint64_t* c) {
  hostio::EpialleleRow r = {pos, pos + 6, {}};
  for (int k = 0; k < 16; ++k) r.n[k] = c[k];
  return r;
}
static void counters_of(const walt_meth_site& r, uint64_t* c) { c[0] = r.meth; c[1] = r.unmeth; }
static void counters_of(const hostio::AllelicRow& r, uint64_t* c) { for (int k = 0; k < 4; ++k) c[k] = r.n[k]; }
static void counters_of(const hostio::EpialleleRow& r, uint64_t* c) { for (int k = 0; k < 16; ++k) c[k] = r.n[k]; }
template <class Row, class Plus>
static uint64_t fold_devices(int width, int n_dev, const uint64_t* n_rows, const uint32_t* pos, const uint64_t* counters, uint32_t* out_pos,
                             uint64_t* out_counters, Plus plus) {
  std::vector<Row> acc, other;
  size_t at = 0;
  for (int d = 0; d < n_dev; ++d) {
    Row* add = static_cast<Row*>(malloc(n_rows[d] ? n_rows[d] * sizeof(Row) : 1));
    for (uint64_t i = 0; i < n_rows[d]; ++i, ++at) add[i] = row_of((const Row*)nullptr, pos[at], counters + at * width);
    hostio::merge_rows(acc, add, (size_t)n_rows[d], other, plus);
    free(add);
  }
  for (size_t i = 0; i < acc.size(); ++i) { out_pos[i] = acc[i].pos; counters_of(acc[i], out_counters + i * width); }
  return acc.size();
}
extern "C" int hio_merge_counters(int kind) { return kind == 0 ? 2 : kind == 1 ? 4 : 16; }
extern "C" uint64_t hio_merge_rows(int kind, int n_dev, const uint64_t* n_rows, const uint32_t* pos, const uint64_t* counters,
                                   uint32_t* out_pos, uint64_t* out_counters) {
  if (kind == 0) return fold_devices<walt_meth_site>(2, n_dev, n_rows, pos, counters, out_pos, out_counters, hostio::add_site_row);
  if (kind == 1) return fold_devices<hostio::AllelicRow>(4, n_dev, n_rows, pos, counters, out_pos, out_counters, hostio::add_counter_row<hostio::AllelicRow>);
  return fold_devices<hostio::EpialleleRow>(16, n_dev, n_rows, pos, counters, out_pos, out_counters, hostio::add_counter_row<hostio::EpialleleRow>);
}
