// batch_host_harness.cpp -- CPU build of what the host-buffer mapping calls do with a caller's offsets array
// (walt_amd/csrc/batch_host.h: scan_offsets, rebase_offsets), driven the way a call drives it: the read sets of one
// call (one for a single-end call, two mates for a paired one) are scanned in order into ONE running maximum, the
// first refusal ends the call, and every accepted set is rebased.  Each offsets array is a heap block of EXACTLY
// n + 1 words, so that a build with -fsanitize=address,undefined reports any word read beyond it.  A program rather
// than a shared library: the sanitizer's runtime has to be the process's own.
// Compiled by tests/test_batch_host_cpu.py:  g++ -O1 -g [-fsanitize=address,undefined] -I walt_amd/csrc tests/batch_host_harness.cpp
//
//   batch_host_harness IN OUT
//   IN   uint64 n_sets; per set: uint64 n, uint64 offsets[n + 1]
//   OUT  per set, one text line:  <message, or "ok">\t<running max_len>\t<1: the caller's own array came back, else 0>\t<n + 1 rebased offsets>
//        (no line after a refused set; a refused set has no third and fourth field)
//
// and what the methylation-side host forms share (pack_strided, the stride and conversion refusals, call_reads_refusal);
// each prints one line, the message or "ok":
//   batch_host_harness pack ELEM STRIDE N     N elements of ELEM (16 or 1) bytes, STRIDE apart, in a heap block of EXACTLY
//                                             (N - 1) * STRIDE + ELEM bytes: a read of STRIDE bytes at the last one is reported
//   batch_host_harness refuse record STRIDE | refuse conv HAVE STRIDE CONVERSION | refuse skip HAVE STRIDE
//   batch_host_harness reads STRIDE N OFFSETS[N + 1] [CONV[N]]    the per-read checks of "who"; CONV bytes STRIDE apart
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "batch_host.h"

static bool read_words(FILE* f, uint64_t* p, size_t n) { return fread(p, 8, n, f) == n; }

struct Elem16 { unsigned char b[16]; };
static unsigned char byte_of(uint32_t i, size_t k) { return (unsigned char)(1 + 31 * i + 7 * k); }

// element i holds byte_of(i, 0 .. sizeof(T) - 1), the gaps between elements 0xEE
template <class T>
static int pack_case(size_t stride, uint32_t n) {
  const size_t bytes = n ? ((size_t)n - 1) * stride + sizeof(T) : 0;
  unsigned char* src = (unsigned char*)malloc(bytes ? bytes : 1);
  if (!src) return 2;
  memset(src, 0xEE, bytes);
  for (uint32_t i = 0; i < n; ++i)
    for (size_t k = 0; k < sizeof(T); ++k) src[(size_t)i * stride + k] = byte_of(i, k);
  const std::vector<T> out = walt::pack_strided<T>(n ? src : nullptr, stride, n);
  free(src);
  if (out.size() != n) return 3;
  for (uint32_t i = 0; i < n; ++i)
    for (size_t k = 0; k < sizeof(T); ++k)
      if (reinterpret_cast<const unsigned char*>(&out[i])[k] != byte_of(i, k)) { printf("element %u differs\n", i); return 3; }
  printf("ok\n");
  return 0;
}

static int say(const std::string& refusal) {
  printf("%s\n", refusal.empty() ? "ok" : refusal.c_str());
  return 0;
}

static int shared_pieces(int argc, char** argv) {
  const std::string mode = argv[1];
  auto num = [&](int i) { return strtoull(argv[i], nullptr, 10); };
  static const char present = 0;  // a non-null array for the refusals that only ask whether there is one
  if (mode == "pack" && argc == 5) return num(2) == 16 ? pack_case<Elem16>(num(3), (uint32_t)num(4)) : pack_case<unsigned char>(num(3), (uint32_t)num(4));
  if (mode == "refuse" && argc == 4 && std::string(argv[2]) == "record") return say(walt::record_stride_refusal(num(3)));
  if (mode == "refuse" && argc == 6 && std::string(argv[2]) == "conv") return say(walt::conv_refusal(num(3) ? &present : nullptr, num(4), (int)num(5)));
  if (mode == "refuse" && argc == 5 && std::string(argv[2]) == "skip") return say(walt::skip_stride_refusal(num(3) ? &present : nullptr, num(4)));
  if (mode == "reads" && argc >= 4) {
    const size_t stride = num(2);
    const uint32_t n = (uint32_t)num(3);
    if (argc != 4 + (int)n + 1 && argc != 4 + 2 * (int)n + 1) return 2;
    uint64_t* offsets = (uint64_t*)malloc(8 * ((size_t)n + 1));
    for (uint32_t i = 0; i <= n; ++i) offsets[i] = num(4 + i);
    unsigned char* conv = nullptr;
    if (argc == 4 + 2 * (int)n + 1 && n) {
      conv = (unsigned char*)malloc(((size_t)n - 1) * stride + 1);
      for (uint32_t i = 0; i < n; ++i) conv[(size_t)i * stride] = (unsigned char)num(4 + n + 1 + i);
    }
    const int rc = say(walt::call_reads_refusal("who", offsets, n, conv, stride));
    free(conv);
    free(offsets);
    return rc;
  }
  return 2;
}

int main(int argc, char** argv) {
  if (argc >= 2 && (!strcmp(argv[1], "pack") || !strcmp(argv[1], "refuse") || !strcmp(argv[1], "reads"))) return shared_pieces(argc, argv);
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 2;
  uint64_t n_sets = 0;
  if (!read_words(in, &n_sets, 1)) return 2;
  uint32_t max_len = 0;
  for (uint64_t s = 0; s < n_sets; ++s) {
    uint64_t n64 = 0;
    if (!read_words(in, &n64, 1) || n64 > 0xFFFFFFFFull) return 2;
    const uint32_t n = (uint32_t)n64;
    uint64_t* offsets = (uint64_t*)malloc(8 * ((size_t)n + 1));
    if (!offsets || !read_words(in, offsets, (size_t)n + 1)) return 2;
    const char* bad = walt::scan_offsets(offsets, n, &max_len);
    if (bad) {
      fprintf(out, "%s\t%u\n", bad, max_len);
      free(offsets);
      break;
    }
    std::vector<uint64_t> rel;
    const uint64_t* r = walt::rebase_offsets(offsets, n, rel);
    if (r != offsets && (r != rel.data() || rel.size() != (size_t)n + 1)) return 3;
    fprintf(out, "ok\t%u\t%d\t", max_len, r == offsets ? 1 : 0);
    for (uint32_t i = 0; i <= n; ++i) fprintf(out, "%s%llu", i ? " " : "", (unsigned long long)r[i]);
    fprintf(out, "\n");
    free(offsets);
  }
  fclose(in);
  return fclose(out) ? 2 : 0;
}
