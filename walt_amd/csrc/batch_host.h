// batch_host.h -- what the host-buffer calls do with a caller's arrays before anything reaches the device.  The mapping
// calls (walt_map_se_batch, walt_map_se_rpbat_batch, walt_map_pe_batch, walt_map_pe_rpbat_batch): the scan of one read
// set and the offsets relative to its first read.  The methylation-side calls (meth.hip, mbias.hip, dedup.hip) as well:
// a strided array packed into a dense one, the stride and conversion refusals they share, and the per-read checks of
// the calling call.  Host only, no HIP: tests/batch_host_harness.cpp compiles it with g++ (plain and under
// -fsanitize=address,undefined), like chrom_core.h.
#ifndef WALT_AMD_BATCH_HOST_H_
#define WALT_AMD_BATCH_HOST_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace walt {

// One read set (one mate): offsets[0 .. n], read i is [offsets[i], offsets[i + 1]).  Null when every pair of
// neighbours is non-decreasing and no read is longer than 1024 bases, else the message of the first read that is not
// (its order before its length).  *max_len is raised to the longest read: a paired call scans both mates into one.
// *refused, when given, is that read's index (n when there is none).
inline const char* scan_offsets(const uint64_t* offsets, uint32_t n, uint32_t* max_len, uint32_t* refused = nullptr) {
  for (uint32_t i = 0; i < n; ++i) {
    if (refused) *refused = i;
    if (offsets[i + 1] < offsets[i]) return "offsets not non-decreasing";
    const uint64_t l = offsets[i + 1] - offsets[i];
    if (l > 1024) return "read length above 1024 is not supported";
    if (l > *max_len) *max_len = (uint32_t)l;
  }
  if (refused) *refused = n;
  return nullptr;
}

// The offsets as the kernels want them: relative to the first read of the set (a caller that shards a batch over
// several devices passes a slice of its offsets array).  The caller's own array when it starts at 0, else `rel`,
// filled with all n + 1 entries.
inline const uint64_t* rebase_offsets(const uint64_t* offsets, uint32_t n, std::vector<uint64_t>& rel) {
  if (offsets[0] == 0) return offsets;
  rel.resize((size_t)n + 1);
  for (uint32_t i = 0; i <= n; ++i) rel[i] = offsets[i] - offsets[0];
  return rel.data();
}

// n elements of type T that lie `stride` bytes apart, as the kernels read them: dense.  sizeof(T) bytes are read per
// element, never `stride`: the last m2 of a walt_pair_result array ends where the array ends.  (n = 0: src is not read.)
template <class T>
inline std::vector<T> pack_strided(const void* src, size_t stride, uint32_t n) {
  std::vector<T> out(n);
  for (uint32_t i = 0; i < n; ++i) memcpy(&out[i], static_cast<const char*>(src) + (size_t)i * stride, sizeof(T));
  return out;
}

// The refusals the methylation-side calls share: empty, or the message for the caller to put "<its name>: " in front of.
inline std::string record_stride_refusal(size_t rec_stride) {  // records are walt_best_match: 16 bytes, read by word
  if (rec_stride >= 16 && rec_stride % 4 == 0) return std::string();
  return "record stride " + std::to_string(rec_stride) + " is smaller than a walt_best_match (16) or not a multiple of 4";
}
// conv: per-read conversions, conv_stride bytes apart; null: `conversion` for the whole batch
inline std::string conv_refusal(const void* conv, size_t conv_stride, int conversion) {
  if (conv && conv_stride < 1) return "conv stride 0 is smaller than its element (1)";
  if (!conv && conversion != 'T' && conversion != 'A') return "conversion " + std::to_string(conversion) + " is neither 'T' nor 'A'";
  return std::string();
}
inline std::string skip_stride_refusal(const void* skip, size_t skip_stride) {
  return skip && skip_stride < 1 ? "skip stride 0 is smaller than its element (1)" : std::string();
}

// The per-read checks of the calling call (walt_meth_call_batch and the forms built on it) in their order: read i's
// order, its length, its conversion byte, then read i + 1.  Empty, or the whole message: only the conversion's names `who`.
inline std::string call_reads_refusal(const char* who, const uint64_t* offsets, uint32_t n, const uint8_t* conv, size_t conv_stride) {
  uint32_t max_len = 0, refused = n;
  const char* bad = scan_offsets(offsets, n, &max_len, &refused);
  for (uint32_t i = 0; conv && i < refused; ++i) {  // (the reads in front of the refused one passed their first two checks)
    const int c = conv[(size_t)i * conv_stride];
    if (c != 'T' && c != 'A')
      return std::string(who) + ": conversion " + std::to_string(c) + " of read " + std::to_string(i) + " is neither 'T' nor 'A'";
  }
  return bad ? std::string(bad) : std::string();
}

}  // namespace walt
#endif
