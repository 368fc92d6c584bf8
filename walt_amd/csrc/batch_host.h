// batch_host.h -- what the host-buffer mapping calls (walt_map_se_batch, walt_map_se_rpbat_batch, walt_map_pe_batch,
// walt_map_pe_rpbat_batch) do with a caller's offsets array before anything reaches the device: the scan of one read
// set and the offsets relative to its first read.  Host only, no HIP: tests/batch_host_harness.cpp compiles it with g++
// (plain and under -fsanitize=address,undefined), like chrom_core.h.
#ifndef WALT_AMD_BATCH_HOST_H_
#define WALT_AMD_BATCH_HOST_H_

#include <stdint.h>

#include <vector>

namespace walt {

// One read set (one mate): offsets[0 .. n], read i is [offsets[i], offsets[i + 1]).  Null when every pair of
// neighbours is non-decreasing and no read is longer than 1024 bases, else the message of the first read that is not
// (its order before its length).  *max_len is raised to the longest read: a paired call scans both mates into one.
inline const char* scan_offsets(const uint64_t* offsets, uint32_t n, uint32_t* max_len) {
  for (uint32_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) return "offsets not non-decreasing";
    const uint64_t l = offsets[i + 1] - offsets[i];
    if (l > 1024) return "read length above 1024 is not supported";
    if (l > *max_len) *max_len = (uint32_t)l;
  }
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

}  // namespace walt
#endif
