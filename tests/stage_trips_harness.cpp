// stage_trips_harness.cpp -- TEST CODE ONLY: which fence plans do the probes of a batch's heavy reads start from?
// tests/test_gpu_stage_trips.py builds its reads so that the staged heavy kernels search slots of every size class; this
// proves it on the host, from the same directory the kernels look up.  It is tests/host_harness.cpp (the CPU index:
// directory, entries, fence keys at the opened dir_bits) plus one function, compiled into a library of its own.
#include "host_harness.cpp"

extern "C" {

// Per read r: out_read[2 r] = 1 when a probe of SEED 0 (either strand) falls into a slot of more than kScanMax entries.
// Pass 1 probes seed 0 of every read on both strands, so it hands such a read to the heavy pass for certain, at seed 0.
// 2: only a later seed meets such a slot -- pass 1 may have finished the read before (not used as heavy or as light).
// out_read[2 r + 1] = the first seed with such a slot.
// tally[fi][c], fi = 0 '+' / 1 '-': probes of the reads flagged 1, any seed (what the staged kernel can come to search: it
// takes a read up at seed 0 and runs its seeds while the read needs them), whose slot's first fence plan is of class c:
//   0: 1 .. kScan entries (no search)   1: entries as pivots, fewer than 16   2: entries as pivots, 16
//   3: sh = 4   4: sh = 8   5: sh = 12   6: sh = 16
int st_probe_plans(void* hp, const char* bases, const uint64_t* offsets, uint32_t n, int ag, uint32_t* out_read,
                   uint64_t* tally /* 2 x 7 */) {
  HIndex* h = reinterpret_cast<HIndex*>(hp);
  const IndexView& iv = h->view;
  constexpr int NW = 64;
  std::vector<uint32_t> rec(packed_fields(NW));
  for (uint32_t i = 0; i < 14; ++i) tally[i] = 0;
  for (uint32_t r = 0; r < n; ++r) {
    out_read[2 * r] = 0; out_read[2 * r + 1] = kPat;
    const uint32_t len = (uint32_t)(offsets[r + 1] - offsets[r]);
    if (len > kMaxReadLen) return -1;
    if (len < kMinReadLen) continue;
    if (!pack_read(reinterpret_cast<const uint8_t*>(bases) + offsets[r], len, ag ? 1 : 0, iv.dir_bits, NW, rec.data(), 1)) return -2;
    uint32_t ne[kPat][2];
    for (uint32_t seed_i = 0; seed_i < kPat; ++seed_i) {
      const uint32_t* care = &rec[1 + NW + seed_i * kPerSeedWords];
      const uint32_t slot = care[kCareWords], span = care[kCareWords + 1];
      for (uint32_t fi = 0; fi < 2; ++fi) {
        const StrandView& sv = iv.s[(ag ? 2 : 0) + fi];
        const uint32_t* dp = sv.dir + (uint32_t)(slot - 1u);  // (core.h seed_lookup_ex)
        const uint32_t lo = dp[1], hi = span == 1 ? dp[0] : sv.dir[(uint32_t)(slot - span)];
        ne[seed_i][fi] = hi > lo ? hi - lo : 0u;
        if (ne[seed_i][fi] > kScanMax && !out_read[2 * r]) { out_read[2 * r] = seed_i == 0 ? 1 : 2; out_read[2 * r + 1] = seed_i; }
      }
    }
    if (out_read[2 * r] != 1) continue;
    for (uint32_t seed_i = out_read[2 * r + 1]; seed_i < kPat; ++seed_i) {
      const uint32_t* care = &rec[1 + NW + seed_i * kPerSeedWords];
      const uint32_t slot = care[kCareWords];
      for (uint32_t fi = 0; fi < 2; ++fi) {
        if (!ne[seed_i][fi]) continue;
        const StrandView& sv = iv.s[(ag ? 2 : 0) + fi];
        const uint32_t lo = sv.dir[(uint32_t)(slot - 1u) + 1];
        const FencePlan p = fence_plan(sv, lo, lo + ne[seed_i][fi]);
        const uint32_t c = ne[seed_i][fi] <= kScan ? 0u : (p.sh == 0 ? (p.m < 16 ? 1u : 2u) : 2u + p.sh / 4);
        tally[7 * fi + c] += 1;
      }
    }
  }
  return 0;
}

}  // extern "C"
