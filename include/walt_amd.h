/* walt_amd.h -- C ABI of the MI355X-native WALT seed-and-extend hot path.
 *
 * This is the drop-in boundary for the body of WALT's two `#pragma omp parallel
 * for` loops (reference src/walt/mapping.cpp:494-499 and paired.cpp:664-669)
 * plus the serial pair-merge loop (paired.cpp:684-699).  Plain pointers and
 * sizes only; no C++/torch types.  Every function returns 0 on success or a
 * negative WALT_E* code; walt_last_error() gives the message.  The library
 * never calls exit().  All four strand indexes stay resident in HBM, so ONE
 * call covers both strand passes that the reference makes per batch
 * (mapping.cpp:491-500).
 *
 * Citations are file:line in smithlabcode/walt v1.0.
 */
#ifndef WALT_AMD_H_
#define WALT_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WALT_OK 0
#define WALT_EINVAL (-1)   /* bad argument */
#define WALT_EIO (-2)      /* file missing / short read (reference: FREAD_CHECK exit, util.hpp:62-69) */
#define WALT_EHIP (-3)     /* HIP runtime error / no device */
#define WALT_EBASE (-4)    /* non-ACGT base in a read (reference: getBits exit, util.hpp:117-119) */
#define WALT_ENOMEM (-5)
#define WALT_EFORMAT (-6)  /* malformed .dbindex */

/* strand_mask bits for walt_index_open: which strand files to make resident */
#define WALT_STRAND_CT00 1u
#define WALT_STRAND_CT01 2u
#define WALT_STRAND_GA10 4u
#define WALT_STRAND_GA11 8u
#define WALT_STRANDS_CT 3u   /* single-end default (mapping.cpp:443-445) */
#define WALT_STRANDS_GA 12u  /* single-end -A (mapping.cpp:446-449) */
#define WALT_STRANDS_ALL 15u /* paired-end (paired.cpp:589-593) */
/* also build the unconverted reference for the methylation calls (below): the genome sections of the strand files
 * the mask does not load are read too (not their hash tables).  Without this bit walt_index_open is unchanged. */
#define WALT_WITH_REFERENCE 16u

/* BestMatch, mapping.hpp:39-52: 16 bytes, strand char at offset 8. */
typedef struct {
  uint32_t genome_pos;
  uint32_t times;
  char strand;
  char pad_[3]; /* written as 0 */
  uint32_t mismatch;
} walt_best_match;

/* CandidatePosition, paired.hpp:35-46: 12 bytes. */
typedef struct {
  uint32_t genome_pos;
  char strand;
  char pad_[3];
  uint32_t mismatch;
} walt_candidate;

/* What MergePairedEndResults (paired.cpp:474-545) derives for one pair. */
typedef struct {
  walt_best_match m1, m2; /* per-mate records the writers print (paired.cpp:515-569) */
  uint32_t best_times;    /* 0: no pair, 1: unique proper pair, >=2: ambiguous */
  int32_t frag_len;       /* `len` of OutputBestPairedResults when best_times==1, else 0 */
  int32_t best_i, best_j; /* indices into the ranked lists when best_times==1, else -1 */
  uint32_t pair_mm;       /* r1.mismatch + r2.mismatch of the reported pair */
  uint32_t pad_[3];
} walt_pair_result;

/* Work/statistics block returned by the batch calls (all counters are sums
 * over the batch; too_short counts one per strand pass like
 * stat.num_of_short_reads++ at mapping.cpp:230-233 / paired.cpp:112-115). */
typedef struct {
  uint64_t too_short;
  /* Diagnostic work counters of the kernels, NOT the reference's.  `probes` counts seed probes that found a
   * NON-EMPTY REGION (at least one index slot whose care characters equal the seed's) -- fewer than the probes into
   * non-empty buckets the reference's loop makes (mapping.cpp:268-274; bench.py's oracle counts those: ~4.0 per
   * read on the benchmark genome against ~1.4 here), although the kernels issue MORE look-ups than the reference
   * (a superset on the '-' strand; every probe of a staged paired-end read up to the exits it can prove).  A read
   * that moves on to the literal pass after part of its work is counted in both places. */
  uint64_t probes;     /* seed probes whose region is not empty */
  uint64_t candidates; /* candidates verified */
  uint64_t big_regions;/* regions handed to a wavefront (work items / cooperative verification) */
} walt_batch_stats;

typedef struct walt_index walt_index;

const char* walt_last_error(void);
int walt_device_count(void);

/* Seed pattern this library was compiled for.  The reference selects it at compile time
 * (-D SEEDPATTERN3 / 5 / 7, src/walt/Makefile:34, FAQ.md:5-13; tables in seedpattern.hpp); here
 * libwalt_amd.so is pattern 3 and libwalt_amd_sp5.so / libwalt_amd_sp7.so are the other two
 * (make PAT=5 / PAT=7).  An index is specific to the pattern of the makedb that wrote it.
 * walt_min_read_len() is MINIMALREADLEN (38 / 32 / 23; shorter reads count as too_short);
 * walt_max_read_len() is the longest read a batch may hold: 1024, or 148 / 152 for patterns 5 / 7,
 * beyond which the reference reads its seed tables out of bounds (mapping.cpp:238 caps the repeats
 * at 50, the tables hold 28 / 20). */
int walt_seed_pattern(void);
uint32_t walt_min_read_len(void);
uint32_t walt_max_read_len(void);

/* Page-locked host memory for the read / result buffers a caller hands to
 * walt_map_se_batch / walt_map_pe_batch (the reference keeps them in
 * std::vector<std::string>, mapping.cpp:462-464); transfers from such buffers
 * run at PCIe rate.  Ordinary pageable pointers are accepted by every call too. */
int walt_host_alloc(size_t bytes, void** out);
void walt_host_free(void* p);

/* ---- index ------------------------------------------------------------- */

/* Replaces ReadIndexHeadInfo + per-batch ReadIndex (reference.cpp:381-417,
 * 324-351; call sites mapping.cpp:437,492 and paired.cpp:583,661): reads
 * <path> and the selected <path>_CT00/_CT01/_GA10/_GA11 files once, uploads
 * them to `device` and builds the derived HBM structures (2-bit genome, entry
 * keys, directory).  dir_bits = directory prefix length in bits (24..32); < 0
 * picks it from the index size. */
int walt_index_open(const char* dbindex_path, int device, unsigned strand_mask, int dir_bits,
                    walt_index** out);

/* Same from host arrays laid out exactly like the .dbindex strand files
 * (reference.cpp:302-322): per strand s in {CT00,CT01,GA10,GA11} (NULL = not
 * present) genome bytes [genome_len], counter [4^12+1], index [index_size]. */
int walt_index_from_host(uint32_t n_chrom, const uint32_t* chrom_len, const char* const* chrom_names,
                         const uint8_t* const genome[4], const uint32_t* const counter[4],
                         const uint32_t* const index[4], const uint32_t index_size[4], int device,
                         int dir_bits, walt_index** out);

void walt_index_close(walt_index* idx);

/* Genome::num_of_chroms / length / name / start_index (reference.hpp:44-70). */
uint32_t walt_index_n_chrom(const walt_index* idx);
uint32_t walt_index_chrom_len(const walt_index* idx, uint32_t i);
const char* walt_index_chrom_name(const walt_index* idx, uint32_t i);
uint64_t walt_index_genome_len(const walt_index* idx);
uint64_t walt_index_device_bytes(const walt_index* idx);
int walt_index_dir_bits(const walt_index* idx);
/* diagnostics, per strand: buckets in which EVERY probe takes the literal search (0 for a
 * makedb-built index), and chromosome-end entries ("outliers") around which probes do */
uint64_t walt_index_bad_buckets(const walt_index* idx, int strand);
uint64_t walt_index_outliers(const walt_index* idx, int strand);
/* index entries whose genome window is also stored in slot order ("dense candidate windows": the regions of
 * thousands of candidates that repeats produce are then verified from contiguous memory) */
uint64_t walt_index_window_entries(const walt_index* idx, int strand);
/* index entries in runs that qualify for a dense window; larger than walt_index_window_entries when the memory budget
 * ended before the last run (those regions are verified from the scattered genome windows: same results, slower) */
uint64_t walt_index_window_eligible(const walt_index* idx, int strand);

/* ---- single-end: replaces the strand loop + omp loop over SingleEndMapping,
 *      mapping.cpp:486-500 / 224-316 ------------------------------------- */

/* Host buffers.  bases: concatenated sanitised reads (only ACGT, as
 * LoadReadsFromFastqFile leaves them, mapping.cpp:101-103); offsets[n+1].
 * out[n] is initialised by the callee to (0,0,'+',max_mm) (mapping.cpp:486-489)
 * and holds the state after the '+' and '-' passes. */
int walt_map_se_batch(walt_index* idx, const char* bases, const uint64_t* offsets, uint32_t n,
                      int ag_wildcard, uint32_t max_mismatches, uint32_t b, walt_best_match* out,
                      walt_batch_stats* stats);

/* Device-resident form (pointers are HBM addresses on idx's device; stream is a
 * hipStream_t or NULL).  Asynchronous: returns after enqueueing; d_stats
 * (walt_batch_stats, device memory) is accumulated into, not cleared.
 * d_workspace must hold walt_se_workspace_bytes(n, max_read_len) bytes; the call is told how many it holds
 * (workspace_bytes) and refuses a smaller one with WALT_EINVAL instead of writing beyond it.  No option of the
 * index (walt_index_set_option) makes a call need more than that.
 * One single-end call at a time per index (its side streams and events belong to the index): a second call that
 * arrives while one is being enqueued is refused with WALT_EINVAL; different indexes are independent. */
size_t walt_se_workspace_bytes(uint32_t n, uint32_t max_read_len);
int walt_map_se_batch_device(walt_index* idx, const void* d_bases, const void* d_offsets, uint32_t n,
                             uint32_t max_read_len, int ag_wildcard, uint32_t max_mismatches,
                             uint32_t b, void* d_out, void* d_stats, void* d_workspace,
                             size_t workspace_bytes, void* stream);

/* ---- single-end random PBAT: each read mapped under BOTH conversions -------
 * For libraries whose reads come in either conversion (random-primed PBAT, most single-cell bisulfite protocols:
 * some reads T-rich, some A-rich).  The reference has no such mode; its contract is defined here.  With
 *   c = the record walt_map_se_batch(..., ag_wildcard = 0, ...) returns for a read (C->T, strands _CT00/_CT01),
 *   g = the record the same call returns with ag_wildcard = 1 (G->A, strands _GA10/_GA11),
 * both with the same max_mismatches and b, the record r and its conversion conv ('T' or 'A') follow from the first
 * rule that applies:
 *   1. c.times == 1 && g.times == 1 && c.genome_pos == g.genome_pos && c.strand == g.strand (the same alignment
 *      under both conversions: a read with no informative C or G): r = c, conv = 'T';
 *   2. g.times == 0, or c.times > 0 && c.mismatch < g.mismatch: r = c, conv = 'T' (both unmapped: c's initial
 *      record (0, 0, '+', max_mismatches));
 *   3. c.times == 0, or g.mismatch < c.mismatch: r = g, conv = 'A';
 *   4. otherwise (both mapped with equal mismatches): r = c with r.times = c.times + g.times (>= 2: ambiguous),
 *      conv = 'T'.
 * Both conversions start from (0, 0, '+', max_mismatches); the G->A pass is not seeded with the C->T result.
 * Statistics: too_short is what a single-conversion call reports (one count per strand pass: a read is short under
 * both conversions); probes, candidates and big_regions are the sums over both conversions.
 * The index must hold all four strands (WALT_STRANDS_ALL); otherwise the call fails with WALT_EINVAL and names the
 * missing ones.  Every option of the index (walt_index_set_option) applies to both conversions, none changes r.
 * Host form: as walt_map_se_batch (offsets relative to offsets[0]; WALT_EBASE for a read with a non-ACGT base,
 * WALT_EINVAL as there); conv[n] receives 'T' / 'A' per read.  A second single-end call on the same index while
 * this one runs is refused with WALT_EINVAL before it touches anything of the first.
 * Device form: as walt_map_se_batch_device, plus d_conv (uint8_t[n]); d_out and d_workspace 16-byte aligned;
 * d_workspace holds walt_se_rpbat_workspace_bytes(n, max_read_len) bytes (walt_se_workspace_bytes plus the G->A
 * records), and a smaller workspace is refused with WALT_EINVAL. */
size_t walt_se_rpbat_workspace_bytes(uint32_t n, uint32_t max_read_len);
int walt_map_se_rpbat_batch(walt_index* idx, const char* bases, const uint64_t* offsets, uint32_t n,
                            uint32_t max_mismatches, uint32_t b, walt_best_match* out, uint8_t* conv,
                            walt_batch_stats* stats);
int walt_map_se_rpbat_batch_device(walt_index* idx, const void* d_bases, const void* d_offsets, uint32_t n,
                                   uint32_t max_read_len, uint32_t max_mismatches, uint32_t b, void* d_out,
                                   void* d_conv, void* d_stats, void* d_workspace, size_t workspace_bytes,
                                   void* stream);

/* The device-resident calls are asynchronous, so invalid input cannot come back as their status.
 * walt_batch_check waits for `stream` and reports what the last call on `d_workspace` found:
 * WALT_EBASE (a read holds a non-ACGT base: the reference's getBits exits, util.hpp:117-119; its
 * record is left as initialised), WALT_EINVAL (a read longer than max_read_len, or a batch of more than
 * n x max_read_len bases -- the workspace is sized by that product: such reads are refused in the kernels, never
 * converted or read beyond the workspace, their records left as initialised), WALT_EHIP (internal: a work-item
 * queue overflowed -- never with a workspace of the promised size), else WALT_OK.
 * The host-buffer calls do this themselves. */
int walt_batch_check(const void* d_workspace, void* stream);

/* ---- paired-end: replaces PairEndMapping over both mates and strands
 *      (paired.cpp:642-672 / 106-201), the heap drain (685-692) and the pair
 *      search of MergePairedEndResults (474-545) ----------------------------- */

/* ranked1/ranked2 (optional, may be NULL): n*top_k candidates per mate in the
 * pop order of the reference's priority_queue, ranked_n1/2[n] their counts. */
int walt_map_pe_batch(walt_index* idx, const char* bases1, const uint64_t* offsets1,
                      const char* bases2, const uint64_t* offsets2, uint32_t n,
                      uint32_t max_mismatches, uint32_t b, uint32_t top_k, int frag_range,
                      walt_pair_result* out, walt_candidate* ranked1, uint32_t* ranked_n1,
                      walt_candidate* ranked2, uint32_t* ranked_n2, walt_batch_stats* stats /*[2]*/);

/* One paired-end call at a time per walt_index: the call's internal streams and events (mate 2 runs beside mate 1,
 * passes alternate between two pipeline slots) belong to the index.  Different indexes (devices) are independent.
 * Workspace: walt_pe_workspace_bytes is the LEAST a call needs (8 M-pair passes, staged lists in four rounds);
 * walt_pe_workspace_bytes_best is what it uses best on idx's device as it stands now -- 10 M-pair passes in one round
 * when the device has that much free memory -- and never less than the former.  The call takes the geometry the
 * workspace it is given has room for (workspace_bytes), so sizing and mapping cannot disagree, and nothing about the
 * choice is kept in the process: two indexes on two devices decide independently. */
size_t walt_pe_workspace_bytes(uint32_t n, uint32_t max_read_len, uint32_t top_k);
size_t walt_pe_workspace_bytes_best(walt_index* idx, uint32_t n, uint32_t max_read_len, uint32_t top_k);
int walt_map_pe_batch_device(walt_index* idx, const void* d_bases1, const void* d_offsets1,
                             const void* d_bases2, const void* d_offsets2, uint32_t n,
                             uint32_t max_read_len, uint32_t max_mismatches, uint32_t b,
                             uint32_t top_k, int frag_range, void* d_out, void* d_stats /*[2]*/,
                             void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- paired-end random PBAT: each pair mapped in BOTH orientations --------
 * For paired-end libraries in which the T-rich read of a pair may sit in either file (random-primed PBAT, most
 * single-cell bisulfite protocols).  The reference has no such mode; its contract is defined here.  For one pair:
 *   p = the record walt_map_pe_batch(bases1, bases2, ...) returns: orientation T (mate 1 C->T on _CT00/_CT01, mate 2
 *       G->A on _GA10/_GA11);
 *   q = the record the same call returns with the mates exchanged, walt_map_pe_batch(bases2, bases1, ...): orientation
 *       A (what bin/walt -P maps), put back into user order: m1 and m2 exchanged, best_i and best_j exchanged
 *       (frag_len and pair_mm do not depend on mate order);
 * both with the same max_mismatches, b, top_k and frag_range.  P = p.best_times, Q = q.best_times; mp, mq = the
 * smallest pair mismatch count of each orientation's pair search (the final min_mm of the pair merge, defined when
 * best_times >= 1: pair_mm for a unique pair; not otherwise visible through this ABI).  The first rule that applies
 * decides the record r and the conversions conv[2i], conv[2i+1] ('T' / 'A') of mate 1 and mate 2:
 *   1. P == 1 && Q == 1 and both mates have the same position and strand in p and q (a pair with no informative C
 *      or G): r = p, conv = (T, A);
 *   2. P > 0 && (Q == 0 || mp < mq): r = p, conv = (T, A);
 *   3. Q > 0 && (P == 0 || mq < mp): r = q in user order, conv = (A, T);
 *   4. P > 0 && Q > 0 && mp == mq (ambiguous across the orientations): r.best_times = P + Q;
 *   5. P == 0 && Q == 0 (no proper pair in either orientation): r.best_times = 0.
 * Under rules 4 and 5 r.frag_len = 0, r.best_i = r.best_j = -1, r.pair_mm = 0, and each mate's record and conversion
 * follow the single-end random-PBAT rules 1-4 above, unchanged, with c = the mate's record where it was mapped C->T
 * and g = its record where it was mapped G->A: mate 1 c = p.m1, g = q.m1; mate 2 c = q.m2, g = p.m2.  pad_ is
 * written as 0.
 * Statistics (stats[2], per mate in user order): too_short is what walt_map_pe_batch reports for that mate (counted
 * once); probes, candidates and big_regions are the sums over both orientations.
 * The index must hold all four strands.  Every option of the index applies to both orientations, none changes r.
 * Host form: as walt_map_pe_batch without the ranked lists; conv[2n].  It takes the index's paired-end lock before it
 * touches anything: a second paired-end call on the same index while this one runs is refused with WALT_EINVAL.
 * Device form: as walt_map_pe_batch_device, plus d_conv (uint8_t[2n], 2-byte aligned); d_out and d_workspace 16-byte
 * aligned.
 * Workspace: walt_pe_rpbat_workspace_bytes(n, L, k) = walt_pe_workspace_bytes(n, L, k) + s * R, with c the pairs of a
 * pass (c = min(n, max(65536, min(2^23, floor(10 GiB / (24 k)))))), s the pipeline slots (2 when n > c, else 1) and
 * R = 64 c rounded up to a multiple of 256: every slot holds orientation A's records of its pass.
 * walt_pe_rpbat_workspace_bytes_best is what the call uses best on idx's device (as walt_pe_workspace_bytes_best);
 * the call takes the geometry workspace_bytes has room for and refuses a smaller workspace with WALT_EINVAL. */
size_t walt_pe_rpbat_workspace_bytes(uint32_t n, uint32_t max_read_len, uint32_t top_k);
size_t walt_pe_rpbat_workspace_bytes_best(walt_index* idx, uint32_t n, uint32_t max_read_len, uint32_t top_k);
int walt_map_pe_rpbat_batch(walt_index* idx, const char* bases1, const uint64_t* offsets1, const char* bases2,
                            const uint64_t* offsets2, uint32_t n, uint32_t max_mismatches, uint32_t b,
                            uint32_t top_k, int frag_range, walt_pair_result* out, uint8_t* conv,
                            walt_batch_stats* stats /*[2]*/);
int walt_map_pe_rpbat_batch_device(walt_index* idx, const void* d_bases1, const void* d_offsets1,
                                   const void* d_bases2, const void* d_offsets2, uint32_t n,
                                   uint32_t max_read_len, uint32_t max_mismatches, uint32_t b, uint32_t top_k,
                                   int frag_range, void* d_out, void* d_conv, void* d_stats /*[2]*/,
                                   void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- methylation calls: the methylation state of every cytosine position a mapped read covers -----------------
 * The reference has no such mode (its users run a second program over the mapped records); the contract is defined
 * here.  The alphabet is Bismark's XM one.
 *
 * Reference bases.  The index holds only converted genomes (makedb.cpp:67-73, reference.cpp:148-162), so the
 * unconverted base is recovered from a pair of strand files: for strand '+', R[p] = 'C' where _GA10's genome byte at
 * p is 'C', else _CT00's byte at p; for strand '-', R'[p] is the same from _GA11 and _CT01.  Both are indexed by
 * genome_pos as the records use it (the '-' genomes are reverse-complemented chromosome by chromosome, so a '-'
 * record's read lies on R' left to right).  For an N-free FASTA R is the FASTA.  Where the FASTA had N, each strand
 * file holds its own fill and R is whatever this rule makes of them; nothing detects that.
 * The two arrays are packed, 2 bits per base (2 x genome_len / 4 bytes plus a little slack), and exist only when asked
 * for: walt_index_open with WALT_WITH_REFERENCE, or walt_index_enable_reference on an index that holds all four
 * strands (WALT_STRANDS_ALL, walt_index_from_host / walt_index_build_device with four strands): one pass over the
 * packed genomes it has resident.  WALT_EINVAL naming the missing strands otherwise; a second call changes nothing.
 * walt_index_device_bytes includes the arrays once they exist.
 *
 * Per read.  Inputs: the sanitised bases (only ACGT) and offsets as given to the mapping call, the read's record, its
 * conversion ('T': mapped C->T, 'A': mapped G->A, as the random-PBAT calls report it in conv) and an optional
 * call_len (bases from call_len on get no call: an adaptor clipped by the caller).  With p = genome_pos, G = R or R'
 * by the record's strand and [lo, hi) the chromosome that holds p, read position i < min(length, call_len) with
 * q = p + i < hi gets a call
 *   conversion 'T': when G[q] == 'C' and the read base is C (methylated) or T (unmethylated); context bases
 *                   n1 = G[q+1], n2 = G[q+2], context key 'G';
 *   conversion 'A': when G[q] == 'G' and the read base is G (methylated) or A (unmethylated); context bases
 *                   n1 = G[q-1], n2 = G[q-2], context key 'C'.
 * Context, first rule that applies: n1 outside [lo, hi): unknown (u / U); n1 == key: CpG (z / Z); n2 outside the
 * chromosome: unknown; n2 == key: CHG (x / X); else CHH (h / H).  Upper case = methylated.  Every other position
 * is '.' (not a cytosine position, a mismatch, beyond call_len, beyond the chromosome).  A record with times == 0
 * gets all '.' and zero counts, and so does one whose genome_pos lies outside the genome, whose conversion is
 * neither 'T' nor 'A', or whose read is longer than 1024 bases (possible only if the caller made it up; the kernel
 * never reads beyond the arrays).  A record with times >= 2 is called at the position it holds.
 *
 * Outputs, each optional (NULL = not wanted): calls, one byte per base at the same offsets as bases, in read order as
 * given; counts[n]; stats, ACCUMULATED into, not cleared, over the records with times == 1 only.
 *
 * records + i * record_stride is read i's walt_best_match (stride 16 for an array of them; 64 with a base of
 * &out[0].m1 or &out[0].m2 for the mates of a walt_pair_result array).  conv + i * conv_stride is its conversion
 * (stride 1 for walt_map_se_rpbat_batch's conv, 2 with a base of conv or conv + 1 for one mate of
 * walt_map_pe_rpbat_batch's); conv == NULL: `conversion` for every read.  call_len: uint32_t[n] or NULL.
 * WALT_EINVAL with a message naming the cause when the index has no reference, when a stride is smaller than its
 * element (a record stride must also be a multiple of 4), or when a conversion is neither 'T' nor 'A' (host form: any
 * read's; device form: `conversion` -- a device conv array cannot be checked by an asynchronous call, see above).
 * Host form: offsets relative to offsets[0] like walt_map_se_batch; calls is written at calls[offsets[i]...].
 * Device form: pointers are HBM addresses on idx's device, offsets[0] == 0, stream a hipStream_t or NULL;
 * asynchronous.  d_records and d_call_len 4-byte aligned, d_counts and d_stats 8-byte aligned; d_bases and d_calls
 * need no alignment (equal alignment modulo 16 is fastest).  No workspace.  The batch totals pass through counters
 * that belong to the index: one methylation call with stats at a time per index. */
typedef struct {
  uint16_t meth[4], unmeth[4]; /* contexts in the order CpG, CHG, CHH, unknown */
} walt_meth_counts;
typedef struct {
  uint64_t reads; /* records with times == 1 */
  uint64_t meth[4], unmeth[4];
} walt_meth_stats;
int walt_index_enable_reference(walt_index* idx);
int walt_index_has_reference(const walt_index* idx);
int walt_meth_call_batch(walt_index* idx, const char* bases, const uint64_t* offsets, uint32_t n, const void* records,
                         size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                         const uint32_t* call_len, char* calls, walt_meth_counts* counts, walt_meth_stats* stats);
int walt_meth_call_batch_device(walt_index* idx, const void* d_bases, const void* d_offsets, uint32_t n,
                                const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                void* stream);

/* ---- methylation pile-up: two counters per cytosine of the genome, fed by the calls above ----------------------
 * The reference has no such mode (its users sort the mapped records and run a second program over them); the contract
 * is defined here.  A pile-up belongs to one index, which must hold the reference (WALT_EINVAL otherwise), and lives on
 * its device; it must be destroyed before the index is closed.
 *
 * Which calls count.  A call is what walt_meth_call_batch writes as a letter other than '.' at read position i of a
 * record.  Only records with times == 1 are piled up: the set walt_meth_stats sums.  A record with times >= 2 adds
 * nothing (its calls string is still written), and neither does one that gets no call above: genome_pos outside the
 * genome, a conversion that is neither 'T' nor 'A', a read longer than 1024 bases.  call_len bounds the called
 * positions as there.  Overlapping mates of a pair are both counted, as walt_meth_stats counts them, unless the caller
 * passes the overlap interval (-NO; "overlap of a pair" below).
 *
 * Where a call lands.  With [lo, hi) the chromosome that holds genome_pos and q = genome_pos + i, the forward position
 * is f = q for a '+' record and f = lo + hi - 1 - q for a '-' record (both strands share the chromosome starts).  The
 * call adds 1 to meth[f] for an upper-case letter, 1 to unmeth[f] for a lower-case one.  ('+', 'T') and ('-', 'A')
 * records land on a forward C, a cytosine of the '+' strand; ('+', 'A') and ('-', 'T') on a forward G, a cytosine of
 * the '-' strand.  A read and its reverse complement pile onto the same sites.
 *
 * What a site is.  A forward position f with meth[f] + unmeth[f] > 0 whose '+' reference base R[f] is C or G.  Strand
 * and context come from R alone, so that every read that reaches f agrees:
 *   R[f] == 'C': strand '+', n1 = R[f+1], n2 = R[f+2], key 'G';
 *   R[f] == 'G': strand '-', n1 = R[f-1], n2 = R[f-2], key 'C';
 * context by the rule above, first match: n1 outside [lo, hi): unknown; n1 == key: CpG; n2 outside: unknown;
 * n2 == key: CHG; else CHH.  On an N-free genome R' is R reverse-complemented per chromosome, so this is the context of
 * every letter that landed on f, and the per-context sums over all sites equal the walt_meth_stats of the same
 * records.  Where the FASTA had N the strand files hold independent fills (see above; nothing detects that), and
 * R[f] can be A or T under a call made on R'.  Such positions are not sites; their calls are summed into the
 * "off-reference" pair the extraction returns, so on any genome reported calls + off-reference calls = the totals.
 *
 * Counts are exact up to 2^32 - 1 each (beyond that a counter wraps).  The counters take 8 x genome_len bytes of
 * device memory (25 GB at 3.1 Gbp) and the extraction's table 1 MiB: walt_pileup_device_bytes = 8 x genome_len +
 * 1048576; walt_index_device_bytes does not include it.  walt_pileup_create zeroes the counters; when the memory
 * is not there it returns WALT_ENOMEM naming the bytes it wanted and leaves the index usable.
 *
 * Feeding.  walt_meth_pileup_batch[_device] are walt_meth_call_batch[_device] with one more destination: every
 * argument, output, alignment and error as there (calls, counts and stats stay optional; with all three NULL only the
 * pile-up is fed), the batch read once; plus WALT_EINVAL for a null pile-up or one of another index.  The adds are
 * ordered by the stream they are launched on, and two streams may feed one pile-up at the same time (the batch totals
 * behind d_stats stay one call at a time per index).  The host forms, walt_pileup_clear and walt_pileup_extract wait
 * for all work on the device first.
 *
 * Extraction.  walt_pileup_extract writes the sites of the forward positions [pos_lo, pos_hi), ascending by pos, and
 * sets *n_sites to how many there are -- also when cap is too small: then WALT_EINVAL naming both numbers, and nothing
 * is written.  offref (optional): the methylated and unmethylated calls in the range that lie on an A or T of R.  A
 * range may cut a chromosome; contexts do not depend on it, nor on the index's options.  WALT_EINVAL when
 * pos_lo > pos_hi or pos_hi > genome_len.  Device form: d_sites (16-byte aligned, cap records), d_n_sites (uint64_t)
 * and d_offref (uint64_t[2], optional; both 8-byte aligned) are HBM addresses; asynchronous on `stream`, so a cap that
 * is too small cannot come back as the status: *d_n_sites > cap says that nothing was written.  One extraction at a
 * time per pile-up (its table belongs to the pile-up), ordered after the adds of its stream. */
typedef struct walt_pileup walt_pileup;
typedef struct {
  uint32_t pos, meth, unmeth;
  uint8_t strand;  /* '+' or '-' */
  uint8_t context; /* 0 CpG, 1 CHG, 2 CHH, 3 unknown */
  uint16_t reserved; /* written as 0 */
} walt_meth_site; /* 16 bytes */
int walt_pileup_create(walt_index* idx, walt_pileup** out);
void walt_pileup_destroy(walt_pileup* p);
int walt_pileup_clear(walt_pileup* p);
uint64_t walt_pileup_device_bytes(const walt_pileup* p);
int walt_meth_pileup_batch(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                           const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                           const uint32_t* call_len, char* calls, walt_meth_counts* counts, walt_meth_stats* stats);
int walt_meth_pileup_batch_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                  const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                  int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                  void* stream);
int walt_pileup_extract(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, walt_meth_site* sites, uint64_t cap,
                        uint64_t* n_sites, uint64_t* offref /*[2]: meth, unmeth*/);
int walt_pileup_extract_device(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, void* d_sites, uint64_t cap,
                               void* d_n_sites, void* d_offref, void* stream);

/* ---- methylation levels: the genome-wide summary of a pile-up, per context and over CpG pairs -------------------
 * The reference has no such mode (MethPipe users run symmetric-cpgs and levels over the counts file and the FASTA,
 * Bismark users read the report); the contract is defined here.  One pass over the counters and the '+' reference R
 * of the pile-up's index gives, over the forward positions [pos_lo, pos_hi), five rows of integers.
 *
 * Rows 0..3 (CpG, CHG, CHH, unknown).  A site is a position f of the range whose R[f] is C or G, classified exactly as
 * the extraction classifies it; uncovered sites count in `sites`.  covered, meth, unmeth and max_depth equal what the
 * records of walt_pileup_extract over the same range add up to, and offref equals the extraction's.
 *
 * Row 4 (CpG pairs, both strands merged).  f with R[f] == C, R[f + 1] == G and f + 1 in f's chromosome; its counts are
 * meth[f] + meth[f + 1] and unmeth[f] + unmeth[f + 1] (up to 2^33 - 2 each: the << 30 of level_sum keeps the numerator
 * below 2^63).  A pair belongs to the range that holds f: f + 1 may lie at or beyond pos_hi and is still read.  A C on a
 * chromosome's last base in front of a G on the next one's first is no pair (that C is `unknown`).
 *
 * Every field except max_depth is additive over a partition of a range, max_depth is the maximum; all are integers and
 * all folds commutative, so the result does not depend on the launch shape (the test hook pile_extract_blocks).
 *
 * Errors and ordering as walt_pileup_extract[_device]: WALT_EINVAL for a null pile-up, a null out, pos_lo > pos_hi or
 * pos_hi > genome_len, and d_out not 8-byte aligned; the host forms wait for all work on the device first; the device
 * form is asynchronous on `stream` (d_out: 656 bytes of HBM).  A summary counts as an extraction under "one at a time
 * per pile-up": its accumulator lives in free words of the extraction's table, and walt_pileup_device_bytes is as before.
 *
 * Raw counters.  walt_pileup_read copies the counters of [pos_lo, pos_hi) to two host arrays (either may be NULL);
 * walt_pileup_add adds two host arrays into them, wrapping as the counters do (either may be NULL: zeros; an empty
 * range is a no-op).  Maxima and covered sites are not additive across pile-ups: the counters of several devices are
 * folded with these two before one summary is taken. */
typedef struct {            /* 128 bytes */
  uint64_t sites;           /* sites of the class in the range, covered or not */
  uint64_t covered;         /* of those, with meth + unmeth > 0 */
  uint64_t meth, unmeth;    /* calls on them */
  uint64_t max_depth;       /* largest meth + unmeth of one site */
  uint64_t level_sum;       /* sum over covered sites of floor((meth << 30) / (meth + unmeth)) */
  uint64_t hist[10];        /* covered sites by min(9, 10 * meth / (meth + unmeth)), integer division */
} walt_level_row;
typedef struct {
  walt_level_row row[5];    /* 0 CpG, 1 CHG, 2 CHH, 3 unknown (the contexts of walt_meth_site), 4 CpG pairs */
  uint64_t offref[2];       /* as walt_pileup_extract returns them */
} walt_levels;              /* 656 bytes */
int walt_pileup_levels(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, walt_levels* out);
int walt_pileup_levels_device(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, void* d_out /*8-byte aligned*/, void* stream);
int walt_pileup_read(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, uint32_t* meth, uint32_t* unmeth);
int walt_pileup_add(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, const uint32_t* meth, const uint32_t* unmeth);

/* ---- methylation levels per region: the summary of many ranges of a pile-up in one call ------------------------
 * The reference has no such mode (MethPipe users run roimethstat over the counts file, Bismark users methylKit's
 * tiling over the coverage file; neither has the denominators without the FASTA); the contract is defined here.
 *
 * Equivalence.  out[i] equals what walt_pileup_levels(p, regions[i].lo, regions[i].hi, ..) returns in the fields of
 * the same name: rows 0..3 are the C/G positions of the range by the extraction's class, uncovered ones included in
 * `sites`; row 4 is the CpG pairs whose C lies in the range -- the G is read wherever it lies, and a C that ends a
 * chromosome in front of a G that starts the next is no pair; level_sum is floor((meth << 30) / (meth + unmeth))
 * summed over covered sites.  max_depth, the histogram and offref are left out on purpose: 160 bytes per region keep
 * 30 million tiles at 4.8 GB.  sites and covered are 32-bit: a region holds fewer than 2^32 positions.
 *
 * Regions are independent: in any order, overlapping, nested, repeated, empty (lo == hi: all zeros), and across
 * chromosome starts (the class of a position does not depend on the range).  All fields are integers and all folds
 * commutative, so the launch shape (the test hook pile_extract_blocks) cannot change a bit.
 *
 * Errors.  WALT_EINVAL for a null pile-up, null `regions` or `out` with n > 0, and any lo > hi or hi > genome_len: the
 * host form names the first such index and writes nothing.  The device form cannot see the regions before it
 * returns: there such a region yields an all-zero record and the others are as ever.  The device form also refuses
 * n above WALT_REGIONS_MAX (2^22) per call and d_regions, d_out or d_work that are null or not 8-byte aligned.
 * n == 0 succeeds and does nothing.  The host form takes any n (it runs windows of WALT_REGIONS_MAX itself with a
 * workspace of its own, which it frees) and waits for all work on the device first; the device form is asynchronous
 * on `stream`: d_regions n walt_region, d_out n walt_region_levels, d_work walt_pileup_regions_workspace_bytes(n)
 * bytes, all in HBM and the caller's.  A regions call counts as an extraction under "one at a time per pile-up";
 * walt_pileup_device_bytes is as before. */
#define WALT_REGIONS_MAX 4194304u
typedef struct { uint32_t lo, hi; } walt_region;      /* forward positions [lo, hi), 8 bytes */
typedef struct {                                       /* 32 bytes */
  uint32_t sites, covered;    /* as walt_level_row's */
  uint64_t meth, unmeth, level_sum;
} walt_region_row;
typedef struct { walt_region_row row[5]; } walt_region_levels;   /* 160 bytes; rows as walt_levels */
uint64_t walt_pileup_regions_workspace_bytes(uint32_t n);
int walt_pileup_regions(walt_pileup* p, const walt_region* regions, uint64_t n, walt_region_levels* out);
int walt_pileup_regions_device(walt_pileup* p, const void* d_regions, uint32_t n, void* d_out, void* d_work, void* stream);

/* ---- duplicates: PCR duplicates marked from the mapped records, and kept out of the methylation counts ---------
 * The reference has no such mode (its users sort the mapped records and run a second program, MethPipe's
 * duplicate-remover, before they count; Bismark users run deduplicate_bismark); the contract is defined here.  It needs
 * the records alone -- no bases, no reference, no index: a duplicate set (walt_dedup) belongs to a device, not to an index.
 *
 * Keys.  A set holds 64-bit keys; each remembers the ordinal of the first record that produced it.
 *   key(kind, conv, strand, aux, pos): bit 63 conv == 'A', bit 62 strand == '-', bits 61:60 kind, bits 59:32 aux (28 bits),
 *   bits 31:0 genome_pos.
 * The all-ones word is the empty slot; it is no key, because a genome_pos of 0xFFFFFFFF makes a record ineligible.
 *
 * Which records have a key.
 *   Single records (walt_dedup_batch; kind 0, 1 or 2 is the caller's: 0 for single-end reads): a walt_best_match is
 *   eligible when times == 1, genome_pos != 0xFFFFFFFF and its conversion is 'T' or 'A'; its key has aux = 0.  genome_pos is
 *   the 5' end of the read in its own strand's coordinates, so two reads are duplicates when 5' end, strand and conversion
 *   agree, whatever their lengths (Bismark's single-end rule).
 *   Pairs (walt_dedup_pairs_batch over walt_pair_result; conv[2n] as walt_map_pe_rpbat_batch writes it, or conv == NULL:
 *   `conversion` for mate 1 and the other letter for mate 2).  best_times == 1: the pair has ONE key -- kind 3,
 *   pos = m1.genome_pos, strand = m1.strand, conv = mate 1's, aux = (uint32_t)frag_len & 0x0FFFFFFF -- and both mates share
 *   its verdict (eligible when m1.genome_pos != 0xFFFFFFFF and mate 1's conversion is 'T' or 'A').  best_times != 1: each
 *   mate with times == 1 is a single record of kind 1 (mate 1) or 2 (mate 2) under its own conversion.  aux is the low 28
 *   bits of the two's-complement length: lengths in [-2^27, 2^27) have distinct keys, lengths of 2^27 and more alias (2^27
 *   with -2^27, 2^28 + x with x).  bin/walt -D refuses -L of 2^27 and more, so no two lengths it can report do.
 *
 * Verdict.  The set numbers every record it is fed 0, 1, 2, ... across calls (a pair takes one number; both of its mate
 * keys use it).  An eligible record is a duplicate exactly when an eligible record with the same key and a smaller number
 * was fed since the last clear: the first one fed wins, within a call the lowest index.  dup[i] (pairs: dup[2i + k] for
 * mate k + 1) is 1 for a duplicate and 0 for everything else, ineligible records included.  The verdicts are a pure
 * function of the sequence of records: they do not depend on how the sequence is cut into calls, on the table's capacity or
 * growth, on the grid or on the hash.
 *
 * The table: open addressing, two planes of 8-byte words (16 bytes per slot), a power of two of slots, load at most 1/2 --
 * 32 bytes of device memory per key at the limit.  walt_dedup_create: initial_slots is rounded up to a power of two, at
 * least 64; 0 picks a default sized for about one batch of 10 M records (2^25 slots, 512 MiB); small values are the test
 * hook for growth.  WALT_EHIP when there is no device.  walt_dedup_reserve(n_more) is synchronous: it waits for the
 * device, reads the number of keys and doubles the table until keys + n_more <= slots / 2 (old and new table exist side
 * by side meanwhile: 1.5 x the new size); WALT_ENOMEM names the bytes and leaves the set usable and unchanged.
 * walt_dedup_count waits too: *keys = distinct keys held, *fed = records numbered since the last clear (either may be
 * NULL).  walt_dedup_clear forgets everything and keeps the capacity.  walt_dedup_device_bytes = 16 x slots + 16.
 *
 * Batch calls.  Strides, conv == NULL and the alignment rules as in walt_meth_call_batch (a record stride of at least 16 and a
 * multiple of 4; conv stride at least 1; `conversion` 'T' or 'A' when conv is NULL; WALT_EINVAL otherwise).  A conv BYTE
 * that is neither letter makes its record ineligible, in both forms.  Host forms reserve for themselves (n keys; 2n for
 * pairs) and wait for the result.  Device forms: pointers are HBM addresses on the set's device (d_records 4-byte,
 * d_pairs 16-byte aligned), asynchronous on `stream` -- insert kernel, then mark kernel -- and unable to grow the table:
 * when the keys at the last count plus everything enqueued since plus this call could exceed slots / 2 they return
 * WALT_EINVAL telling the caller to reserve first, and enqueue nothing.  A probe that runs through the whole table (never
 * under that limit) sets an error word that the next synchronous call returns as WALT_EHIP; the kernel ends, it never
 * spins.  One call at a time per set: the ordinals and the mark-after-insert order are the set's.
 *
 * Skipping duplicates.  walt_meth_pileup_batch_skip[_device] are walt_meth_pileup_batch[_device] plus skip: a record whose
 * byte skip[i * skip_stride] is non-zero adds nothing to the pile-up and nothing to stats (stats.reads included); its
 * calls and counts are written as before.  skip == NULL: no record is skipped.  skip_stride 1 for walt_dedup_batch's dup;
 * 2 with a base of dup or dup + 1 for one mate of walt_dedup_pairs_batch's.  Here the pile-up may be NULL: the calls are
 * made and nothing is piled up. */
typedef struct walt_dedup walt_dedup;
int walt_dedup_create(int device, uint64_t initial_slots, walt_dedup** out);
void walt_dedup_destroy(walt_dedup* dd);
int walt_dedup_clear(walt_dedup* dd);
int walt_dedup_reserve(walt_dedup* dd, uint64_t n_more);
int walt_dedup_count(walt_dedup* dd, uint64_t* keys, uint64_t* fed);
uint64_t walt_dedup_device_bytes(const walt_dedup* dd);
int walt_dedup_batch(walt_dedup* dd, const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                     int conversion, int kind, uint32_t n, uint8_t* dup);
int walt_dedup_pairs_batch(walt_dedup* dd, const walt_pair_result* pairs, const uint8_t* conv, int conversion, uint32_t n,
                           uint8_t* dup /*[2n]*/);
int walt_dedup_batch_device(walt_dedup* dd, const void* d_records, size_t record_stride, const void* d_conv,
                            size_t conv_stride, int conversion, int kind, uint32_t n, void* d_dup, void* stream);
int walt_dedup_pairs_batch_device(walt_dedup* dd, const void* d_pairs, const void* d_conv, int conversion, uint32_t n,
                                  void* d_dup /*[2n]*/, void* stream);
int walt_meth_pileup_batch_skip(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride);
int walt_meth_pileup_batch_skip_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                       const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                       int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                       const void* d_skip, size_t skip_stride, void* stream);

/* ---- overlap of a pair: a base that both mates of a unique proper pair cover is called once ------------------------
 * The reference has no such mode.  When the fragment is shorter than the two reads together, both mates sequence the same
 * bases of one molecule; counting them twice doubles that molecule's weight.  Here mate 1 keeps its calls and the part of
 * mate 2 that lies on mate 1's called span gets none (Bismark's --no_overlap rule).  The contract is defined here.
 *
 * For one walt_pair_result, in forward positions as the pile-up defines them: with [lo, hi) the chromosome that holds
 * genome_pos, strand position q has f(q) = q on a '+' record and f(q) = lo + hi - 1 - q on a '-' record.  len1, len2 are
 * the mates' lengths (differences of their offsets), p1, p2 their genome_pos, call_len1 / call_len2 as in the
 * methylation calls (NULL: the whole read).
 *   Mate 1's called span  S1 = { f(p1 + j) : 0 <= j < min(len1, call_len1), p1 + j < hi }: a contiguous interval
 *   [A1, B1) of forward positions.
 *   The excluded interval: the read positions j of mate 2 with f(p2 + j) inside [A1, B1) form one interval
 *   [ex_lo, ex_hi) in mate 2's read coordinates, clipped to [0, len2]: [A1 - p2, B1 - p2) for a '+' mate 2,
 *   [lo + hi - p2 - B1, lo + hi - p2 - A1) for a '-' one.  When mate 1 lies strictly inside mate 2 (it is short or
 *   clipped) the interval lies in the middle of mate 2.
 *   Encoding: one uint32_t per pair, ex_lo | ex_hi << 16.  It is 0 when nothing is excluded: an empty interval,
 *   best_times != 1, a mate with times != 1, a genome_pos outside the genome, mates on different chromosomes, a read
 *   longer than 1024 bases.
 * The definition is in forward coordinates alone and does not ask the mates' strands to differ: hand-made records with
 * equal strands follow the same formula.  The conversions play no part.
 *
 * walt_pair_overlap_batch[_device] write excl[n] from pairs[n] and the two mates' offsets (n + 1 each; only their
 * differences are used).  They need an index for the chromosome starts -- with any strands, with or without the
 * reference.  totals (optional, uint64_t[2], ACCUMULATED into, not cleared): [0] pairs with a non-empty interval, [1] the
 * read positions of those intervals below min(len2, call_len2) -- the positions at which mate 2 could have been called.
 * Host form: offsets relative to offsets[0] or not, as the caller has them; waits for the result.  Device form: pointers
 * are HBM addresses on idx's device, asynchronous on `stream`; d_pairs, d_call_len1 / 2 and d_excl 4-byte aligned,
 * d_offsets1 / 2 and d_totals 8-byte aligned.  WALT_EINVAL for a null index, a null array with n > 0, or a misaligned one.
 *
 * Effect on calling.  walt_meth_pileup_batch_excl[_device] are walt_meth_pileup_batch_skip[_device] plus excl
 * (uint32_t[n], one word per record of the batch in the encoding above, 4-byte aligned; NULL: none).  A read position
 * inside its record's interval is treated exactly like a position at or beyond call_len: letter '.', no count, no
 * total, no add to the pile-up.  `reads` of walt_meth_stats is unchanged.  The pile-up may be NULL and skip may be NULL.
 * For a pair: call mate 1 as before and mate 2 with walt_pair_overlap_batch's excl.  Every older entry point is the same
 * call with excl == NULL and gives what it always gave. */
int walt_pair_overlap_batch(walt_index* idx, const walt_pair_result* pairs, const uint64_t* offsets1, const uint64_t* offsets2,
                            uint32_t n, const uint32_t* call_len1, const uint32_t* call_len2, uint32_t* excl,
                            uint64_t* totals /*[2]: pairs, bases*/);
int walt_pair_overlap_batch_device(walt_index* idx, const void* d_pairs, const void* d_offsets1, const void* d_offsets2,
                                   uint32_t n, const void* d_call_len1, const void* d_call_len2, void* d_excl, void* d_totals,
                                   void* stream);
int walt_meth_pileup_batch_excl(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl);
int walt_meth_pileup_batch_excl_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                       const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                       int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                       const void* d_skip, size_t skip_stride, const void* d_excl, void* stream);

/* ---- methylation bias by read position: calls per position of the read as sequenced, context and state ------------
 * The reference has no such mode (its users run a second program over the mapped reads: Bismark's M-bias.txt, MethPipe's
 * per-position bsrate); the contract is defined here.  The table shows end-repair bias at the 5' end of mate 2, adaptor and
 * low-quality bias at the 3' end, and -- in its CHG / CHH rows -- the conversion rate per sequencing cycle.  It needs the
 * calls, their offsets, the records and the skip bytes alone: a set (walt_mbias) belongs to a device, like walt_dedup, not
 * to an index.
 *
 * The set holds n_tables tables, 1 to 8; a caller uses one table per mate.  A table is
 *   uint64_t count[4][2][1024]   (WALT_MBIAS_POSITIONS = 1024, WALT_MBIAS_WORDS = 8192)
 * first index the context (0 CpG, 1 CHG, 2 CHH, 3 unknown), second index 0 methylated / 1 unmethylated, third index the
 * read position.  Counts are exact 64-bit.
 *
 * What counts.  For record r of a batch, read position i in [0, offsets[r + 1] - offsets[r]) adds 1 to count[c][m][i] when
 * calls[offsets[r] + i] is one of the eight letters: z / Z CpG, x / X CHG, h / H CHH, u / U unknown context; upper case is
 * methylated (m = 0), lower case unmethylated (m = 1).  Every other byte adds nothing -- '.', and so the positions that
 * call_len clips and that an excluded interval ("overlap of a pair") blanks.  A record adds only when times == 1 and its
 * skip byte, if given, is zero: the records that walt_meth_stats and the pile-up count.  A read longer than 1024 bases adds
 * nothing (the kernel tests the length before it forms an index).  Consequently, for the same records and calls,
 *   sum over i of count[c][0][i] = walt_meth_stats.meth[c]   and   sum over i of count[c][1][i] = walt_meth_stats.unmeth[c].
 *
 * Life cycle.  walt_mbias_create: WALT_EINVAL when n_tables is outside 1..8 or the device does not exist, WALT_EHIP when
 * there is no device at all; the tables start at zero.  walt_mbias_clear zeroes every table.  walt_mbias_read waits for the
 * device and writes table `table` to out[4][2][1024], folding the replicas the set keeps on the device (8 per table, so
 * that the blocks of a batch do not all add to one line).  walt_mbias_device_bytes = n_tables x 8 x 65536.
 *
 * Batch calls.  walt_mbias_batch[_device] add the calls of one batch to one table.  Strides and alignment as in
 * walt_meth_call_batch: a record stride of at least 16 and a multiple of 4 (64 with a base of &pairs->m1 or &pairs->m2 for
 * one mate of a walt_pair_result array), a skip stride of at least 1 (skip == NULL: none); d_records 4-byte aligned,
 * d_offsets 8-byte aligned, d_calls at any address.  Host form: offsets relative to offsets[0] or not, as the caller has
 * them (calls + offsets[0] is the first byte read); a read longer than 1024 bases is rejected as the calling host form
 * rejects it; it waits for the result.  Device form: pointers are HBM addresses on the set's device, asynchronous on
 * `stream`.  Adds are ordered by their stream, and two streams may feed one set at the same time.  WALT_EINVAL, with a
 * message naming the cause, for a null set, a table index >= n_tables, a null array with n > 0, a bad stride, a
 * misaligned pointer.
 *
 * With the calling.  walt_meth_pileup_batch_mbias[_device] are walt_meth_pileup_batch_excl[_device] plus mb and table:
 * the calls of the batch are added to that table of mb as walt_mbias_batch would add them, under the same skip.  mb == NULL
 * gives exactly the excl form.  The host form keeps its device copy of the calls and counts it before freeing it, also when
 * the caller's `calls` is NULL (it then allocates the device array for itself).  The device form launches the bias kernel
 * behind the calling kernel on the same stream; WALT_EINVAL when mb is given and d_calls is NULL (the table is counted from
 * the calls).  WALT_EINVAL when the set lives on another device than the index, or for a table index >= n_tables.  The
 * pile-up, skip and excl may each be NULL as before.  Every older entry point is this call with mb == NULL and gives what
 * it always gave. */
#define WALT_MBIAS_POSITIONS 1024
#define WALT_MBIAS_WORDS 8192
typedef struct walt_mbias walt_mbias;
int walt_mbias_create(int device, uint32_t n_tables, walt_mbias** out);
void walt_mbias_destroy(walt_mbias* mb);
int walt_mbias_clear(walt_mbias* mb);
uint64_t walt_mbias_device_bytes(const walt_mbias* mb);
int walt_mbias_read(walt_mbias* mb, uint32_t table, uint64_t* out /*[4][2][1024]*/);
int walt_mbias_batch(walt_mbias* mb, uint32_t table, const char* calls, const uint64_t* offsets, uint32_t n,
                     const void* records, size_t record_stride, const uint8_t* skip, size_t skip_stride);
int walt_mbias_batch_device(walt_mbias* mb, uint32_t table, const void* d_calls, const void* d_offsets, uint32_t n,
                            const void* d_records, size_t record_stride, const void* d_skip, size_t skip_stride, void* stream);
int walt_meth_pileup_batch_mbias(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                 const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                 int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                 walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                                 walt_mbias* mb, uint32_t table);
int walt_meth_pileup_batch_mbias_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                        const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                        int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                        const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                        uint32_t table, void* stream);

/* ---- ignored read ends: the first and last bases of a read kept out of the calls, per calling call ---------------------
 * The reference has no such mode.  The bias table above shows which sequencing cycles are biased -- the end-repair fill-in
 * at the 5' end of mate 2, adaptor and low-quality calls at the 3' end, the first cycles of random-primed PBAT libraries;
 * these bounds keep them out of the counts (Bismark's --ignore, --ignore_3prime, --ignore_r2, --ignore_3prime_r2).  The
 * contract is defined here.
 *
 * trim5 and trim3 are two uint32_t per calling call, uniform over the batch; a caller that calls one mate's reads per call
 * so has per-mate values.  For a record of the batch, limit = min(length, call_len) as in the methylation calls.  Read
 * position i may get a call exactly when  trim5 <= i  and  i + trim3 < limit  and every other rule allows it.  Positions
 * are those of `bases` as given: the read as sequenced.  A position outside these bounds is treated exactly like a position
 * at or beyond call_len: letter '.', no count in walt_meth_counts, no total in walt_meth_stats, no add to the pile-up --
 * and nothing in the bias table, which is counted from the calls.  `reads` of walt_meth_stats is unchanged.  trim3 counts
 * back from the clip point, not from the raw length: an adaptor that call_len clipped is not part of the molecule.  Any
 * value is legal: trim5 >= limit, trim3 >= limit or trim5 + trim3 >= limit leaves a record with all '.' and zero counts.
 * trim5 == trim3 == 0 is the call as it was.
 *
 * walt_meth_pileup_batch_trim[_device] are walt_meth_pileup_batch_mbias[_device] plus trim5 and trim3.  They refuse what
 * the bias forms refuse and nothing else: alignment, strides and null arguments as there; the pile-up, skip, excl and the
 * bias set may each be NULL.  Every older entry point is this call with both bounds 0 and gives what it always gave.
 *
 * walt_pair_overlap_batch_trim[_device] are walt_pair_overlap_batch[_device] plus the bounds of both mates.  Mate 1's
 * called span becomes
 *   S1 = { f(p1 + j) : trim5_1 <= j, j + trim3_1 < min(len1, call_len1), p1 + j < hi }
 * -- still one interval of forward positions; the word is 0 when it is empty.  Bases of mate 1 that are ignored are not
 * called by mate 1, so mate 2 keeps its calls there.  The word's encoding and its clipping to [0, len2] are unchanged.
 * Mate 2's own bounds do not move the interval (the calling call applies them); they enter totals[1], which counts the
 * interval's positions j with trim5_2 <= j and j + trim3_2 < min(len2, call_len2): the calls mate 2 can actually lose.
 * totals[0] counts the pairs with a non-zero word, as before.  All four bounds 0: the older call. */
int walt_meth_pileup_batch_trim(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                                walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3);
int walt_meth_pileup_batch_trim_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                       const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                       int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                       const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                       uint32_t table, uint32_t trim5, uint32_t trim3, void* stream);
int walt_pair_overlap_batch_trim(walt_index* idx, const walt_pair_result* pairs, const uint64_t* offsets1, const uint64_t* offsets2,
                                 uint32_t n, const uint32_t* call_len1, const uint32_t* call_len2, uint32_t* excl,
                                 uint64_t* totals /*[2]: pairs, bases*/, uint32_t trim5_1, uint32_t trim3_1, uint32_t trim5_2,
                                 uint32_t trim3_2);
int walt_pair_overlap_batch_trim_device(walt_index* idx, const void* d_pairs, const void* d_offsets1, const void* d_offsets2,
                                        uint32_t n, const void* d_call_len1, const void* d_call_len2, void* d_excl, void* d_totals,
                                        uint32_t trim5_1, uint32_t trim3_1, uint32_t trim5_2, uint32_t trim3_2, void* stream);

/* ---- non-converted reads: reads that bisulfite did not convert, judged from their calls ----------------------------------
 * The reference has no such mode (its users run a second program over the mapped reads: Bismark's filter_non_conversion
 * with --threshold, --consecutive, --percentage_cutoff and --minimum_count); the contract is defined here.  A molecule that
 * escaped conversion keeps its cytosines in non-CpG context, where most mammalian tissue has next to no methylation, so
 * several methylated CHG / CHH calls in one read are a conversion failure, not biology.  The verdict needs the calls, their
 * offsets and the records' times alone; acting on it is the caller's step: OR the byte into the skip array of the calling
 * call that counts ("duplicates" above).
 *
 * Tally of a read.  Scan the bytes of its calls in read order, as walt_meth_call_batch wrote them:
 *   meth  = the number of H and X bytes (methylated CHH and CHG);
 *   total = meth + the number of h and x bytes;
 *   run   = the longest run of H / X in read order, where only an h or an x ends a run.
 * Every other byte -- '.', z, Z, u, U and anything else -- neither extends nor ends a run.
 *
 * Rule.  A judged read fails when any enabled test fires:
 *   min_meth > 0     and  meth >= min_meth;
 *   min_run > 0      and  run >= min_run;
 *   min_percent > 0  and  total >= max(min_total, 1)  and  100 * meth >= min_percent * total   (integer arithmetic).
 * A field of 0 switches its test off; a rule of all zeros filters nobody.  min_percent > 100 is WALT_EINVAL.
 *
 * Which records are judged.  A record is judged when times == 1 and its read has 1 to 1024 calls (device form: and its
 * offsets lie inside [offsets[0], offsets[n])).  Every other record gets filt = 0 and a zero tally, and the kernel forms
 * no address from it.  The verdict is a pure function of the read's calls and the rule: it does not depend on the grid,
 * on the alignment of the calls or on how a stream of reads is cut into calls.
 *
 * walt_nonconv_batch[_device] judge calls that exist.  idx names the device (any strands, with or without the reference).
 * filt[i * filt_stride] is written as 0 or 1 for every record (filt_stride at least 1; 2 with a base of filt or filt + 1 for
 * one mate of a pair); tally[n] is optional (NULL: not wanted).  Strides and alignment as in walt_mbias_batch: a record
 * stride of at least 16 and a multiple of 4; d_records 4-byte aligned, d_offsets and d_tally 8-byte aligned, d_calls and
 * d_filt at any address.  Host form: offsets relative to offsets[0] or not, as the caller has them (calls + offsets[0] is
 * the first byte read); a read of more than 1024 calls is not refused, it is not judged; it waits for the result.  Device
 * form: pointers are HBM addresses on idx's device, asynchronous on `stream`.  WALT_EINVAL, with a message naming the
 * cause, for a null index or rule, min_percent > 100, a null array with n > 0, a bad stride, a misaligned pointer.
 *
 * walt_meth_nonconv_batch[_device] call and judge in one step: the arguments of walt_meth_call_batch[_device] up to
 * call_len, the optional output calls, then rule, filt, filt_stride and tally as above.  They refuse what the calling call
 * refuses, and what walt_nonconv_batch refuses of the rule and filt.  They neither pile up nor sum statistics, and take
 * no skip, excluded interval or ignored read end: the verdict is made from the whole read up to call_len, as Bismark's
 * filter sees the whole XM string.  The host form stages the batch once and keeps its device copy of the calls for the
 * judging kernel (it allocates the device array for itself when the caller's calls is NULL), so the calls do not cross the
 * bus for the verdict.  The device form launches the judging kernel behind the calling kernel on the same stream;
 * WALT_EINVAL when d_calls is NULL (the verdict is made from the calls).
 *
 * walt_nonconv_pairs_batch[_device] apply the pair rule in place on filt[2n], mate k + 1 of pair i at filt[2i + k]: for a
 * pair with best_times == 1 both bytes become filt[2i] | filt[2i + 1] -- when either mate fails the pair goes, as in
 * Bismark; any other pair keeps its mates' own verdicts.  The rule is symmetric in the mates.  d_pairs 4-byte aligned.
 *
 * Every older entry point is unchanged. */
typedef struct {
  uint16_t meth, total, run, reserved; /* reserved written as 0 */
} walt_nonconv_tally; /* 8 bytes */
typedef struct {
  uint32_t min_meth, min_run, min_percent, min_total;
} walt_nonconv_rule;
int walt_nonconv_batch(walt_index* idx, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                       size_t record_stride, const walt_nonconv_rule* rule, uint8_t* filt, size_t filt_stride,
                       walt_nonconv_tally* tally);
int walt_nonconv_batch_device(walt_index* idx, const void* d_calls, const void* d_offsets, uint32_t n, const void* d_records,
                              size_t record_stride, const walt_nonconv_rule* rule, void* d_filt, size_t filt_stride,
                              void* d_tally, void* stream);
int walt_meth_nonconv_batch(walt_index* idx, const char* bases, const uint64_t* offsets, uint32_t n, const void* records,
                            size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                            const uint32_t* call_len, char* calls, const walt_nonconv_rule* rule, uint8_t* filt,
                            size_t filt_stride, walt_nonconv_tally* tally);
int walt_meth_nonconv_batch_device(walt_index* idx, const void* d_bases, const void* d_offsets, uint32_t n,
                                   const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                   int conversion, const void* d_call_len, void* d_calls, const walt_nonconv_rule* rule,
                                   void* d_filt, size_t filt_stride, void* d_tally, void* stream);
int walt_nonconv_pairs_batch(walt_index* idx, const walt_pair_result* pairs, uint32_t n, uint8_t* filt /*[2n]*/);
int walt_nonconv_pairs_batch_device(walt_index* idx, const void* d_pairs, uint32_t n, void* d_filt /*[2n]*/, void* stream);

/* ---- adjacent CpG pairs: which states two neighbouring CpGs had together on one read -------------------------------------
 * The reference has no such mode (its users run a second program over the sorted mapped reads: MethPipe's allelicmeth and
 * amrfinder, epipolymorphism and entropy tools); the contract is defined here.  Every other count of this library collapses
 * a read into independent positions; this table keeps the joint state of neighbouring CpGs of one molecule, which cannot be
 * rebuilt from per-position counts.
 *
 * Pairs.  A pair is a forward position c with R[c] == C, R[c + 1] == G and c + 1 in c's chromosome -- the pairs of
 * "methylation levels" above, so a C that ends a chromosome in front of a G that starts the next is no pair.  Pairs are
 * numbered j = 0 .. n_pairs - 1 by ascending c over the whole genome; n_pairs equals row[4].sites of
 * walt_pileup_levels(p, 0, genome_len, ...).  The table is
 *   uint32_t count[n_pairs][4]
 * exact up to 2^32 - 1, wrapping beyond.  Entry j describes the couple (pair j, pair j + 1).  Columns: 0 MM, 1 MU, 2 UM,
 * 3 UU; the first letter is the state of pair j, the lower forward position.
 *
 * What a read adds.  A record counts when times == 1, its skip byte, if given, is 0, its read has 1 to 1024 calls and
 * genome_pos < genome_len: the records walt_mbias_batch counts, plus the position test.  With [lo, hi) the chromosome of
 * genome_pos, read position i whose calls byte is z or Z has q = genome_pos + i and is ignored when q >= hi; otherwise its
 * forward position is f = q for a '+' record and f = lo + hi - 1 - q for a '-' record, and its pair is f if f is a pair,
 * else f - 1 if that is a pair, else the call is ignored.  R alone decides this, not the conversion, so every read that
 * reaches f agrees.  (On an N-free genome no call of the calling kernel is ever ignored; hand-made calls and N fills can
 * be.)  Let the calls that have a pair be (j_1, m_1) .. (j_k, m_k) in read order, m = upper case.  For t = 1 .. k - 1: when
 * |j_{t+1} - j_t| == 1, add 1 to count[min(j_t, j_{t+1})][2 * u_lo + u_hi], u = 1 for an unmethylated call, lo the call on
 * the lower pair.  Every other couple adds nothing: an uncalled or mismatched CpG in between, the two calls of one pair in
 * a made-up string.  Every other byte is skipped, so call_len, excluded intervals and ignored read ends act through the '.'
 * they leave: a pair whose partner was blanked is not counted.  A '-' record walks the pairs downwards; min and lo / hi
 * make its entry the reverse-complement read's.  Each mate counts by itself; the two mates are not joined into a fragment.
 *
 * Life cycle.  walt_cpgpairs_create builds, on the index's device, one bit per forward position (set where a pair
 * starts) and the number of pairs in front of every 128 positions -- genome_len / 8 + genome_len / 32 bytes -- and the
 * zeroed table, 16 bytes per pair.  WALT_EINVAL when the index holds no reference; WALT_ENOMEM, naming the bytes wanted,
 * when the device has no room, and the index stays usable.  The object must be destroyed before the index is closed.
 * walt_cpgpairs_clear zeroes the table.  walt_cpgpairs_device_bytes: what the object holds.
 *
 * Batch calls.  walt_cpgpairs_batch[_device] add the calls of one batch.  Strides, alignment, the host and the device form,
 * the refusals and the ordering -- adds are ordered by their stream, two streams may feed one table -- are those of
 * walt_mbias_batch[_device]; a null object is WALT_EINVAL.
 *
 * Extraction.  walt_cpgpairs_extract[_device] return the entries with c_j in [pos_lo, pos_hi) and a non-zero counter,
 * ascending, as walt_cpgpair_site records: pos = c_j, next = c_{j+1}, n = the four counters.  A non-zero entry has
 * next < pos + 1024, because one read held both calls (pos + 1024 itself only from a hand-made string that calls the G of
 * one pair and the C of the other). cap, *n_out, the range errors and "one extraction at a time" are
 * those of walt_pileup_extract[_device]: the host form returns WALT_EINVAL with *n_out set when the range holds more than
 * cap entries; the device form writes the count to *d_n_out and nothing else when it exceeds cap.  d_out and d_n_out
 * 8-byte aligned.  The records do not depend on the launch shape (option pile_extract_blocks).
 *
 * With the calling.  walt_meth_pileup_batch_pairs[_device] are walt_meth_pileup_batch_trim[_device] plus ap: the calls of the
 * batch are added as walt_cpgpairs_batch would add them under the same skip, behind the calling kernel on the same stream.
 * The host form counts from its device copy of the calls, also when the caller's `calls` is NULL.  ap == NULL is exactly
 * the trim form.  WALT_EINVAL when ap belongs to another index or (device form) when d_calls is NULL.  Every older entry
 * point is this call with ap == NULL and launches what it always launched. */
typedef struct walt_cpgpairs walt_cpgpairs;
typedef struct {
  uint32_t pos, next; /* forward positions of the C of pair j and of pair j + 1 */
  uint32_t n[4];      /* MM, MU, UM, UU */
} walt_cpgpair_site;  /* 24 bytes */
int walt_cpgpairs_create(walt_index* idx, walt_cpgpairs** out);
void walt_cpgpairs_destroy(walt_cpgpairs* ap);
int walt_cpgpairs_clear(walt_cpgpairs* ap);
uint64_t walt_cpgpairs_device_bytes(const walt_cpgpairs* ap);
uint64_t walt_cpgpairs_n_pairs(const walt_cpgpairs* ap);
int walt_cpgpairs_batch(walt_cpgpairs* ap, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                        size_t record_stride, const uint8_t* skip, size_t skip_stride);
int walt_cpgpairs_batch_device(walt_cpgpairs* ap, const void* d_calls, const void* d_offsets, uint32_t n, const void* d_records,
                               size_t record_stride, const void* d_skip, size_t skip_stride, void* stream);
int walt_cpgpairs_extract(walt_cpgpairs* ap, uint32_t pos_lo, uint32_t pos_hi, walt_cpgpair_site* out, uint64_t cap,
                          uint64_t* n_out);
int walt_cpgpairs_extract_device(walt_cpgpairs* ap, uint32_t pos_lo, uint32_t pos_hi, void* d_out, uint64_t cap, void* d_n_out,
                                 void* stream);
int walt_meth_pileup_batch_pairs(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                 const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                 int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                 walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                                 walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap);
int walt_meth_pileup_batch_pairs_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                        const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                        int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                        const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                        uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, void* stream);

/* ---- four-CpG epialleles: which of the 16 patterns four neighbouring CpGs showed on one read --------------------------------
 * The reference has no such mode (its users write SAM, sort it and run a second program over every XM:Z: string); the
 * contract is defined here.  Epipolymorphism (Landan 2012), methylation entropy (Xie 2011), methclone's clonality shift
 * (Li 2014) and the proportion of discordant reads (Landau 2014) are all defined on this table.  It cannot be rebuilt from
 * the pair table above, for the reason that table cannot be rebuilt from per-position counts.
 *
 * Pairs and numbering are those of "adjacent CpG pairs": j = 0 .. n_pairs - 1 by ascending forward position c_j of the C,
 * the chromosome rule included.  The table is
 *   uint32_t count[n_pairs][16]
 * exact up to 2^32 - 1, wrapping beyond.  Entry j describes the window of pairs j, j + 1, j + 2, j + 3.  Column
 * p = 8 u0 + 4 u1 + 2 u2 + u3, u_i the state of pair j + i, 1 = unmethylated: 0 is MMMM, 15 is UUUU, and the first letter
 * belongs to the lowest forward position (this extends the pair table's 2 u_lo + u_hi).  The last three entries never
 * receive an add.
 *
 * What a read adds.  The records that count, the calls that have a pair and how a call finds its pair number are word for
 * word those of walt_cpgpairs_batch: times == 1, skip byte 0, 1 to 1024 calls, genome_pos < genome_len, the q >= hi rule,
 * the C or the G of the pair, '-' records mirrored.  Let the calls with a pair be (j_1, u_1) .. (j_k, u_k) in read order.
 * For every t with t + 3 <= k: when j_{t+i} = j_t + i s for i = 1, 2, 3 with one s in {+1, -1}, the read adds 1 to
 * count[min(j_t, j_{t+3})][p], p formed from the four states in forward order.  Four calls qualify only if they follow
 * each other among the calls that have a pair: a '.' where a CpG was blanked (a mismatch, a clip, an ignored end, an
 * overlap position) makes the pair numbers on its two sides no neighbours, and so does the second call of one pair in a
 * made-up string; nothing is counted across such a break.  A chain of m neighbouring calls adds m - 3 windows.  A '-'
 * record and its reverse complement add to the same entry and column.  Each mate counts by itself.
 *   Every read that adds a window also adds the three couples inside it to a pair table fed the same batch, so for all j,
 * a, b: the sum over the p with (u0, u1) = (a, b) of count[j][p] is at most pairs[j][2 a + b], and likewise against the
 * pair table's entries j + 1 and j + 2 for (u1, u2) and (u2, u3).
 *
 * Life cycle.  walt_epialleles_create builds, on the index's device, the object's own pair bitmap and rank directory -- by
 * the code walt_cpgpairs_create builds them with; one rank structure shared between a pair table and a window table is
 * not offered -- and the zeroed table, 64 bytes per pair (1.8 GB for the 28 M CpGs of a human genome).  WALT_EINVAL when
 * the index holds no reference; WALT_ENOMEM, naming the bytes wanted, when the device has no room, and the index stays
 * usable.  The object must be destroyed before the index is closed.  walt_epialleles_clear zeroes the table.
 *
 * Batch calls.  walt_epialleles_batch[_device] take the arguments, strides, refusals and stream ordering of
 * walt_cpgpairs_batch[_device]; two streams may feed one table.
 *
 * Extraction.  walt_epialleles_extract[_device] return the entries with c_j in [pos_lo, pos_hi) whose sixteen counters sum
 * (in 64 bits) to at least min_total, ascending, as walt_epiallele_site records: pos = c_j, last = c_{j+3}, n = the
 * sixteen counters.  min_total == 0 is WALT_EINVAL.  Membership goes by pos alone: a window that starts inside the range
 * and ends behind it is returned, one that starts in front of it is not.  last <= pos + 1024: a returned entry got an add,
 * so one read of at most 1024 calls, which spans positions q .. q + 1023, held a call on each of the four pairs; a call
 * sits on the C or the G of its pair, so c_j >= q - 1 and c_{j+3} <= q + 1023, and the extreme pos + 1024 needs a
 * hand-made string that calls the G of the first pair and the C of the last (calls the library made give
 * last <= pos + 1023).  last is found by three steps along the bitmap, each of which looks at least 1056 positions ahead.  cap,
 * *n_out, the range errors, the alignment and "nothing written when over cap" are those of walt_cpgpairs_extract[_device].
 * The records do not depend on the launch shape (option pile_extract_blocks).
 *
 * With the calling.  walt_meth_pileup_batch_epi[_device] are walt_meth_pileup_batch_pairs[_device] plus ep: the calls of the
 * batch are added as walt_epialleles_batch would add them under the same skip, behind the calling kernel (and the pair
 * kernel, if ap is given) on the same stream.  ep == NULL is exactly the pairs form.  WALT_EINVAL when ep belongs to
 * another index or (device form) when d_calls is NULL.  Every older entry point is this call with ep == NULL and launches
 * what it always launched. */
typedef struct walt_epialleles walt_epialleles;
typedef struct {
  uint32_t pos, last; /* forward positions of the C of pair j and of pair j + 3 */
  uint32_t n[16];     /* MMMM, MMMU, MMUM, .. UUUU */
} walt_epiallele_site; /* 72 bytes */
int walt_epialleles_create(walt_index* idx, walt_epialleles** out);
void walt_epialleles_destroy(walt_epialleles* ep);
int walt_epialleles_clear(walt_epialleles* ep);
uint64_t walt_epialleles_device_bytes(const walt_epialleles* ep);
uint64_t walt_epialleles_n_pairs(const walt_epialleles* ep);
int walt_epialleles_batch(walt_epialleles* ep, const char* calls, const uint64_t* offsets, uint32_t n, const void* records,
                          size_t record_stride, const uint8_t* skip, size_t skip_stride);
int walt_epialleles_batch_device(walt_epialleles* ep, const void* d_calls, const void* d_offsets, uint32_t n, const void* d_records,
                                 size_t record_stride, const void* d_skip, size_t skip_stride, void* stream);
int walt_epialleles_extract(walt_epialleles* ep, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, walt_epiallele_site* out,
                            uint64_t cap, uint64_t* n_out);
int walt_epialleles_extract_device(walt_epialleles* ep, uint32_t pos_lo, uint32_t pos_hi, uint64_t min_total, void* d_out,
                                   uint64_t cap, void* d_n_out, void* stream);
int walt_meth_pileup_batch_epi(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                               const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                               int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                               walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                               walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap,
                               walt_epialleles* ep);
int walt_meth_pileup_batch_epi_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                      const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                      int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                      const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                      uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, walt_epialleles* ep,
                                      void* stream);

/* ---- opposite-strand evidence: C>T variant sites found from the reads of the other strand, and kept out of the counts ------
 * The reference has no such mode (MethPipe's methcounts tags a site as mutated, CpGx, when fewer than half of the
 * opposite-strand reads show the expected base; MethylDackel drops such sites, --maxVariantFrac / --minOppositeDepth; both
 * over sorted SAM); the contract is defined here.  Bisulfite turns an unmethylated C into T, so a sample that has T where
 * the reference has C piles up as a fully unmethylated cytosine.  A read of the other strand covers the same position and
 * bisulfite leaves it alone there: it shows G for a real C and A for a C>T variant.
 *
 * Evidence.  Use the same reference arrays the calling uses: G = R for a '+' record and G = R' for a '-' record.  Use the
 * same validity rule as the pile-up: times == 1; skip byte 0; genome_pos < genome_len; conversion 'T' or 'A'; read length
 * 1 to 1024.  A record that passes, at read position i < min(length, call_len) with q = genome_pos + i < hi, adds
 * evidence as follows.
 *   conversion 'T': an evidence position is one with G[q] == 'G'; match: the read base is G; other: any other base;
 *   conversion 'A': an evidence position is one with G[q] == 'C'; match: the read base is C; other: any other base.
 * This is the calling rule with the conversion exchanged, and with "anything but the reference base" in place of "the
 * converted base".  A byte that is not A, C, G or T counts as the letter whose bits 2..1 it shares, as in
 * meth_read_fields.
 *   The evidence lands on the forward position that pile_forward gives, f = q or f = lo + hi - 1 - q.  Evidence from
 * ('+','T') and ('-','A') records therefore lands on forward G's, and evidence from ('+','A') and ('-','T') records lands
 * on forward C's.  Each lands on the site whose methylation calls come from the other two kinds of record.
 *   -C acts on the evidence through call_len.  -D and -F act on it through skip.  -I5, -I3 and -NO do not act on it: they
 * are about methylation bias, not about which base was read.  Each mate counts by itself.
 *   Evidence landing on a forward A or T of R (the N-fill case of "methylation pile-up") is never read.
 *
 * Storage.  The evidence lives in a second walt_pileup of the same index: plane 0 (what walt_pileup_read returns as
 * meth) is match, plane 1 (unmeth) is other; exact 32-bit counters, wrapping beyond 2^32 - 1.  walt_pileup_create,
 * _clear, _read and _add serve it as they serve the calls, and _read / _add give the fold over several devices.  It takes
 * 8 x genome_len more bytes of device memory (25 GB at 3.1 Gbp); WALT_ENOMEM as there.
 *
 * Rule.  A forward position f with R[f] C or G is judged when match[f] + other[f] >= min_depth.  It is flagged when it is
 * judged and 100 * other[f] > max_percent * (match[f] + other[f]), computed in 64 bits.  min_depth is 1 to 2^32 - 1,
 * max_percent 0 to 99 (WALT_EINVAL otherwise).  With max_percent = 50 this is MethPipe's rule exactly.
 *
 * walt_meth_evidence_batch[_device] run the evidence kernel alone over a batch given as walt_meth_call_batch[_device]
 * takes it, plus skip as walt_meth_pileup_batch_skip takes it: strides, refusals, alignment and stream ordering as there;
 * nothing but the evidence is written.  WALT_EINVAL for a null evidence object or one of another index.  Two streams may
 * feed one object.
 *
 * walt_meth_pileup_batch_ev[_device] are walt_meth_pileup_batch_epi[_device] plus ev: the evidence kernel runs behind the
 * calling kernel on the same stream, over the batch as staged once.  ev == NULL is exactly the epi form.  WALT_EINVAL when
 * ev belongs to another index or when ev == p.  Every older entry point is this call with ev == NULL and launches what it
 * always launched.
 *
 * walt_pileup_variants[_device] return the flagged positions of [pos_lo, pos_hi) in ascending order as walt_variant_site
 * records: strand and context as the extraction gives them, meth and unmeth from p (both may be 0), match and other from
 * ev.  cap and *n_out behave as in walt_pileup_extract[_device]: nothing is written when the result is over cap (host
 * form: WALT_EINVAL naming both numbers; device form: *d_n_out > cap says so).  d_out and d_n_out 8-byte aligned.  The
 * result does not depend on the launch shape (option pile_extract_blocks).
 *
 * walt_pileup_mask_variants[_device] zero meth[f] and unmeth[f] of every flagged position of the range in p and give
 * out[5] = {judged, flagged, masked sites (flagged with a call), methylated calls removed, unmethylated calls removed}.
 * Masked sites and calls removed are what this call removed: a second call over the same range returns the same judged
 * and flagged, and zeros for the other three.  All folds are integer and commutative.  d_out: uint64_t[5], 8-byte aligned.
 *
 * Both passes: WALT_EINVAL for a null object, for ev == p, for an ev of another index and for a range outside the genome.
 * They use the table of ev: one of them at a time per evidence object, ordered after the adds of its stream; the host
 * forms wait for all work on the device first. */
typedef struct {
  uint32_t pos, meth, unmeth;
  uint8_t strand;  /* '+' or '-' */
  uint8_t context; /* 0 CpG, 1 CHG, 2 CHH, 3 unknown */
  uint16_t reserved; /* written as 0 */
  uint32_t match, other; /* the opposite-strand reads that show the reference base / another base */
} walt_variant_site; /* 24 bytes */
int walt_meth_evidence_batch(walt_index* idx, walt_pileup* ev, const char* bases, const uint64_t* offsets, uint32_t n,
                             const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                             int conversion, const uint32_t* call_len, const uint8_t* skip, size_t skip_stride);
int walt_meth_evidence_batch_device(walt_index* idx, walt_pileup* ev, const void* d_bases, const void* d_offsets, uint32_t n,
                                    const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                    int conversion, const void* d_call_len, const void* d_skip, size_t skip_stride,
                                    void* stream);
int walt_meth_pileup_batch_ev(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                              const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                              int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                              walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                              walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap,
                              walt_epialleles* ep, walt_pileup* ev);
int walt_meth_pileup_batch_ev_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                     const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                     int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                     const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                     uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, walt_epialleles* ep,
                                     walt_pileup* ev, void* stream);
int walt_pileup_variants(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth,
                         uint32_t max_percent, walt_variant_site* out, uint64_t cap, uint64_t* n_out);
int walt_pileup_variants_device(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth,
                                uint32_t max_percent, void* d_out, uint64_t cap, void* d_n_out, void* stream);
int walt_pileup_mask_variants(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth,
                              uint32_t max_percent, uint64_t* out /*[5]*/);
int walt_pileup_mask_variants_device(walt_pileup* p, walt_pileup* ev, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_depth,
                                     uint32_t max_percent, void* d_out, void* stream);

/* ---- minimum base quality: read bases below a quality floor get no call and give no evidence -----------------
 *
 * A sequencing error C<->T at a cytosine looks like a methylation state; the base qualities say where one is likely.
 * (bin/walt also gives every non-ACGT read character a random base for mapping; such bases come with the lowest
 * quality, and a floor is what keeps them out of the counts.)
 *
 * quals     one byte per base, at the same offsets and in the same order as `bases`: the read as sequenced.
 * min_qual  uniform over the call, 0 to 127, compared with the raw byte, unsigned: the caller adds the Phred offset.
 *           A larger value: WALT_EINVAL.  A byte of 128 or more passes every legal floor.
 *
 * Read position i of a record may get a call exactly when quals[off + i] >= min_qual AND every other rule allows it
 * (call_len, the chromosome, excl, trim5 / trim3, the record rules): the masks compose by AND.  A masked position is
 * treated exactly like one at or beyond call_len: the letter is '.', no count in walt_meth_counts, no total in
 * walt_meth_stats, no add to the pile-up, nothing in the bias, pair and window tables (they are counted from the calls;
 * the '.' breaks a run of neighbouring CpGs like any other), and `reads` is unchanged.
 *   opposite-strand evidence  a masked position adds neither match nor other: this is about which base was read, so
 *                             unlike trim5 / trim3 and excl it does act on the evidence.
 *   non-conversion verdict    made from the masked calls: a base that was not read reliably is no evidence of a
 *                             failed conversion.
 *   overlap of a pair         the interval of walt_pair_overlap_batch[_trim] does not change: a position where mate 1 is
 *                             masked and mate 2 is excluded is called by neither.
 * quals == NULL requires min_qual == 0 (else WALT_EINVAL) and is the call as it was; quals != NULL with min_qual == 0
 * gives what the call without qualities gives, byte for byte.
 *
 * walt_meth_pileup_batch_qual[_device] is walt_meth_pileup_batch_ev[_device] plus quals, min_qual: the pile-up, evidence,
 * bias set, pair table, window table, skip, excl and calls may each be NULL; with only an evidence object it runs the
 * evidence kernel alone.  walt_meth_nonconv_batch_qual[_device] is walt_meth_nonconv_batch[_device] plus the two.
 * Every older entry point is the new one with quals = NULL.  Device forms: d_quals needs no alignment and may differ
 * from d_bases and d_calls modulo 16; nothing is read in front of d_quals[0] or at or beyond d_quals[offsets[n]]. */
int walt_meth_pileup_batch_qual(walt_index* idx, walt_pileup* p, const char* bases, const uint64_t* offsets, uint32_t n,
                                const void* records, size_t record_stride, const uint8_t* conv, size_t conv_stride,
                                int conversion, const uint32_t* call_len, char* calls, walt_meth_counts* counts,
                                walt_meth_stats* stats, const uint8_t* skip, size_t skip_stride, const uint32_t* excl,
                                walt_mbias* mb, uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap,
                                walt_epialleles* ep, walt_pileup* ev, const uint8_t* quals, uint32_t min_qual);
int walt_meth_pileup_batch_qual_device(walt_index* idx, walt_pileup* p, const void* d_bases, const void* d_offsets, uint32_t n,
                                       const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                       int conversion, const void* d_call_len, void* d_calls, void* d_counts, void* d_stats,
                                       const void* d_skip, size_t skip_stride, const void* d_excl, walt_mbias* mb,
                                       uint32_t table, uint32_t trim5, uint32_t trim3, walt_cpgpairs* ap, walt_epialleles* ep,
                                       walt_pileup* ev, const void* d_quals, uint32_t min_qual, void* stream);
int walt_meth_nonconv_batch_qual(walt_index* idx, const char* bases, const uint64_t* offsets, uint32_t n, const void* records,
                                 size_t record_stride, const uint8_t* conv, size_t conv_stride, int conversion,
                                 const uint32_t* call_len, char* calls, const walt_nonconv_rule* rule, uint8_t* filt,
                                 size_t filt_stride, walt_nonconv_tally* tally, const uint8_t* quals, uint32_t min_qual);
int walt_meth_nonconv_batch_qual_device(walt_index* idx, const void* d_bases, const void* d_offsets, uint32_t n,
                                        const void* d_records, size_t record_stride, const void* d_conv, size_t conv_stride,
                                        int conversion, const void* d_call_len, void* d_calls, const walt_nonconv_rule* rule,
                                        void* d_filt, size_t filt_stride, void* d_tally, const void* d_quals, uint32_t min_qual,
                                        void* stream);

/* ---- called sites: which cytosines are methylated at all ------------------------------------------------------
 * The reference has no such mode (methylpy's call_methylated_sites and Lister 2009 test every site with a binomial test
 * against the sample's non-conversion rate and control the false discovery rate per context; MethPipe users take bsrate
 * and thresholds); the contract is defined here.  The p-value of a site depends on its context and on the pair
 * (depth, meth) alone, so the device side is exact: a joint histogram of (depth, meth) per context, and an extraction
 * with a table "smallest significant meth per depth" as its predicate.  The p-values, Benjamini-Hochberg and the table
 * are the host's (walt_amd/csrc/sitecall_core.h); the device runs no floating point.
 *
 * A site is exactly what walt_pileup_extract returns: a covered position f of the range whose R[f] is C or G, with the
 * context the extraction gives it.  Positions covered on an A or T of R are no sites and appear nowhere here.  For a site,
 * d = meth + unmeth (in 64 bits: up to 2^33 - 2) and m = meth.
 *
 * Histogram.  walt_pileup_depth_hist adds, for every site of [pos_lo, pos_hi) with context c,
 *   d <= WALT_SITECALL_DEPTH:  hist[c][bin(d, m)] += 1,   bin(d, m) = (d - 1) * (d + 2) / 2 + m   (1 <= d, 0 <= m <= d)
 *   otherwise:                 deep[c] += 1
 * into arrays it has zeroed: hist uint64_t[4][WALT_SITECALL_BINS], deep uint64_t[4].  sum(hist[c]) + deep[c] is the number
 * of records the extraction returns for context c; the result is additive over any partition of a range, all folds are
 * integer and commutative, and the launch shape (option pile_extract_blocks) cannot change a bit.  Device form: d_hist
 * (264,160 bytes) and d_deep (32 bytes) are HBM addresses, 8-byte aligned, zeroed by the call itself on `stream`.  The
 * histogram lives in the caller's memory; the pile-up's table is not used.
 *
 * Called sites.  walt_pileup_call_sites writes, ascending by pos, a walt_meth_site for every site of the range with
 *   d <= WALT_SITECALL_DEPTH and meth >= min_meth[c][d]:  reserved = 0  (a value above d: none at this depth; index 0 of a
 *                                                         row is never read)
 *   d >  WALT_SITECALL_DEPTH:                             reserved = 1  (a deep site: the caller judges it)
 * min_meth: uint32_t[4][128].  With min_meth[c][d] = d + 1 everywhere the call returns exactly the deep sites.  cap, *n_out
 * and a cap that is too small behave as in walt_pileup_extract[_device]: the host form returns WALT_EINVAL naming both
 * numbers with *n_out set, the device form leaves *d_n_out > cap, and nothing is written.  Device form: d_min_meth 4-byte,
 * d_out 16-byte, d_n_out 8-byte aligned.
 *
 * Errors and ordering as walt_pileup_extract[_device]: WALT_EINVAL for a null pile-up, a null array, pos_lo > pos_hi,
 * pos_hi > genome_len or a misaligned device address; the host forms wait for all work on the device first, the device
 * forms are asynchronous on `stream`.  walt_pileup_call_sites keeps its block offsets in the pile-up's table and counts as
 * an extraction under "one at a time per pile-up"; walt_pileup_device_bytes is as before. */
#define WALT_SITECALL_DEPTH 127u          /* depths 1..127 are histogrammed; deeper sites are "deep" */
#define WALT_SITECALL_BINS  8255u         /* per context: sum over d = 1..127 of (d + 1) = 127 * 130 / 2 */
int walt_pileup_depth_hist(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, uint64_t* hist /*[4][WALT_SITECALL_BINS]*/,
                           uint64_t* deep /*[4]*/);
int walt_pileup_depth_hist_device(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, void* d_hist, void* d_deep, void* stream);
int walt_pileup_call_sites(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, const uint32_t* min_meth /*[4][128]*/,
                           walt_meth_site* out, uint64_t cap, uint64_t* n_out);
int walt_pileup_call_sites_device(walt_pileup* p, uint32_t pos_lo, uint32_t pos_hi, const void* d_min_meth, void* d_out,
                                  uint64_t cap, void* d_n_out, void* stream);

/* ---- options ---------------------------------------------------------------------------------
 * Tuning values and test hooks of the mapping calls, per index.  The mapping calls read NO environment
 * variable: an index maps the same way whatever the process environment holds (the library's only
 * environment inputs are read once, when an index is opened or built: WALT_AMD_WIN / _WIN_GB /
 * _WIN_RESERVE_GB (dense candidate windows: on/off, memory cap, memory left free), WALT_AMD_FENCE,
 * WALT_AMD_TABLE, WALT_AMD_VERBOSE; and WALT_AMD_RCCL, the library walt_comm_* binds).  Every option
 * changes the schedule of a call, never its results.  Names (value 0 / 1 unless said otherwise):
 *   se_pipe        1  staged heavy pass in two halves on two streams
 *   se_heavy_chunk 0  reads per chunk of the heavy list (0: default; a test hook for several chunks on a small batch)
 *   se_lit_side    1  literal pass on a side stream beside the end of the heavy pass (0: after it, on the call's stream)
 *   se_defer_min  -1  long seeds: key-equal ranges of more slots than this go to the verifier unnarrowed (-1: default 4, 0: never)
 *   se_stage_occ   0  wavefronts per SIMD the stage kernel is built for (0: chosen by read length and sequence count;
 *                     3 / 4 for reads of up to 128 bases, 2 / 3 up to 160)
 *   se_carry       1  pass 1 hands its state to the staged rounds (0: they start over at seed 0)
 *   se_heavy_mono  0  the one-kernel heavy pass instead of the staged rounds
 *   se_verify_share 1 reads of up to 128 bases: the dense work items of a round grouped by the region they name, a
 *                     region's records streamed once per group of reads (0: once per item, the launches as they were;
 *                     2: grouped and counted, verified one by one -- tools/verify_share_bench.py)
 *   se_share_r     0  with se_verify_share = 2 only: items per counted group at most (0: 4, as the verifier's; up to 64)
 *   se_share_cap   0  items of a launch that are grouped (0: all; a test hook: the others are verified one by one)
 *   grid           0  blocks of the persistent kernels (0: 8 per compute unit)
 *   pe_mode        0  0: staged path, 1: list kernels only
 *   pe_chunk       0  pairs per pass (0: default)          pe_rounds    0  rounds of a staged list (0: default, 1, 2, 4)
 *   pe_stage_cap   0  staged reads per round (0: default)  pe_small_heaps 0  force the 8-slot heaps of long literal lists
 *   pe_serial      0  mates and passes on one stream (profiling)   pe_push_wide 0  4-byte heap entries in the push kernel (A/B)
 *   pe_defer_min  -1  as se_defer_min                      pe_roomy    -1  -1: by the workspace's size, 0 / 1: forced
 *   pe_lit_fuse    1  the literal round's three seed shifts in one launch when its list is short (0: seed by seed)
 *   pile_rows      0  pile-up adds with neighbouring lanes on neighbouring positions instead of one lane per 16-base slice (A/B)
 *   pile_extract_blocks 0  blocks of the pile-up's extraction kernels (0: by the range; a test hook: the table is the same)
 * Set between calls, not during one.  WALT_EINVAL for an unknown name. */
int walt_index_set_option(walt_index* idx, const char* name, long long value);
int walt_index_get_option(const walt_index* idx, const char* name, long long* value);

/* ---- makedb-compatible index builders (reference.cpp:79-322,
 *      makedb.cpp:46-159) ---------------------------------------------------- */

/* Host builder: reads FASTA (file or directory of .fa), writes the five .dbindex
 * files.  Byte-identical to the reference makedb for N-free FASTA. */
int walt_makedb(const char* fasta_path, const char* out_dbindex_path, int threads);

/* The same files from the GPU builder (walt_index_build_device + walt_index_write): seconds
 * instead of hours at 3 Gbp.  Identical to the host builder except for the order of entries
 * whose 60 compared characters are all equal (ascending position here, whatever std::sort
 * leaves in the reference, reference.cpp:296-298); one N fill serves all four strands. */
int walt_makedb_device(const char* fasta_path, const char* out_dbindex_path, int device);

/* GPU builder: d_genome_ascii is the concatenated genome (upper-case ACGT, no N)
 * in HBM on `device`; builds the selected strand indexes there and leaves them
 * resident (BuildIndex, makedb.cpp:46-85).  Same result as the reference makedb
 * except for the order of entries whose 60 care characters are all equal
 * (std::sort leaves those in an unspecified order, reference.cpp:296-298). */
int walt_index_build_device(const void* d_genome_ascii, uint32_t n_chrom, const uint32_t* chrom_len,
                            const char* const* chrom_names, int device, unsigned strand_mask,
                            int dir_bits, walt_index** out);

/* HashTable::index_size of a resident strand (reference.hpp:84). */
uint32_t walt_index_size(const walt_index* idx, int strand);

/* Copy a resident strand back to host arrays laid out like the strand file
 * (reference.cpp:302-322): genome_out[genome_len] chars, counter_out[4^12+1],
 * index_out[index_size].  Any pointer may be NULL. */
int walt_index_export_strand(const walt_index* idx, int strand, uint8_t* genome_out,
                             uint32_t* counter_out, uint32_t* index_out);

/* WriteIndex x4 + WriteIndexHeadInfo (reference.cpp:302-322, 353-379) from the
 * resident index.  Writes the head file and the strand file of every resident
 * strand (a C->T-only index writes <path>, <path>_CT00 and <path>_CT01, which is
 * all the reference's single-end mode without -A reads, mapping.cpp:491-492). */
int walt_index_write(const walt_index* idx, const char* dbindex_path);

/* ---- multi-GPU: one process per GPU, the statistics block is the only exchange -----------------
 *
 * The reference is a single process; what it carries ACROSS reads is the statistics block that
 * ProcessSingledEndReads / ProcessPairedEndReads accumulate and print as <out>.mapstats
 * (StatSingleReads: total, unique, ambiguous, unmapped, too_short, mapping.hpp:94-100, updated at
 * mapping.cpp:318-327,504; StatPairedReads: 4 pair counters + one StatSingleReads per mate +
 * fragment_len_count[frag_range + 1], paired.hpp:96-105, updated at paired.cpp:519-547).  Reads shard
 * over the ranks in contiguous blocks, every rank holds an index replica, and at the end of the run
 * each rank hands its block to walt_stats_allreduce: ONE sum over RCCL (ncclAllReduce, uint64).
 *
 * walt_comm_unique_id: rank 0 makes the 128-byte id (ncclGetUniqueId) and the caller distributes it out
 * of band (a file, MPI, torch.distributed ...).  walt_comm_init: every rank joins with the same id
 * (ncclCommInitRank; collective, blocks until all ranks have called).  walt_stats_allreduce sums v[0..n)
 * over the ranks in place (host vector; collective, same n on every rank); with comm == NULL it is
 * the identity, which is what a single process needs.  bin/walt, one process driving several GPUs,
 * adds its per-device blocks on the host instead.
 * walt_comm_available: WALT_OK when librccl could be loaded in this process (no communication) -- a job can
 * agree on that BEFORE any rank enters the blocking calls (walt_comm_init and walt_stats_allreduce have no
 * timeout: a rank that never arrives leaves its peers waiting, as with ncclCommInitRank / ncclAllReduce
 * themselves). */
#define WALT_COMM_ID_BYTES 128
typedef struct walt_comm walt_comm;
int walt_comm_available(void);
int walt_comm_unique_id(void* id_out /* WALT_COMM_ID_BYTES */);
int walt_comm_init(int device, int rank, int world, const void* id, walt_comm** out);
int walt_stats_allreduce(walt_comm* comm, uint64_t* v, size_t n);
int walt_comm_rank(const walt_comm* comm);
int walt_comm_world(const walt_comm* comm);
void walt_comm_close(walt_comm* comm);

/* ---- measurement hooks (bench.py) ---------------------------------------- */

/* When enabled, the *_device batch calls record HIP events on their stream
 * around the read-packing and the mapping kernels; walt_profile_last waits for
 * the last call's events and returns the two durations in milliseconds. */
int walt_profile_enable(walt_index* idx, int on);
int walt_profile_last(walt_index* idx, float* pack_ms, float* map_ms);
/* The last single-end call's mapping time by kernel group, from events between the groups: out4 = milliseconds of
 * {pass 1, heavy stages, region verifier, literal pass incl. its sort}. */
int walt_profile_detail(walt_index* idx, float* out4);
/* Diagnostic BUILD only (make -C walt_amd/csrc diag: libwalt_amd_diag.so, environment WALT_AMD_STAMPS=1):
 * in-kernel s_memtime sums per phase of the single-end mapping kernel, cycles summed over waves; reading
 * clears them.  The product library returns WALT_EINVAL. */
int walt_profile_stamps(unsigned long long* out16);

#ifdef __cplusplus
}
#endif
#endif /* WALT_AMD_H_ */
