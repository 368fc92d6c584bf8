// walt_main.cpp -- host driver with WALT's command-line surface on top of the
// C ABI (include/walt_amd.h).  It restates, in its own code, the parts of the
// reference that sit AROUND the hot path so that a user can swap binaries:
//   option table ............ walt.cpp:130-166 (single-dash long names)
//   FASTQ batch loader ...... mapping.cpp:65-121 (srand(0) per batch, N -> rand()%4)   [hostio.h]
//   adaptor clipping -C ..... util.hpp:189-233                                          [hostio.h]
//   SAM / MR / mapstats ..... mapping.cpp:47-63,329-419; paired.cpp:52-77,210-294,333-435,515-569
// The mapping itself (mapping.cpp:486-500, paired.cpp:642-699) is one library call
// per batch.  Ingest and output formatting run on -t host threads (default: all),
// each thread owning a contiguous range of the batch, so the files come out in
// read order and byte-identical to the reference binary's
// (tests/test_gpu_cli.py compares against the golden files).
// process_se and process_pe hold what differs between the modes (loading, the mapping call, formatting, .mapstats);
// what the extensions share exists once: kOutput / Append (the side files), HandleSet (one handle per device),
// write_window_table (.methcounts / .allelic / .epialleles), Consumers (all that takes the methylation calls: open,
// start_batch, view + call_slot, finish), run_batch (a batch's schedule, -D included), reserve_records.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <exception>
#include <fstream>
#include <iostream>
#include <map>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <unistd.h>
#include <vector>

#include "../../../include/walt_amd.h"
#include "hostio.h"
#include "../sitecall_core.h"

using std::string;
using std::vector;
using hostio::Batch;
using hostio::OutFile;
using hostio::Sink;
using hostio::View;

static const uint32_t MAX_LINE_LENGTH = 1000;  // util.hpp:43
#define MINIMALREADLEN walt_min_read_len()       // seedpattern.hpp:359 / 230 / 33 (38 / 32 / 23 by seed pattern)

static void die(const string& msg) { throw std::runtime_error(msg); }
static void check(int rc) { if (rc != WALT_OK) die(walt_last_error()); }

// ---------------------------------------------------------------- options
struct Options {
  string index_file, se_csv, pe1_csv, pe2_csv, out_csv, adaptor;
  bool sam = false, ambiguous = false, unmapped = false, ag = false, verbose = false, pbat = false;
  bool rpbat = false;  // -R: single-end random PBAT, every read under both conversions (walt_map_se_rpbat_batch)
  bool rpbat_pe = false;  // -RP: paired-end random PBAT, every pair in both orientations (walt_map_pe_rpbat_batch)
  bool meth = false;  // -M: per-read methylation calls (walt_meth_call_batch): XM:Z: on SAM lines, <out>.methstats
  bool methcounts = false;  // -MC: per-cytosine pile-up on the device (walt_meth_pileup_batch): <out>.methcounts
  bool levels = false;  // -ML: genome-wide methylation levels of the pile-up (walt_pileup_levels): <out>.levels
  string regions_file;  // -MR: methylation levels per region of a BED file (walt_pileup_regions): <out>.regions
  bool regions() const { return !regions_file.empty(); }
  bool piling() const { return methcounts || levels || regions() || variants || sites; }  // the run keeps pile-ups
  bool consumer() const { return meth || methcounts || mbias || levels || regions() || allelic || epialleles || variants || sites; }  // something takes the methylation calls
  bool dedup = false;  // -D: PCR duplicates marked on the device (walt_dedup_*) and kept out of -M / -MC: <out>.dupstats
  bool no_overlap = false;  // -NO: a base both mates of a unique proper pair cover is called once, for mate 1 (walt_pair_overlap_batch)
  bool mbias = false;  // -MB: methylation bias by read position (walt_meth_pileup_batch_mbias): <out>.mbias
  bool allelic = false;  // -MA: adjacent-CpG state pairs per read (walt_meth_pileup_batch_pairs): <out>.allelic
  bool epialleles = false;  // -ME: four-CpG epiallele patterns per read (walt_meth_pileup_batch_epi): <out>.epialleles
  uint32_t epi_min = 1;     // -MEN: the fewest reads of a window that is written
  bool epi_min_given = false;
  // -MV: opposite-strand evidence beside the pile-up (walt_meth_pileup_batch_ev); the flagged positions go to <out>.variants,
  // the totals to <out>.variantstats, and their counters are zeroed before .methcounts, .levels and .regions are written
  bool variants = false;
  uint32_t variant_depth = 5, variant_percent = 50;  // -MVD, -MVP: min_depth and max_percent of the rule
  bool variant_depth_given = false, variant_percent_given = false;
  // -MS: methylated sites called at the end of a read file (walt_pileup_depth_hist, walt_pileup_call_sites): a binomial test
  // per site against the non-conversion rate and Benjamini-Hochberg per context: <out>.methsites, <out>.sitestats.
  // -MSN: the control sequence the rate is taken from (left out of the test); -MSR: the rate itself; -MSA: the FDR;
  // -MSD: the minimum depth of a tested site
  bool sites = false;
  string site_control;
  double site_rate = 0.0, site_alpha = 0.01;
  uint32_t site_depth = 1;
  bool site_control_given = false, site_rate_given = false, site_alpha_given = false, site_depth_given = false;
  // -MQ, -MQO: a read base whose Phred quality is below min_qual gets no methylation call and gives no opposite-strand
  // evidence (walt_meth_pileup_batch_qual, walt_meth_nonconv_batch_qual); qual_offset: the FASTQ's Phred offset.  0: no floor
  uint32_t min_qual = 0, qual_offset = 33;
  bool qual_offset_given = false;
  uint32_t qual_floor() const { return min_qual ? min_qual + qual_offset : 0u; }  // what the raw bytes are compared with
  // -I5 -I3 -I5R2 -I3R2: the first / last bases of a read that get no methylation call (walt_meth_pileup_batch_trim), of
  // the reads of -r or -1 ([0], [1]) and of the reads of -2 ([2], [3]); the user's order, also under -P and -RP
  uint32_t ignore[4] = {0, 0, 0, 0};
  bool ignore_given[4] = {false, false, false, false};
  bool ignoring() const { return ignore[0] || ignore[1] || ignore[2] || ignore[3]; }
  // -F -FC -FP -FM: reads whose non-CpG calls say that bisulfite did not convert them (walt_meth_nonconv_batch) are kept out
  // of the methylation counts: min_meth, min_run, min_percent, min_total of the rule; [3] is accepted only beside [2]
  uint32_t filter[4] = {0, 0, 0, 0};
  bool filter_given[4] = {false, false, false, false};
  bool filtering() const { return filter_given[0] || filter_given[1] || filter_given[2]; }
  uint32_t max_mismatches = 6, batch_size = 10000000, b = 5000, top_k = 50;
  int frag_range = 1000, threads = 0;
  std::vector<int> devices;  // -g 0,1,...: every listed GPU holds an index replica and maps a contiguous share of each batch
  std::vector<std::pair<string, long long>> tune;  // -X name=value: walt_index_set_option on every replica (schedule only, never results)
};

static bool is_opt(const string& a, const char* s, const char* l) { return a == string("-") + s || a == string("-") + l || a == string("--") + l; }

static vector<string> split_csv(const string& s) {
  vector<string> out;
  std::istringstream is(s);
  string tok;
  while (std::getline(is, tok, ',')) if (!tok.empty()) out.push_back(tok);
  return out;
}
static Options parse(int argc, const char** argv) {
  Options o;
  for (int i = 1; i < argc; ++i) {
    string a = argv[i];
    auto val = [&]() -> string {
      if (i + 1 >= argc) die("missing value for " + a);
      return argv[++i];
    };
    if (is_opt(a, "i", "index")) o.index_file = val();
    else if (is_opt(a, "r", "reads")) o.se_csv = val();
    else if (is_opt(a, "1", "reads1")) o.pe1_csv = val();
    else if (is_opt(a, "2", "reads2")) o.pe2_csv = val();
    else if (is_opt(a, "o", "output")) o.out_csv = val();
    else if (is_opt(a, "m", "mismatch")) o.max_mismatches = (uint32_t)strtoul(val().c_str(), 0, 10);
    else if (is_opt(a, "N", "number")) o.batch_size = (uint32_t)strtoul(val().c_str(), 0, 10);
    else if (is_opt(a, "a", "ambiguous")) o.ambiguous = true;
    else if (is_opt(a, "u", "unmapped")) o.unmapped = true;
    else if (is_opt(a, "C", "clip")) o.adaptor = val();
    else if (is_opt(a, "A", "ag-wild")) o.ag = true;
    else if (is_opt(a, "P", "pbat")) o.pbat = true;  // README.md:64,100-104; no code in the reference snapshot
    else if (is_opt(a, "R", "random-pbat")) o.rpbat = true;  // extension: reads of either conversion (abismal's -R)
    else if (is_opt(a, "RP", "random-pbat-pe")) o.rpbat_pe = true;  // extension: pairs of either orientation
    else if (is_opt(a, "M", "meth") || a == "--meth-calls") o.meth = true;  // extension: methylation calls per read
    else if (is_opt(a, "MC", "methcounts") || a == "--meth-counts") o.methcounts = true;  // extension: methylation counts per cytosine
    else if (is_opt(a, "ML", "levels") || a == "--meth-levels") o.levels = true;  // extension: genome-wide methylation levels
    else if (is_opt(a, "MR", "regions") || a == "--meth-regions") {  // extension: methylation levels per region of a BED file
      o.regions_file = val();
      if (o.regions_file.empty()) die(a + " (methylation levels per region) wants the name of a BED file");
    }
    else if (is_opt(a, "D", "dedup") || a == "--remove-duplicates") o.dedup = true;  // extension: mark PCR duplicates
    else if (is_opt(a, "NO", "no-overlap")) o.no_overlap = true;  // extension: the overlap of a pair counted once
    else if (is_opt(a, "MB", "mbias") || a == "--m-bias") o.mbias = true;  // extension: methylation bias by read position
    else if (is_opt(a, "MA", "allelic") || a == "--allelic-meth") o.allelic = true;  // extension: adjacent-CpG state pairs per read
    else if (is_opt(a, "ME", "epialleles")) o.epialleles = true;  // extension: four-CpG epiallele patterns per read
    else if (is_opt(a, "MEN", "epiallele-min") || a == "--epiallele-min-reads") {  // extension: the fewest reads of a written window
      const string v = val();
      if (!hostio::parse_epiallele_min(v, o.epi_min))
        die(a + " (epialleles) wants a number of reads from 1 to 1000000, not \"" + v + "\"");
      o.epi_min_given = true;
    }
    else if (is_opt(a, "MV", "variants") || a == "--mask-variants") o.variants = true;  // extension: C>T variant sites kept out of the counts
    else if (is_opt(a, "MVD", "variant-min-depth")) {  // extension: the fewest opposite-strand reads a position is judged by
      const string v = val();
      if (!hostio::parse_variant_value(v, 1, hostio::kMaxVariantDepth, o.variant_depth))
        die(a + " (variant sites) wants a number of reads from 1 to 1000000, not \"" + v + "\"");
      o.variant_depth_given = true;
    }
    else if (is_opt(a, "MVP", "variant-max-percent")) {  // extension: the percentage of other bases a position may show
      const string v = val();
      if (!hostio::parse_variant_value(v, 0, 99, o.variant_percent))
        die(a + " (variant sites) wants a percentage from 0 to 99, not \"" + v + "\"");
      o.variant_percent_given = true;
    }
    else if (is_opt(a, "MS", "sites") || a == "--call-sites") o.sites = true;  // extension: methylated sites by binomial test and FDR
    else if (is_opt(a, "MSN", "sites-control")) {  // extension: the unmethylated control sequence
      o.site_control = val();
      if (o.site_control.empty()) die(a + " (called sites) wants the name of a sequence of the index");
      o.site_control_given = true;
    }
    else if (is_opt(a, "MSR", "sites-rate")) {  // extension: the non-conversion rate, given
      const string v = val();
      if (!hostio::parse_site_fraction(v, true, o.site_rate))
        die(a + " (called sites) wants a non-conversion rate r with 0 <= r < 1, not \"" + v + "\"");
      o.site_rate_given = true;
    }
    else if (is_opt(a, "MSA", "sites-alpha")) {  // extension: the false discovery rate
      const string v = val();
      if (!hostio::parse_site_fraction(v, false, o.site_alpha))
        die(a + " (called sites) wants a false discovery rate a with 0 < a < 1, not \"" + v + "\"");
      o.site_alpha_given = true;
    }
    else if (is_opt(a, "MSD", "sites-min-depth")) {  // extension: the minimum depth of a tested site
      const string v = val();
      if (!hostio::parse_site_depth(v, o.site_depth))
        die(a + " (called sites) wants a depth from 1 to 127, not \"" + v + "\"");
      o.site_depth_given = true;
    }
    else if (is_opt(a, "MQ", "min-qual") || a == "--min-base-quality") {  // extension: a quality floor under the methylation calls
      const string v = val();
      if (!hostio::parse_min_qual(v, o.min_qual))
        die(a + " (minimum base quality) wants a Phred quality from 1 to 93, not \"" + v + "\"");
    }
    else if (is_opt(a, "MQO", "qual-offset") || a == "--quality-offset") {  // extension: the FASTQ's Phred offset
      const string v = val();
      if (!hostio::parse_qual_offset(v, o.qual_offset))
        die(a + " (the FASTQ's Phred offset) wants 33 or 64, not \"" + v + "\"");
      o.qual_offset_given = true;
    }
    else if (is_opt(a, "I5", "ignore") || is_opt(a, "I3", "ignore-3prime") || is_opt(a, "I5R2", "ignore-r2") ||
             is_opt(a, "I3R2", "ignore-3prime-r2")) {  // extension: read ends kept out of the methylation calls
      const int k = is_opt(a, "I5", "ignore") ? 0 : is_opt(a, "I3", "ignore-3prime") ? 1 : is_opt(a, "I5R2", "ignore-r2") ? 2 : 3;
      const string v = val();
      if (!hostio::parse_ignore_value(v, o.ignore[k]))
        die(a + " (ignored read ends) wants a number of bases from 0 to 1024, not \"" + v + "\"");
      o.ignore_given[k] = true;
    }
    else if (is_opt(a, "F", "filter-nonconv") || a == "--filter-non-conversion" || is_opt(a, "FC", "filter-consecutive") ||
             is_opt(a, "FP", "filter-percent") || is_opt(a, "FM", "filter-min-count")) {  // extension: non-converted reads
      const int k = is_opt(a, "FC", "filter-consecutive") ? 1 : is_opt(a, "FP", "filter-percent") ? 2 : is_opt(a, "FM", "filter-min-count") ? 3 : 0;
      const uint32_t hi = k == 2 ? 100 : 1024;
      const string v = val();
      if (!hostio::parse_filter_value(v, 1, hi, o.filter[k]))
        die(a + " (non-converted reads) wants a number from 1 to " + std::to_string(hi) + ", not \"" + v + "\"");
      o.filter_given[k] = true;
    }
    else if (is_opt(a, "b", "bucket")) o.b = (uint32_t)strtoul(val().c_str(), 0, 10);
    else if (is_opt(a, "k", "topk")) o.top_k = (uint32_t)strtoul(val().c_str(), 0, 10);
    else if (is_opt(a, "L", "fraglen")) o.frag_range = atoi(val().c_str());
    else if (a == "-sam" || a == "--sam") o.sam = true;
    else if (is_opt(a, "v", "verbose")) o.verbose = true;
    else if (is_opt(a, "t", "thread")) o.threads = atoi(val().c_str());
    else if (is_opt(a, "g", "gpu")) {  // extension: device ordinal(s), comma separated
      o.devices.clear();
      for (const string& t : split_csv(val())) o.devices.push_back(atoi(t.c_str()));
    }
    else if (a == "-X") {  // extension: an option of the mapping library (include/walt_amd.h, walt_index_set_option)
      const string kv = val();
      const size_t eq = kv.find('=');
      if (eq == string::npos || eq == 0) die("-X wants name=value");
      o.tune.emplace_back(kv.substr(0, eq), atoll(kv.c_str() + eq + 1));
    }
    else die("unknown option " + a);
  }
  if (o.index_file.empty() || o.out_csv.empty()) die("options -i and -o are required");
  if (o.devices.empty()) o.devices.push_back(0);
  if (o.rpbat_pe && o.rpbat) die("-RP (paired-end random PBAT) cannot be combined with -R (single-end random PBAT)");
  if (o.rpbat_pe && !o.se_csv.empty()) die("-RP (random PBAT) is paired-end only: it cannot be combined with -r (use -R)");
  if (o.rpbat_pe && o.ag) die("-RP (random PBAT) maps every pair in both orientations: it cannot be combined with -A");
  if (o.rpbat_pe && o.pbat) die("-RP (random PBAT) maps every pair in both orientations: it cannot be combined with -P");
  if (o.rpbat && o.ag) die("-R (random PBAT) maps every read under both conversions: it cannot be combined with -A");
  if (o.rpbat && o.pbat) die("-R (random PBAT) cannot be combined with -P");
  if (o.rpbat && (!o.pe1_csv.empty() || !o.pe2_csv.empty())) die("-R (random PBAT) is single-end only: it cannot be combined with -1 / -2 (use -RP)");
  if (o.dedup && o.frag_range >= (1 << 27))
    die("-D (duplicates) keys a pair by its fragment length in 28 bits: it cannot be combined with -L of 134217728 (2^27) or more");
  if (o.no_overlap && !o.se_csv.empty())
    die("-NO (no overlap) is about the two mates of a pair: it is paired-end only and cannot be combined with -r");
  if (o.no_overlap && !o.consumer())
    die("-NO (no overlap) changes methylation calls only: without -M or -MC (or -MB, -ML, -MR, -MA, -ME, -MV) there is nothing for it to do");
  if ((o.ignore_given[0] || o.ignore_given[1] || o.ignore_given[2] || o.ignore_given[3]) && !o.consumer())
    die("-I5 / -I3 / -I5R2 / -I3R2 (ignored read ends) change methylation calls only: without -M, -MC, -MB, -ML, -MR, -MA, -ME or -MV there is nothing for them to do");
  if ((o.ignore_given[2] || o.ignore_given[3]) && !o.se_csv.empty())
    die("-I5R2 / -I3R2 (ignored read ends of mate 2) are about the reads of -2: they cannot be combined with -r (use -I5 / -I3)");
  if (o.filter_given[3] && !o.filter_given[2])
    die("-FM (the fewest non-CpG calls a read is judged by its percentage with) goes with -FP: without it there is nothing for it to do");
  if ((o.filtering() || o.filter_given[3]) && !o.consumer())
    die("-F / -FC / -FP / -FM (non-converted reads) change methylation calls only: without -M, -MC, -MB, -ML, -MR, -MA, -ME or -MV there is nothing for them to do");
  if (o.epi_min_given && !o.epialleles)
    die("-MEN (the fewest reads of a written window) goes with -ME: without it there is nothing for it to do");
  if ((o.variant_depth_given || o.variant_percent_given) && !o.variants)
    die("-MVD / -MVP (the rule that flags a variant site) go with -MV: without it there is nothing for them to do");
  if ((o.site_control_given || o.site_rate_given || o.site_alpha_given || o.site_depth_given) && !o.sites)
    die("-MSN / -MSR / -MSA / -MSD (the control, the rate, the FDR and the minimum depth of called sites) go with -MS: without it there is nothing for them to do");
  if (o.sites && o.site_control_given == o.site_rate_given)
    die(o.site_control_given ? "-MS (called sites) takes its non-conversion rate from -MSN (a control sequence) or from -MSR (the rate itself), not from both"
                             : "-MS (called sites) wants the non-conversion rate: -MSN <name> (an unmethylated control sequence of the index) or -MSR <r>");
  if (o.qual_offset_given && !o.min_qual)
    die("-MQO (the FASTQ's Phred offset) goes with -MQ: without it there is nothing for it to do");
  if (o.min_qual && !o.consumer())
    die("-MQ (minimum base quality) changes methylation calls only: without -M, -MC, -MB, -ML, -MR, -MA, -ME or -MV there is nothing for it to do");
  uint32_t floor = 0;
  if (o.min_qual && !hostio::quality_floor(o.min_qual, o.qual_offset, floor))
    die("-MQ " + std::to_string(o.min_qual) + " with -MQO " + std::to_string(o.qual_offset) + ": a quality byte of " +
        std::to_string(floor) + " does not exist (the sum must not exceed 127)");
  if (o.filter_given[2] && !o.filter_given[3]) o.filter[3] = 5;  // (Bismark's --minimum_count)
  if (o.pbat && !o.se_csv.empty()) o.ag = true;  // single-end PBAT reads are A-rich: same as -A
  return o;
}

static bool valid_suffix(const string& fn) {  // walt.cpp:58-64 (checks .fastq / .fq)
  auto ends = [&](const string& sfx) { return fn.size() >= sfx.size() && fn.compare(fn.size() - sfx.size(), sfx.size(), sfx) == 0; };
  return ends(".fastq") || ends(".fq");
}
static bool exists(const string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }

// -C "T_adaptor[:A_adaptor]" (walt.cpp:150-152): one adaptor serves both mates, two are split at the colon
struct AdaptorPair {
  string mate1, mate2;
};
static AdaptorPair split_adaptor_option(const string& opt) {
  const size_t colons = (size_t)std::count(opt.begin(), opt.end(), ':');
  if (colons > 1) die("ERROR: adaptor format \"T_adaptor[:A_adaptor]\"");
  AdaptorPair ap;
  const size_t cut = colons ? opt.find(':') : opt.size();
  ap.mate1 = opt.substr(0, cut);
  ap.mate2 = colons ? opt.substr(cut + 1) : ap.mate1;
  return ap;
}

// ---------------------------------------------------------------- genome info + helpers
struct GenomeInfo {
  vector<string> name;
  vector<uint32_t> length, start;
};
static GenomeInfo genome_of(const walt_index* idx) {
  GenomeInfo g;
  uint32_t n = walt_index_n_chrom(idx);
  g.start.assign(n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    g.name.push_back(walt_index_chrom_name(idx, i));
    g.length.push_back(walt_index_chrom_len(idx, i));
    g.start[i + 1] = g.start[i] + g.length[i];
  }
  return g;
}
static uint32_t chrom_id(const GenomeInfo& g, uint32_t pos) {  // getChromID, reference.cpp:43-60
  uint32_t l = 0, h = (uint32_t)g.start.size() - 1;
  while (l < h) {
    uint32_t m = (l + h + 1) / 2;
    if (pos >= g.start[m]) l = m; else h = m - 1;
  }
  return l;
}
static string sam_head(const GenomeInfo& g) {  // SAMHead, reference.cpp:430-440
  std::ostringstream os;
  os << "@HD\tVN:1.0\n";
  for (size_t i = 0; i < g.name.size(); ++i) os << "@SQ\tSN:" << g.name[i] << "\tLN:" << g.length[i] << "\n";
  os << "@PG\tID:WALT\tVN:1.0\tCL:walt\n";
  return os.str();
}

// sinks of one host thread: main output, then the _ambiguous / _unmapped side files of mate 1 and mate 2
enum { kMain = 0, kAmb1 = 1, kUnm1 = 2, kAmb2 = 3, kUnm2 = 4, kSinks = 5 };

struct SeCounts {  // StatSingleReads, mapping.hpp:55-108
  uint32_t total = 0, unique = 0, ambiguous = 0, unmapped = 0, too_short = 0;
  void update(uint32_t times) {  // StatInfoUpdate, mapping.cpp:318-327
    ++total;
    if (times == 0) unmapped++; else if (times == 1) unique++; else ambiguous++;
  }
  void add(const SeCounts& o) {
    total += o.total; unique += o.unique; ambiguous += o.ambiguous; unmapped += o.unmapped; too_short += o.too_short;
  }
  // the block StatSingleReads prints into <out>.mapstats (mapping.cpp:47-63): `depth` levels of four spaces in front
  // of every line, no newline behind the last; percent_unique in the stream's default %g form (0 reads: "-nan")
  void put_block(Sink& f, int depth) const {
    auto line = [&](int extra, const char* key) {
      for (int i = 0; i < 4 * (depth + extra); ++i) f.ch(' ');
      f.lit(key);
    };
    char pct[40];
    snprintf(pct, sizeof pct, "%g", (100.0 * unique) / total);
    line(0, "total_reads: "); f.u32(total); f.ch('\n');
    line(0, "mapped:\n");
    line(1, "unique: "); f.u32(unique); f.ch('\n');
    line(1, "percent_unique: "); f.lit(pct); f.ch('\n');
    line(1, "ambiguous: "); f.u32(ambiguous); f.ch('\n');
    line(0, "unmapped: "); f.u32(unmapped); f.ch('\n');
    line(0, "min_read_length: "); f.u32(MINIMALREADLEN); f.ch('\n');
    line(0, "too_short: "); f.u32(too_short);
  }
};
struct SideFiles {  // the _ambiguous / _unmapped files of StatSingleReads (mapping.hpp:75-87)
  OutFile amb, unm;
  bool out_amb = false, out_unm = false;
  void open(bool a, bool u, const string& out, bool sam) {
    out_amb = a; out_unm = u;
    if (a && !sam && !amb.open_trunc(out + "_ambiguous")) die("cannot open input file " + out + "_ambiguous");
    if (u && !sam && !unm.open_trunc(out + "_unmapped")) die("cannot open input file " + out + "_unmapped");
  }
  void close() { amb.close(); unm.close(); }
};

// The files a run writes beside its main output, <out><suffix>: main truncates those whose option is on (walt.cpp:230-233
// for the first), and the end of every read file appends its block to each.
enum { kMapstats, kMethstats, kMethcounts, kLevels, kRegions, kMbias, kAllelic, kEpialleles, kDupstats, kFilterstats, kVariants, kVariantstats, kMethsites, kSitestats, kOutputs };
static const struct { bool (*on)(const Options&); const char* suffix; } kOutput[kOutputs] = {
    {[](const Options&) { return true; }, ".mapstats"},
    {[](const Options& o) { return o.meth; }, ".methstats"},
    {[](const Options& o) { return o.methcounts; }, ".methcounts"},
    {[](const Options& o) { return o.levels; }, ".levels"},
    {[](const Options& o) { return o.regions(); }, ".regions"},
    {[](const Options& o) { return o.mbias; }, ".mbias"},
    {[](const Options& o) { return o.allelic; }, ".allelic"},
    {[](const Options& o) { return o.epialleles; }, ".epialleles"},
    {[](const Options& o) { return o.dedup; }, ".dupstats"},
    {[](const Options& o) { return o.filtering(); }, ".filterstats"},
    {[](const Options& o) { return o.variants; }, ".variants"},
    {[](const Options& o) { return o.variants; }, ".variantstats"},
    {[](const Options& o) { return o.sites; }, ".methsites"},
    {[](const Options& o) { return o.sites; }, ".sitestats"},
};
struct Append {  // one of them, open for appending
  OutFile f;
  Append(const string& out_file, int which) {
    const string path = out_file + kOutput[which].suffix;
    if (!f.open_append(path)) die("cannot open input file " + path);
  }
  ~Append() { f.close(); }
  void write(const Sink& s) { if (s.n) f.write(s.p, s.n); }
};

// ---------------------------------------------------------------- single-end writers, mapping.cpp:329-419
static void out_mr_line(const walt_best_match& bm, View name, View seq, View score, bool flip, const GenomeInfo& g,
                        bool ag, Sink& f) {
  uint32_t chr = chrom_id(g, bm.genome_pos);
  uint32_t start = bm.genome_pos - g.start[chr];
  if (bm.strand == '-') start = g.length[chr] - start - seq.len;
  uint32_t end = start + seq.len;
  char strand = bm.strand;
  if (ag) strand = bm.strand == '+' ? '-' : '+';
  f.put(g.name[chr]); f.ch('\t'); f.u32(start); f.ch('\t'); f.u32(end); f.ch('\t'); f.put(name); f.ch('\t');
  f.u32(bm.mismatch); f.ch('\t'); f.ch(strand); f.ch('\t');
  if (flip) { f.revcomp(seq); f.ch('\t'); f.rev(score); } else { f.put(seq); f.ch('\t'); f.put(score); }
  f.ch('\n');
}
// OutputSingleResults, mapping.cpp:329-380: A-rich reads are printed reverse-complemented
static void out_single_results(const walt_best_match& bm, View name, View seq, View score, const GenomeInfo& g, bool ag,
                               bool out_amb, bool out_unm, Sink& fout, Sink& famb, Sink& funm) {
  if (bm.times == 0 && out_unm) {
    funm.put(name); funm.ch('\t');
    if (ag) { funm.revcomp(seq); funm.ch('\t'); funm.rev(score); } else { funm.put(seq); funm.ch('\t'); funm.put(score); }
    funm.ch('\n');
  } else if (bm.times == 1) {
    out_mr_line(bm, name, seq, score, ag, g, ag, fout);
  } else if (bm.times >= 2 && out_amb) {
    out_mr_line(bm, name, seq, score, ag, g, ag, famb);
  }
}
static void put_seq_qual(Sink& f, View seq, View score, bool flip) {
  if (flip) { f.revcomp(seq); f.ch('\t'); f.rev(score); } else { f.put(seq); f.ch('\t'); f.put(score); }
}
// OutputSingleSAM, mapping.cpp:382-419
// tag: appended to the main and -a lines (-R: "\tCV:A:T" / "\tCV:A:A", the conversion of the record), or null
// xm: the read's methylation calls (-M), appended as XM:Z: in the order of SEQ; xm.p null: none
static void put_xm(Sink& f, View xm, bool flip) {
  if (!xm.p) return;
  f.lit("\tXM:Z:");
  if (flip) f.rev(xm); else f.put(xm);
}
static void out_single_sam(const walt_best_match& bm, View name, View seq, View score, const GenomeInfo& g,
                           bool out_amb, bool out_unm, Sink& f, const char* tag = nullptr, View xm = View{nullptr, 0},
                           int flag_extra = 0 /* -D: 0x400 on a duplicate */) {
  uint32_t chr = chrom_id(g, bm.genome_pos);
  uint32_t start = bm.genome_pos - g.start[chr];
  if (bm.strand == '-') start = g.length[chr] - start - seq.len;
  const bool flip = bm.strand == '-';
  int flag = (bm.times == 0 ? 0x4 : 0) + (bm.strand == '-' ? 0x10 : 0) + (bm.times >= 2 ? 0x100 : 0) + flag_extra;
  if (bm.times == 0 && out_unm) {
    f.put(name); f.ch('\t'); f.i32(flag); f.lit("\t*\t0\t255\t*\t*\t0\t0\t");
    put_seq_qual(f, seq, score, flip);
    f.lit("\tNM:i:0\n");
  } else if (bm.times == 1 || (bm.times >= 2 && out_amb)) {
    f.put(name); f.ch('\t'); f.i32(flag); f.ch('\t'); f.put(g.name[chr]); f.ch('\t'); f.u32(start + 1);
    f.lit("\t255\t"); f.u32(seq.len); f.lit("M\t*\t0\t0\t");
    put_seq_qual(f, seq, score, flip);
    f.lit("\tNM:i:"); f.u32(bm.mismatch);
    if (tag) f.lit(tag);
    put_xm(f, xm, flip);
    f.ch('\n');
  }
}

// ---------------------------------------------------------------- -M: methylation calls
// <out>.methstats: the batch totals over the records with times == 1 (walt_meth_stats), one block per mate
static void put_meth_block(Sink& ms, const walt_meth_stats& st) {
  static const char* ctx[4] = {"CpG", "CHG", "CHH", "unknown"};
  char num[96];
  snprintf(num, sizeof num, "reads\t%llu\n", (unsigned long long)st.reads);
  ms.lit(num);
  for (int c = 0; c < 4; ++c) {
    const unsigned long long m = st.meth[c], u = st.unmeth[c];
    if (m + u) snprintf(num, sizeof num, "%s\t%llu\t%llu\t%.6f\n", ctx[c], m, u, (double)m / (double)(m + u));
    else snprintf(num, sizeof num, "%s\t%llu\t%llu\tNA\n", ctx[c], m, u);
    ms.lit(num);
  }
}
static void add_meth(walt_meth_stats& a, const walt_meth_stats& b) {
  a.reads += b.reads;
  for (int c = 0; c < 4; ++c) { a.meth[c] += b.meth[c]; a.unmeth[c] += b.unmeth[c]; }
}
// -C: where each read of the batch was clipped (the loader replaced the bases from there on by random ones)
static void clip_points(const Batch& b, const string& adaptor, int T, vector<uint32_t>& out) {
  out.resize(b.n);
  const View ad{adaptor.data(), (uint32_t)adaptor.size()};
#pragma omp parallel for schedule(static) num_threads(T)
  for (uint32_t j = 0; j < b.n; ++j)
    out[j] = hostio::adaptor_clip_point(View{b.base + (b.seq_v[j] >> 16), (uint32_t)(b.seq_v[j] & 0xFFFF)}, ad);
}

// ---------------------------------------------------------------- one handle per device of the run
// A pile-up (-MC -ML -MR), a bias set (-MB), a pair table (-MA) or a window table (-ME): a share's calls are counted on
// the device that made them, and the end of a read file adds the devices' counters up on the host.  The handles are
// destroyed before their indexes are closed (Consumers::finish; when an error unwinds, the destructor).
template <class H, void (*Destroy)(H*)>
struct HandleSet {
  vector<H*> p;
  HandleSet() {}
  HandleSet(const HandleSet&) = delete;
  HandleSet& operator=(const HandleSet&) = delete;
  ~HandleSet() { close(); }
  template <class Create>  // create(d, &handle) -> status
  void open(size_t n_devices, Create create) {
    p.assign(n_devices, nullptr);
    for (size_t d = 0; d < n_devices; ++d)
      if (create(d, &p[d]) != WALT_OK) { const string e = walt_last_error(); close(); die(e); }
  }
  void close() {
    for (H* q : p) if (q) Destroy(q);
    p.clear();
  }
  bool on() const { return !p.empty(); }
  H* of(size_t d) const { return on() ? p[d] : nullptr; }
};
typedef HandleSet<walt_pileup, walt_pileup_destroy> PileUps;
typedef HandleSet<walt_mbias, walt_mbias_destroy> MbiasSet;  // one table per mate: table k takes slot k
typedef HandleSet<walt_cpgpairs, walt_cpgpairs_destroy> PairTables;
typedef HandleSet<walt_epialleles, walt_epialleles_destroy> WindowTables;

// ---------------------------------------------------------------- -MC -MA -ME: tables written by forward position
// At the end of a read file a table is written window by window of forward positions (a bounded buffer: capacity() says
// how many entries a window can hold), the windows of several devices merged by position with their counters added.
// A Table supplies its file and window (kOut, kWindow), the record of its extraction and the row the host merges (Site,
// Row; row() where the row's counters are wider), extract(), how two rows of a position add(), whether a merged row is
// written (keep(), which also tallies), its line() and its -v line (report()).
static const uint32_t kCountsWindow = 1u << 22;  // positions per extraction (64 MB of records at most)
template <class F>  // fn(lo, hi) for every window of the genome
static void for_each_window(uint64_t genome_len, uint64_t window, F fn) {
  for (uint64_t lo = 0; lo < genome_len; lo += window) fn((uint32_t)lo, (uint32_t)std::min<uint64_t>(lo + window, genome_len));
}
template <class Table, class Handles>
static void write_window_table(Table& t, const Handles& set, const string& out_file, const GenomeInfo& g, bool verbose) {
  Append mf(out_file, Table::kOut);
  const uint64_t genome_len = g.start.back();
  const uint64_t window = std::min<uint64_t>(Table::kWindow, genome_len);
  const uint64_t cap = Table::capacity(window);
  typedef typename Table::Site Site;
  typedef typename Table::Row Row;
  vector<Site> buf((size_t)cap);  // allocated once
  vector<Row> rows, add, other;
  uint64_t n_total = 0;
  uint32_t chr = 0;
  Sink out;
  for_each_window(genome_len, window, [&](uint32_t lo, uint32_t hi) {
    const Row* cur = nullptr;  // the window's rows: one device's as extracted, several devices' merged
    size_t n_cur = 0;
    for (size_t d = 0; d < set.p.size(); ++d) {
      uint64_t n = 0;
      check(t.extract(set.p[d], lo, hi, buf.data(), cap, &n));
      const Row* src;
      if constexpr (std::is_same<Site, Row>::value) {
        src = buf.data();  // a site is a row: nothing to copy
      } else {
        add.resize((size_t)n);
        for (uint64_t i = 0; i < n; ++i) add[i] = Table::row(buf[i]);
        src = add.data();
      }
      if (set.p.size() == 1) { cur = src; n_cur = (size_t)n; break; }
      if (d == 0) rows.clear();
      hostio::merge_rows(rows, src, (size_t)n, other, Table::add);
      cur = rows.data(); n_cur = rows.size();
    }
    out.clear();
    for (size_t k = 0; k < n_cur; ++k) {
      const Row& r = cur[k];
      if (!t.keep(r)) continue;
      while (r.pos >= g.start[chr + 1]) ++chr;  // (ascending positions; an entry lies inside one chromosome)
      t.line(out, g.name[chr], g.start[chr], r);
      ++n_total;
    }
    mf.write(out);
  });
  if (verbose) t.report(n_total);
}

// -MC: the per-cytosine pile-up; a window holds at most as many sites as positions
struct SiteTable {
  typedef walt_meth_site Site;
  typedef walt_meth_site Row;
  static constexpr int kOut = kMethcounts;
  static constexpr uint32_t kWindow = kCountsWindow;
  uint64_t off[2];
  static uint64_t capacity(uint64_t window) { return window; }
  int extract(walt_pileup* p, uint32_t lo, uint32_t hi, Site* buf, uint64_t cap, uint64_t* n) {
    uint64_t o2[2] = {0, 0};
    const int rc = walt_pileup_extract(p, lo, hi, buf, cap, n, o2);
    off[0] += o2[0]; off[1] += o2[1];
    return rc;
  }
  static void add(Row& r, const Row& o) { hostio::add_site_row(r, o); }
  bool keep(const Row&) { return true; }
  void line(Sink& out, const string& chrom, uint32_t chrom_start, const Row& s) {
    static const char* ctx[4] = {"CpG", "CHG", "CHH", "unknown"};
    out.put(chrom); out.ch('\t'); out.u32(s.pos - chrom_start); out.ch('\t'); out.ch((char)s.strand); out.ch('\t');
    out.lit(ctx[s.context & 3]); out.ch('\t'); out.u32(s.meth); out.ch('\t'); out.u32(s.unmeth); out.ch('\n');
  }
  void report(uint64_t n_rows) {
    fprintf(stderr, "[walt_amd methcounts: %llu sites; off-reference calls (on an A or T of the reference): %llu methylated, %llu unmethylated]\n",
            (unsigned long long)n_rows, (unsigned long long)off[0], (unsigned long long)off[1]);
  }
};

// ---------------------------------------------------------------- -ML: genome-wide methylation levels
// Maxima and covered sites are not additive across devices: the other devices' counters are folded into the first
// device's pile-up, window by window (once per read file, shared with -MR), and one summary runs there over the whole
// genome.
static void fold_pileups(PileUps& ps, uint64_t genome_len) {
  if (ps.p.size() < 2) return;
  const uint64_t window = std::min<uint64_t>(kCountsWindow, genome_len);
  vector<uint32_t> m((size_t)window), u((size_t)window);
  for (size_t d = 1; d < ps.p.size(); ++d)
    for_each_window(genome_len, window, [&](uint32_t lo, uint32_t hi) {
      check(walt_pileup_read(ps.p[d], lo, hi, m.data(), u.data()));
      check(walt_pileup_add(ps.p[0], lo, hi, m.data(), u.data()));
    });
}
// (the counters are folded by now)
static void write_levels(const string& out_file, PileUps& ps, const GenomeInfo& g, bool verbose) {
  walt_levels lv;
  check(walt_pileup_levels(ps.p[0], 0, (uint32_t)g.start.back(), &lv));
  Sink out;
  hostio::put_levels_block(out, lv);
  Append(out_file, kLevels).write(out);
  if (verbose) fwrite(out.p, 1, out.n, stderr);
}

// ---------------------------------------------------------------- -MR: methylation levels per region
// The BED file is read once, before anything is opened; its regions become forward ranges with the first index that is
// opened (every read file maps against the same one).  At the end of a read file one call on the first device's
// folded pile-up gives every region's record, and one block goes to <out>.regions.
struct RegionSet {
  string file;
  vector<hostio::BedRegion> bed;
  vector<walt_region> regions;
  bool resolved = false;
  void read(const string& f) {
    file = f;
    string err;
    if (!hostio::read_bed_file(f, bed, err)) die("-MR (methylation levels per region): " + err);
  }
  void resolve(const GenomeInfo& g, bool verbose) {
    if (resolved) return;
    string err;
    uint64_t n_unknown = 0;
    if (!hostio::resolve_bed(bed, g.name, g.start, file, regions, n_unknown, err)) die("-MR (methylation levels per region): " + err);
    resolved = true;
    if (verbose)
      fprintf(stderr, "[walt_amd regions: %zu regions of %s, %llu on chromosomes the index does not have]\n", bed.size(), file.c_str(),
              (unsigned long long)n_unknown);
  }
};
static RegionSet g_regions;
static void write_regions(const string& out_file, PileUps& ps) {
  vector<walt_region_levels> lv(g_regions.regions.size());
  check(walt_pileup_regions(ps.p[0], g_regions.regions.data(), g_regions.regions.size(), lv.data()));
  Sink out;
  hostio::put_regions_block(out, g_regions.bed, lv.data());
  Append(out_file, kRegions).write(out);
}

// ---------------------------------------------------------------- -MV: C>T variant sites kept out of the counts
// Whether a position is flagged depends on all of its evidence: the other devices' counters and evidence are folded into
// the first device's (fold_pileups, as -ML does), and everything that follows reads the first device alone.  The flagged
// positions go to <out>.variants window by window, in genome order; then one masking pass, and its totals to
// <out>.variantstats.
static void write_variants(const Options& o, const string& out_file, walt_pileup* p, walt_pileup* ev, const GenomeInfo& g) {
  const uint64_t genome_len = g.start.back();
  const uint64_t window = std::min<uint64_t>(kCountsWindow, genome_len);
  vector<walt_variant_site> buf((size_t)window);
  {
    Append vf(out_file, kVariants);
    uint32_t chr = 0;
    Sink out;
    for_each_window(genome_len, window, [&](uint32_t lo, uint32_t hi) {
      uint64_t n = 0;
      check(walt_pileup_variants(p, ev, lo, hi, o.variant_depth, o.variant_percent, buf.data(), window, &n));
      out.clear();
      for (uint64_t k = 0; k < n; ++k) {
        while (buf[k].pos >= g.start[chr + 1]) ++chr;  // (ascending positions)
        hostio::put_variant_line(out, g.name[chr], g.start[chr], buf[k]);
      }
      vf.write(out);
    });
  }
  uint64_t tot[5] = {0, 0, 0, 0, 0};
  check(walt_pileup_mask_variants(p, ev, 0, (uint32_t)genome_len, o.variant_depth, o.variant_percent, tot));
  Sink block;
  hostio::put_variant_block(block, tot, o.variant_depth, o.variant_percent);
  Append(out_file, kVariantstats).write(block);
  if (o.verbose) fwrite(block.p, 1, block.n, stderr);
}

// ---------------------------------------------------------------- -MS: methylated sites by binomial test and FDR
// The p-value of a site depends on its context, depth and meth alone: the device gives the joint histogram of the sites
// outside the control and the deep sites one by one, the host tests every occupied bin once (sitecall_core.h) and turns
// each context's cutoff into the table the extraction takes as its predicate.  Everything reads the first device's folded
// counters.
static uint32_t site_control_of(const Options& o, const GenomeInfo& g) {  // the control's sequence, refused before a read is mapped
  for (size_t i = 0; i < g.name.size(); ++i)
    if (g.name[i] == o.site_control) return (uint32_t)i;
  die("-MSN (called sites): the index has no sequence named \"" + o.site_control + "\"");
  return 0;
}
static void write_sites(const Options& o, const string& out_file, walt_pileup* p, const GenomeInfo& g) {
  using walt::kSiteBins;
  const uint32_t genome_len = g.start.back();
  // the control's range [c_lo, c_hi) (empty under -MSR) and its counts
  uint32_t c_lo = 0, c_hi = 0;
  uint64_t counts[2] = {0, 0};
  double rate = o.site_rate;
  bool has_rate = true;
  if (o.site_control_given) {
    const uint32_t c = site_control_of(o, g);
    c_lo = g.start[c]; c_hi = g.start[c + 1];
    walt_levels lv;
    check(walt_pileup_levels(p, c_lo, c_hi, &lv));
    for (int r = 0; r < 4; ++r) { counts[0] += lv.row[r].meth; counts[1] += lv.row[r].unmeth; }
    has_rate = counts[0] + counts[1] != 0;
    rate = has_rate ? (double)counts[0] / ((double)counts[0] + (double)counts[1]) : 0.0;
    if (has_rate && counts[1] == 0) {
      has_rate = false;
      fprintf(stderr, "[walt_amd sites: every call on the control %s is methylated: no rate below 1, no site is called]\n", o.site_control.c_str());
    } else if (!has_rate) {
      fprintf(stderr, "[walt_amd sites: the control %s has no call: no non-conversion rate, no site is called]\n", o.site_control.c_str());
    }
  }
  const uint32_t part[2][2] = {{0, c_lo}, {c_hi, genome_len}};  // in front of and behind the control
  hostio::SiteStatsRow row[4];
  memset(row, 0, sizeof row);
  double cutoff[4] = {0, 0, 0, 0};
  if (has_rate) {
    vector<uint64_t> hist(4 * (size_t)kSiteBins, 0), one(4 * (size_t)kSiteBins);
    uint64_t deep[4] = {0, 0, 0, 0};
    for (int k = 0; k < 2; ++k) {
      uint64_t d4[4];
      check(walt_pileup_depth_hist(p, part[k][0], part[k][1], one.data(), d4));
      for (size_t i = 0; i < hist.size(); ++i) hist[i] += one[i];
      for (int c = 0; c < 4; ++c) deep[c] += d4[c];
    }
    // the deep sites: the table that is d + 1 everywhere returns exactly them.  Fetched in the windows .methcounts uses and
    // kept as one entry per (depth, meth) pair with its count, so the host holds a window's records and the distinct pairs
    const uint64_t window = std::min<uint64_t>(kCountsWindow, genome_len);
    vector<uint32_t> table(walt::kSiteTable);
    for (uint32_t i = 0; i < walt::kSiteTable; ++i) table[i] = (i & walt::kSiteDepth) + 1u;
    vector<walt_meth_site> buf((size_t)window);
    std::map<std::pair<uint64_t, uint64_t>, uint64_t> pairs_of[4];
    if (deep[0] + deep[1] + deep[2] + deep[3])
      for_each_window(genome_len, window, [&](uint32_t w_lo, uint32_t w_hi) {
        for (int k = 0; k < 2; ++k) {
          const uint32_t lo = std::max(w_lo, part[k][0]), hi = std::min(w_hi, part[k][1]);
          if (lo >= hi) continue;
          uint64_t n = 0;
          check(walt_pileup_call_sites(p, lo, hi, table.data(), buf.data(), window, &n));
          for (uint64_t i = 0; i < n; ++i) pairs_of[buf[i].context & 3][{(uint64_t)buf[i].meth + buf[i].unmeth, (uint64_t)buf[i].meth}] += 1;
        }
      });
    vector<walt::SitecallDeep> deep_of[4];
    for (int c = 0; c < 4; ++c)
      for (const auto& e : pairs_of[c]) deep_of[c].push_back({e.first.first, e.first.second, e.second});
    for (int c = 0; c < 4; ++c) {
      const walt::SitecallContext r = walt::sitecall_context(hist.data() + (size_t)c * kSiteBins, deep_of[c].data(), deep_of[c].size(), rate,
                                                              o.site_alpha, o.site_depth, table.data() + (size_t)c * (walt::kSiteDepth + 1));
      row[c] = {r.tested, r.called, r.has_cutoff, r.cutoff};
      cutoff[c] = r.has_cutoff ? r.cutoff : -1.0;  // (no p-value is at or below it)
    }
    // the called sites, in the windows .methcounts uses; a deep record stays when its own p-value meets its context's cutoff
    vector<double> pv_of(kSiteBins);  // a shallow site's p-value depends on (depth, meth) alone
    for (uint32_t d = 1; d <= walt::kSiteDepth; ++d)
      for (uint32_t m = 0; m <= d; ++m) pv_of[walt::sitecall_bin(d, m)] = walt::sitecall_pval(d, m, rate);
    Append sf(out_file, kMethsites);
    uint32_t chr = 0;
    Sink out;
    for_each_window(genome_len, window, [&](uint32_t w_lo, uint32_t w_hi) {
      out.clear();
      for (int k = 0; k < 2; ++k) {
        const uint32_t lo = std::max(w_lo, part[k][0]), hi = std::min(w_hi, part[k][1]);
        if (lo >= hi) continue;
        uint64_t n = 0;
        check(walt_pileup_call_sites(p, lo, hi, table.data(), buf.data(), window, &n));
        for (uint64_t i = 0; i < n; ++i) {
          const walt_meth_site& s = buf[i];
          const double pv = s.reserved ? walt::sitecall_pval((uint64_t)s.meth + s.unmeth, s.meth, rate)
                                       : pv_of[walt::sitecall_bin(s.meth + s.unmeth, s.meth)];
          if (s.reserved && !(pv <= cutoff[s.context & 3])) continue;
          while (s.pos >= g.start[chr + 1]) ++chr;  // (ascending positions)
          hostio::put_site_line(out, g.name[chr], g.start[chr], s, pv);
        }
      }
      sf.write(out);
    });
  }
  Sink block;
  hostio::put_sitestats_block(block, o.site_control_given ? o.site_control : string("given"), o.site_control_given ? counts : nullptr, has_rate,
                              rate, o.site_alpha, o.site_depth, row);
  Append(out_file, kSitestats).write(block);
  if (o.verbose) fwrite(block.p, 1, block.n, stderr);
}

// the end of a read file: under -MV the variant sites first (ev: the evidence, as many objects as pile-ups); then
// <out>.methcounts (-MC) as ever, then <out>.levels (-ML) and <out>.regions (-MR), then the called sites (-MS:
// <out>.methsites, <out>.sitestats), which like the two before them read the first device's folded counters; then the
// counters cleared
static void end_of_file_pileups(const Options& o, const string& out_file, PileUps& ps, PileUps& ev, const GenomeInfo& g) {
  bool folded = false;
  if (o.variants) {
    fold_pileups(ps, g.start.back());
    fold_pileups(ev, g.start.back());
    folded = true;
    write_variants(o, out_file, ps.p[0], ev.p[0], g);
  }
  if (o.methcounts) {
    SiteTable t = {{0, 0}};
    if (folded) {  // the first device's counters hold every device's: a view of that one handle, which stays ps's
      struct { vector<walt_pileup*> p; } first = {{ps.p[0]}};
      write_window_table(t, first, out_file, g, o.verbose);
    } else {
      write_window_table(t, ps, out_file, g, o.verbose);
    }
  }
  if ((o.levels || o.regions() || o.sites) && !folded) fold_pileups(ps, g.start.back());
  if (o.levels) write_levels(out_file, ps, g, o.verbose);
  if (o.regions()) write_regions(out_file, ps);
  if (o.sites) write_sites(o, out_file, ps.p[0], g);
  for (walt_pileup* q : ps.p) check(walt_pileup_clear(q));
  for (walt_pileup* q : ev.p) check(walt_pileup_clear(q));
}

// ---------------------------------------------------------------- -MB: methylation bias by read position
// One set per device of the run, one table per mate; a share's calls are counted on the device that made them.  At the
// end of a read file the host adds the devices' tables, writes the blocks and clears the sets.
static void mbias_block(const MbiasSet& mbs, Sink& out, uint32_t table) {  // the table summed over the devices
  vector<uint64_t> sum(WALT_MBIAS_WORDS, 0), one(WALT_MBIAS_WORDS);
  for (walt_mbias* q : mbs.p) {
    check(walt_mbias_read(q, table, one.data()));
    for (size_t w = 0; w < sum.size(); ++w) sum[w] += one[w];
  }
  hostio::put_mbias_block(out, sum.data());
}
static void mbias_write(MbiasSet& mbs, const string& out_file, const Sink& ms) {
  Append(out_file, kMbias).write(ms);
  for (walt_mbias* q : mbs.p) check(walt_mbias_clear(q));
}

// ---------------------------------------------------------------- -MA: adjacent-CpG state pairs per read
// Pairs do not overlap, so a window holds at most half as many entries as positions; each line carries the test of its
// table.  The device counts in 32 bits, the host adds the devices' counters in 64.
struct PairTable {
  typedef walt_cpgpair_site Site;
  typedef hostio::AllelicRow Row;
  static constexpr int kOut = kAllelic;
  static constexpr uint32_t kWindow = kCountsWindow;
  uint64_t couples;
  static uint64_t capacity(uint64_t window) { return window / 2 + 1; }
  int extract(walt_cpgpairs* p, uint32_t lo, uint32_t hi, Site* buf, uint64_t cap, uint64_t* n) {
    return walt_cpgpairs_extract(p, lo, hi, buf, cap, n);
  }
  static Row row(const Site& b) { return Row{b.pos, b.next, {b.n[0], b.n[1], b.n[2], b.n[3]}}; }
  static void add(Row& r, const Row& o) { hostio::add_counter_row(r, o); }
  bool keep(const Row& r) { couples += r.n[0] + r.n[1] + r.n[2] + r.n[3]; return true; }
  void line(Sink& out, const string& chrom, uint32_t chrom_start, const Row& r) {  // (next lies in the same chromosome)
    hostio::put_allelic_line(out, chrom, r.pos - chrom_start, r.next - chrom_start, r.n);
  }
  void report(uint64_t n_rows) {
    fprintf(stderr, "[walt_amd allelic: %llu entries, %llu couples of neighbouring CpGs]\n", (unsigned long long)n_rows,
            (unsigned long long)couples);
  }
};

// ---------------------------------------------------------------- -ME: four-CpG epiallele patterns per read
// As the pair table, in windows of half as many positions (an entry is three times as large).  On one device -MEN is
// the extraction's min_total; with several the host extracts every entry that got a read, merges, and applies -MEN to
// the merged totals.
struct WindowTable {
  typedef walt_epiallele_site Site;
  typedef hostio::EpialleleRow Row;
  static constexpr int kOut = kEpialleles;
  static constexpr uint32_t kWindow = kCountsWindow / 2;
  uint32_t min_reads, min_extracted;  // -MEN; the same on one device, 1 on several
  uint64_t windows;
  static uint64_t capacity(uint64_t window) { return window / 2 + 1; }  // pairs do not overlap
  int extract(walt_epialleles* p, uint32_t lo, uint32_t hi, Site* buf, uint64_t cap, uint64_t* n) {
    return walt_epialleles_extract(p, lo, hi, min_extracted, buf, cap, n);
  }
  static Row row(const Site& b) {
    Row r = {b.pos, b.last, {}};
    for (int k = 0; k < 16; ++k) r.n[k] = b.n[k];
    return r;
  }
  static void add(Row& r, const Row& o) { hostio::add_counter_row(r, o); }
  bool keep(const Row& r) {
    const uint64_t total = hostio::epiallele_row_total(r);
    if (total >= min_reads) windows += total;
    return total >= min_reads;
  }
  void line(Sink& out, const string& chrom, uint32_t chrom_start, const Row& r) {  // (last lies in the same chromosome)
    hostio::put_epiallele_line(out, chrom, r.pos - chrom_start, r.last - chrom_start, r.n);
  }
  void report(uint64_t n_rows) {
    fprintf(stderr, "[walt_amd epialleles: %llu entries, %llu windows of four neighbouring CpGs]\n", (unsigned long long)n_rows,
            (unsigned long long)windows);
  }
};

// ---------------------------------------------------------------- -D: PCR duplicates
// One duplicate set per read file, on the first device of the run.  A batch is mapped by all devices first; then the
// whole batch's records are fed to the set in input order (so the verdict depends neither on -N nor on -g); only then are
// the methylation calls and the pile-up made, share by share, with the verdicts as their skip bytes.
struct DupSet {
  walt_dedup* dd = nullptr;
  vector<uint8_t> dup;  // the current batch's verdicts: one per read, two per pair
  uint64_t records = 0, duplicates = 0;  // eligible keys fed (reads, unique pairs, lone mates); those that were duplicates
  void open(int device) { check(walt_dedup_create(device, 0, &dd)); }
  void close() { if (dd) walt_dedup_destroy(dd); dd = nullptr; }
  bool on() const { return dd != nullptr; }
  void feed_se(const walt_best_match* res, const uint8_t* conv, int conversion, uint32_t n) {
    dup.assign(n, 0);
    check(walt_dedup_batch(dd, res, sizeof(walt_best_match), conv, 1, conversion, 0, n, dup.data()));
    for (uint32_t j = 0; j < n; ++j) { records += res[j].times == 1; duplicates += dup[j]; }
  }
  void feed_pe(const walt_pair_result* pr, const uint8_t* conv, uint32_t n) {
    dup.assign(2 * (size_t)n, 0);
    check(walt_dedup_pairs_batch(dd, pr, conv, 'T', n, dup.data()));
    for (uint32_t j = 0; j < n; ++j) {
      if (pr[j].best_times == 1) { records += 1; duplicates += dup[2 * (size_t)j]; continue; }
      records += (pr[j].m1.times == 1) + (pr[j].m2.times == 1);
      duplicates += dup[2 * (size_t)j] + dup[2 * (size_t)j + 1];
    }
  }
  void write_stats(const string& out_file) const {
    char num[160];
    if (records) snprintf(num, sizeof num, "records: %llu\nduplicates: %llu\nduplication rate: %.6f\n", (unsigned long long)records,
                          (unsigned long long)duplicates, (double)duplicates / (double)records);
    else snprintf(num, sizeof num, "records: 0\nduplicates: 0\nduplication rate: NA\n");
    Sink ms;
    ms.lit(num);
    Append(out_file, kDupstats).write(ms);
  }
};

// ---------------------------------------------------------------- -F -FC -FP -FM: non-converted reads
// The verdicts of the current batch -- one byte per read, two per pair, as DupSet's -- made share by share on the device
// that mapped the share: a first calling pass whose calls stay on the device and are judged there, then the pair rule.
// skip is what the calling call that counts takes: the verdict ORed with the duplicate's byte.  A duplicate is judged like
// any read, and a filtered read still enters the duplicate set (walt_dedup_* has no skip).
struct FilterSet {
  bool active = false;
  walt_nonconv_rule rule = {0, 0, 0, 0};
  vector<uint8_t> filt, skip;
  uint64_t records = 0, filtered = 0;  // unique reads, unique pairs and lone unique mates that are no duplicates; those that failed
  void open(const Options& o) {
    active = o.filtering();
    rule = walt_nonconv_rule{o.filter[0], o.filter[1], o.filter[2], o.filter[3]};
  }
  bool on() const { return active; }
  void start(size_t bytes) { filt.assign(bytes, 0); skip.assign(bytes, 0); }
  // the skip bytes [lo, hi) of the batch, stride 1 (a share's thread owns its range)
  void merge(size_t lo, size_t hi, const uint8_t* dup) {
    for (size_t j = lo; j < hi; ++j) skip[j] = (uint8_t)(filt[j] | (dup ? dup[j] : 0));
  }
  void count_se(const walt_best_match* res, const uint8_t* dup, uint32_t n) {
    for (uint32_t j = 0; j < n; ++j)
      if (res[j].times == 1 && !(dup && dup[j])) { ++records; filtered += filt[j] != 0; }
  }
  void count_pe(const walt_pair_result* pr, const uint8_t* dup, uint32_t n) {
    for (uint32_t j = 0; j < n; ++j) {
      const size_t a = 2 * (size_t)j;
      if (pr[j].best_times == 1) {
        if (!(dup && dup[a])) { ++records; filtered += filt[a] != 0; }
        continue;
      }
      if (pr[j].m1.times == 1 && !(dup && dup[a])) { ++records; filtered += filt[a] != 0; }
      if (pr[j].m2.times == 1 && !(dup && dup[a + 1])) { ++records; filtered += filt[a + 1] != 0; }
    }
  }
  void write_stats(const string& out_file, bool verbose) const {
    Sink ms;
    const uint32_t r[4] = {rule.min_meth, rule.min_run, rule.min_percent, rule.min_total};
    hostio::put_filter_block(ms, records, filtered, r);
    Append(out_file, kFilterstats).write(ms);
    if (verbose) fwrite(ms.p, 1, ms.n, stderr);
  }
};

static double g_t_main = 0;  // start of main (timeline under -v)
static int host_threads(const Options& o) { return o.threads > 0 ? o.threads : hostio::effective_cpus(); }
static double now_s() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

// ---------------------------------------------------------------- the GPUs of a run (-g)
// Every device holds a full index replica (opened side by side); a batch is cut into contiguous shares AFTER the
// loader has replaced its non-ACGT characters (the draws depend on the -N batch, not on the share: mapping.cpp:73),
// each share is mapped by its device from the same host arrays, and the records land in read order.  The
// statistics of the shares are added on the host -- this is one process; across processes the same sum is
// walt_stats_allreduce (include/walt_amd.h).
struct DeviceSet {
  vector<int> ids;
  vector<walt_index*> idx;
  void open(const Options& o, unsigned strands) {
    ids = o.devices;
    idx.assign(ids.size(), nullptr);
    vector<string> err(ids.size());
    vector<std::thread> th;
    for (size_t d = 0; d < ids.size(); ++d)
      th.emplace_back([&, d]() {
        if (walt_index_open(o.index_file.c_str(), ids[d], strands, -1, &idx[d]) != WALT_OK) err[d] = walt_last_error();
      });
    for (auto& t : th) t.join();
    for (const string& e : err) if (!e.empty()) { close(); die(e); }
    for (walt_index* i : idx)
      for (const auto& kv : o.tune)
        if (walt_index_set_option(i, kv.first.c_str(), kv.second) != WALT_OK) { const string e = walt_last_error(); close(); die(e); }
  }
  void close() {
    for (walt_index*& i : idx) { if (i) walt_index_close(i); i = nullptr; }
  }
  size_t size() const { return ids.size(); }
  void share(uint32_t n, size_t d, uint32_t& lo, uint32_t& hi) const {
    lo = (uint32_t)((uint64_t)n * d / ids.size());
    hi = (uint32_t)((uint64_t)n * (d + 1) / ids.size());
  }
  // fn(d, lo, hi) -> status, run for every device at once; the first failure is reported
  template <class F>
  void for_each_share(uint32_t n, F fn) const {
    if (ids.size() == 1) { uint32_t lo, hi; share(n, 0, lo, hi); if (fn(0, lo, hi) != WALT_OK) die(walt_last_error()); return; }
    vector<string> err(ids.size());
    vector<std::thread> th;
    for (size_t d = 0; d < ids.size(); ++d)
      th.emplace_back([&, d]() {
        uint32_t lo, hi;
        share(n, d, lo, hi);
        if (hi > lo && fn(d, lo, hi) != WALT_OK) err[d] = walt_last_error();
      });
    for (auto& t : th) t.join();
    for (const string& e : err) if (!e.empty()) die(e);
  }
};

// The next batch is read while the current one is mapped and written: the loader runs on its own thread with a
// share of the host threads (its N draws use rand(), which nothing else in the process calls meanwhile).
struct Prefetch {
  std::thread th;
  std::exception_ptr err;
  ~Prefetch() { if (th.joinable()) th.join(); }  // an error elsewhere unwinds past a running helper
  template <class F>
  void start(F fn) {
    err = nullptr;
    th = std::thread([this, fn]() { try { fn(); } catch (...) { err = std::current_exception(); } });
  }
  void wait() {
    if (th.joinable()) th.join();
    if (err) std::rethrow_exception(err);
  }
};

// -v: what this box's host side can move at all, measured where the run's output went -- T threads copying between private
// buffers (what formatting a line into a buffer costs at least) and T threads storing their buffers with pwrite at
// prefix-summed offsets into ONE scratch file beside the output (what OutFile does; one inode lock).  The run's format and
// write stages are to be read against these two figures (bench.py's end-to-end leg carries them).
static void host_ceiling(const string& out_file, int T) {
  const size_t per = 64u << 20;  // 64 MiB per thread and round
  std::vector<std::vector<char>> a((size_t)T), b((size_t)T);
#pragma omp parallel for num_threads(T) schedule(static)
  for (int t = 0; t < T; ++t) { a[(size_t)t].assign(per, (char)('A' + t)); b[(size_t)t].assign(per, 'x'); }
  double t0 = now_s();
  const int rounds = 4;
  for (int r = 0; r < rounds; ++r) {
#pragma omp parallel for num_threads(T) schedule(static)
    for (int t = 0; t < T; ++t) memcpy(b[(size_t)t].data(), a[(size_t)t].data(), per);
  }
  const double copy_gbs = (double)rounds * T * per / (now_s() - t0) / 1e9;
  const string tmp = out_file + ".ceiling.tmp";
  double write_gbs = 0.0;
  const int fd = ::open(tmp.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0600);
  if (fd >= 0) {
    t0 = now_s();
    for (int r = 0; r < rounds; ++r) {
#pragma omp parallel for num_threads(T) schedule(static)
      for (int t = 0; t < T; ++t) {
        size_t done = 0;
        while (done < per) {
          const ssize_t w = ::pwrite(fd, b[(size_t)t].data() + done, per - done, (off_t)(((size_t)r * T + (size_t)t) * per + done));
          if (w <= 0) break;
          done += (size_t)w;
        }
      }
    }
    write_gbs = (double)rounds * T * per / (now_s() - t0) / 1e9;
    ::close(fd);
    ::unlink(tmp.c_str());
  }
  fprintf(stderr, "[walt_amd host ceiling: memcpy %.1f GB/s on %d threads, pwrite into one file %.1f GB/s]\n", copy_gbs, T, write_gbs);
}

// The last read file is done, every output file closed, the indexes released: leave without unwinding.  What the
// destructors and the runtime's exit handlers would do -- hand back gigabytes of line buffers, unmap the read file,
// unload the HIP runtime -- took 0.6 s of a 2 s run, and the operating system does it anyway.
// Not when something else in the process counts on the exit handlers -- a preloaded tool that writes its trace there
// (LD_PRELOAD, rocprofv3's ROCP_TOOL_LIBRARIES), or WALT_AMD_FAST_EXIT=0 -- then main returns as usual.  A late failure
// of the standard streams still changes the exit status.
static void leave_now(bool verbose) {
  if (verbose) fprintf(stderr, "[walt_amd: %.2f s in main]\n", now_s() - g_t_main);
  const char* fe = getenv("WALT_AMD_FAST_EXIT");
  const char* pre = getenv("LD_PRELOAD");
  const char* tool = getenv("ROCP_TOOL_LIBRARIES");
  if ((fe && atoi(fe) == 0) || (pre && *pre) || (tool && *tool)) return;
  std::cout.flush();
  std::cerr.flush();
  const bool bad = fflush(stdout) != 0 || fflush(stderr) != 0 || ferror(stdout) || ferror(stderr) || !std::cout || !std::cerr;
  _exit(bad ? EXIT_FAILURE : EXIT_SUCCESS);
}

// ---------------------------------------------------------------- what takes the methylation calls of a read file
// A slot is one read of a record: the read of a single-end run, mate k of a paired-end one.  The batch's per-record bytes
// (conversions, duplicate and filter verdicts, skip bytes) hold n_slots bytes per record, slot k's at offset k.
// One slot's view of a share: what the calling calls take, each pointer at the share's first record
struct SlotView {
  const char* bases;
  const uint64_t* offsets;
  const void* rec;  // the slot's walt_best_match of the first record; rec_stride bytes to the next
  size_t rec_stride;
  const uint8_t* conv;  // -R -RP: the conversion of each record, or null: `conversion` for all
  int conversion;
  const uint32_t* clip;  // -C
  char* calls;           // -M -sam: the batch's calls, at the offsets of its bases
  walt_meth_stats* stats;
  uint8_t* filt;        // -F: the verdicts
  const uint8_t* skip;  // -D -F: what keeps a record out of the counts
  size_t stride;        // of conv, filt and skip: n_slots
  const uint32_t* excl;  // -NO: the interval words (the user's mate 2 only)
  uint32_t table;        // -MB
  uint32_t ignore5, ignore3;
  const uint8_t* quals;  // -MQ: the batch's quality bytes, at the offsets of its bases; else null
  uint32_t min_qual;     // the floor the raw bytes are compared with; 0 without -MQ
};

struct Consumers {
  const DeviceSet* dev = nullptr;
  bool calling = false;  // something takes the calls
  int n_slots = 1;
  PileUps pile;        // both mates into the device's pile-up
  PileUps evid;        // -MV: both mates' opposite-strand evidence, a second pile-up per device
  MbiasSet mbs;
  PairTables pairs;    // both mates into the same table, each by itself
  WindowTables epi;    // likewise
  DupSet dups;
  FilterSet flt;
  // the current batch
  vector<uint8_t> conv;      // -R -RP: the conversion of every record's slots ('T' / 'A')
  vector<char> calls[2];     // -M -sam: the methylation calls of each slot's batch, at the offsets of its bases
  vector<uint32_t> clip[2];  // -C: the clip point of every read
  // -NO: per pair, the read positions of the user's mate 2 that its mate 1 already calls (include/walt_amd.h, "overlap of
  // a pair").  The totals: pairs with an overlap, mate-2 bases left uncalled
  vector<uint32_t> excl;
  vector<walt_meth_stats> meth_of;  // [device * n_slots + slot]
  vector<uint64_t> overlap_of;      // [device * 2 + total]
  // the read file so far
  walt_meth_stats meth_total[2];  // per slot
  uint64_t overlap_total[2] = {0, 0};

  void open(const Options& o, const DeviceSet& devices, int slots) {
    dev = &devices;
    calling = o.consumer();
    n_slots = slots;
    const size_t n = dev->size();
    if (o.piling()) pile.open(n, [&](size_t d, walt_pileup** h) { return walt_pileup_create(dev->idx[d], h); });
    if (o.variants) evid.open(n, [&](size_t d, walt_pileup** h) { return walt_pileup_create(dev->idx[d], h); });
    if (o.mbias) mbs.open(n, [&](size_t d, walt_mbias** h) { return walt_mbias_create(dev->ids[d], (uint32_t)slots, h); });
    if (o.allelic) pairs.open(n, [&](size_t d, walt_cpgpairs** h) { return walt_cpgpairs_create(dev->idx[d], h); });
    if (o.epialleles) epi.open(n, [&](size_t d, walt_epialleles** h) { return walt_epialleles_create(dev->idx[d], h); });
    if (o.dedup) dups.open(dev->ids[0]);
    flt.open(o);
    memset(meth_total, 0, sizeof meth_total);
  }
  // bt[k], adaptors[k]: slot k's reads and the adaptor they were clipped at
  void start_batch(const Options& o, const Batch* bt, const string* adaptors, bool both_conversions, int T) {
    const size_t n_devices = dev->size();
    const uint32_t n = bt[0].n;
    const size_t bytes = (size_t)n_slots * n;
    if (both_conversions && conv.size() < bytes) conv.resize(bytes);
    meth_of.resize(n_slots * n_devices);
    memset(meth_of.data(), 0, meth_of.size() * sizeof(walt_meth_stats));
    for (int k = 0; k < n_slots && calling; ++k) {
      if (o.meth && o.sam && calls[k].size() < bt[k].offsets[n]) calls[k].resize(bt[k].offsets[n]);
      if (!adaptors[k].empty()) clip_points(bt[k], adaptors[k], T, clip[k]);
    }
    if (o.no_overlap) {
      overlap_of.assign(2 * n_devices, 0);
      if (excl.size() < n) excl.resize(n);
    }
    if (flt.on()) flt.start(bytes);
  }
  const uint8_t* dup_bytes() const { return dups.on() ? dups.dup.data() : nullptr; }
  // slot k of the share of device d that starts at record lo; ignore: the slot's -I5 / -I3 bounds
  SlotView view(const Options& o, size_t d, uint32_t lo, int k, const Batch& b, const void* rec, size_t rec_stride,
                bool both_conversions, int conversion, const uint32_t* ignore) {
    const size_t at = (size_t)n_slots * lo + k;
    const uint8_t* skip = flt.on() ? flt.skip.data() : dup_bytes();  // (-F: the verdicts ORed with -D's, FilterSet::merge)
    SlotView v;
    v.bases = b.bases; v.offsets = b.offsets + lo;
    v.rec = rec; v.rec_stride = rec_stride;
    v.conv = both_conversions ? conv.data() + at : nullptr; v.conversion = conversion;
    v.clip = clip[k].empty() ? nullptr : clip[k].data() + lo;
    v.calls = o.meth && o.sam ? calls[k].data() : nullptr;
    v.stats = o.meth ? &meth_of[n_slots * d + k] : nullptr;
    v.filt = flt.on() ? flt.filt.data() + at : nullptr;
    v.skip = skip ? skip + at : nullptr;
    v.stride = n_slots;
    v.excl = nullptr;
    v.table = (uint32_t)k;
    v.ignore5 = ignore[0]; v.ignore3 = ignore[1];
    v.quals = o.min_qual ? reinterpret_cast<const uint8_t*>(b.quals) : nullptr;
    v.min_qual = o.qual_floor();
    return v;
  }
  // The calls of one slot of a share, on the device that mapped it.  With a rule (-F -FC -FP) the verdict pass: the calls
  // of the whole read up to its clip point, whatever -I5 / -I3 say, stay on the device and are judged there.  Without one
  // the pass that counts: one call takes whatever the options give it -- pile-up, skip bytes, interval words, bias set,
  // pair table, window table, evidence -- each null without its option (all null: walt_meth_call_batch) and the ignored read ends
  // 0 without theirs, so that a run launches only the kernels its options ask for.
  int call_slot(size_t d, uint32_t n, const SlotView& v, const walt_nonconv_rule* rule) const {
    walt_index* idx = dev->idx[d];
    // (quals null, without -MQ: each of the two is the older entry point, walt_meth_nonconv_batch and walt_meth_pileup_batch_ev)
    if (rule)
      return walt_meth_nonconv_batch_qual(idx, v.bases, v.offsets, n, v.rec, v.rec_stride, v.conv, v.stride, v.conversion, v.clip,
                                          nullptr, rule, v.filt, v.stride, nullptr, v.quals, v.min_qual);
    return walt_meth_pileup_batch_qual(idx, pile.of(d), v.bases, v.offsets, n, v.rec, v.rec_stride, v.conv, v.stride,
                                       v.conversion, v.clip, v.calls, nullptr, v.stats, v.skip, v.stride, v.excl, mbs.of(d),
                                       v.table, v.ignore5, v.ignore3, pairs.of(d), epi.of(d), evid.of(d), v.quals, v.min_qual);
  }
  // The end of a read file: <out>.methstats, the pile-up's files, <out>.mbias, .allelic, .epialleles, .dupstats and
  // .filterstats, each table cleared or closed behind its file.  slot_of_user_mate: null for single-end reads; for pairs
  // the slot that holds the user's mate 1 and mate 2 (exchanged under -P), whose blocks get a heading each.
  void finish(const Options& o, const string& out_file, const GenomeInfo& g, const int* slot_of_user_mate) {
    auto blocks = [&](Sink& ms, auto put) {
      for (int u = 0; u < n_slots; ++u) {
        if (slot_of_user_mate) ms.lit(u ? "mate2\n" : "mate1\n");
        put(slot_of_user_mate ? slot_of_user_mate[u] : 0);
      }
    };
    Sink settings;  // the lines behind the blocks of <out>.methstats, also written under -v
    if (o.no_overlap) {  // over all unique proper pairs, duplicates (-D) included
      char overlap[96];
      snprintf(overlap, sizeof overlap, "overlap\t%llu\t%llu\n", (unsigned long long)overlap_total[0], (unsigned long long)overlap_total[1]);
      settings.lit(overlap);
    }
    if (o.ignoring()) hostio::put_ignore_line(settings, o.ignore, 2 * n_slots);
    if (o.min_qual) hostio::put_minqual_line(settings, o.min_qual, o.qual_offset);
    if (o.meth) {
      Sink ms;
      blocks(ms, [&](int slot) { put_meth_block(ms, meth_total[slot]); });
      if (settings.n) ms.put(settings.p, settings.n);
      Append(out_file, kMethstats).write(ms);
    }
    if (o.verbose && settings.n) fwrite(settings.p, 1, settings.n, stderr);
    if (pile.on()) { end_of_file_pileups(o, out_file, pile, evid, g); pile.close(); evid.close(); }
    if (mbs.on()) {
      Sink ms;
      blocks(ms, [&](int slot) { mbias_block(mbs, ms, (uint32_t)slot); });
      mbias_write(mbs, out_file, ms);
      mbs.close();
    }
    if (pairs.on()) {
      PairTable t = {0};
      write_window_table(t, pairs, out_file, g, o.verbose);
      pairs.close();
    }
    if (epi.on()) {
      WindowTable t = {o.epi_min, epi.p.size() > 1 ? 1 : o.epi_min, 0};
      write_window_table(t, epi, out_file, g, o.verbose);
      epi.close();
    }
    if (dups.on()) { dups.write_stats(out_file); dups.close(); }
    if (flt.on()) flt.write_stats(out_file, o.verbose);
  }
};

// One batch.  Without -D every device maps its share and makes the share's calls behind it.  With -D every share is
// mapped first, then feed() puts the whole batch's records through the duplicate set in input order (so the verdict
// depends neither on -N nor on -g), and only then are the calls made, share by share, with the verdicts as skip bytes.
// map_share(d, lo, hi) and meth_share(d, lo, hi) return a status; the batch's totals are added to the read file's.
template <class Map, class Feed, class Meth>
static void run_batch(Consumers& c, uint32_t n, Map map_share, Feed feed, Meth meth_share) {
  const DeviceSet& dev = *c.dev;
  if (!c.dups.on()) {
    dev.for_each_share(n, [&](size_t d, uint32_t lo, uint32_t hi) {
      const int rc = map_share(d, lo, hi);
      return rc == WALT_OK && c.calling ? meth_share(d, lo, hi) : rc;
    });
  } else {
    dev.for_each_share(n, map_share);
    feed();
    if (c.calling) dev.for_each_share(n, meth_share);
  }
  for (size_t i = 0; i < c.meth_of.size(); ++i) add_meth(c.meth_total[i % c.n_slots], c.meth_of[i]);
  for (size_t i = 0; i < c.overlap_of.size(); ++i) c.overlap_total[i & 1] += c.overlap_of[i];
}

// the batch's records in page-locked memory, grown by an eighth more than asked so that equal batches allocate once
template <class R>
static void reserve_records(R*& res, size_t& cap, uint32_t n) {
  if (cap >= n) return;
  walt_host_free(res);
  res = nullptr;
  cap = n + n / 8;
  check(walt_host_alloc(cap * sizeof(R), (void**)&res));
}

// ProcessSingledEndReads, mapping.cpp:421-526
static void process_se(const Options& o, const string& reads_file, const string& out_file, bool last_file) {
  const int T = host_threads(o);
  const int T_bg = std::max(1, T / 4);  // the loader's share while a batch is being formatted
  double t0 = now_s();
  // the first batch is read WHILE the index is opened (seconds of file reads and kernels that leave most host cores
  // idle); the loader's N draws are the only rand() calls of the process, as before
  hostio::FastqReader rd;
  Batch bt[2];
  Prefetch first;
  double t_open_reads = 0;
  first.start([&]() {
    const double t_o0 = now_s();
    rd.want_quals = o.min_qual != 0;
    rd.open(reads_file, std::max(1, T / 2));
    t_open_reads = now_s() - t_o0;
    rd.load(o.batch_size, o.adaptor, bt[0]);
  });
  DeviceSet dev;
  dev.open(o, (o.rpbat ? WALT_STRANDS_ALL : o.ag ? WALT_STRANDS_GA : WALT_STRANDS_CT) | (o.consumer() ? WALT_WITH_REFERENCE : 0u));
  Consumers cs;
  cs.open(o, dev, 1);
  double t_index = now_s() - t0, t_load = 0, t_map = 0, t_out = 0, t_write = 0;
  GenomeInfo g = genome_of(dev.idx[0]);
  if (o.regions()) g_regions.resolve(g, o.verbose);  // (a region beyond its chromosome: refused before a read is mapped)
  if (o.sites && o.site_control_given) (void)site_control_of(o, g);
  OutFile fout;
  if (!fout.open_append(out_file)) die("cannot open input file " + out_file);
  SideFiles side;
  side.open(o.ambiguous, o.unmapped, out_file, o.sam);
  SeCounts st;
  if (o.verbose) std::cerr << "input_file: " << reads_file << std::endl << "output_file: " << out_file << std::endl;
  if (o.sam) { string h = sam_head(g); fout.write(h.data(), h.size()); }
  walt_best_match* res = nullptr;
  size_t res_cap = 0;
  vector<Sink> sinks((size_t)T * kSinks);
  vector<SeCounts> acc(T);
  // Only the ingest runs ahead.  Storing a batch's lines from a helper thread while the next batch is formatted was
  // tried and lost: both are memory copies on the same cores (40 M reads: format 0.67 -> 0.96 s, and 1.3 s more
  // waiting for the writer).
  Prefetch pre;
  // The last batch: the idle buffer's page-locked memory is handed back while the batch is formatted, the batch's own
  // while its lines are written (unlocking 2.6 GB at the end of the run was 0.5 s of a 2 s run).
  Prefetch unlock_idle, unlock_last;
  t0 = now_s();
  first.wait();  // what is still left of the first batch's ingest
  rd.threads = T;
  t_load += now_s() - t0;
  for (int cur = 0;; cur ^= 1) {
    Batch& b = bt[cur];
    if (b.n == 0) break;
    const uint32_t n = b.n;
    const bool more = n == o.batch_size;  // mapping.cpp:515-516: a short batch is the last one
    if (more) {
      rd.threads = T_bg;
      pre.start([&, cur]() { rd.load(o.batch_size, o.adaptor, bt[cur ^ 1]); });
    }
    reserve_records(res, res_cap, n);
    t0 = now_s();
    vector<uint64_t> short_of(dev.size(), 0);
    cs.start_batch(o, &b, &o.adaptor, o.rpbat, T);
    auto map_share = [&](size_t d, uint32_t lo, uint32_t hi) {
      walt_batch_stats bs;
      const int rc = o.rpbat ? walt_map_se_rpbat_batch(dev.idx[d], b.bases, b.offsets + lo, hi - lo, o.max_mismatches, o.b, res + lo, cs.conv.data() + lo, &bs)
                             : walt_map_se_batch(dev.idx[d], b.bases, b.offsets + lo, hi - lo, o.ag, o.max_mismatches, o.b, res + lo, &bs);
      short_of[d] = bs.too_short;
      return rc;
    };
    auto meth_share = [&](size_t d, uint32_t lo, uint32_t hi) {
      const SlotView v = cs.view(o, d, lo, 0, b, res + lo, sizeof(walt_best_match), o.rpbat, o.ag ? 'A' : 'T', o.ignore);
      if (cs.flt.on()) {  // first the share's verdicts, ORed into the skip bytes beside -D's
        const int rc = cs.call_slot(d, hi - lo, v, &cs.flt.rule);
        if (rc != WALT_OK) return rc;
        cs.flt.merge(lo, hi, cs.dup_bytes());
      }
      return cs.call_slot(d, hi - lo, v, nullptr);
    };
    run_batch(cs, n, map_share, [&]() { cs.dups.feed_se(res, o.rpbat ? cs.conv.data() : nullptr, o.ag ? 'A' : 'T', n); }, meth_share);
    if (cs.flt.on()) cs.flt.count_se(res, cs.dup_bytes(), n);
    for (uint64_t v : short_of) st.too_short += (uint32_t)v;
    t_map += now_s() - t0;
    if (!more) unlock_idle.start([&, cur]() { bt[cur ^ 1].release(); });
    t0 = now_s();
#pragma omp parallel for schedule(static, 1) num_threads(T)
    for (int t = 0; t < T; ++t) {
      Sink* s = &sinks[(size_t)t * kSinks];
      for (int k = 0; k < kSinks; ++k) s[k].clear();
      SeCounts c;
      const uint32_t lo = (uint32_t)((uint64_t)n * t / T), hi = (uint32_t)((uint64_t)n * (t + 1) / T);
      // one allocation per thread and batch instead of doubling: name + 2 x read + fixed fields per line
      s[kMain].grow((b.offsets[hi] - b.offsets[lo]) * 2 + (size_t)(hi - lo) * 96);
      for (uint32_t j = lo; j < hi; ++j) {
        c.update(res[j].times);
        // -R: a record of the G->A conversion is written as a -A run writes it (MR), or tagged (SAM)
        const bool ag = o.rpbat ? cs.conv[j] == 'A' : o.ag;
        const bool dup = cs.dups.on() && cs.dups.dup[j];  // (a duplicate has times == 1: its only line is the main file's)
        const bool gone = cs.flt.on() && cs.flt.filt[j];  // (and so has a filtered read)
        if (!o.sam) { if (!dup && !gone) out_single_results(res[j], b.name(j), b.seq(j), b.score(j), g, ag, side.out_amb, side.out_unm,
                                                   s[kMain], s[kAmb1], s[kUnm1]); }
        else out_single_sam(res[j], b.name(j), b.seq(j), b.score(j), g, side.out_amb, side.out_unm, s[kMain],
                            o.rpbat ? (ag ? "\tCV:A:A" : "\tCV:A:T") : nullptr,
                            o.meth ? View{cs.calls[0].data() + b.offsets[j], b.seq(j).len} : View{nullptr, 0},
                            (dup ? 0x400 : 0) + (gone ? 0x200 : 0));
      }
      acc[t] = c;
    }
    for (int t = 0; t < T; ++t) st.add(acc[t]);
    t_out += now_s() - t0;
    if (!more) unlock_last.start([&, cur]() { bt[cur].release(); });  // (the lines are in the sinks; names and qualities are views into the file)
    t0 = now_s();
    fout.write_sinks(sinks, kSinks, kMain, T);
    side.amb.write_sinks(sinks, kSinks, kAmb1, T);
    side.unm.write_sinks(sinks, kSinks, kUnm1, T);
    t_write += now_s() - t0;
    if (!more) { unlock_idle.wait(); unlock_last.wait(); break; }
    t0 = now_s();
    pre.wait();  // what is still left of the next batch's ingest
    t_load += now_s() - t0;
  }
  if (o.verbose)
    fprintf(stderr, "[walt_amd ingest: line scan %.2f s, views %.2f s, buffers %.2f s, copy %.2f s, N draws %.2f s]\n",
            rd.t_scan, rd.t_views, rd.t_alloc, rd.t_copy, rd.t_rng);
  rd.close();
  fout.close();
  side.close();
  walt_host_free(res);
  {
    Sink ms;
    st.put_block(ms, 0);
    ms.ch('\n');
    Append(out_file, kMapstats).write(ms);
  }
  cs.finish(o, out_file, g, nullptr);
  const double t_c0 = now_s();
  dev.close();
  if (o.verbose)
    fprintf(stderr, "[walt_amd: %d host threads, %zu GPU(s); index %.2f s, ingest not hidden behind the previous batch %.2f s, map %.2f s, "
            "format %.2f s, write %.2f s; opening the reads %.2f s, closing the index %.2f s, since main %.2f s]\n", T, dev.size(), t_index,
            t_load, t_map, t_out, t_write, t_open_reads, now_s() - t_c0, now_s() - g_t_main);
  if (o.verbose && last_file && getenv("WALT_AMD_HOST_CEILING")) host_ceiling(out_file, T);
  if (last_file) leave_now(o.verbose);
}

// ---------------------------------------------------------------- paired-end writers
static void forward_pos(uint32_t gp, char strand, uint32_t chr, uint32_t read_len, const GenomeInfo& g, uint32_t& s,
                        uint32_t& e) {  // paired.cpp:98-104
  s = gp - g.start[chr];
  s = strand == '+' ? s : g.length[chr] - s - read_len;
  e = s + read_len;
}
// A uniquely paired fragment (OutputBestPairedResults, paired.cpp:210-294): its length, and in MR mode the FRAG line.
// Both mates are laid over the fragment, which is written in mate 1's reading direction: position x of the line is
// base x of mate 1 and base j2(x) of the reverse-complemented mate 2.  Where only one mate covers x its base is
// printed; where both do, the base of the mate with more informative positions (length minus Ns minus mismatches;
// mate 1 on a tie); where neither does (mates that do not meet), 'N' with quality 'B'.
static inline char comp_base(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }
static uint32_t count_n(View v) {
  uint32_t n = 0;
  for (uint32_t i = 0; i < v.len; ++i) n += v.p[i] == 'N';
  return n;
}
static int put_fragment(const walt_candidate& r1, const walt_candidate& r2, int frag_range, const GenomeInfo& g, View name,
                        View seq1, View scr1, View seq2, View scr2, bool length_only, Sink& fout) {
  const uint32_t c1 = chrom_id(g, r1.genome_pos), c2 = chrom_id(g, r2.genome_pos);
  uint32_t s1, s2, e1, e2;
  forward_pos(r1.genome_pos, r1.strand, c1, seq1.len, g, s1, e1);
  forward_pos(r2.genome_pos, r2.strand, c2, seq2.len, g, s2, e2);
  const bool fwd = r1.strand == '+';
  // the fragment runs from mate 1's 5' end to mate 2's: [s1, e2) read upwards, or [s2, e1) read downwards
  const int len = fwd ? (int)(e2 - s1) : (int)(e1 - s2);
  if (length_only) return len;
  const bool lay = len > 0 && len <= frag_range;
  const int info1 = (int)seq1.len - (int)(count_n(seq1) + r1.mismatch);
  const int info2 = (int)seq2.len - (int)(count_n(seq2) + r2.mismatch);
  const bool mate1_wins = info1 >= info2;
  // index into the reverse-complemented mate 2 of line position x: (s1 + x) - s2 upwards, e2 - 1 - (e1 - 1 - x) downwards
  const int64_t shift = fwd ? (int64_t)s1 - (int64_t)s2 : (int64_t)e2 - (int64_t)e1;
  const uint32_t start_pos = fwd ? s1 : s2;
  fout.put(g.name[c1]); fout.ch('\t'); fout.u32(start_pos); fout.ch('\t'); fout.u32(start_pos + len);
  fout.lit("\tFRAG:"); fout.put(name); fout.ch('\t'); fout.u32(r1.mismatch + r2.mismatch); fout.ch('\t');
  fout.ch(r1.strand); fout.ch('\t');
  for (int pass = 0; pass < 2; ++pass) {  // bases, then qualities
    char* out = fout.grow((size_t)len);
    for (int x = 0; x < len; ++x) {
      const int64_t j2 = (int64_t)x + shift;
      const bool in1 = lay && (uint32_t)x < seq1.len, in2 = lay && j2 >= 0 && j2 < (int64_t)seq2.len;
      char ch = pass ? 'B' : 'N';
      if (in1 && (!in2 || mate1_wins)) {
        ch = pass ? scr1.p[x] : seq1.p[x];
      } else if (in2) {
        const uint32_t k = seq2.len - 1 - (uint32_t)j2;  // the reverse complement is never materialised
        ch = pass ? scr2.p[k] : comp_base(seq2.p[k]);
      }
      out[x] = ch;
    }
    fout.n += (size_t)len;
    fout.ch(pass ? '\n' : '\t');
  }
  return len;
}
static int sam_flag(bool paired_mapped, bool unmapped, bool next_unmapped, bool rev, bool next_rev, bool first,
                    bool secondary) {  // GetSAMFLAG, paired.cpp:80-95
  return 0x1 + (paired_mapped ? 0x2 : 0) + (unmapped ? 0x4 : 0) + (next_unmapped ? 0x8 : 0) + (rev ? 0x10 : 0) +
         (next_rev ? 0x20 : 0) + (first ? 0x40 : 0x80) + (secondary ? 0x100 : 0);
}
static void sam_mate_line(Sink& f, View name, int flag, bool mapped, const string& chrom, uint32_t pos, uint32_t read_len,
                          const string& rnext, uint32_t pnext, int tlen, View seq, View score, bool flip, uint32_t mm,
                          const char* tag, View xm) {
  f.put(name); f.ch('\t'); f.i32(flag); f.ch('\t');
  if (mapped) { f.put(chrom); f.ch('\t'); f.u32(pos); f.lit("\t255\t"); f.u32(read_len); f.lit("M\t"); }
  else { f.lit("*\t"); f.u32(pos); f.lit("\t255\t*\t"); }
  f.put(rnext); f.ch('\t'); f.u32(pnext); f.ch('\t'); f.i32(tlen); f.ch('\t');
  put_seq_qual(f, seq, score, flip);
  f.lit("\tNM:i:"); f.u32(mm);
  if (tag) f.lit(tag);
  if (mapped) put_xm(f, xm, flip);
  f.ch('\n');
}
// OutputPairedSAM, paired.cpp:333-435
// tag_1 / tag_2: appended to the mate's line (-RP: "\tCV:A:T" / "\tCV:A:A", the conversion of its record), or null
static void out_paired_sam(const walt_best_match& b1, const walt_best_match& b2, const GenomeInfo& g, View name,
                           View seq1, View scr1, View seq2, View scr2, int len, int flag_1, int flag_2, bool out_amb,
                           bool out_unm, bool second_first, Sink& fout, const char* tag_1 = nullptr,
                           const char* tag_2 = nullptr, View xm1 = View{nullptr, 0}, View xm2 = View{nullptr, 0}) {
  uint32_t c1 = chrom_id(g, b1.genome_pos), c2 = chrom_id(g, b2.genome_pos);
  uint32_t s1, s2, e1, e2;
  forward_pos(b1.genome_pos, b1.strand, c1, seq1.len, g, s1, e1);
  forward_pos(b2.genome_pos, b2.strand, c2, seq2.len, g, s2, e2);
  uint32_t mm1 = b1.mismatch, mm2 = b2.mismatch;
  if (b1.times == 0) { s1 = 0; mm1 = 0; } else s1 += 1;
  if (b2.times == 0) { s2 = 0; mm2 = 0; } else s2 += 1;
  int len1 = b1.strand == '+' ? len : -len;
  int len2 = b2.strand == '+' ? len : -len;
  string rn1 = "=", rn2 = "=";
  if (!(flag_1 & 0x2)) {
    rn1 = b1.times == 0 ? "*" : g.name[c1];
    rn2 = b2.times == 0 ? "*" : g.name[c2];
  }
  auto first = [&]() {
    if (b1.times == 0 && out_unm)
      sam_mate_line(fout, name, flag_1, false, g.name[c1], s1, seq1.len, rn2, s2, len1, seq1, scr1, b1.strand == '-', mm1, tag_1, xm1);
    else if (b1.times == 1 || (b1.times >= 2 && out_amb))
      sam_mate_line(fout, name, flag_1, true, g.name[c1], s1, seq1.len, rn2, s2, len1, seq1, scr1, b1.strand == '-', mm1, tag_1, xm1);
  };
  auto second = [&]() {
    if (b2.times == 0 && out_unm)
      sam_mate_line(fout, name, flag_2, false, g.name[c2], s2, seq2.len, rn1, s1, len2, seq2, scr2, b2.strand == '-', mm2, tag_2, xm2);
    else if (b2.times == 1 || (b2.times >= 2 && out_amb))
      sam_mate_line(fout, name, flag_2, true, g.name[c2], s2, seq2.len, rn1, s1, len2, seq2, scr2, b2.strand == '-', mm2, tag_2, xm2);
  };
  if (second_first) { second(); first(); } else { first(); second(); }
}

struct PeAcc {
  SeCounts st1, st2;
  uint32_t unique_pairs = 0, ambiguous_pairs = 0, unmapped_pairs = 0;
  vector<uint32_t> frag_count;
};

// ProcessPairedEndReads, paired.cpp:572-713.
// -P (PBAT): the snapshot of the reference has no code for it ("parity unpinned"); it is DEFINED
// here by equivalence to a run the reference can do: mate 1 is the A-rich read, so the pair is mapped with the
// mate files exchanged (mate 2 against the C->T indexes, mate 1 against the G->A indexes), and the output is
// then put back in the user's order: mate 1's record / line / _1 side files / mapstats block first, FLAG
// 0x40 on mate 1 and 0x80 on mate 2, QNAME from the -1 file.
// -RP (paired-end random PBAT): every pair is mapped in both orientations by walt_map_pe_rpbat_batch, which returns
// one record per pair in user order and the conversion of each mate (include/walt_amd.h).  A unique pair that the
// mate-exchanged orientation decided (rule 3, conversions (A, T)) gets the FRAG line a -P run writes; every other line
// is written in user order, each mate's single-end line by the writer of its conversion, and SAM lines carry the
// mate's conversion as CV:A:T / CV:A:A.  Since -P output is in user order too, rule-3 pairs are written as -P writes
// them and the other rules as the plain run does.
static void process_pe(const Options& o, const string& file1, const string& file2, const string& out_file, bool last_file) {
  const bool pbat = o.pbat;
  const bool rp = o.rpbat_pe;
  const string& f1 = pbat ? file2 : file1;  // slot 0: the T-rich mate, mapped on _CT00/_CT01
  const string& f2 = pbat ? file1 : file2;  // slot 1: the A-rich mate, mapped on _GA10/_GA11
  const int name_slot = pbat ? 1 : 0;       // paired.cpp:694 prints the -1 file's name for both records
  const int T = host_threads(o);
  const int T_bg = std::max(1, T / 4);
  double t0 = now_s();
  DeviceSet dev;
  dev.open(o, WALT_STRANDS_ALL | (o.consumer() ? WALT_WITH_REFERENCE : 0u));  // (all four strands are resident: one pass over them)
  Consumers cs;
  cs.open(o, dev, 2);
  double t_index = now_s() - t0, t_load = 0, t_map = 0, t_out = 0;
  GenomeInfo g = genome_of(dev.idx[0]);
  if (o.regions()) g_regions.resolve(g, o.verbose);  // (a region beyond its chromosome: refused before a read is mapped)
  if (o.sites && o.site_control_given) (void)site_control_of(o, g);
  hostio::FastqReader rd[2];
  rd[0].want_quals = rd[1].want_quals = o.min_qual != 0;
  rd[0].open(f1, T);
  rd[1].open(f2, T);
  const AdaptorPair ap = split_adaptor_option(o.adaptor);
  const string adaptors[2] = {ap.mate1, ap.mate2};
  OutFile fout;
  if (!fout.open_append(out_file)) die("cannot open input file " + out_file);
  SideFiles side1, side2;  // StatPairedReads, paired.hpp:78-106
  side1.open(o.ambiguous, o.unmapped, out_file + "_1", o.sam);
  side2.open(o.ambiguous, o.unmapped, out_file + "_2", o.sam);
  SeCounts st1, st2;
  uint32_t total_pairs = 0, unique_pairs = 0, ambiguous_pairs = 0, unmapped_pairs = 0;
  vector<uint32_t> frag_count(o.frag_range + 1, 0);
  fprintf(stderr, "[MAPPING PAIRED-END READS FROM THE FOLLOWING TWO FILES]\n   %s (AND)\n   %s\n", file1.c_str(), file2.c_str());
  fprintf(stderr, "[OUTPUT MAPPING RESULTS TO %s]\n", out_file.c_str());
  if (o.sam) { string h = sam_head(g); fout.write(h.data(), h.size()); }
  Batch bts[2][2];  // [buffer][mate]: one pair of batches is mapped and written while the next is read
  walt_pair_result* pr = nullptr;
  size_t pr_cap = 0;
  // the slots of the user's mate 1 and mate 2: under -P slot 0 holds the user's mate 2.  -NO gives the interval words to
  // the calls of the user's mate 2; -I5 -I3 -I5R2 -I3R2 are given for the user's mate 1 and mate 2
  const int user_slot[2] = {pbat ? 1 : 0, pbat ? 0 : 1};
  const int over_slot = user_slot[1];
  const uint32_t* const trim_slot[2] = {o.ignore + 2 * user_slot[0], o.ignore + 2 * user_slot[1]};
  vector<Sink> sinks((size_t)T * kSinks);
  vector<PeAcc> acc(T);
  Prefetch pre, unlock_idle;  // (the idle buffers of the last batch: see process_se)
  auto load_pair = [&](Batch* b) {  // mate 1's file, then mate 2's: each load starts its own srand(0) sequence (paired.cpp:648)
    rd[0].load(o.batch_size, adaptors[0], b[0]);
    if (b[0].n) rd[1].load(o.batch_size, adaptors[1], b[1]); else b[1].n = 0;
  };
  t0 = now_s();
  load_pair(bts[0]);
  t_load += now_s() - t0;
  for (int cur = 0;; cur ^= 1) {
    Batch* bt = bts[cur];
    if (bt[0].n && bt[0].n != bt[1].n) {
      fprintf(stderr, "The number of reads in paired-end files should be the same.\n");
      exit(EXIT_FAILURE);
    }
    if (bt[0].n == 0) break;
    const uint32_t n = bt[0].n;
    const bool more = n == o.batch_size;
    if (more) {
      rd[0].threads = rd[1].threads = T_bg;
      pre.start([&, cur]() { load_pair(bts[cur ^ 1]); });
    }
    total_pairs += n;
    reserve_records(pr, pr_cap, n);
    t0 = now_s();
    // the best pair's two candidates come back inside walt_pair_result (m1/m2), so the ranked lists stay on the GPU
    vector<uint64_t> short1(dev.size(), 0), short2(dev.size(), 0);
    cs.start_batch(o, bt, adaptors, rp, T);
    auto map_share = [&](size_t d, uint32_t lo, uint32_t hi) {
      walt_batch_stats bs[2];
      const int rc = rp ? walt_map_pe_rpbat_batch(dev.idx[d], bt[0].bases, bt[0].offsets + lo, bt[1].bases, bt[1].offsets + lo,
                                                  hi - lo, o.max_mismatches, o.b, o.top_k, o.frag_range, pr + lo,
                                                  cs.conv.data() + 2 * (size_t)lo, bs)
                        : walt_map_pe_batch(dev.idx[d], bt[0].bases, bt[0].offsets + lo, bt[1].bases, bt[1].offsets + lo, hi - lo,
                                            o.max_mismatches, o.b, o.top_k, o.frag_range, pr + lo, nullptr, nullptr, nullptr, nullptr, bs);
      short1[d] = bs[0].too_short;
      short2[d] = bs[1].too_short;
      return rc;
    };
    // Slot 0 was mapped C->T, slot 1 G->A (-RP: as conv says).  -F -FC -FP: first the verdicts of the share's two slots and
    // the pair rule over them, ORed into the skip bytes beside -D's.  -NO: then the share's intervals, from the records in
    // user order.  Then the calls of both slots.
    auto meth_share = [&](size_t d, uint32_t lo, uint32_t hi) {
      int rc = WALT_OK;
      SlotView v[2] = {cs.view(o, d, lo, 0, bt[0], &pr[lo].m1, sizeof(walt_pair_result), rp, 'T', trim_slot[0]),
                       cs.view(o, d, lo, 1, bt[1], &pr[lo].m2, sizeof(walt_pair_result), rp, 'A', trim_slot[1])};
      if (cs.flt.on()) {
        for (int k = 0; k < 2 && rc == WALT_OK; ++k) rc = cs.call_slot(d, hi - lo, v[k], &cs.flt.rule);
        if (rc == WALT_OK) rc = walt_nonconv_pairs_batch(dev.idx[d], pr + lo, hi - lo, cs.flt.filt.data() + 2 * (size_t)lo);
        if (rc != WALT_OK) return rc;
        cs.flt.merge(2 * (size_t)lo, 2 * (size_t)hi, cs.dup_bytes());
      }
      if (o.no_overlap) {
        const int u1 = user_slot[0];
        vector<walt_pair_result> user;  // -P: mate 1 of the records is the user's mate 2
        if (pbat) {
          user.assign(pr + lo, pr + hi);
          for (walt_pair_result& p : user) std::swap(p.m1, p.m2);
        }
        // (with ignored read ends, mate 1's called span is what they leave of it; mate 2's enter the second total)
        rc = walt_pair_overlap_batch_trim(dev.idx[d], pbat ? user.data() : pr + lo, bt[u1].offsets + lo, bt[over_slot].offsets + lo, hi - lo,
                                          v[u1].clip, v[over_slot].clip, cs.excl.data() + lo, &cs.overlap_of[2 * d], o.ignore[0],
                                          o.ignore[1], o.ignore[2], o.ignore[3]);
        v[over_slot].excl = cs.excl.data() + lo;
      }
      for (int k = 0; k < 2 && rc == WALT_OK; ++k) rc = cs.call_slot(d, hi - lo, v[k], nullptr);
      return rc;
    };
    run_batch(cs, n, map_share, [&]() { cs.dups.feed_pe(pr, rp ? cs.conv.data() : nullptr, n); }, meth_share);
    if (cs.flt.on()) cs.flt.count_pe(pr, cs.dup_bytes(), n);
    for (size_t d = 0; d < dev.size(); ++d) { st1.too_short += (uint32_t)short1[d]; st2.too_short += (uint32_t)short2[d]; }
    t_map += now_s() - t0;
    if (!more) unlock_idle.start([&, cur]() { bts[cur ^ 1][0].release(); bts[cur ^ 1][1].release(); });
    t0 = now_s();
#pragma omp parallel for schedule(static, 1) num_threads(T)
    for (int t = 0; t < T; ++t) {
      Sink* s = &sinks[(size_t)t * kSinks];
      for (int k = 0; k < kSinks; ++k) s[k].clear();
      PeAcc a;
      a.frag_count.assign(o.frag_range + 1, 0);
      const uint32_t lo = (uint32_t)((uint64_t)n * t / T), hi = (uint32_t)((uint64_t)n * (t + 1) / T);
      for (uint32_t j = lo; j < hi; ++j) {  // MergePairedEndResults tail, paired.cpp:515-569
        const walt_pair_result& p = pr[j];
        const View name = bt[name_slot].name(j), q1 = bt[0].seq(j), k1 = bt[0].score(j), q2 = bt[1].seq(j), k2 = bt[1].score(j);
        walt_best_match bm1 = {0, 0, '+', {0, 0, 0}, o.max_mismatches}, bm2 = bm1;
        bool is_paired = false;
        int len = 0;
        const bool ag1 = rp && cs.conv[2 * (size_t)j] == 'A', ag2 = !rp || cs.conv[2 * (size_t)j + 1] == 'A';
        // -D: a duplicate's MR line is not written (the one fragment line of a duplicate pair), its SAM lines get 0x400
        const bool dup1 = cs.dups.on() && cs.dups.dup[2 * (size_t)j], dup2 = cs.dups.on() && cs.dups.dup[2 * (size_t)j + 1];
        // -F -FC -FP: the same for a filtered record, with 0x200 (a unique pair's two bytes are equal: the pair rule)
        const bool gone1 = cs.flt.on() && cs.flt.filt[2 * (size_t)j], gone2 = cs.flt.on() && cs.flt.filt[2 * (size_t)j + 1];
        if (p.best_times == 1) {
          a.unique_pairs++;
          walt_candidate r1 = {p.m1.genome_pos, p.m1.strand, {0, 0, 0}, p.m1.mismatch};
          walt_candidate r2 = {p.m2.genome_pos, p.m2.strand, {0, 0, 0}, p.m2.mismatch};
          if (ag1)  // -RP rule 3: the fragment of the mate-exchanged orientation, written from the T-rich mate 2 as -P writes it
            len = put_fragment(r2, r1, o.frag_range, g, name, q2, k2, q1, k1, o.sam || dup1 || gone1, s[kMain]);
          else
            len = put_fragment(r1, r2, o.frag_range, g, name, q1, k1, q2, k2, o.sam || dup1 || gone1, s[kMain]);
          a.frag_count[len]++;
          if (o.sam) { is_paired = true; bm1 = p.m1; bm2 = p.m2; }
        } else {
          if (p.best_times >= 2) a.ambiguous_pairs++; else a.unmapped_pairs++;
          bm1 = p.m1; bm2 = p.m2;
          a.st1.update(bm1.times);
          a.st2.update(bm2.times);
          if (!o.sam && !pbat) {  // (-RP: each mate by the writer of its conversion)
            if (!dup1 && !gone1) out_single_results(bm1, name, q1, k1, g, ag1, side1.out_amb, side1.out_unm, s[kMain], s[kAmb1], s[kUnm1]);
            if (!dup2 && !gone2) out_single_results(bm2, name, q2, k2, g, ag2, side2.out_amb, side2.out_unm, s[kMain], s[kAmb2], s[kUnm2]);
          } else if (!o.sam) {  // the user's mate 1 sits in slot 1
            if (!dup2 && !gone2) out_single_results(bm2, name, q2, k2, g, true, side1.out_amb, side1.out_unm, s[kMain], s[kAmb1], s[kUnm1]);
            if (!dup1 && !gone1) out_single_results(bm1, name, q1, k1, g, false, side2.out_amb, side2.out_unm, s[kMain], s[kAmb2], s[kUnm2]);
          }
        }
        if (o.sam) {
          int fl1 = sam_flag(is_paired, bm1.times == 0, bm2.times == 0, bm1.strand == '-', bm2.strand == '-', !pbat, bm1.times >= 2);
          int fl2 = sam_flag(is_paired, bm2.times == 0, bm1.times == 0, bm2.strand == '-', bm1.strand == '-', pbat, bm2.times >= 2);
          fl1 += (dup1 ? 0x400 : 0) + (gone1 ? 0x200 : 0);
          fl2 += (dup2 ? 0x400 : 0) + (gone2 ? 0x200 : 0);
          out_paired_sam(bm1, bm2, g, name, q1, k1, q2, k2, len, fl1, fl2, o.ambiguous, o.unmapped, pbat, s[kMain],
                         rp ? (ag1 ? "\tCV:A:A" : "\tCV:A:T") : nullptr, rp ? (ag2 ? "\tCV:A:A" : "\tCV:A:T") : nullptr,
                         o.meth ? View{cs.calls[0].data() + bt[0].offsets[j], q1.len} : View{nullptr, 0},
                         o.meth ? View{cs.calls[1].data() + bt[1].offsets[j], q2.len} : View{nullptr, 0});
        }
      }
      acc[t] = std::move(a);
    }
    for (int t = 0; t < T; ++t) {
      st1.add(acc[t].st1);
      st2.add(acc[t].st2);
      unique_pairs += acc[t].unique_pairs; ambiguous_pairs += acc[t].ambiguous_pairs; unmapped_pairs += acc[t].unmapped_pairs;
      for (size_t i = 0; i < frag_count.size(); ++i) frag_count[i] += acc[t].frag_count[i];
    }
    fout.write_sinks(sinks, kSinks, kMain, T);
    side1.amb.write_sinks(sinks, kSinks, kAmb1, T);
    side1.unm.write_sinks(sinks, kSinks, kUnm1, T);
    side2.amb.write_sinks(sinks, kSinks, kAmb2, T);
    side2.unm.write_sinks(sinks, kSinks, kUnm2, T);
    t_out += now_s() - t0;
    if (!more) { unlock_idle.wait(); break; }
    t0 = now_s();
    pre.wait();
    t_load += now_s() - t0;
  }
  rd[0].close(); rd[1].close();
  fout.close();
  side1.close(); side2.close();
  walt_host_free(pr);
  {  // the block StatPairedReads prints (paired.cpp:52-77): pair counters, one mate block each, the fragment histogram
    Sink ms;
    char num[48];
    ms.lit("pairs:\n    total_read_pairs: "); ms.u32(total_pairs);
    ms.lit("\n    mapped:\n        unique: "); ms.u32(unique_pairs);
    snprintf(num, sizeof num, "%g", (100.0 * unique_pairs) / total_pairs);
    ms.lit("\n        percent_unique: "); ms.lit(num);
    ms.lit("\n        ambiguous: "); ms.u32(ambiguous_pairs);
    ms.lit("\n    unmapped: "); ms.u32(unmapped_pairs);
    ms.lit("\nmate1:\n"); (pbat ? st2 : st1).put_block(ms, 1);
    ms.lit("\nmate2:\n"); (pbat ? st1 : st2).put_block(ms, 1);
    ms.lit("\nfrag_len_distribution:\n");
    double weighted = 0.0, pairs_in_hist = 0.0;
    for (size_t i = 0; i < frag_count.size(); ++i) {
      ms.lit("    "); ms.u32((uint32_t)i); ms.lit(": "); ms.u32(frag_count[i]); ms.ch('\n');
      weighted += (double)i * frag_count[i];
      pairs_in_hist += frag_count[i];
    }
    snprintf(num, sizeof num, "%g", weighted / pairs_in_hist);
    ms.lit("frag_len_mean: "); ms.lit(num); ms.ch('\n');
    Append(out_file, kMapstats).write(ms);
  }
  cs.finish(o, out_file, g, user_slot);  // in the user's order
  dev.close();
  if (o.verbose)
    fprintf(stderr, "[walt_amd: %d host threads, %zu GPU(s); index %.2f s, ingest not hidden behind the previous batch %.2f s, map %.2f s, "
            "output %.2f s]\n", T, dev.size(), t_index, t_load, t_map, t_out);
  if (last_file) leave_now(o.verbose);
}

int main(int argc, const char** argv) {
  g_t_main = now_s();
  try {
    if (argc == 1) {
      fprintf(stderr, "Usage: walt -i <index> -r <reads> | -1 <reads1> -2 <reads2> -o <out> [-m -N -a -u -C -A -P -R -RP -M -MC -ML -MR <bed> -D -NO -MB -MA -ME -MEN <n> -MV -MVD <n> -MVP <p> -MS -MSN <name> -MSR <r> -MSA <a> -MSD <n> -MQ <n> -MQO <b> -I5 <n> -I3 <n> -I5R2 <n> -I3R2 <n> -F <n> -FC <n> -FP <p> -FM <m> -b -k -L -sam -v -t -g <gpu>[,<gpu>...]]\n");
      return EXIT_SUCCESS;
    }
    Options o = parse(argc, argv);
    if (o.regions()) g_regions.read(o.regions_file);  // refused before anything is opened or truncated
    setenv("GPU_MAX_HW_QUEUES", "8", 0);  // paired-end keeps several streams busy; read by the HIP runtime at start-up
    static const char* sfx[5] = {"", "_CT00", "_CT01", "_GA10", "_GA11"};  // validate_index_file, walt.cpp:67-85
    for (const char* s : sfx) if (!exists(o.index_file + s)) die("index file missing: " + o.index_file + s);
    vector<string> se = split_csv(o.se_csv), p1 = split_csv(o.pe1_csv), p2 = split_csv(o.pe2_csv);
    for (auto& f : se) if (!valid_suffix(f)) die("read file invalid suffix: " + f);
    if (p1.size() != p2.size()) die("unequal number of end1 and end2 files");
    for (auto& f : p1) if (!valid_suffix(f)) die("read file invalid suffix: " + f);
    for (auto& f : p2) if (!valid_suffix(f)) die("read file invalid suffix: " + f);
    vector<string> outs = split_csv(o.out_csv);
    if (outs.size() != 1 && outs.size() != se.size() + p1.size()) die("wrong number of output files: " + o.out_csv);
    if (outs.size() == 1) outs.assign(se.size() + p1.size(), outs[0]);
    for (auto& f : outs) { std::ofstream out(f); }  // walt.cpp:230-233
    for (const auto& side : kOutput)
      if (side.on(o)) for (auto& f : outs) { std::ofstream stat(f + side.suffix); }
    if (o.batch_size > 100000000) die("batch size may not exceed100000000");
    if (o.top_k < 2 || o.top_k > 300) die("paired-end candidates must be in [2, 300]");
    size_t k = 0;
    const size_t n_files = se.size() + p1.size();
    for (auto& f : se) { process_se(o, f, outs[k], k + 1 == n_files); ++k; }
    for (size_t i = 0; i < p1.size(); ++i) { process_pe(o, p1[i], p2[i], outs[k], k + 1 == n_files); ++k; }
    if (o.verbose) fprintf(stderr, "[walt_amd: %.2f s in main]\n", now_s() - g_t_main);
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
