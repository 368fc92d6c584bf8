// hostio.h -- multi-threaded FASTQ ingest and output assembly for the walt
// driver.  The reference loads and prints serially (mapping.cpp:65-121,
// 329-419); at GPU mapping rates that is the whole run time, so the driver
// splits both sides over host threads while keeping every byte the reference
// would produce:
//   * batch boundaries, blank-line skipping, "drop the last character of every
//     fgets line" and name cutting follow LoadReadsFromFastqFile line by line;
//   * the N -> rand()%4 draws (util.hpp:156-163, srand(0) per batch,
//     mapping.cpp:73) are applied by ONE thread in file order after the
//     parallel copy has listed the characters that need one;
//   * a line of 999+ bytes, which fgets would split, makes the SAME scanner run over the
//     rest of the file as one chunk on one thread with the split rule applied; a file
//     that cannot be mmapped (a pipe) is read into memory first and scanned there.
#ifndef WALT_AMD_HOSTIO_H_
#define WALT_AMD_HOSTIO_H_
#include <fcntl.h>
#include <math.h>
#include <omp.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/walt_amd.h"

// Read / offset buffers come from the library's page-locked allocator; the CPU
// test harness (tests/hostio_harness.cpp) substitutes malloc to run without a GPU.
#ifndef HOSTIO_ALLOC
#define HOSTIO_ALLOC(bytes, out) walt_host_alloc((bytes), (out))
#define HOSTIO_FREE(p) walt_host_free(p)
#define HOSTIO_ALLOC_ERROR() walt_last_error()
#endif

namespace hostio {

static const uint32_t kMaxLine = 1000;  // MAX_LINE_LENGTH, util.hpp:43

struct View {
  const char* p;
  uint32_t len;
};

// ---------------------------------------------------------------- output buffers
struct Sink {
  char* p = nullptr;
  size_t n = 0, cap = 0;
  Sink() {}
  Sink(const Sink&) = delete;
  Sink& operator=(const Sink&) = delete;
  ~Sink() { free(p); }
  void clear() { n = 0; }
  char* grow(size_t add) {
    if (n + add > cap) {
      size_t nc = std::max(cap * 2, n + add + 4096);
      char* q = static_cast<char*>(realloc(p, nc));
      if (!q) throw std::bad_alloc();
      p = q;
      cap = nc;
    }
    return p + n;
  }
  void put(const char* s, size_t len) { memcpy(grow(len), s, len); n += len; }
  void put(const std::string& s) { put(s.data(), s.size()); }
  void put(View v) { put(v.p, v.len); }
  void lit(const char* s) { put(s, strlen(s)); }
  void ch(char c) { *grow(1) = c; n += 1; }
  void u32(uint32_t v) {
    char tmp[12];
    int k = 0;
    do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    char* q = grow(k);
    for (int i = 0; i < k; ++i) q[i] = tmp[k - 1 - i];
    n += k;
  }
  void i32(int v) {
    if (v < 0) { ch('-'); u32((uint32_t)(-(int64_t)v)); } else u32((uint32_t)v);
  }
  // reversed / reverse-complemented copies (revcomp as in smithlab_utils, used at mapping.cpp:337,393)
  void rev(View v) {
    char* q = grow(v.len);
    for (uint32_t i = 0; i < v.len; ++i) q[i] = v.p[v.len - 1 - i];
    n += v.len;
  }
  void revcomp(View v) {
    char* q = grow(v.len);
    for (uint32_t i = 0; i < v.len; ++i) {
      char c = v.p[v.len - 1 - i];
      q[i] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
    }
    n += v.len;
  }
};

// An output file written at explicit offsets so that per-thread buffers can be
// stored concurrently and still land in read order.
struct OutFile {
  int fd = -1;
  off_t pos = 0;
  bool open_append(const std::string& path) {  // fopen(path, "a") of the reference (mapping.cpp:460)
    fd = ::open(path.c_str(), O_WRONLY | O_CREAT, 0666);
    if (fd < 0) return false;
    pos = lseek(fd, 0, SEEK_END);
    return true;
  }
  bool open_trunc(const std::string& path) {  // fopen(path, "w") (mapping.hpp:75-87)
    fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    pos = 0;
    return fd >= 0;
  }
  void close() { if (fd >= 0) ::close(fd); fd = -1; }
  static void pwrite_all(int fd, const char* p, size_t len, off_t at) {
    while (len) {
      ssize_t w = ::pwrite(fd, p, len, at);
      if (w < 0) throw std::runtime_error("write failed");
      p += w; len -= (size_t)w; at += w;
    }
  }
  void write(const char* p, size_t len) { pwrite_all(fd, p, len, pos); pos += (off_t)len; }
  // sinks[t * stride + which] for t in [0, T): stored in thread order.  (Growing the file and copying into a shared
  // mapping of the new part, to get around the inode lock pwrite calls on one file take turns on, was tried: the page
  // faults of a tmpfs mapping cost more than the lock -- 2.95 s against 1.41 s for 10 GB.)
  void write_sinks(std::vector<Sink>& sinks, size_t stride, size_t which, int threads) {
    if (fd < 0) return;
    const size_t T = sinks.size() / stride;
    std::vector<off_t> at(T + 1, pos);
    for (size_t t = 0; t < T; ++t) at[t + 1] = at[t] + (off_t)sinks[t * stride + which].n;
    bool failed = false;
#pragma omp parallel for schedule(static, 1) num_threads(threads)
    for (long t = 0; t < (long)T; ++t) {
      const Sink& s = sinks[t * stride + which];
      try { if (s.n) pwrite_all(fd, s.p, s.n, at[t]); } catch (...) { failed = true; }
    }
    if (failed) throw std::runtime_error("write failed");
    pos = at[T];
  }
};

// ---------------------------------------------------------------- read batches
struct Batch {
  uint32_t n = 0;
  const char* base = nullptr;            // the input file's bytes (mapped, or read into memory)
  std::vector<uint64_t> name_v, score_v, seq_v;  // (offset << 16) | length
  char* bases = nullptr;                 // sanitised sequences, packed; pinned host memory
  uint64_t* offsets = nullptr;           // n + 1
  // -MQ only: the quality bytes of the sequences as the file has them, packed at the offsets of `bases`; pinned host
  // memory (include/walt_amd.h, "minimum base quality").  Null without -MQ: no allocation, no copy.
  char* quals = nullptr;
  size_t bases_cap = 0, off_cap = 0, quals_cap = 0;
  Batch() {}
  Batch(const Batch&) = delete;
  Batch& operator=(const Batch&) = delete;
  ~Batch() { release(); }
  // give the page-locked buffers back (unlocking a gigabyte takes ~0.2 s: the driver does it on a helper thread while
  // the last batch is formatted and written, walt_main.cpp)
  void release() {
    HOSTIO_FREE(bases); HOSTIO_FREE(offsets);
    if (quals) HOSTIO_FREE(quals);
    bases = nullptr; offsets = nullptr; quals = nullptr;
    bases_cap = off_cap = quals_cap = 0;
    n = 0;
  }
  static uint64_t pack(size_t off, size_t len) { return ((uint64_t)off << 16) | (uint64_t)len; }
  View name(uint32_t j) const { return View{base + (name_v[j] >> 16), (uint32_t)(name_v[j] & 0xFFFF)}; }
  View score(uint32_t j) const { return View{base + (score_v[j] >> 16), (uint32_t)(score_v[j] & 0xFFFF)}; }
  View seq(uint32_t j) const { return View{bases + offsets[j], (uint32_t)(offsets[j + 1] - offsets[j])}; }
  void reserve_reads(size_t reads) {
    if (name_v.size() < reads) { name_v.resize(reads); score_v.resize(reads); seq_v.resize(reads); }
    if (off_cap < reads + 1) {
      HOSTIO_FREE(offsets);
      offsets = nullptr;
      off_cap = reads + 1;
      if (HOSTIO_ALLOC(off_cap * sizeof(uint64_t), (void**)&offsets) != 0) throw std::runtime_error(HOSTIO_ALLOC_ERROR());
    }
  }
  void reserve_bases(size_t bytes) {
    if (bases_cap < bytes + 16) {
      HOSTIO_FREE(bases);
      bases = nullptr;
      bases_cap = bytes + bytes / 8 + 4096;
      if (HOSTIO_ALLOC(bases_cap, (void**)&bases) != 0) throw std::runtime_error(HOSTIO_ALLOC_ERROR());
    }
  }
  void reserve_quals(size_t bytes) {
    if (quals_cap < bytes + 16) {
      if (quals) HOSTIO_FREE(quals);
      quals = nullptr;
      quals_cap = bytes + bytes / 8 + 4096;
      if (HOSTIO_ALLOC(quals_cap, (void**)&quals) != 0) throw std::runtime_error(HOSTIO_ALLOC_ERROR());
    }
  }
};

// ---------------------------------------------------------------- adaptor clipping (-C)
// What util.hpp:189-218 decides, stated per start position: the read's tail from `at` on is taken for adaptor
// when, of the first min(tail, adaptor, 14) characters of the adaptor, at least 11 agree with it (tails of 14
// bases or more), or all but one of the whole tail do (tails of 13 down to 5 bases).  Returns the first such
// `at`, or the read's length when there is none; the caller writes 'N' from there on (the loader then draws
// random bases for them like for any other non-ACGT character).
// The reference computes its loop bounds as size_t differences, which wrap for reads of fewer than 13 bases and
// send it reading far outside the string (it crashes: tests/test_hostio_cpu.py pins both sides of that limit
// against the reference binary); such reads are left alone here.
static const uint32_t kAdaptorHead = 14, kAdaptorHeadHits = 11, kAdaptorMinTail = 5;
inline uint32_t adaptor_clip_point(View read, View adaptor) {
  if (read.len < kAdaptorHead - 1) return read.len;
  for (uint32_t at = 0; at + kAdaptorMinTail <= read.len; ++at) {
    const uint32_t tail = read.len - at;
    const uint32_t window = std::min(std::min(tail, adaptor.len), kAdaptorHead);
    const uint32_t need = tail >= kAdaptorHead ? kAdaptorHeadHits : tail - 1;
    if (window < need) continue;
    uint32_t hits = 0;
    for (uint32_t k = 0; k < window; ++k) hits += read.p[at + k] == adaptor.p[k] ? 1u : 0u;
    if (hits >= need) return at;
  }
  return read.len;
}

inline bool is_acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// CPUs this process may actually use: the affinity mask, capped by the cgroup CPU
// quota (containers often expose every core of the host but grant far fewer;
// running more threads than the quota only gets them throttled).
inline int effective_cpus() {
  int n = omp_get_num_procs();
  long long quota = -1, period = 100000;
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
    char q[64];
    if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
    fclose(f);
  } else {
    FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r");
    FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
    if (fq && fp && fscanf(fq, "%lld", &quota) == 1 && fscanf(fp, "%lld", &period) == 1) {}
    if (fq) fclose(fq);
    if (fp) fclose(fp);
  }
  if (quota > 0 && period > 0) {
    int c = (int)((quota + period - 1) / period);
    if (c >= 1 && c < n) n = c;
  }
  return n < 1 ? 1 : n;
}

inline double now_s() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

struct FastqReader {
  bool want_quals = false;  // -MQ: every batch gets its packed quality buffer (Batch::quals)
  double t_scan = 0, t_views = 0, t_alloc = 0, t_copy = 0, t_rng = 0;  // -v breakdown
  std::string path;
  const char* data = nullptr;
  size_t size = 0, pos = 0;
  bool mapped = false;
  std::vector<char> slurped;  // contents of an input that cannot be mmapped
  bool serial = false;        // a long line was met: one chunk, one thread from there on (kept for the tests)
  int threads = 1;

  void open(const std::string& p, int nthreads) {
    path = p;
    threads = std::max(1, nthreads);
    int fd = ::open(p.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("cannot open input file " + p);
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && !getenv("WALT_AMD_SERIAL_IO")) {
      void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m != MAP_FAILED) {
        data = static_cast<const char*>(m);
        size = (size_t)st.st_size;
        mapped = true;
        madvise(m, size, MADV_SEQUENTIAL);
      }
    }
    if (!data) {  // pipe, empty file, or WALT_AMD_SERIAL_IO (tests): read it all, then scan the copy on one thread
      char buf[1 << 16];
      for (;;) {
        const ssize_t got = ::read(fd, buf, sizeof buf);
        if (got < 0) { ::close(fd); throw std::runtime_error("cannot read input file " + p); }
        if (got == 0) break;
        slurped.insert(slurped.end(), buf, buf + got);
      }
      data = slurped.data();
      size = slurped.size();
      serial = true;
    }
    ::close(fd);
  }
  void close() {
    if (mapped) munmap(const_cast<char*>(data), size);
    data = nullptr;
    mapped = false;
    slurped.clear();
  }

  // ---- one fgets(cline, 1000, f) call of the reference (mapping.cpp:81) starting at s: the bytes [s, e) it returns --
  // up to and including the next newline, but never more than 999 of them
  inline size_t line_end(size_t s) const {
    const size_t lim = std::min(size, s + (kMaxLine - 1));
    const void* nl = memchr(data + s, '\n', lim - s);
    return nl ? (size_t)(static_cast<const char*>(nl) - data) + 1 : lim;
  }
  // first line start at or behind a chunk boundary (only used while no line is long enough to be split)
  inline size_t first_line_at_or_after(size_t a, size_t batch_start) const {
    if (a <= batch_start) return batch_start;
    if (a >= size) return size;
    if (data[a - 1] == '\n') return a;
    const void* nl = memchr(data + a, '\n', size - a);
    return nl ? (size_t)(static_cast<const char*>(nl) - data) + 1 : size;
  }

  // LoadReadsFromFastqFile, mapping.cpp:65-121
  void load(uint32_t n_per_batch, const std::string& adaptor, Batch& bt) {
    const uint64_t lim = (uint64_t)n_per_batch * 4;
    const size_t start = pos;
    bt.n = 0;
    bt.base = data;
    if (start >= size || lim == 0) { finish_sequences(adaptor, bt); return; }
    double tm = now_s();
    std::vector<uint64_t> lines;  // non-empty lines that start in each chunk
    uint64_t total = 0;
    size_t covered = start, chunk = 1u << 20;
    for (;;) {
      // pass 1: count lines per chunk, in waves of chunks until `lim` lines or the end of the file
      const int T = serial ? 1 : threads;
      if (serial) chunk = size - start + 1;  // one chunk: the scan follows the split rule from the batch's first byte
      lines.clear();
      total = 0;
      covered = start;
      bool long_line = false;
      size_t wave = 1;  // 1, 2, 4, ... chunks per wave: a small -N must not scan far beyond its batch
      while (total < lim && covered < size) {
        const size_t first = lines.size();
        const size_t want = std::min<size_t>((size - covered + chunk - 1) / chunk, wave);
        wave = std::min<size_t>(wave * 2, (size_t)T * 4);
        lines.resize(first + want, 0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(T) reduction(|| : long_line)
        for (long c = 0; c < (long)want; ++c) {
          const size_t a = start + (first + c) * chunk, b = std::min(a + chunk, size);
          size_t s = first_line_at_or_after(a, start);
          uint64_t cnt = 0;
          const uint64_t stop = (first + c == 0) ? lim : ~0ull;  // the batch's first chunk may stop at `lim` lines
          while (s < b && cnt < stop) {
            const size_t e = line_end(s);
            if (e - s >= kMaxLine - 1 && data[e - 1] != '\n') long_line = true;  // fgets filled its buffer: the line goes on
            cnt += (e - s) > 1;  // the piece minus its last character is non-empty (mapping.cpp:82-85)
            s = e;
          }
          lines[first + c] = cnt;
        }
        for (size_t c = first; c < first + want; ++c) total += lines[c];
        covered = std::min(size, start + (first + want) * chunk);
      }
      if (!long_line || serial) break;
      serial = true;  // chunk starts are not piece starts once a line is split: scan again as one chunk
    }
    t_scan += now_s() - tm;
    tm = now_s();
    const uint64_t use = std::min<uint64_t>(total, lim);
    bt.n = (uint32_t)(use / 4);  // a record counts when its 4th line has been read (mapping.cpp:110-113)
    bt.reserve_reads(bt.n + 1);
    std::vector<uint64_t> first_line(lines.size() + 1, 0);
    for (size_t c = 0; c < lines.size(); ++c) first_line[c + 1] = first_line[c] + lines[c];
    // pass 2: record name / sequence / quality views; line L belongs to read L/4, role L%4
    size_t next_pos = covered;
    const uint64_t n_lines_used = (uint64_t)bt.n * 4;
#pragma omp parallel for schedule(dynamic, 1) num_threads(serial ? 1 : threads)
    for (long c = 0; c < (long)lines.size(); ++c) {
      uint64_t L = first_line[c];
      if (L >= lim) continue;
      const size_t a = start + (size_t)c * chunk, b = std::min(a + chunk, size);
      size_t s = first_line_at_or_after(a, start);
      while (s < b) {
        const size_t e = line_end(s);
        const size_t len = e - s - 1;  // content after dropping the last character
        s = e;
        if (len == 0) continue;
        if (L < n_lines_used) {
          const uint32_t r = (uint32_t)(L >> 2);
          const size_t at = e - 1 - len;
          switch (L & 3) {
            case 0: {  // name: up to the first space, without the leading character (mapping.cpp:87-95)
              const void* sp = memchr(data + at, ' ', len);
              size_t cut = sp ? (size_t)(static_cast<const char*>(sp) - (data + at)) : len;
              if (sp && cut == 0) cut = len;  // substr(1, 0 - 1): the unsigned wrap keeps the whole rest
              bt.name_v[r] = Batch::pack(at + 1, cut - 1);
              break;
            }
            case 1: bt.seq_v[r] = Batch::pack(at, len); break;
            case 3: bt.score_v[r] = Batch::pack(at, len); break;
            default: break;
          }
        }
        ++L;
        if (L == lim) {
#pragma omp critical(walt_next_pos)
          next_pos = e;
          break;
        }
      }
    }
    pos = total >= lim ? next_pos : size;
    t_views += now_s() - tm;
    finish_sequences(adaptor, bt);
  }

  // sequences: copy into the packed buffer, clip, and give non-ACGT characters their rand()%4 in file order
  void finish_sequences(const std::string& adaptor, Batch& bt) {
    const uint32_t n = bt.n;
    bt.reserve_reads(n + 1);
    const int T = threads;
    const View ad{adaptor.data(), (uint32_t)adaptor.size()};
    std::vector<uint64_t> part(T + 1, 0);
    auto lo_of = [&](int t) { return (uint32_t)((uint64_t)n * t / T); };
#pragma omp parallel for schedule(static, 1) num_threads(T)
    for (int t = 0; t < T; ++t) {
      uint64_t sum = 0;
      for (uint32_t j = lo_of(t); j < lo_of(t + 1); ++j) sum += bt.seq_v[j] & 0xFFFF;
      part[t + 1] = sum;
    }
    for (int t = 0; t < T; ++t) part[t + 1] += part[t];
    double tm = now_s();
    bt.reserve_bases(part[T]);
    if (want_quals) bt.reserve_quals(part[T]);
    t_alloc += now_s() - tm;
    tm = now_s();
    std::vector<std::vector<uint64_t>> fix(T);
    std::vector<uint32_t> bad_qual(T, ~0u);  // -MQ: per thread, its first read whose quality line has another length
#pragma omp parallel for schedule(static, 1) num_threads(T)
    for (int t = 0; t < T; ++t) {
      uint64_t o = part[t];
      for (uint32_t j = lo_of(t); j < lo_of(t + 1); ++j) {
        const char* src = bt.base + (bt.seq_v[j] >> 16);
        const uint32_t len = (uint32_t)(bt.seq_v[j] & 0xFFFF);
        bt.offsets[j] = o;
        // -C: the adaptor part becomes 'N' (mapping.cpp:97-99), i.e. one more kind of character that needs a draw
        const uint32_t keep = ad.len ? adaptor_clip_point(View{src, len}, ad) : len;
        char* dst = bt.bases + o;
        for (uint32_t i = 0; i < len; ++i) {
          const char c = i < keep ? src[i] : 'N';
          dst[i] = c;
          if (!is_acgt(c)) fix[t].push_back(o + i);
        }
        // the qualities stay where they are, also behind a clip point: a clipped base is an 'N' with the quality it had
        if (want_quals) {
          if ((uint32_t)(bt.score_v[j] & 0xFFFF) == len) memcpy(bt.quals + o, bt.base + (bt.score_v[j] >> 16), len);
          else if (bad_qual[t] == ~0u) bad_qual[t] = j;
        }
        o += len;
      }
    }
    for (int t = 0; t < T; ++t)
      if (bad_qual[t] != ~0u) {
        const View name = bt.name(bad_qual[t]);
        throw std::runtime_error(path + ": read " + std::string(name.p, name.len) + ": the quality line has " +
                                 std::to_string(bt.score_v[bad_qual[t]] & 0xFFFF) + " characters, the sequence " +
                                 std::to_string(bt.seq_v[bad_qual[t]] & 0xFFFF) + " (-MQ reads a quality per base)");
      }
    bt.offsets[n] = part[T];
    t_copy += now_s() - tm;
    tm = now_s();
    srand(0);  // mapping.cpp:73
    for (int t = 0; t < T; ++t)
      for (uint64_t at : fix[t]) bt.bases[at] = "ACGT"[rand() % 4];  // toACGT, util.hpp:156-163
    t_rng += now_s() - tm;
  }
};

// ---------------------------------------------------------------- <out>.mbias (bin/walt -MB)
// One block of the methylation bias table (include/walt_amd.h, "methylation bias by read position"): count[4][2][1024]
// as walt_mbias_read returns it.  For each context in the order CpG, CHG, CHH, unknown, one line per position 1 .. L:
//   context <TAB> position (1-based) <TAB> methylated <TAB> unmethylated <TAB> level
// L = the highest position with a non-zero count in any context of the block (no line when there is none); the level is
// %.6f, or NA where both counts are 0, as <out>.methstats prints it.
static const uint32_t kMbiasPositions = 1024;
inline void put_mbias_block(Sink& out, const uint64_t* count) {
  static const char* ctx[4] = {"CpG", "CHG", "CHH", "unknown"};
  uint32_t L = 0;
  for (uint32_t cell = 0; cell < 8; ++cell)
    for (uint32_t i = L; i < kMbiasPositions; ++i)
      if (count[(size_t)cell * kMbiasPositions + i]) L = i + 1;
  char num[128];
  for (uint32_t c = 0; c < 4; ++c)
    for (uint32_t i = 0; i < L; ++i) {
      const unsigned long long m = count[(size_t)(2 * c) * kMbiasPositions + i], u = count[(size_t)(2 * c + 1) * kMbiasPositions + i];
      if (m + u) snprintf(num, sizeof num, "%s\t%u\t%llu\t%llu\t%.6f\n", ctx[c], i + 1, m, u, (double)m / ((double)m + (double)u));
      else snprintf(num, sizeof num, "%s\t%u\t%llu\t%llu\tNA\n", ctx[c], i + 1, m, u);
      out.lit(num);
    }
}

// ---------------------------------------------------------------- <out>.levels (bin/walt -ML)
// One read file's block (include/walt_amd.h, "methylation levels"): a header line and six lines, tab-separated:
//   context sites covered meth unmeth max_depth mean_depth covered_fraction mean_meth weighted_meth h0 .. h9
// for cytosines (rows 0..3 folded: sums, the maximum for max_depth), CpG, CHG, CHH, unknown and CpG_symmetric (row 4).
// mean_depth = (meth + unmeth) / sites, covered_fraction = covered / sites, mean_meth = level_sum / (covered * 2^30),
// weighted_meth = meth / (meth + unmeth); each %.6f, or NA on a zero denominator.
inline void put_levels_block(Sink& out, const walt_levels& lv) {
  static const char* name[6] = {"cytosines", "CpG", "CHG", "CHH", "unknown", "CpG_symmetric"};
  walt_level_row all;
  memset(&all, 0, sizeof all);
  for (int r = 0; r < 4; ++r) {
    const walt_level_row& x = lv.row[r];
    all.sites += x.sites; all.covered += x.covered; all.meth += x.meth; all.unmeth += x.unmeth; all.level_sum += x.level_sum;
    all.max_depth = std::max(all.max_depth, x.max_depth);
    for (int b = 0; b < 10; ++b) all.hist[b] += x.hist[b];
  }
  out.lit("context\tsites\tcovered\tmeth\tunmeth\tmax_depth\tmean_depth\tcovered_fraction\tmean_meth\tweighted_meth"
          "\th0\th1\th2\th3\th4\th5\th6\th7\th8\th9\n");
  char num[192];
  auto ratio = [&](double a, double b) {
    if (b != 0.0) snprintf(num, sizeof num, "\t%.6f", a / b); else snprintf(num, sizeof num, "\tNA");
    out.lit(num);
  };
  for (int k = 0; k < 6; ++k) {
    const walt_level_row& x = k == 0 ? all : lv.row[k - 1];
    snprintf(num, sizeof num, "%s\t%llu\t%llu\t%llu\t%llu\t%llu", name[k], (unsigned long long)x.sites, (unsigned long long)x.covered,
             (unsigned long long)x.meth, (unsigned long long)x.unmeth, (unsigned long long)x.max_depth);
    out.lit(num);
    ratio((double)(x.meth + x.unmeth), (double)x.sites);
    ratio((double)x.covered, (double)x.sites);
    ratio((double)x.level_sum, (double)x.covered * 1073741824.0);
    ratio((double)x.meth, (double)(x.meth + x.unmeth));
    for (int b = 0; b < 10; ++b) { snprintf(num, sizeof num, "\t%llu", (unsigned long long)x.hist[b]); out.lit(num); }
    out.ch('\n');
  }
}

// ---------------------------------------------------------------- <out>.regions (bin/walt -MR)
// The BED file of -MR (include/walt_amd.h, "methylation levels per region"): `chrom start end [name ...]`, 0-based and
// half-open, columns separated by tabs or blanks.  Empty lines and lines that start with '#', "track" or "browser"
// are skipped; a missing name is "."; further columns are ignored (a strand column restricts nothing).  Lines end in
// LF or CRLF; the last one needs neither.
struct BedRegion {
  std::string chrom, name;
  uint64_t start = 0, end = 0;
  uint32_t line = 0;  // 1-based line of the file
};
// digits only, below 2^63
inline bool parse_bed_number(const char* p, size_t len, uint64_t& out) {
  if (!len || len > 18) return false;
  uint64_t v = 0;
  for (size_t i = 0; i < len; ++i) {
    if (p[i] < '0' || p[i] > '9') return false;
    v = v * 10 + (uint64_t)(p[i] - '0');
  }
  out = v;
  return true;
}
// The regions of a BED text in the file's order.  false: `err` is "<file>:<line>: <what>" (line 0 for a text without
// any region).
inline bool parse_bed_text(const char* text, size_t len, const std::string& file, std::vector<BedRegion>& out, std::string& err) {
  out.clear();
  uint32_t line = 0;
  auto bad = [&](const std::string& what) { err = file + ":" + std::to_string(line) + ": " + what; out.clear(); return false; };
  for (size_t at = 0; at < len;) {
    size_t end = at;
    while (end < len && text[end] != '\n') ++end;
    size_t stop = end;
    if (stop > at && text[stop - 1] == '\r') --stop;
    const char* p = text + at;
    const size_t n = stop - at;
    at = end + 1;
    ++line;
    auto blank = [](char c) { return c == ' ' || c == '\t'; };
    auto starts = [&](const char* w) { const size_t k = strlen(w); return n >= k && !memcmp(p, w, k) && (n == k || blank(p[k])); };
    size_t i = 0;
    while (i < n && blank(p[i])) ++i;
    if (i == n || p[0] == '#' || starts("track") || starts("browser")) continue;
    View col[4];
    int n_col = 0;
    while (i < n && n_col < 4) {
      const size_t c0 = i;
      while (i < n && !blank(p[i])) ++i;
      col[n_col].p = p + c0; col[n_col].len = (uint32_t)(i - c0);
      ++n_col;
      while (i < n && blank(p[i])) ++i;
    }
    if (n_col < 3) return bad("a region needs three columns (chrom start end), this line has " + std::to_string(n_col));
    BedRegion r;
    if (!parse_bed_number(col[1].p, col[1].len, r.start)) return bad("start '" + std::string(col[1].p, col[1].len) + "' is not a number");
    if (!parse_bed_number(col[2].p, col[2].len, r.end)) return bad("end '" + std::string(col[2].p, col[2].len) + "' is not a number");
    if (r.start > r.end) return bad("start " + std::to_string(r.start) + " lies behind end " + std::to_string(r.end));
    r.chrom.assign(col[0].p, col[0].len);
    r.name = n_col > 3 ? std::string(col[3].p, col[3].len) : std::string(".");
    r.line = line;
    out.push_back(r);
  }
  line = 0;
  if (out.empty()) return bad("the file holds no region");
  return true;
}
inline bool read_bed_file(const std::string& file, std::vector<BedRegion>& out, std::string& err) {
  FILE* f = fopen(file.c_str(), "rb");
  if (!f) { err = file + ":0: cannot open the regions file"; return false; }
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
  const bool failed = ferror(f) != 0;
  fclose(f);
  if (failed) { err = file + ":0: cannot read the regions file"; return false; }
  return parse_bed_text(text.data(), text.size(), file, out, err);
}
// The forward ranges of the regions in a genome of n_chrom chromosomes (name[c], start[c] .. start[c + 1]).  A region
// on a chromosome the genome does not have becomes the empty range [0, 0) and is counted: it keeps its output line.
// false: a region ends beyond its chromosome, `err` as above.
inline bool resolve_bed(const std::vector<BedRegion>& bed, const std::vector<std::string>& name, const std::vector<uint32_t>& start,
                        const std::string& file, std::vector<walt_region>& regions, uint64_t& n_unknown, std::string& err) {
  std::vector<std::pair<std::string, uint32_t> > by_name;
  for (uint32_t c = 0; c < (uint32_t)name.size(); ++c) by_name.push_back(std::make_pair(name[c], c));
  std::sort(by_name.begin(), by_name.end());
  regions.assign(bed.size(), walt_region{0u, 0u});
  n_unknown = 0;
  for (size_t i = 0; i < bed.size(); ++i) {
    const BedRegion& r = bed[i];
    auto it = std::lower_bound(by_name.begin(), by_name.end(), std::make_pair(r.chrom, 0u));
    if (it == by_name.end() || it->first != r.chrom) { ++n_unknown; continue; }
    const uint32_t c = it->second;
    const uint64_t length = (uint64_t)start[c + 1] - start[c];
    if (r.end > length) {
      err = file + ":" + std::to_string(r.line) + ": end " + std::to_string(r.end) + " lies beyond the " + std::to_string(length) +
            " bases of " + r.chrom;
      return false;
    }
    regions[i].lo = start[c] + (uint32_t)r.start;
    regions[i].hi = start[c] + (uint32_t)r.end;
  }
  return true;
}
// One read file's block: a header line, then one line per region in the file's order, tab-separated:
//   chrom start end name, then for CpG, CHG, CHH, unknown and CpG_symmetric (rows 0..4):
//   <ctx>_sites <ctx>_covered <ctx>_meth <ctx>_unmeth <ctx>_mean_meth <ctx>_weighted_meth
// mean_meth = level_sum / (covered * 2^30) and weighted_meth = meth / (meth + unmeth) as put_levels_block computes
// them: %.6f, or NA on a zero denominator (every ratio of a region on an unknown chromosome).
inline void put_regions_block(Sink& out, const std::vector<BedRegion>& bed, const walt_region_levels* lv) {
  static const char* ctx[5] = {"CpG", "CHG", "CHH", "unknown", "CpG_symmetric"};
  static const char* col[6] = {"sites", "covered", "meth", "unmeth", "mean_meth", "weighted_meth"};
  out.lit("chrom\tstart\tend\tname");
  for (int r = 0; r < 5; ++r)
    for (int k = 0; k < 6; ++k) { out.ch('\t'); out.lit(ctx[r]); out.ch('_'); out.lit(col[k]); }
  out.ch('\n');
  char num[192];
  auto ratio = [&](double a, double b) {
    if (b != 0.0) snprintf(num, sizeof num, "\t%.6f", a / b); else snprintf(num, sizeof num, "\tNA");
    out.lit(num);
  };
  for (size_t i = 0; i < bed.size(); ++i) {
    out.put(bed[i].chrom);
    snprintf(num, sizeof num, "\t%llu\t%llu\t", (unsigned long long)bed[i].start, (unsigned long long)bed[i].end);
    out.lit(num);
    out.put(bed[i].name);
    for (int r = 0; r < 5; ++r) {
      const walt_region_row& x = lv[i].row[r];
      snprintf(num, sizeof num, "\t%u\t%u\t%llu\t%llu", x.sites, x.covered, (unsigned long long)x.meth, (unsigned long long)x.unmeth);
      out.lit(num);
      ratio((double)x.level_sum, (double)x.covered * 1073741824.0);
      ratio((double)x.meth, (double)(x.meth + x.unmeth));
    }
    out.ch('\n');
  }
}

// ---------------------------------------------------------------- ignored read ends (bin/walt -I5 -I3 -I5R2 -I3R2)
// The value of one of the four options (include/walt_amd.h, "ignored read ends"): a decimal integer from 0 to 1024
// (no read is longer), nothing in front of or behind the digits.
static const uint32_t kMaxIgnore = 1024;
inline bool parse_ignore_value(const std::string& text, uint32_t& out) {
  if (text.empty() || text.size() > 4) return false;
  uint32_t v = 0;
  for (const char c : text) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (uint32_t)(c - '0');
  }
  out = v;
  return v <= kMaxIgnore;
}
// The settings line that ends a read file's part of <out>.methstats when a bound is non-zero, in the user's order:
//   ignore <TAB> i5 <TAB> i3                              single-end (n = 2)
//   ignore <TAB> i5 <TAB> i3 <TAB> i5r2 <TAB> i3r2        paired (n = 4)
inline void put_ignore_line(Sink& out, const uint32_t* v, int n) {
  out.lit("ignore");
  for (int k = 0; k < n; ++k) { out.ch('\t'); out.u32(v[k]); }
  out.ch('\n');
}

// ---------------------------------------------------------------- minimum base quality (bin/walt -MQ -MQO)
// The value of -MQ: a Phred quality from 1 to 93 (the printable range above '!'), a decimal integer, nothing in front of
// or behind its digits.  The value of -MQO: the FASTQ's Phred offset, 33 or 64.  quality_floor: what the library compares
// the raw bytes with (include/walt_amd.h, "minimum base quality"), or false when it would exceed 127.
static const uint32_t kMaxMinQual = 93;
inline bool parse_min_qual(const std::string& text, uint32_t& out) {
  uint32_t v = 0;
  if (!parse_ignore_value(text, v) || v < 1 || v > kMaxMinQual) return false;
  out = v;
  return true;
}
inline bool parse_qual_offset(const std::string& text, uint32_t& out) {
  uint32_t v = 0;
  if (!parse_ignore_value(text, v) || (v != 33 && v != 64)) return false;
  out = v;
  return true;
}
inline bool quality_floor(uint32_t min_qual, uint32_t offset, uint32_t& out) {
  out = min_qual + offset;
  return out <= 127;
}
// The settings line that ends a read file's part of <out>.methstats under -MQ, behind the overlap and ignore lines:
//   minqual <TAB> n <TAB> offset
inline void put_minqual_line(Sink& out, uint32_t min_qual, uint32_t offset) {
  out.lit("minqual");
  out.ch('\t'); out.u32(min_qual);
  out.ch('\t'); out.u32(offset);
  out.ch('\n');
}

// ---------------------------------------------------------------- non-converted reads (bin/walt -F -FC -FP -FM)
// The value of one of the four options (include/walt_amd.h, "non-converted reads"): a decimal integer from lo to hi (at
// most four digits), nothing in front of or behind the digits.
inline bool parse_filter_value(const std::string& text, uint32_t lo, uint32_t hi, uint32_t& out) {
  uint32_t v = 0;
  if (!parse_ignore_value(text, v) || v < lo || v > hi) return false;
  out = v;
  return true;
}
// One read file's block of <out>.filterstats: the unique reads, unique pairs and lone unique mates that are not
// duplicates, those of them the rule filtered, the rate as %.6f (NA without records), and the rule's four fields:
//   rule <TAB> min_meth <TAB> min_run <TAB> min_percent <TAB> min_total
inline void put_filter_block(Sink& out, uint64_t records, uint64_t filtered, const uint32_t rule[4]) {
  char num[160];
  if (records) snprintf(num, sizeof num, "records: %llu\nfiltered: %llu\nfilter rate: %.6f\n", (unsigned long long)records,
                        (unsigned long long)filtered, (double)filtered / (double)records);
  else snprintf(num, sizeof num, "records: %llu\nfiltered: %llu\nfilter rate: NA\n", (unsigned long long)records, (unsigned long long)filtered);
  out.lit(num);
  out.lit("rule");
  for (int k = 0; k < 4; ++k) { out.ch('\t'); out.u32(rule[k]); }
  out.ch('\n');
}

// ---------------------------------------------------------------- <out>.allelic (bin/walt -MA)
// log(k!) through lgamma; the small arguments, which are nearly all there are, from a table filled once
inline double log_factorial(uint64_t k) {
  static const std::vector<double> small = [] {
    std::vector<double> t(4096);
    for (size_t i = 0; i < t.size(); ++i) t[i] = lgamma((double)i + 1.0);
    return t;
  }();
  return k < small.size() ? small[(size_t)k] : lgamma((double)k + 1.0);
}
// The two-sided Fisher exact test of the table [[a, b], [c, d]]: the sum of the hypergeometric probabilities of all
// tables with the same margins whose probability is at most P(observed) * (1 + 1e-7) -- the slack takes in the exact
// ties of a symmetric table, which differ in the last bits here -- capped at 1.  The empty table gives 1.  The work
// grows with the smaller margin.
inline double fisher_exact_two_sided(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  const uint64_t r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d, n = r1 + r2;
  if (!n) return 1.0;
  const uint64_t lo = r1 + c1 > n ? r1 + c1 - n : 0, hi = std::min(r1, c1);
  const double margins = log_factorial(r1) + log_factorial(r2) + log_factorial(c1) + log_factorial(c2) - log_factorial(n);
  auto log_p = [&](uint64_t x) {  // the table whose first cell is x
    return margins - log_factorial(x) - log_factorial(r1 - x) - log_factorial(c1 - x) - log_factorial(n - r1 - c1 + x);
  };
  const double bound = log_p(a) + log1p(1e-7);
  double sum = 0.0;
  for (uint64_t x = lo; x <= hi; ++x) {
    const double lp = log_p(x);
    if (lp <= bound) sum += exp(lp);
  }
  return sum < 1.0 ? sum : 1.0;
}
// One entry of a pair table (include/walt_amd.h, "adjacent CpG pairs") as a line, tab-separated:
//   chrom  pos  next  pval  total  MM  MU  UM  UU
// pos and next 0-based within the chromosome, total the sum of the four counts, pval fisher_exact_two_sided as %.6g.
inline void put_allelic_line(Sink& out, const std::string& chrom, uint32_t pos, uint32_t next, const uint64_t n[4]) {
  char num[192];
  out.put(chrom);
  snprintf(num, sizeof num, "\t%u\t%u\t%.6g\t%llu\t%llu\t%llu\t%llu\t%llu\n", pos, next, fisher_exact_two_sided(n[0], n[1], n[2], n[3]),
           (unsigned long long)(n[0] + n[1] + n[2] + n[3]), (unsigned long long)n[0], (unsigned long long)n[1],
           (unsigned long long)n[2], (unsigned long long)n[3]);
  out.lit(num);
}

// ---------------------------------------------------------------- <out>.epialleles (bin/walt -ME)
// The value of -MEN: a decimal integer from 1 to 1,000,000, nothing in front of or behind its digits.
constexpr uint32_t kMaxEpialleleMin = 1000000;
inline bool parse_epiallele_min(const std::string& text, uint32_t& out) {
  if (text.empty() || text.size() > 7) return false;
  uint32_t v = 0;
  for (const char c : text) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (uint32_t)(c - '0');
  }
  if (v < 1 || v > kMaxEpialleleMin) return false;
  out = v;
  return true;
}
// A window's statistics from its sixteen counts (column p = 8 u0 + 4 u1 + 2 u2 + u3, u = 1 unmethylated), in double:
// meth = sum n_p (4 - popcount p) / (4 total), epipoly = 1 - sum (n_p / total)^2 (Landan 2012), entropy =
// -1/4 sum (n_p / total) log2 (n_p / total) with 0 log 0 = 0 (Xie 2011), discordant = 1 - (n_0 + n_15) / total (Landau
// 2014).  An empty window gives zeros.
struct EpialleleStats {
  uint64_t total;
  double meth, epipoly, entropy, discordant;
};
inline EpialleleStats epiallele_stats(const uint64_t n[16]) {
  EpialleleStats s = {0, 0.0, 0.0, 0.0, 0.0};
  uint64_t meth = 0;
  for (int p = 0; p < 16; ++p) {
    s.total += n[p];
    meth += n[p] * (uint64_t)(4 - __builtin_popcount((unsigned)p));
  }
  if (!s.total) return s;
  const double t = (double)s.total;
  double squares = 0.0, plogp = 0.0;
  for (int p = 0; p < 16; ++p) {
    if (!n[p]) continue;
    const double f = (double)n[p] / t;
    squares += f * f;
    plogp += f * log2(f);
  }
  s.meth = (double)meth / (4.0 * t);
  s.epipoly = 1.0 - squares;
  s.entropy = plogp == 0.0 ? 0.0 : -0.25 * plogp;  // (no -0.000000)
  s.discordant = 1.0 - (double)(n[0] + n[15]) / t;
  return s;
}
// One entry of a window table (include/walt_amd.h, "four-CpG epialleles") as a line, tab-separated:
//   chrom  pos  end  total  n0 .. n15  meth  epipoly  entropy  discordant
// pos and end 0-based within the chromosome: the first and the fourth C; the four statistics as %.6f.
inline void put_epiallele_line(Sink& out, const std::string& chrom, uint32_t pos, uint32_t end, const uint64_t n[16]) {
  const EpialleleStats s = epiallele_stats(n);
  char num[640];
  int at = snprintf(num, sizeof num, "\t%u\t%u\t%llu", pos, end, (unsigned long long)s.total);
  for (int p = 0; p < 16; ++p) at += snprintf(num + at, sizeof num - (size_t)at, "\t%llu", (unsigned long long)n[p]);
  snprintf(num + at, sizeof num - (size_t)at, "\t%.6f\t%.6f\t%.6f\t%.6f\n", s.meth, s.epipoly, s.entropy, s.discordant);
  out.put(chrom);
  out.lit(num);
}
// The merge of two devices' windows of a table written by position (-MC, -MA, -ME): `add`, ascending by `pos`, into
// `rows`, ascending too; a position both hold becomes one row, plus(row, other_row) adding the counters (they are
// additive: each device counted its own share of the reads).  `other` is scratch.
template <class Row, class Plus>
inline void merge_rows(std::vector<Row>& rows, const Row* add, size_t n_add, std::vector<Row>& other, Plus plus) {
  other.clear();
  size_t i = 0, j = 0;
  while (i < rows.size() || j < n_add) {
    if (j == n_add || (i < rows.size() && rows[i].pos < add[j].pos)) { other.push_back(rows[i++]); continue; }
    Row r = add[j++];
    if (i < rows.size() && rows[i].pos == r.pos) plus(r, rows[i++]);
    other.push_back(r);
  }
  rows.swap(other);
}
// The rows of the three tables and how two rows of one position add.  A site of -MC is the device's record, its counters
// added in 32 bits as on the device; an entry of -MA and a window of -ME are held with counters of 64 bits.
inline void add_site_row(walt_meth_site& r, const walt_meth_site& o) { r.meth += o.meth; r.unmeth += o.unmeth; }
struct AllelicRow {
  uint32_t pos, next;
  uint64_t n[4];
};
struct EpialleleRow {
  uint32_t pos, last;
  uint64_t n[16];
};
template <class Row>  // (an AllelicRow or an EpialleleRow)
inline void add_counter_row(Row& r, const Row& o) {
  for (size_t k = 0; k < sizeof r.n / sizeof r.n[0]; ++k) r.n[k] += o.n[k];
}
inline void merge_epiallele_rows(std::vector<EpialleleRow>& rows, const EpialleleRow* add, size_t n_add, std::vector<EpialleleRow>& other) {
  merge_rows(rows, add, n_add, other, add_counter_row<EpialleleRow>);
}
inline uint64_t epiallele_row_total(const EpialleleRow& r) {
  uint64_t t = 0;
  for (int k = 0; k < 16; ++k) t += r.n[k];
  return t;
}


// ---------------------------------------------------------------- <out>.variants, <out>.variantstats (bin/walt -MV)
// The value of -MVD (lo 1, hi 1,000,000) or -MVP (lo 0, hi 99): a decimal integer, nothing in front of or behind its digits.
constexpr uint32_t kMaxVariantDepth = 1000000;
inline bool parse_variant_value(const std::string& text, uint32_t lo, uint32_t hi, uint32_t& out) {
  if (text.empty() || text.size() > 7) return false;
  uint32_t v = 0;
  for (const char c : text) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (uint32_t)(c - '0');
  }
  if (v < lo || v > hi) return false;
  out = v;
  return true;
}
// One flagged position (include/walt_amd.h, "opposite-strand evidence") as a line, tab-separated:
//   chrom  pos  strand  context  meth  unmeth  opp_match  opp_other
// pos 0-based within the chromosome; the first six columns are those of <out>.methcounts.
inline void put_variant_line(Sink& out, const std::string& chrom, uint32_t chrom_start, const walt_variant_site& s) {
  static const char* ctx[4] = {"CpG", "CHG", "CHH", "unknown"};
  out.put(chrom); out.ch('\t'); out.u32(s.pos - chrom_start); out.ch('\t'); out.ch((char)s.strand); out.ch('\t');
  out.lit(ctx[s.context & 3]); out.ch('\t'); out.u32(s.meth); out.ch('\t'); out.u32(s.unmeth); out.ch('\t');
  out.u32(s.match); out.ch('\t'); out.u32(s.other); out.ch('\n');
}
// One read file's block of <out>.variantstats: the five totals of walt_pileup_mask_variants and the rule.
inline void put_variant_block(Sink& out, const uint64_t tot[5], uint32_t min_depth, uint32_t max_percent) {
  char num[320];
  snprintf(num, sizeof num, "judged: %llu\nflagged: %llu\nmasked sites: %llu\nmasked meth: %llu\nmasked unmeth: %llu\nrule\t%u\t%u\n",
           (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[2], (unsigned long long)tot[3],
           (unsigned long long)tot[4], min_depth, max_percent);
  out.lit(num);
}

// ---------------------------------------------------------------- <out>.methsites, <out>.sitestats (bin/walt -MS)
// The value of -MSR (0 <= r < 1) or -MSA (0 < a < 1): a decimal fraction in digits, at most one point and an optional
// exponent, nothing in front of or behind it, at most 24 characters.
inline bool parse_site_fraction(const std::string& text, bool zero_allowed, double& out) {
  if (text.empty() || text.size() > 24) return false;
  bool digit = false;
  for (size_t i = 0; i < text.size(); ++i) {
    const char c = text[i];
    if (c >= '0' && c <= '9') { digit = true; continue; }
    if (c == '.' || c == 'e' || c == 'E') continue;
    if ((c == '-' || c == '+') && i > 0 && (text[i - 1] == 'e' || text[i - 1] == 'E')) continue;
    return false;
  }
  if (!digit || text[0] == 'e' || text[0] == 'E') return false;
  char* end = nullptr;
  const double v = strtod(text.c_str(), &end);
  if (!end || *end != '\0' || !(v >= 0.0) || !(v < 1.0) || (v == 0.0 && !zero_allowed)) return false;
  out = v;
  return true;
}
// The value of -MSD: the minimum depth of a tested site, 1 to 127.
inline bool parse_site_depth(const std::string& text, uint32_t& out) { return parse_variant_value(text, 1, 127, out); }
// One called site (include/walt_amd.h, "called sites") as a line, tab-separated:
//   chrom  pos  strand  context  meth  unmeth  pval
// pos 0-based within the chromosome; the first six columns are those of <out>.methcounts; pval %.6g.
inline void put_site_line(Sink& out, const std::string& chrom, uint32_t chrom_start, const walt_meth_site& s, double pval) {
  static const char* ctx[4] = {"CpG", "CHG", "CHH", "unknown"};
  out.put(chrom); out.ch('\t'); out.u32(s.pos - chrom_start); out.ch('\t'); out.ch((char)s.strand); out.ch('\t');
  out.lit(ctx[s.context & 3]); out.ch('\t'); out.u32(s.meth); out.ch('\t'); out.u32(s.unmeth);
  char num[48];
  snprintf(num, sizeof num, "\t%.6g\n", pval);
  out.lit(num);
}
// One read file's block of <out>.sitestats.  control: the sequence's name, or "given" under -MSR, where the control's
// counts are NA (counts == nullptr); has_rate false: the control has no call, the rate is NA and nothing was called.
// Then the rule and one line per context: context <TAB> tested <TAB> called <TAB> cutoff (%.6g, NA when no group passed).
struct SiteStatsRow {
  uint64_t tested, called;
  bool has_cutoff;
  double cutoff;
};
inline void put_sitestats_block(Sink& out, const std::string& control, const uint64_t* counts, bool has_rate, double rate,
                                double alpha, uint32_t min_depth, const SiteStatsRow row[4]) {
  static const char* ctx[4] = {"CpG", "CHG", "CHH", "unknown"};
  char num[160];
  out.lit("control: "); out.put(control); out.ch('\n');
  if (counts) snprintf(num, sizeof num, "control meth: %llu\ncontrol unmeth: %llu\n", (unsigned long long)counts[0], (unsigned long long)counts[1]);
  else snprintf(num, sizeof num, "control meth: NA\ncontrol unmeth: NA\n");
  out.lit(num);
  if (has_rate) snprintf(num, sizeof num, "non-conversion rate: %.6g\n", rate);
  else snprintf(num, sizeof num, "non-conversion rate: NA\n");
  out.lit(num);
  snprintf(num, sizeof num, "rule\t%.6g\t%u\n", alpha, min_depth);
  out.lit(num);
  for (int c = 0; c < 4; ++c) {
    if (row[c].has_cutoff) snprintf(num, sizeof num, "%s\t%llu\t%llu\t%.6g\n", ctx[c], (unsigned long long)row[c].tested,
                                    (unsigned long long)row[c].called, row[c].cutoff);
    else snprintf(num, sizeof num, "%s\t%llu\t%llu\tNA\n", ctx[c], (unsigned long long)row[c].tested, (unsigned long long)row[c].called);
    out.lit(num);
  }
}

}  // namespace hostio
#endif  // WALT_AMD_HOSTIO_H_
