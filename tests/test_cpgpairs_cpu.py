"""Adjacent-CpG state pairs (include/walt_amd.h, "adjacent CpG pairs"), the parts that need no device: what the kernels
run per lane (walt_amd/csrc/cpgpairs_core.h), compiled with g++ (tests/cpgpairs_harness.cpp) and compared with the
pure-Python restatement of tests/test_gpu_cpgpairs.py; the Fisher test and the <out>.allelic writer of hostio.h; the
exports of the three libraries, the binding's surface and refusals without a device; and bin/walt's option: spellings,
modes and what it goes with."""
import ctypes
import inspect
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_cpgpairs import (Hand, LENGTHS, allelic_line, edge_cases, expected_table, find_pairs, fisher_exact, pair_genome,
                               random_reads)

NAMES = ("walt_cpgpairs_create", "walt_cpgpairs_destroy", "walt_cpgpairs_clear", "walt_cpgpairs_device_bytes", "walt_cpgpairs_n_pairs",
         "walt_cpgpairs_batch", "walt_cpgpairs_batch_device", "walt_cpgpairs_extract", "walt_cpgpairs_extract_device",
         "walt_meth_pileup_batch_pairs", "walt_meth_pileup_batch_pairs_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")


@pytest.fixture(scope="module")
def harness(scratch):
    so = os.path.join(scratch, "libcpgpairs_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                    os.path.join(refio.HERE, "cpgpairs_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.cpgpairs_harness_bit_words.argtypes = [u64]
    L.cpgpairs_harness_bit_words.restype = u64
    L.cpgpairs_harness_dir_entries.argtypes = [u64]
    L.cpgpairs_harness_dir_entries.restype = u64
    L.cpgpairs_harness_build.argtypes = [ctypes.c_char_p, u32, vp, u32, vp, vp]
    L.cpgpairs_harness_build.restype = u32
    L.cpgpairs_harness_rank.argtypes = [vp, vp, u32]
    L.cpgpairs_harness_rank.restype = u32
    L.cpgpairs_harness_pair_at.argtypes = [vp, u32]
    L.cpgpairs_harness_pair_at.restype = ctypes.c_longlong
    L.cpgpairs_harness_next.argtypes = [vp, u32, u64]
    L.cpgpairs_harness_next.restype = u32
    L.cpgpairs_harness_range_mask.argtypes = [u64, u32, u32]
    L.cpgpairs_harness_range_mask.restype = u32
    L.cpgpairs_harness_counted.argtypes = [u32, u32, u64, u64, u32, u32]
    L.cpgpairs_harness_call.argtypes = [u32, u32]
    L.cpgpairs_harness_call.restype = u64
    L.cpgpairs_harness_combine.argtypes = [u64, u64]
    L.cpgpairs_harness_combine.restype = u64
    L.cpgpairs_harness_couple.argtypes = [u64, u64, vp]
    L.cpgpairs_harness_read.argtypes = [vp, u32, u64, u64, vp, vp, u32]
    L.cpgpairs_harness_read.restype = u32
    L.cpgpairs_harness_batch.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32, vp, u64, vp, u64, vp]
    L.cpgpairs_harness_batch.restype = ctypes.c_longlong
    L.cpgpairs_harness_fisher.argtypes = [u64, u64, u64, u64]
    L.cpgpairs_harness_fisher.restype = ctypes.c_double
    L.cpgpairs_harness_allelic_line.argtypes = [ctypes.c_char_p, u32, u32, vp, vp, u32]
    L.cpgpairs_harness_allelic_line.restype = u32
    return L


# ---------------------------------------------------------------------------
# the bitmap, the rank, the next pair
# ---------------------------------------------------------------------------
def built(harness, seqs):
    text = "".join(seqs)
    start = np.zeros(len(seqs) + 1, dtype=np.uint32)
    start[1:] = np.cumsum([len(s) for s in seqs])
    n_words = harness.cpgpairs_harness_bit_words(len(text))
    bits = np.full(n_words, 0xFFFFFFFF, dtype=np.uint32)
    dirs = np.full(harness.cpgpairs_harness_dir_entries(len(text)), 0xFFFFFFFF, dtype=np.uint32)
    n_pairs = harness.cpgpairs_harness_build(text.encode(), len(text), start.ctypes.data, len(seqs), bits.ctypes.data, dirs.ctypes.data)
    return text, start, bits, dirs, n_pairs


def check_genome(harness, seqs):
    text, start, bits, dirs, n_pairs = built(harness, seqs)
    pairs = find_pairs(text, start)
    assert n_pairs == len(pairs)
    n_words = bits.size
    assert n_words % 4 == 0 and n_words * 32 >= len(text) + 256 and dirs.size * 4 + 8 == n_words
    flat = np.unpackbits(bits.view(np.uint8), bitorder="little")
    assert np.nonzero(flat)[0].tolist() == pairs  # the bitmap is the scan, its padding is zero
    is_pair = set(pairs)
    rank = 0
    for p in range(len(text)):
        assert harness.cpgpairs_harness_rank(bits.ctypes.data, dirs.ctypes.data, p) == rank, p
        want_pair = p if p in is_pair else p - 1 if p - 1 in is_pair else -1
        assert harness.cpgpairs_harness_pair_at(bits.ctypes.data, p) == want_pair, p
        rank += p in is_pair
    for j, c in enumerate(pairs):
        nxt = harness.cpgpairs_harness_next(bits.ctypes.data, c, n_words)
        if j + 1 < len(pairs) and pairs[j + 1] - c <= 1025:  # as far as the calls of one read reach: always found
            assert nxt == pairs[j + 1], (c, nxt)
        else:  # farther: found or not, never a wrong one
            assert nxt in [0xFFFFFFFF] + pairs[j + 1:j + 2], (c, nxt)
    return pairs


def test_bitmap_and_rank_against_the_scan(harness):
    rng = random.Random(41)
    rnd = lambda n, al="ACGT": "".join(rng.choice(al) for _ in range(n))
    total = 0
    for trial in range(60):
        n_chrom = rng.randrange(1, 6)
        lens = None
        while lens is None or not all(sum(lens[:k]) % 128 for k in range(1, n_chrom)):  # starts off the directory's blocks
            lens = [rng.choice([1, 2, 3, 31, 33, 127, 129, 300, 700]) + rng.randrange(0, 3) * 128 for _ in range(n_chrom)]
        seqs = [rnd(n) for n in lens]
        total += len(check_genome(harness, seqs))
    assert total > 2000
    # a chromosome ending in C followed by one starting with G: no pair across the boundary, at every bit of a word
    for tail in range(1, 70):
        seqs = [rnd(tail, "AT") + "C", "G" + rnd(5, "AT"), "CG", "C", "G", "CG" * 3 + "C", "G"]
        assert check_genome(harness, seqs) == [tail + 1 + 6, tail + 1 + 6 + 2 + 2, tail + 1 + 6 + 2 + 2 + 2, tail + 1 + 6 + 2 + 2 + 4]
    # CGCGCG runs across word and block boundaries; a genome with no pair; one base
    assert check_genome(harness, ["CG" * 200]) == list(range(0, 400, 2))
    assert check_genome(harness, ["A" + "CG" * 200 + "C"]) == list(range(1, 401, 2))
    assert check_genome(harness, ["CA" * 150, "GT" * 90, "C"]) == []
    assert check_genome(harness, ["C"]) == [] and check_genome(harness, ["C", "G"]) == [] and check_genome(harness, ["CG"]) == [0]
    # two pairs 1,022 and 1,023 apart, and 1,100 apart: beyond what a read spans, no next
    for gap, found in ((1022, True), (1023, True), (1024, True), (1100, False)):
        text, start, bits, dirs, _ = built(harness, ["CG" + "A" * (gap - 2) + "CG" + "AAA"])
        nxt = harness.cpgpairs_harness_next(bits.ctypes.data, 0, bits.size)
        assert nxt == (gap if found else 0xFFFFFFFF)


def test_range_mask_and_which_records_count(harness):
    rng = random.Random(42)
    for _ in range(3000):
        w = rng.randrange(0, 40)
        lo = rng.randrange(0, 1400)
        hi = rng.randrange(lo, 1400)
        want = sum(1 << k for k in range(32) if lo <= 32 * w + k < hi)
        assert harness.cpgpairs_harness_range_mask(w, lo, hi) == want, (w, lo, hi)
    assert harness.cpgpairs_harness_range_mask((1 << 27) - 1, 0, 0xFFFFFFFF) == 0x7FFFFFFF
    c = harness.cpgpairs_harness_counted
    assert c(1, 0, 10, 11, 5, 6) == 1 and c(1, 0, 10, 1034, 0, 1) == 1
    assert c(1, 0, 10, 1035, 5, 6) == 0 and c(1, 0, 10, 10, 5, 6) == 0 and c(1, 0, 11, 10, 5, 6) == 0
    assert c(0, 0, 10, 20, 5, 6) == 0 and c(2, 0, 10, 20, 5, 6) == 0 and c(1, 1, 10, 20, 5, 6) == 0 and c(1, 200, 10, 20, 5, 6) == 0
    assert c(1, 0, 10, 20, 6, 6) == 0 and c(1, 0, 10, 20, 0xFFFFFFFF, 6) == 0 and c(1, 0, 2 ** 40, 2 ** 40 + 5, 5, 6) == 1


# ---------------------------------------------------------------------------
# the slice summary, the combine, the scan across the lanes
# ---------------------------------------------------------------------------
def walk(calls, numbers):
    """the contract's walk over one read: calls (bytes), numbers[i] = the pair number of read position i or -1"""
    out, prev = [], None
    for i, b in enumerate(calls):
        if b not in (0x7A, 0x5A) or numbers[i] < 0:
            continue
        cur = (numbers[i], 1 if b == 0x7A else 0)
        if prev is not None and abs(cur[0] - prev[0]) == 1:
            (jl, ul), (jh, uh) = sorted([prev, cur])
            out.append((jl, 2 * ul + uh))
        prev = cur
    return out


def read_through_the_fold(harness, body, numbers, lead, shift, tail=16):
    """the read behind `lead` bytes and in front of `tail` bytes of neighbours full of z, the batch at address 16 k + shift"""
    n = len(body)
    raw = np.full(lead + n + tail + 64, ord("z"), dtype=np.uint8)
    a = (-raw.ctypes.data) % 16 + shift
    raw[a + lead:a + lead + n] = np.frombuffer(bytes(body), dtype=np.uint8)
    adds = np.zeros(2 * 1100, dtype=np.uint32)
    num = np.ascontiguousarray(numbers, dtype=np.int64)
    k = harness.cpgpairs_harness_read(raw.ctypes.data + a + lead, n, lead, n + tail, num.ctypes.data, adds.ctypes.data, 1100)
    return [(int(adds[2 * i]), int(adds[2 * i + 1])) for i in range(k)]


@pytest.mark.parametrize("length", LENGTHS + (40, 130))
def test_every_eight_lane_split_of_random_call_strings_against_the_walk(harness, length):
    rng = random.Random(length)
    couples = 0
    for al, step in (("zZ", 1), ("zZ..", 1), ("zZ" + "." * 14, 1), ("zZxXhHuU.A", 1), ("zZ", 0), ("zZ.", 2)):
        body = bytes(ord(rng.choice(al)) for _ in range(length))
        # pair numbers along the read: ascending or descending by `step` per call position, with gaps, repeats and holes
        numbers, j = [], 5000
        down = rng.random() < 0.5
        for i in range(length):
            r = rng.random()
            numbers.append(-1 if r < 0.1 else j)
            if r > 0.3:
                j += (-1 if down else 1) * (step if rng.random() < 0.8 else 2)
        want = sorted(walk(body, numbers))
        couples += len(want)
        for shift in range(16):
            for lead in (range(16) if length < 1024 else [(shift * 7 + 3) % 16, 0]):
                for tail in (0, 16):
                    got = sorted(read_through_the_fold(harness, body, numbers, lead, shift, tail))
                    assert got == want, (length, al, shift, lead, tail)
    assert couples > 0 or length == 1


def test_combine_is_associative_and_couples_are_symmetric(harness):
    rng = random.Random(43)
    call = harness.cpgpairs_harness_call
    comb = harness.cpgpairs_harness_combine
    assert call(0, 0) == 1 and call(0, 1) == 2 and call(0xFFFFFFFF, 1) == 2 ** 33 and comb(0, 0) == 0
    out = np.zeros(3, dtype=np.uint32)
    for _ in range(5000):
        a, b, c = (rng.choice([0, call(rng.choice([0, 1, 2, 3, 77, 0xFFFFFFFE, 0xFFFFFFFF]), rng.randrange(2))]) for _ in range(3))
        assert comb(comb(a, b), c) == comb(a, comb(b, c)) == (c or b or a)
        assert comb(a, 0) == a == comb(0, a)
        harness.cpgpairs_harness_couple(a, b, out.ctypes.data)
        got = out.tolist()
        harness.cpgpairs_harness_couple(b, a, out.ctypes.data)
        assert got == out.tolist()  # the entry and the column do not depend on the direction the read walks in
        if a and b:
            (ja, ua), (jb, ub) = (((x - 1) >> 1, (x - 1) & 1) for x in (a, b))
            want = walk(b"zZ"[1 - ua:2 - ua] + b"zZ"[1 - ub:2 - ub], [ja, jb])
            assert got == ([1, want[0][0], want[0][1]] if want else [0, 0, 0]), (a, b)
        else:
            assert got == [0, 0, 0]


# ---------------------------------------------------------------------------
# batches as the kernel takes them
# ---------------------------------------------------------------------------
def harness_table(harness, seqs, h, skip=None, stride=16, shift=0):
    text, start, bits, dirs, n_pairs = built(harness, seqs)
    calls, offsets, rec = h.arrays(stride)
    raw = np.full(calls.size + 64, ord("z"), dtype=np.uint8)
    a = (-raw.ctypes.data) % 16 + shift
    raw[a:a + calls.size] = calls
    table = np.zeros((max(n_pairs, 1), 4), dtype=np.uint32)
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
    harness.cpgpairs_harness_batch(bits.ctypes.data, dirs.ctypes.data, len(text), start.ctypes.data, len(seqs), raw.ctypes.data + a,
                                   offsets.ctypes.data, len(h.pos), rec.ctypes.data, rec.strides[0] if len(h.pos) > 1 else stride,
                                   None if sk is None else sk.ctypes.data, 1, table.ctypes.data)
    return table[:n_pairs].astype(np.uint64)


def test_batches_as_the_kernel_takes_them(harness):
    g, where = pair_genome()
    h, couples, n_exact = edge_cases(g, where)
    for shift in (0, 5, 15):
        got = harness_table(harness, g.seqs, h, shift=shift)
        assert np.array_equal(got, h.want(g)) and int(got.sum()) > couples
    assert int(harness_table(harness, g.seqs, h.head(n_exact)).sum()) == couples
    rng = random.Random(44)
    for trial in range(12):
        hr = random_reads(g, rng, 300, trial % 2 == 0)
        skip = [rng.choice([0, 0, 0, 1, 200]) for _ in hr.pos]
        got = harness_table(harness, g.seqs, hr, skip, stride=64 if trial % 3 == 0 else 16, shift=trial)
        assert np.array_equal(got, hr.want(g, skip)) and got.sum() > 20, trial
    # many small chromosomes, reads across their ends, on both strands
    rnd = lambda n: "".join(rng.choice("ACGTCG") for _ in range(n))
    from test_gpu_meth_contigs import Genome
    small = Genome(["s%d" % i for i in range(40)], [rnd(rng.choice([1, 2, 3, 40, 90, 200])) for _ in range(40)])
    hr = random_reads(small, rng, 600, True)
    got = harness_table(harness, small.seqs, hr)
    assert np.array_equal(got, hr.want(small)) and got.sum() > 100


# ---------------------------------------------------------------------------
# the Fisher test and the writer
# ---------------------------------------------------------------------------
def fisher_tables():
    tables = [(a, b, c, d) for a in range(13) for b in range(13 - a) for c in range(13 - a - b) for d in range(13 - a - b - c)]
    assert (0, 0, 0, 0) in tables and len(tables) == 1820
    tables += [(0, 0, 5, 9), (7, 3, 0, 0), (0, 4, 0, 6), (5, 0, 8, 0), (0, 0, 0, 1), (40, 0, 0, 0)]  # a zero row, a zero column
    tables += [(5, 5, 5, 5), (10, 0, 0, 10), (0, 10, 10, 0), (3, 7, 7, 3), (20, 30, 30, 20), (100, 1, 1, 100), (17, 17, 17, 17)]  # exact ties
    # counts up to 50,000, one margin small: the restatement's sum has as many terms as the smallest margin
    tables += [(50000, 3, 40000, 5), (50000, 0, 49999, 7), (4, 50000, 2, 45000), (30000, 29500, 10, 12), (12000, 3, 11000, 40),
               (4095, 4096, 40, 41), (50000, 50000, 30, 30)]
    # strong association: p-values far below what a sum of rounded terms could hide
    tables += [(50000, 3, 5, 40), (40, 2, 3, 50000), (30, 0, 0, 30), (25, 1, 2, 30), (0, 35, 35, 0), (45000, 10, 12, 60)]
    return tables


def test_fisher_against_exact_arithmetic(harness):
    small_p = 0
    for t in fisher_tables():
        want = float(fisher_exact(*t))
        got = harness.cpgpairs_harness_fisher(*t)
        assert 0.0 <= got <= 1.0
        if want == 0.0:  # (below the smallest double: both must say so)
            assert got == 0.0, t
            continue
        # what the file keeps: six significant digits lose up to 5e-6 relative; lgamma's error is orders below
        assert abs(float("%.6g" % got) - want) <= 1e-5 * want, (t, got, want)
        small_p += want < 1e-3
    assert small_p >= 8
    assert harness.cpgpairs_harness_fisher(0, 0, 0, 0) == 1.0 and harness.cpgpairs_harness_fisher(5, 5, 5, 5) == 1.0


def test_allelic_writer_byte_for_byte(harness):
    buf = ctypes.create_string_buffer(512)
    rows = [("chr1", 0, 2, (0, 0, 0, 1)), ("chr1", 10, 1033, (10, 0, 0, 10)), ("scaffold_12|x", 4294967000, 4294967290, (3, 1, 1, 3)),
            ("c", 5, 9, (20, 30, 30, 20)), ("c", 6, 8, (2 ** 32 + 5, 7, 9, 0)), ("c", 7, 9, (50000, 3, 40000, 5)), ("c", 8, 12, (100, 1, 1, 100)),
            ("c", 9, 11, (1, 2, 3, 4)), ("c", 11, 13, (12, 0, 1, 9))]
    for chrom, pos, nxt, n in rows:
        arr = np.array(n, dtype=np.uint64)
        k = harness.cpgpairs_harness_allelic_line(chrom.encode(), pos, nxt, arr.ctypes.data, ctypes.addressof(buf), 512)
        got = buf.raw[:k].decode()
        assert got == allelic_line(chrom, pos, nxt, n), (got, allelic_line(chrom, pos, nxt, n))
        p = got.rstrip("\n").split("\t")
        assert p[:3] == [chrom, str(pos), str(nxt)] and [int(v) for v in p[4:]] == [sum(n)] + list(n) and got.endswith("\n")
    assert allelic_line("c", 9, 11, (1, 2, 3, 4)) == "c\t9\t11\t1\t10\t1\t2\t3\t4\n"
    assert allelic_line("chr1", 10, 1033, (10, 0, 0, 10)) == "chr1\t10\t1033\t1.08251e-05\t20\t10\t0\t0\t10\n"


# ---------------------------------------------------------------------------
# exports, binding, command line
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert "adjacent CpG pairs" in hdr and hdr.index("non-converted reads") < hdr.index("---- adjacent CpG pairs") < hdr.index("---- options")


def test_binding_surface_and_refusals_without_a_device():
    import walt_amd
    for nm in ("add", "add_device", "extract", "extract_device", "n_pairs", "clear", "close", "device_bytes"):
        assert hasattr(walt_amd.CpgPairs, nm), nm
    assert callable(walt_amd.Index.cpg_pairs)
    for fn in (walt_amd.Index.meth_call_batch, walt_amd.Index.meth_call_batch_device, walt_amd.Pileup.add_batch,
               walt_amd.Pileup.add_batch_device):
        p = inspect.signature(fn).parameters
        assert p["pairs"].default is None and "mbias" in p, fn
    dt = walt_amd.cpgpair_site_dtype
    assert dt.itemsize == 24 and dt.names == ("pos", "next", "n") and dt["n"].shape == (4,)
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm

    class Named:  # stands for the library: _meth_form only looks the function up by name
        def __getattr__(self, name):
            return name

    form = lambda **kw: walt_amd._meth_form(Named(), kw.pop("device", False), kw.pop("pile", None), **kw)
    assert form(pairs=(7,)) == ("walt_meth_pileup_batch_pairs", (None,), (None, 1, None, None, 0, 0, 0, 7))
    assert form(pairs=(7,), device=True, pile=3, skip=(5, 2), excl=(6,), mbias=(8, 1), trim=(2, 4)) == \
        ("walt_meth_pileup_batch_pairs_device", (3,), (5, 2, 6, 8, 1, 2, 4, 7))
    assert form(trim=(2, 4))[0] == "walt_meth_pileup_batch_trim" and form(mbias=(8, 1))[0] == "walt_meth_pileup_batch_mbias"
    assert form()[0] == "walt_meth_call_batch"  # without pairs: the forms a call always reached
    # no device: null objects are refused, not crashed on, and the message names the call
    E = walt_amd.WALT_EINVAL
    h = ctypes.c_void_p()
    assert L.walt_cpgpairs_create(None, ctypes.byref(h)) == E and not h.value and b"walt_cpgpairs_create:" in L.walt_last_error()
    assert L.walt_cpgpairs_batch(None, None, None, 0, None, 16, None, 1) == E
    assert b"walt_cpgpairs_batch:" in L.walt_last_error() and b"null pair table" in L.walt_last_error()
    assert L.walt_cpgpairs_batch_device(None, None, None, 0, None, 16, None, 1, None) == E and b"walt_cpgpairs_batch_device:" in L.walt_last_error()
    n = ctypes.c_uint64(0)
    assert L.walt_cpgpairs_extract(None, 0, 0, None, 0, ctypes.byref(n)) == E and b"walt_cpgpairs_extract:" in L.walt_last_error()
    assert L.walt_cpgpairs_extract_device(None, 0, 0, None, 0, None, None) == E and b"walt_cpgpairs_extract_device:" in L.walt_last_error()
    assert L.walt_cpgpairs_clear(None) == E and b"walt_cpgpairs_clear:" in L.walt_last_error()
    assert L.walt_cpgpairs_device_bytes(None) == 0 and L.walt_cpgpairs_n_pairs(None) == 0
    L.walt_cpgpairs_destroy(None)
    assert L.walt_meth_pileup_batch_pairs(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None, 1, None,
                                          None, 0, 0, 0, None) == E and b"walt_meth_pileup_batch_pairs:" in L.walt_last_error()
    assert L.walt_meth_pileup_batch_pairs_device(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None, 1,
                                                 None, None, 0, 0, 0, None, None) == E
    assert b"walt_meth_pileup_batch_pairs_device:" in L.walt_last_error()


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


def test_cli_parses_the_option_in_every_mode(tmp_path):
    pr = run([])
    assert pr.returncode == 0 and " -MA " in pr.stdout, pr.stdout
    idx, out = str(tmp_path / "none.dbindex"), str(tmp_path / "o.mr")
    pair, single = ["-1", "a.fastq", "-2", "b.fastq"], ["-r", "x.fastq"]
    base = ["-i", idx, "-o", out]
    modes = [(single, []), (single, ["-A"]), (single, ["-R"]), (pair, []), (pair, ["-P"]), (pair, ["-RP"])]
    # the three spellings are known in every mode, alone (a consumer) and beside the others: the run gets as far as the index check
    for reads, mode in modes:
        for flag in ("-MA", "-allelic", "--allelic-meth"):
            for extra in ([], ["-M", "-sam"], ["-MC", "-MB", "-ML"], ["-D", "-C", "AGATCGGAAGAGC"], ["-I5", "3"], ["-F", "3", "-FP", "20"], ["-g", "0,0"]):
                pr = run(base + reads + mode + extra + [flag])
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, mode, extra, pr.stdout)
    # -I5 3 -MA, -NO -MA with -1 / -2, the -F options: -MA is something for them to act on
    for args in (single + ["-I5", "3", "-MA"], pair + ["-NO", "-MA"], pair + ["-I3R2", "2", "-NO", "-MA"], single + ["-FC", "2", "-MA"]):
        pr = run(base + args)
        assert pr.returncode != 0 and "index file missing" in pr.stdout, (args, pr.stdout)
    # and their refusals name it
    for args in (pair + ["-NO"], single + ["-I5", "3"], single + ["-F", "3"]):
        pr = run(base + args)
        assert pr.returncode != 0 and "-MA" in pr.stdout and "index file missing" not in pr.stdout, (args, pr.stdout)
    pr = run(base + single + ["-NO", "-MA"])
    assert pr.returncode != 0 and "paired-end only" in pr.stdout
    assert not os.path.exists(out) and not os.path.exists(out + ".allelic")


def test_per_lane_logic_under_the_host_sanitizers(scratch):
    """tests/cpgpairs_sanitize_main.cpp, a stand-alone program over tests/cpgpairs_harness.cpp built with the host's address and
    undefined-behaviour sanitizers: random genomes and batches, bitmap, directory, table and calls each in a heap block of
    exactly its size -- a load or an add outside them ends the program, and so does a table that differs from a plain walk"""
    exe = os.path.join(scratch, "cpgpairs_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(refio.HERE, "cpgpairs_sanitize_main.cpp"), os.path.join(refio.HERE, "cpgpairs_harness.cpp"), "-o", exe],
                   check=True, timeout=300)
    pr = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert pr.returncode == 0 and pr.stdout.startswith("ok "), pr.stdout[-2000:]
