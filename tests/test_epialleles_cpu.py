"""Four-CpG epialleles (include/walt_amd.h, "four-CpG epialleles"), the parts that need no device: what the kernel runs
per lane (walt_amd/csrc/epialleles_core.h), compiled with g++ (tests/epialleles_harness.cpp) and compared with the
pure-Python restatement of tests/test_gpu_epialleles.py; the statistics, the <out>.epialleles writer and the merge of
hostio.h; the exports of the three libraries, the binding's surface and refusals without a device; and bin/walt's options:
spellings, modes and what they go with."""
import ctypes
import inspect
import math
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import refio
from test_gpu_cpgpairs import find_pairs
from test_gpu_epialleles import edge_cases, epi_genome, epi_stats, epi_walk, placement_cases, random_reads, want_of

NAMES = ("walt_epialleles_create", "walt_epialleles_destroy", "walt_epialleles_clear", "walt_epialleles_device_bytes",
         "walt_epialleles_n_pairs", "walt_epialleles_batch", "walt_epialleles_batch_device", "walt_epialleles_extract",
         "walt_epialleles_extract_device", "walt_meth_pileup_batch_epi", "walt_meth_pileup_batch_epi_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")
SOURCES = [os.path.join(refio.HERE, "epialleles_harness.cpp"), os.path.join(refio.HERE, "cpgpairs_harness.cpp")]


@pytest.fixture(scope="module")
def harness(scratch):
    so = os.path.join(scratch, "libepialleles_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC] + SOURCES +
                   ["-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.cpgpairs_harness_bit_words.argtypes = [u64]
    L.cpgpairs_harness_bit_words.restype = u64
    L.cpgpairs_harness_dir_entries.argtypes = [u64]
    L.cpgpairs_harness_dir_entries.restype = u64
    L.cpgpairs_harness_build.argtypes = [ctypes.c_char_p, u32, vp, u32, vp, vp]
    L.cpgpairs_harness_build.restype = u32
    L.epi_harness_chain.argtypes = [vp, vp, u32]
    L.epi_harness_chain.restype = u64
    L.epi_harness_pack.argtypes = [u32, u32, u32, u32, u32]
    L.epi_harness_pack.restype = u64
    L.epi_harness_check_all.argtypes = [vp, u32, u32, vp]
    L.epi_harness_check_all.restype = u64
    L.epi_harness_read.argtypes = [vp, u32, u64, u64, vp, vp, u32, vp]
    L.epi_harness_read.restype = u32
    L.epi_harness_batch.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32, vp, u64, vp, u64, vp]
    L.epi_harness_batch.restype = ctypes.c_longlong
    L.epi_harness_stats.argtypes = [vp, vp]
    L.epi_harness_stats.restype = u64
    L.epi_harness_line.argtypes = [ctypes.c_char_p, u32, u32, vp, vp, u32]
    L.epi_harness_line.restype = u32
    L.epi_harness_merge.argtypes = [vp, vp, u32, vp, u32]
    L.epi_harness_merge.restype = u32
    return L


# ---------------------------------------------------------------------------
# the chain and the combine
# ---------------------------------------------------------------------------
def chain_of(stretch):
    """chain(S) from its definition: the longest suffix of S whose pair numbers step by one s in {+1, -1}, cut to its last
    three calls; "whole" when S is nothing but these calls -> (pair number of the last call, calls, s == -1, states, whole)"""
    if not stretch:
        return None
    best = 1
    for n in range(2, len(stretch) + 1):
        tail = stretch[-n:]
        if any(all(tail[i][0] == tail[0][0] + i * s for i in range(1, n)) for s in (1, -1)):
            best = n
        else:
            break
    kept = stretch[-min(best, 3):]
    down = 1 if len(kept) > 1 and kept[1][0] < kept[0][0] else 0
    states = sum(u << (len(kept) - 1 - k) for k, (_, u) in enumerate(kept))
    return kept[-1][0], len(kept), down, states, 1 if best == len(stretch) <= 3 else 0


def test_the_combine_exhaustively_on_six_pair_numbers(harness):
    numbers, max_calls = 6, 5
    base = 2 * numbers
    ref = []
    for n in range(max_calls + 1):
        for s in range(base ** n):
            stretch = [((s // base ** k % base) >> 1, (s // base ** k % base) & 1) for k in range(n)]
            c = chain_of(stretch)
            ref.append(0 if c is None else harness.epi_harness_pack(*c))
    assert len(ref) == sum(base ** n for n in range(max_calls + 1)) == 271453 and ref[0] == 0 and all(ref[1:])
    arr = np.array(ref, dtype=np.uint64)
    bad = ctypes.c_uint64(0)
    assert harness.epi_harness_check_all(arr.ctypes.data, numbers, max_calls, ctypes.byref(bad)) == 0, bad.value
    # (the check can fail: one wrong chain is found, and so is the split it spoils)
    arr[1000] ^= np.uint64(16)
    assert harness.epi_harness_check_all(arr.ctypes.data, numbers, max_calls, ctypes.byref(bad)) > 0
    # the packing: 0 is no call; pair numbers use all 32 bits
    assert harness.epi_harness_pack(0, 1, 0, 0, 1) == 5 and harness.epi_harness_pack(0xFFFFFFFF, 3, 1, 7, 0) == (0xFFFFFFFF << 8) | 0x7B
    js = np.array([0xFFFFFFFC, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF, 0], dtype=np.uint32)
    us = np.array([1, 0, 1, 1, 0], dtype=np.uint32)
    assert harness.epi_harness_chain(js.ctypes.data, us.ctypes.data, 4) == harness.epi_harness_pack(0xFFFFFFFF, 3, 0, 3, 0)
    assert harness.epi_harness_chain(js.ctypes.data, us.ctypes.data, 5) == harness.epi_harness_pack(0, 1, 0, 0, 0)  # no wrap-around neighbour


# ---------------------------------------------------------------------------
# one read through slices, trips and scan
# ---------------------------------------------------------------------------
def read_through_the_fold(harness, body, numbers, lead, shift, tail=16, asked=None):
    """the read behind `lead` bytes and in front of `tail` bytes of neighbours full of z, the batch at address 16 k + shift"""
    n = len(body)
    raw = np.full(lead + n + tail + 64, ord("z"), dtype=np.uint8)
    a = (-raw.ctypes.data) % 16 + shift
    raw[a + lead:a + lead + n] = np.frombuffer(bytes(body), dtype=np.uint8)
    adds = np.zeros(2 * 1100, dtype=np.uint32)
    num = np.ascontiguousarray(numbers, dtype=np.int64)
    k = harness.epi_harness_read(raw.ctypes.data + a + lead, n, lead, n + tail, num.ctypes.data, adds.ctypes.data, 1100,
                                 None if asked is None else asked.ctypes.data)
    return sorted((int(adds[2 * i]), int(adds[2 * i + 1])) for i in range(k))


def placed(length, at, states, j0=700, step=1):
    """a read of `length` '.' with the calls `states` at read positions `at`, on neighbouring pairs from j0 on"""
    body = bytearray(b"." * length)
    numbers = [-1] * length
    for k, (i, s) in enumerate(zip(at, states)):
        body[i] = ord(s)
        numbers[i] = j0 + k * step
    return bytes(body), numbers


# where the calls of a chain fall relative to a slice boundary at read position 128 (head 0): 4/0, 3/1, 2/2, 1/3 on two
# neighbouring slices, 1/1/1/1 on four, the last also across the trip boundary
SPLITS = {"4/0": [112, 115, 120, 127], "3/1": [118, 122, 127, 128], "2/2": [120, 127, 128, 135], "1/3": [127, 128, 133, 143],
          "1/1/1/1": [100, 116, 132, 148], "trip": [90, 120, 130, 200]}


@pytest.mark.parametrize("m", [4, 5, 9])
def test_chains_placed_over_slices_and_trips_against_the_walk(harness, m):
    rng = random.Random(m)
    windows = 0
    for name, at4 in SPLITS.items():
        at = list(at4)
        while len(at) < m:  # the rest of a longer chain: one call per slice, then across an empty trip
            at.append(at[-1] + (16 if len(at) < 7 else 140))
        for length in (300, 640, 1024):
            if at[-1] >= length:
                continue
            for step in (1, -1):
                states = "".join(rng.choice("zZ") for _ in at)
                body, numbers = placed(length, at, states, 700, step)
                want = sorted(epi_walk(body, numbers))
                assert len(want) == m - 3
                for head in range(16):  # the array address of the read's first call: every head alignment
                    for lead in (0, 16 - head if head else 5):
                        asked = np.zeros(length, dtype=np.uint32)
                        got = read_through_the_fold(harness, body, numbers, lead, (head - lead) % 16, asked=asked)
                        assert got == want, (name, length, step, head, lead)
                        assert asked.sum() == m and asked.max() == 1  # the rank of a call is gathered once
                        windows += len(got)
    # one and two empty trips between the calls (a trip is 128 bases), and three of them
    for gaps in ([260, 2, 2], [2, 260, 2], [2, 2, 390], [260, 260, 260], [390, 130, 390], [130, 390, 16, 260, 2, 2, 5, 16]):
        at = [7]
        for d in gaps[:m - 1]:
            at.append(at[-1] + d)
        if len(at) < 4:
            continue
        for step in (1, -1):
            body, numbers = placed(1024, at, "".join(rng.choice("zZ") for _ in at), 5, step) if step == 1 else \
                placed(1024, at, "".join(rng.choice("zZ") for _ in at), 5 + len(at), step)
            want = sorted(epi_walk(body, numbers))
            assert len(want) == len(at) - 3
            for head in range(16):
                assert read_through_the_fold(harness, body, numbers, 3, (head - 3) % 16) == want, (gaps, step, head)
                windows += len(want)
    assert windows > 500


def test_dense_slices_blanks_doubled_calls_and_long_reads(harness):
    # the densest slice, CGCGCGCG x 2: eight calls in sixteen bases, at every alignment; then a whole read of them
    for n_calls, length in ((8, 16), (8, 40), (512, 1024)):
        at = [2 * k for k in range(n_calls)]
        for step in (1, -1):
            body, numbers = placed(length, at, "zZzzZZzZ" * (n_calls // 8), 1000, step)
            want = sorted(epi_walk(body, numbers))
            assert len(want) == n_calls - 3 and len(set(want)) == len(want)
            for head in range(16):
                assert read_through_the_fold(harness, body, numbers, 1, (head - 1) % 16) == want, (n_calls, head)
    # a '.' on each of the four members of a chain of 7, calls 20 apart: chains of 6, 1 + 5, 2 + 4, 3 + 3
    at = [9 + 20 * k for k in range(7)]
    for blank, left in ((0, 3), (1, 2), (2, 1), (3, 0)):
        body, numbers = placed(300, at, "zzZzZZz")
        body = body[:at[blank]] + b"." + body[at[blank] + 1:]
        want = sorted(epi_walk(body, numbers))
        assert len(want) == left
        for head in range(16):
            assert read_through_the_fold(harness, body, numbers, 0, head) == want, (blank, head)
    # a mismatch (another letter) and an uncalled reference CpG break the chain the same way; a z off every pair does not
    body, numbers = placed(300, at, "zzZxZZz")
    assert epi_walk(body, numbers) == [] == read_through_the_fold(harness, body, numbers, 0, 0)
    body, numbers = placed(300, at, "zzZzZZz")
    for i in (11, 30, 50):  # z's that lie on no pair
        body = body[:i] + b"z" + body[i + 1:]
    assert len(epi_walk(body, numbers)) == 4 and read_through_the_fold(harness, body, numbers, 0, 3) == sorted(epi_walk(body, numbers))
    # a doubled call: the same pair twice in a chain of 8 splits it into 5 and 4 (the second call starts the second chain)
    for where in range(8):
        at = [3 + 6 * k for k in range(9)]
        body, numbers = placed(300, at, "zZzZzzZZz")
        for k in range(where + 1, 9):
            numbers[at[k]] -= 1
        want = sorted(epi_walk(body, numbers))
        assert len(want) == max(where + 1 - 3, 0) + max(8 - where - 3, 0)
        for head in range(16):
            assert read_through_the_fold(harness, body, numbers, 0, head) == want, (where, head)
    # a chain that turns round: 5 6 7 8 7 6 5 gives the windows 5..8 up and 8..5 down, nothing across the turn
    at = [4 + 9 * k for k in range(7)]
    body, numbers = placed(300, at, "zZzZzZz")
    for k, j in enumerate([5, 6, 7, 8, 7, 6, 5]):
        numbers[at[k]] = j
    want = sorted(epi_walk(body, numbers))
    assert [w[0] for w in want] == [5, 5]
    for head in range(16):
        assert read_through_the_fold(harness, body, numbers, 0, head) == want
    # random call strings on random pair numbers, every length that matters
    rng = random.Random(46)
    windows = 0
    for length in (1, 3, 4, 15, 16, 17, 31, 127, 128, 129, 300, 1024):
        for al in ("zZ", "zZ..", "zZ" + "." * 14, "zZxXhHuU.A"):
            body = bytes(ord(rng.choice(al)) for _ in range(length))
            numbers, j, down = [], 5000, rng.random() < 0.5
            for i in range(length):
                r = rng.random()
                numbers.append(-1 if r < 0.05 else j)
                if r > 0.1:
                    j += (-1 if down else 1) * (1 if rng.random() < 0.9 else rng.choice([0, 2, -1]))
            want = sorted(epi_walk(body, numbers))
            windows += len(want)
            for shift in range(16):
                for lead, tail in ((0, 0), (shift * 7 % 16, 16)):
                    assert read_through_the_fold(harness, body, numbers, lead, shift, tail) == want, (length, al, shift, lead)
    assert windows > 1000


# ---------------------------------------------------------------------------
# batches as the kernel takes them
# ---------------------------------------------------------------------------
def built(harness, seqs):
    text = "".join(seqs)
    start = np.zeros(len(seqs) + 1, dtype=np.uint32)
    start[1:] = np.cumsum([len(s) for s in seqs])
    bits = np.full(harness.cpgpairs_harness_bit_words(len(text)), 0xFFFFFFFF, dtype=np.uint32)
    dirs = np.full(harness.cpgpairs_harness_dir_entries(len(text)), 0xFFFFFFFF, dtype=np.uint32)
    n_pairs = harness.cpgpairs_harness_build(text.encode(), len(text), start.ctypes.data, len(seqs), bits.ctypes.data, dirs.ctypes.data)
    return text, start, bits, dirs, n_pairs


def harness_table(harness, seqs, h, skip=None, stride=16, shift=0):
    text, start, bits, dirs, n_pairs = built(harness, seqs)
    calls, offsets, rec = h.arrays(stride)
    raw = np.full(calls.size + 64, ord("z"), dtype=np.uint8)
    a = (-raw.ctypes.data) % 16 + shift
    raw[a:a + calls.size] = calls
    table = np.zeros((max(n_pairs, 1), 16), dtype=np.uint32)
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
    harness.epi_harness_batch(bits.ctypes.data, dirs.ctypes.data, len(text), start.ctypes.data, len(seqs), raw.ctypes.data + a,
                              offsets.ctypes.data, len(h.pos), rec.ctypes.data, rec.strides[0] if len(h.pos) > 1 else stride,
                              None if sk is None else sk.ctypes.data, 1, table.ctypes.data)
    return table[:n_pairs].astype(np.uint64)


def test_batches_as_the_kernel_takes_them(harness):
    g, where = epi_genome()
    pairs = find_pairs(g.text, g.start_index)
    hp, n_windows = placement_cases(g, where)
    assert int(want_of(hp, g).sum()) == n_windows
    he, n_edge, n_exact = edge_cases(g, where)
    assert int(want_of(he.head(n_exact), g).sum()) == n_edge
    # reads of 1,024 calls count, reads of 1,025 do not
    st = where["stretch"]
    he.add(st, "+", (b"z." * 40 + b"." * 1024)[:1024]).add(st, "+", (b"z." * 40 + b"." * 1024)[:1025])
    for h in (hp, he):
        want = want_of(h, g)
        for shift in (0, 5, 15):
            assert np.array_equal(harness_table(harness, g.seqs, h, shift=shift), want), shift
    end1 = int(g.start_index[2])
    j = pairs.index(end1 - 9)
    want = want_of(he, g)
    assert want[j].sum() > 0 and not want[j + 1:j + 4].any() and not want[-3:].any()  # no window across the chromosome end
    rng = random.Random(44)
    for trial in range(12):
        hr = random_reads(g, rng, 300, trial % 2 == 0)
        skip = [rng.choice([0, 0, 0, 1, 200]) for _ in hr.pos]
        got = harness_table(harness, g.seqs, hr, skip, stride=64 if trial % 3 == 0 else 16, shift=trial)
        assert np.array_equal(got, want_of(hr, g, skip)) and got.sum() > 20, trial
    # many small chromosomes of CpG-rich sequence, reads across their ends, on both strands
    rnd = lambda n: "".join(rng.choice("ACGTCGCG") for _ in range(n))
    from test_gpu_meth_contigs import Genome
    small = Genome(["s%d" % i for i in range(40)], [rnd(rng.choice([1, 2, 3, 40, 90, 200])) for _ in range(40)])
    hr = random_reads(small, rng, 600, True)
    got = harness_table(harness, small.seqs, hr)
    assert np.array_equal(got, want_of(hr, small)) and got.sum() > 100


# ---------------------------------------------------------------------------
# the statistics, the writer, the merge
# ---------------------------------------------------------------------------
def count_vectors():
    rng = random.Random(45)
    out = [tuple(1 if p == k else 0 for p in range(16)) for k in range(16)]  # total = 1: one pattern, entropy 0
    out += [(7,) + (0,) * 15, (0,) * 15 + (9,), (5,) + (0,) * 14 + (5,), (1,) * 16, (3,) * 16, (2 ** 32 - 1,) * 16]
    out += [(50000, 0, 0, 1) + (0,) * 12, (0, 2, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 1, 0, 0), (2 ** 32 + 5, 7) + (0,) * 13 + (9,)]
    for _ in range(300):
        k = rng.randrange(1, 17)
        cols = rng.sample(range(16), k)
        out.append(tuple(rng.choice([1, 2, 3, 10, 1000, 50000]) if p in cols else 0 for p in range(16)))
    return out


def test_statistics_and_the_line_writer(harness):
    buf = ctypes.create_string_buffer(1024)
    stats = (ctypes.c_double * 4)()
    for i, n in enumerate(count_vectors()):
        arr = np.array(n, dtype=np.uint64)
        assert harness.epi_harness_stats(arr.ctypes.data, stats) == sum(n)
        want = epi_stats(n)
        for got, w in zip(stats, want):
            assert abs(got - float(w)) <= 1e-12, (n, got, w)
        chrom, pos, end = "chr%d|x" % i, 4294967000 - i, 4294967290
        k = harness.epi_harness_line(chrom.encode(), pos, end, arr.ctypes.data, ctypes.addressof(buf), 1024)
        p = buf.raw[:k].decode()
        assert p.endswith("\n") and p.count("\n") == 1
        p = p[:-1].split("\t")
        assert len(p) == 24 and p[:3] == [chrom, str(pos), str(end)] and [int(v) for v in p[3:20]] == [sum(n)] + list(n)  # counts are exact
        for text, w in zip(p[20:], want):
            assert len(text.split(".")[1]) == 6 and not text.startswith("-") and abs(float(text) - float(w)) <= 1.5e-6, (n, p[20:], want)
    one = np.array((0, 0, 0, 0, 0, 1) + (0,) * 10, dtype=np.uint64)
    k = harness.epi_harness_line(b"c", 9, 30, one.ctypes.data, ctypes.addressof(buf), 1024)
    assert buf.raw[:k].decode() == "c\t9\t30\t1\t0\t0\t0\t0\t0\t1" + "\t0" * 10 + "\t0.500000\t0.000000\t0.000000\t1.000000\n"
    flat = np.array((1,) * 16, dtype=np.uint64)
    k = harness.epi_harness_line(b"c", 0, 6, flat.ctypes.data, ctypes.addressof(buf), 1024)
    assert buf.raw[:k].decode() == "c\t0\t6\t16" + "\t1" * 16 + "\t0.500000\t0.937500\t1.000000\t0.875000\n"
    # Fraction arithmetic of the definitions, spelt out once
    n = (3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 4)
    meth, epipoly, entropy, discordant = epi_stats(n)
    assert meth == Fraction(3 * 4 + 1 * 2, 32) and epipoly == 1 - Fraction(9 + 1 + 16, 64) and discordant == Fraction(1, 8)
    assert abs(entropy + 0.25 * (3 / 8 * math.log2(3 / 8) + 1 / 8 * math.log2(1 / 8) + 0.5 * math.log2(0.5))) < 1e-15


def test_the_merge_of_several_devices(harness):
    rng = random.Random(47)
    for trial in range(200):
        n_dev = rng.randrange(1, 5)
        per_dev, want = [], {}
        for d in range(n_dev):
            rows = []
            for pos in sorted(rng.sample(range(60), rng.randrange(0, 25))):
                n = [rng.choice([0, 0, 1, 5, 2 ** 32 - 1]) for _ in range(16)]
                rows.append([pos, pos + 9] + n)
                acc = want.setdefault(pos, [pos, pos + 9] + [0] * 16)
                for k in range(16):
                    acc[2 + k] += n[k]
            per_dev.append(rows)
        flat = np.array([v for rows in per_dev for r in rows for v in r], dtype=np.uint64)
        counts = np.array([len(rows) for rows in per_dev], dtype=np.uint32)
        out = np.zeros(18 * 64, dtype=np.uint64)
        k = harness.epi_harness_merge(flat.ctypes.data if flat.size else None, counts.ctypes.data, n_dev, out.ctypes.data, 64)
        assert out[:18 * k].reshape(k, 18).tolist() == [want[p] for p in sorted(want)], trial


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
    assert hdr.index("---- adjacent CpG pairs") < hdr.index("---- four-CpG epialleles") < hdr.index("---- options")


def test_binding_surface_and_refusals_without_a_device():
    import walt_amd
    for nm in ("add", "add_device", "extract", "extract_device", "n_pairs", "clear", "handle", "device_bytes", "close"):
        assert hasattr(walt_amd.Epialleles, nm), nm
    assert callable(walt_amd.Index.epialleles)
    p = inspect.signature(walt_amd.Epialleles.extract).parameters
    assert (p["pos_lo"].default, p["pos_hi"].default, p["min_total"].default) == (0, None, 1)
    for fn in (walt_amd.Index.meth_call_batch_device, walt_amd.Pileup.add_batch, walt_amd.Pileup.add_batch_device):
        p = inspect.signature(fn).parameters
        assert p["epi"].default is None and p["epi"].kind is inspect.Parameter.KEYWORD_ONLY and list(p)[-1] == "epi", fn
        assert p["pairs"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    # Index.meth_call_batch shows the parameter list it had (its end is pinned by an older test) and takes epi= all the same,
    # by keyword only
    assert "epi" not in inspect.signature(walt_amd.Index.meth_call_batch).parameters

    class Recorder:
        def _meth_batch(self, pile, *args, **kw):
            return pile, args, kw

    every = ("b", "o", "r", "A", 1, False, False, 2, False, 3, 4, 5, 6, 7, 8, 9)  # bases .. trim3, pairs in its place
    in_order = ("b", "o", "r", "A", 1, False, False, 2, False, 4, 5, 6, 7, 8, 9, 3)  # as the method hands them on
    assert walt_amd.Index.meth_call_batch(Recorder(), *every) == (None, in_order, {})
    pile, args, kw = walt_amd.Index.meth_call_batch(Recorder(), "b", "o", "r", trim3=9, epi="E")
    assert pile is None and args == () and kw["epi"] == "E" and kw["trim3"] == 9 and kw["pairs"] is None and kw["conv"] == "T"
    pile, args, kw = walt_amd.Index.meth_call_batch(Recorder(), *every, epi="E")
    assert dict(kw, epi=None) == dict(zip(("bases", "offsets", "records", "conv", "call_len", "want_calls", "want_counts", "stats",
                                           "want_stats", "pairs", "skip", "excl", "mbias", "mbias_table", "trim5", "trim3"), every), epi=None)
    with pytest.raises(TypeError):
        walt_amd.Index.meth_call_batch(Recorder(), *every, "E")
    dt = walt_amd.epiallele_site_dtype
    assert dt.itemsize == 72 and dt.names == ("pos", "last", "n") and dt["n"].shape == (16,)
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm

    class Named:  # stands for the library: _meth_form only looks the function up by name
        def __getattr__(self, name):
            return name

    form = lambda **kw: walt_amd._meth_form(Named(), kw.pop("device", False), kw.pop("pile", None), **kw)
    assert form(epi=(9,)) == ("walt_meth_pileup_batch_epi", (None,), (None, 1, None, None, 0, 0, 0, None, 9))
    assert form(epi=(9,), pairs=(7,), device=True, pile=3, skip=(5, 2), excl=(6,), mbias=(8, 1), trim=(2, 4)) == \
        ("walt_meth_pileup_batch_epi_device", (3,), (5, 2, 6, 8, 1, 2, 4, 7, 9))
    # without epi: the forms a call always reached
    assert form(pairs=(7,)) == ("walt_meth_pileup_batch_pairs", (None,), (None, 1, None, None, 0, 0, 0, 7))
    assert form(trim=(2, 4))[0] == "walt_meth_pileup_batch_trim" and form()[0] == "walt_meth_call_batch"
    # no device: null objects are refused, not crashed on, and the message names the call
    E = walt_amd.WALT_EINVAL
    h = ctypes.c_void_p()
    assert L.walt_epialleles_create(None, ctypes.byref(h)) == E and not h.value and b"walt_epialleles_create:" in L.walt_last_error()
    assert L.walt_epialleles_batch(None, None, None, 0, None, 16, None, 1) == E
    assert b"walt_epialleles_batch:" in L.walt_last_error() and b"null epiallele table" in L.walt_last_error()
    assert L.walt_epialleles_batch_device(None, None, None, 0, None, 16, None, 1, None) == E and b"walt_epialleles_batch_device:" in L.walt_last_error()
    n = ctypes.c_uint64(0)
    assert L.walt_epialleles_extract(None, 0, 0, 1, None, 0, ctypes.byref(n)) == E and b"walt_epialleles_extract:" in L.walt_last_error()
    assert L.walt_epialleles_extract_device(None, 0, 0, 1, None, 0, None, None) == E and b"walt_epialleles_extract_device:" in L.walt_last_error()
    assert L.walt_epialleles_clear(None) == E and b"walt_epialleles_clear:" in L.walt_last_error()
    assert L.walt_epialleles_device_bytes(None) == 0 and L.walt_epialleles_n_pairs(None) == 0
    L.walt_epialleles_destroy(None)
    assert L.walt_meth_pileup_batch_epi(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None, 1, None,
                                        None, 0, 0, 0, None, None) == E and b"walt_meth_pileup_batch_epi:" in L.walt_last_error()
    assert L.walt_meth_pileup_batch_epi_device(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None, 1,
                                               None, None, 0, 0, 0, None, None, None) == E
    assert b"walt_meth_pileup_batch_epi_device:" in L.walt_last_error()


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


def test_cli_parses_the_options_in_every_mode(tmp_path):
    pr = run([])
    assert pr.returncode == 0 and " -ME " in pr.stdout and " -MEN <n> " in pr.stdout and " -MA " in pr.stdout, pr.stdout
    idx, out = str(tmp_path / "none.dbindex"), str(tmp_path / "o.mr")
    pair, single = ["-1", "a.fastq", "-2", "b.fastq"], ["-r", "x.fastq"]
    base = ["-i", idx, "-o", out]
    modes = [(single, []), (single, ["-A"]), (single, ["-R"]), (pair, []), (pair, ["-P"]), (pair, ["-RP"])]
    # the three spellings are known in every mode, alone (a consumer) and beside the others: the run gets as far as the index check
    for reads, mode in modes:
        for flag in ("-ME", "-epialleles", "--epialleles"):
            for extra in ([], ["-M", "-sam"], ["-MA", "-MC", "-MB", "-ML"], ["-D", "-C", "AGATCGGAAGAGC"], ["-I5", "3"], ["-F", "3", "-FP", "20"],
                          ["-g", "0,0"], ["-MEN", "5"]):
                pr = run(base + reads + mode + extra + [flag])
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, mode, extra, pr.stdout)
    # -I5 3 -ME, -NO -ME with -1 / -2, the -F options: -ME is something for them to act on
    for args in (single + ["-I5", "3", "-ME"], pair + ["-NO", "-ME"], pair + ["-I3R2", "2", "-NO", "-ME"], single + ["-FC", "2", "-ME"]):
        pr = run(base + args)
        assert pr.returncode != 0 and "index file missing" in pr.stdout, (args, pr.stdout)
    pr = run(base + single + ["-NO", "-ME"])
    assert pr.returncode != 0 and "paired-end only" in pr.stdout
    # -MEN: its spellings and its range, and that it goes with -ME only
    for flag in ("-MEN", "-epiallele-min", "--epiallele-min-reads"):
        for value in ("1", "3", "1000000"):
            pr = run(base + single + ["-ME", flag, value])
            assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, value, pr.stdout)
        for value in ("0", "1000001", "-3", "x", "2.5", ""):
            pr = run(base + single + ["-ME", flag, value])
            assert pr.returncode != 0 and "1 to 1000000" in pr.stdout and "index file missing" not in pr.stdout, (flag, value, pr.stdout)
        for others in ([], ["-MA"], ["-M", "-MC"]):
            pr = run(base + single + others + [flag, "3"])
            assert pr.returncode != 0 and "-ME" in pr.stdout and "index file missing" not in pr.stdout, (flag, others, pr.stdout)
    assert not os.path.exists(out) and not os.path.exists(out + ".epialleles")


def test_per_lane_logic_under_the_host_sanitizers(scratch):
    """tests/epialleles_sanitize_main.cpp, a stand-alone program over tests/epialleles_harness.cpp built with the host's
    address and undefined-behaviour sanitizers: random genomes and batches, bitmap, directory, table and calls each in a heap
    block of exactly its size -- a load or an add outside them ends the program, and so does a table that differs from a
    plain walk"""
    exe = os.path.join(scratch, "epialleles_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(refio.HERE, "epialleles_sanitize_main.cpp")] + SOURCES + ["-o", exe], check=True, timeout=300)
    pr = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert pr.returncode == 0 and pr.stdout.startswith("ok "), pr.stdout[-2000:]
