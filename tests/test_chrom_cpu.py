"""The chromosome look-up every kernel takes a record's bounds [lo, hi) from (walt_amd/csrc/chrom_core.h: ChromTab,
chrom_find, chrom_bounds), compiled with g++ (tests/chrom_harness.cpp) and compared with numpy.searchsorted over the
chromosome starts on all three of its paths: every start staged (up to 1,023 sequences), five neighbouring words (up to
4,092), a second bisection over the full array (more).  The harness is built twice, plain and with
-fsanitize=address,undefined, and keeps both arrays in heap blocks of exactly the words the look-up may touch, so the
second build also pins that nothing beyond start[n_chrom] is read -- for positions at or beyond the genome's end too,
which the look-up answers with the last chromosome."""
import os
import random
import subprocess

import numpy as np
import pytest

import refio

K_LDS = 1023  # chrom_core.h kLdsChroms

# every count at which the path or the shift changes, its neighbours, and counts that are no multiple of 2^shift
COUNTS = [1, 2, 3, 1022, 1023, 1024, 1025, 2046, 2047, 3001, 4092, 4093, 6007, 8184, 8185, 20011]


def shift_of(n):
    """smallest shift with ceil(n / 2^shift) <= K_LDS"""
    sh = 0
    while -(-n // (1 << sh)) > K_LDS:
        sh += 1
    return sh


def lengths_of(kind, n):
    if kind == "uniform":  # 7 bases each, chromosomes of 1 and 2 bases among them (also first and last where n allows)
        L = [7] * n
        for i in range(n):
            if i % 5 == 1 or (i == n - 1 and n > 2):
                L[i] = 1
            elif i % 5 == 3 or (i == 0 and n > 2):
                L[i] = 2
        return L
    rng = random.Random(1000 + n)
    return [rng.choice([1, 1, 2, 2, 3, 16, 17, rng.randrange(1, 400), rng.randrange(1, 400), rng.randrange(1, 70000)]) for _ in range(n)]


def queries_of(start):
    """every chromosome's first, second, last and last-but-one base, and the genome's last base (all inside the genome)"""
    lo, hi = start[:-1].astype(np.int64), start[1:].astype(np.int64)
    q = np.concatenate([lo, lo + 1, hi - 1, hi - 2, [int(start[-1]) - 1]])
    q = q[(q >= 0) & (q < int(start[-1]))]
    return q.astype(np.uint32)


@pytest.fixture(scope="module", params=["plain", "sanitised"])
def chrom_harness(request, scratch):
    exe = os.path.join(scratch, "chrom_harness_" + request.param)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] if request.param == "sanitised" else []
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-I", os.path.join(refio.ROOT, "walt_amd", "csrc"),
                    os.path.join(refio.HERE, "chrom_harness.cpp"), "-o", exe], check=True, timeout=300)
    if request.param == "sanitised":
        assert b"__asan_report_load4" in open(exe, "rb").read(), "the sanitised build carries no address checks"
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    serial = [0]

    def run(start, pos):
        serial[0] += 1
        fin, fout = os.path.join(scratch, "chrom_%s_%d.in" % (request.param, serial[0])), os.path.join(scratch, "chrom_%s_%d.out" % (request.param, serial[0]))
        start = np.ascontiguousarray(start, dtype="<u4")
        pos = np.ascontiguousarray(pos, dtype="<u4")
        with open(fin, "wb") as f:
            f.write(np.array([start.size - 1, pos.size], dtype="<u4").tobytes() + start.tobytes() + pos.tobytes())
        pr = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
        assert pr.returncode == 0, "chrom_harness (%s) exit %d:\n%s" % (request.param, pr.returncode, pr.stdout[-4000:])
        out = np.fromfile(fout, dtype="<u4")
        os.remove(fin)
        os.remove(fout)
        assert out.size == 3 + 3 * pos.size
        return tuple(int(x) for x in out[:3]), out[3:].reshape(-1, 3)

    return run


def test_shift_thresholds():
    """the counts above sit on both sides of every threshold, and some are no multiple of their 2^shift"""
    assert [shift_of(n) for n in (1023, 1024, 2046, 2047, 4092, 4093, 8184, 8185)] == [0, 1, 1, 2, 2, 3, 3, 4]
    assert {shift_of(n) for n in COUNTS} == {0, 1, 2, 3, 4, 5}
    for sh in (1, 2, 3, 4, 5):
        assert any(shift_of(n) == sh and n % (1 << sh) for n in COUNTS), sh  # a partial final interval
    for sh in (1, 2, 3):
        assert any(shift_of(n) == sh and n % (1 << sh) == 0 for n in COUNTS), sh  # a full one


@pytest.mark.parametrize("kind", ["uniform", "random"])
@pytest.mark.parametrize("n_chrom", COUNTS)
def test_lookup_equals_searchsorted(chrom_harness, n_chrom, kind):
    L = lengths_of(kind, n_chrom)
    if n_chrom > 100 or (kind == "uniform" and n_chrom > 2):
        assert 1 in L and 2 in L
    start = np.zeros(n_chrom + 1, dtype=np.uint32)
    start[1:] = np.cumsum(L)
    pos = queries_of(start)
    assert pos.size >= min(4 * n_chrom, int(start[-1])) - 3 and int(pos.max()) == int(start[-1]) - 1
    (shift, m, top), got = chrom_harness(start, pos)
    sh = shift_of(n_chrom)
    assert (shift, m) == (sh, -(-n_chrom // (1 << sh))) and top == 1 << (m.bit_length() - 1)
    want = np.searchsorted(start, pos, "right").astype(np.int64) - 1
    assert want.min() == 0 and want.max() == n_chrom - 1 and np.unique(want).size == n_chrom  # every chromosome is asked for
    bad = np.flatnonzero((got[:, 0] != want) | (got[:, 1] != start[want]) | (got[:, 2] != start[want + 1]))
    assert bad.size == 0, "n_chrom %d %s: %d of %d differ, first pos %d got %s want (%d, %d, %d)" % (
        n_chrom, kind, bad.size, pos.size, pos[bad[0]], got[bad[0]], want[bad[0]], start[want[bad[0]]], start[want[bad[0]] + 1])


@pytest.mark.parametrize("kind", ["uniform", "random"])
@pytest.mark.parametrize("n_chrom", COUNTS)
def test_beyond_the_genome_is_the_last_chromosome(chrom_harness, n_chrom, kind):
    """positions at or beyond the genome's end: the last chromosome's bounds, and (sanitised build) no word past the arrays"""
    L = lengths_of(kind, n_chrom)
    start = np.zeros(n_chrom + 1, dtype=np.uint32)
    start[1:] = np.cumsum(L)
    glen = int(start[-1])
    pos = np.array([glen, glen + 1, 2 ** 32 - 1, glen - 1], dtype=np.uint32)
    _, got = chrom_harness(start, pos)
    for p, g in zip(pos, got):
        assert tuple(int(x) for x in g) == (n_chrom - 1, int(start[n_chrom - 1]), glen), (n_chrom, kind, int(p), g)
