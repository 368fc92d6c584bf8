"""Called sites (include/walt_amd.h, "called sites"), the parts that need no device: the bin, the verdict, the binomial tail,
Benjamini-Hochberg over bins and the table (walt_amd/csrc/sitecall_core.h), compiled with g++ (tests/sitecall_harness.cpp)
and compared with exact fractions and with the pure-Python restatement of tests/test_gpu_sitecall.py; the <out>.methsites
and <out>.sitestats writers and the value parsers of hostio.h; the exports, the binding's surface and refusals without a
device; bin/walt's options; and the harness as a stand-alone program under the host's sanitizers."""
import ctypes
import math
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import refio
from test_gpu_sitecall import BINS, DEPTH, bh_clearance, py_pval, site_bin, table_from_cutoffs, textbook_bh

NAMES = ("walt_pileup_depth_hist", "walt_pileup_depth_hist_device", "walt_pileup_call_sites", "walt_pileup_call_sites_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")
SOURCES = [os.path.join(refio.HERE, "sitecall_harness.cpp")]

# The agreement of the C++ tail with exact arithmetic.  Measured over every d <= 60, every m and the four rates of
# test_pval_against_exact_fractions: the worst relative error is 1.2e-13 (d 56, m 49, r 1/1000: 49 terms of which the
# first carries the sum; the error is lgamma's and exp's, a few units in the last place of an exponent near 320).  The
# bound is that times a margin of 8.
EXACT_TOLERANCE = 8 * 1.2e-13


def large_tolerance(d):
    """At larger depths the error is that of the exponent's largest summand: lgamma(d + 1) is known to half a unit in its
    last place, and so are the two it is subtracted from; a margin of 8 over one such unit, and never below the bound of
    the small depths.  (Measured against the Python restatement at d = 10000: 2.9e-11, where this gives 1.2e-10.)"""
    lg = math.lgamma(d + 1)
    return max(EXACT_TOLERANCE, 8 * (math.nextafter(lg, math.inf) - lg))


@pytest.fixture(scope="module")
def harness(scratch):
    so = os.path.join(scratch, "libsitecall_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC] + SOURCES +
                   ["-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci, dbl = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_double
    L.sitecall_harness_bin.argtypes = [u32, u32]
    L.sitecall_harness_bin.restype = u32
    L.sitecall_harness_pval.argtypes = [u64, u64, dbl]
    L.sitecall_harness_pval.restype = dbl
    L.sitecall_harness_verdict.argtypes = [vp, u32, u32, u32]
    L.sitecall_harness_verdict.restype = u32
    L.sitecall_harness_context.argtypes = [vp, vp, vp, u64, dbl, dbl, u32, vp, vp, vp]
    L.sitecall_harness_parse_fraction.argtypes = [ctypes.c_char_p, ci, vp]
    L.sitecall_harness_parse_depth.argtypes = [ctypes.c_char_p, vp]
    L.sitecall_harness_line.argtypes = [ctypes.c_char_p, u32, vp, dbl, vp, u32]
    L.sitecall_harness_line.restype = u32
    L.sitecall_harness_block.argtypes = [ctypes.c_char_p, vp, ci, dbl, dbl, u32, vp, vp, vp, vp, vp, u32]
    L.sitecall_harness_block.restype = u32
    return L


# ---------------------------------------------------------------------------
# per lane: the bin and the verdict
# ---------------------------------------------------------------------------
def test_bin_is_a_bijection(harness):
    import walt_amd
    seen = []
    for d in range(1, DEPTH + 1):
        for m in range(d + 1):
            b = harness.sitecall_harness_bin(d, m)
            assert b == site_bin(d, m) == walt_amd.sitecall_bin(d, m)
            seen.append(b)
    assert seen == list(range(BINS)) and BINS == walt_amd.SITECALL_BINS and DEPTH == walt_amd.SITECALL_DEPTH
    for d, m in ((0, 0), (128, 0), (5, 6), (5, -1)):
        with pytest.raises(ValueError):
            walt_amd.sitecall_bin(d, m)


def test_verdict_against_the_table(harness):
    rng = random.Random(2)
    table = np.array([[rng.randrange(0, d + 3) for d in range(128)] for _ in range(4)], dtype=np.uint32)
    full = 0xFFFFFFFF
    seen = set()
    for trial in range(20000):
        c = rng.randrange(4)
        m, u = rng.choice([(rng.randrange(0, 130), rng.randrange(0, 130)), (full, full), (full, 0), (0, full), (127, 0), (0, 127),
                           (128, 0), (64, 64), (63, 64)])
        if m + u == 0:
            continue
        want = 2 if m + u > DEPTH else 1 if m >= table[c, m + u] else 0
        assert harness.sitecall_harness_verdict(table.ctypes.data, c, m, u) == want, (c, m, u)
        seen.add((want, m + u == DEPTH, m + u == DEPTH + 1))
    assert {(2, False, True), (1, True, False), (0, True, False)} <= seen


# ---------------------------------------------------------------------------
# the binomial tail
# ---------------------------------------------------------------------------
def test_pval_against_exact_fractions(harness):
    """every d <= 60 and every m at four rates: the measured worst relative error is 1.2e-13, the bound 8 times that"""
    worst = 0.0
    for r in (Fraction(1, 1000), Fraction(1, 200), Fraction(1, 20), Fraction(1, 2)):
        rf = float(r)
        re = Fraction(rf)  # the rate the code is given, exactly
        for d in range(1, 61):
            tail = Fraction(0)
            for m in range(d, -1, -1):
                tail += math.comb(d, m) * re ** m * (1 - re) ** (d - m)
                got = harness.sitecall_harness_pval(d, m, rf)
                if m == 0:
                    assert got == 1.0 and tail == 1
                    continue
                worst = max(worst, float(abs(Fraction(got) - tail) / tail))
    print("worst relative error against exact fractions: %.3g" % worst)
    assert worst <= EXACT_TOLERANCE


def test_pval_at_large_depths_against_the_restatement(harness):
    worst = {}
    for d in (127, 128, 1000, 10000):
        for r in (0.001, 0.005, 0.05, 0.5):
            mode = int(d * r)
            for m in sorted({1, 2, 3, 5, 8, 13, 30, 59, mode, mode + 1, mode + 5, 2 * mode + 3, d // 2, d - 1, d} - {0}):
                if m > d:
                    continue
                want = py_pval(d, m, r)
                got = harness.sitecall_harness_pval(d, m, r)
                if want < 1e-300:  # below the doubles' normal range the restatement's own terms lose their digits
                    assert got < 1e-290
                    continue
                worst[d] = max(worst.get(d, 0.0), abs(got - want) / want)
    print("worst relative error against the restatement by depth:", {d: "%.3g" % w for d, w in worst.items()})
    for d, w in worst.items():
        assert w <= large_tolerance(d), (d, w)


def test_pval_edges_and_the_cost_of_deep_sites(harness):
    import time
    p = harness.sitecall_harness_pval
    for d in (1, 2, 127, 128, 10 ** 6, 2 ** 33 - 2):
        assert p(d, 0, 0.01) == 1.0 and p(d, 0, 0.0) == 1.0          # m == 0
        assert p(d, 1, 0.0) == 0.0 and p(d, d, 0.0) == 0.0            # r == 0, m >= 1
    for d in (1, 2, 7, 60, 127):
        for r in (0.001, 0.05, 0.5):
            assert abs(p(d, d, r) - r ** d) <= EXACT_TOLERANCE * r ** d  # m == d: one term
            assert abs(p(d, 1, r) - (1 - (1 - r) ** d)) <= 1e-12           # m == 1: all but one term
    # monotone in m, and a deep site costs the width of its distribution, not its depth
    t0 = time.time()
    for d in (10 ** 6, 2 ** 33 - 2):
        last = 1.0
        for m in (0, 1, int(d * 0.005) - 1000, int(d * 0.005), int(d * 0.005) + 1000, d // 2, d):
            got = p(d, max(m, 0), 0.005)
            assert 0.0 <= got <= last
            last = got
        assert 0.4 < p(d, int(d * 0.005), 0.005) < 0.6
    assert time.time() - t0 < 5.0


# ---------------------------------------------------------------------------
# Benjamini-Hochberg over bins, and the table
# ---------------------------------------------------------------------------
def run_context(harness, hist, deep, r, alpha, min_depth):
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    dd = np.array([d for d, _ in deep], dtype=np.uint64)
    dm = np.array([m for _, m in deep], dtype=np.uint64)
    table = np.zeros(128, dtype=np.uint32)
    out = np.zeros(2, dtype=np.uint64)
    cutoff = ctypes.c_double(0.0)
    has = harness.sitecall_harness_context(hist.ctypes.data, dd.ctypes.data, dm.ctypes.data, len(deep), r, alpha, min_depth,
                                           table.ctypes.data, out.ctypes.data, ctypes.byref(cutoff))
    return (cutoff.value if has else None), int(out[0]), int(out[1]), table


def expand(hist, deep, r, min_depth):
    """one p-value per tested site: the bins' sites one by one, then the deep sites"""
    ps = []
    for d in range(min_depth, DEPTH + 1):
        for m in range(d + 1):
            ps += [py_pval(d, m, r)] * int(hist[site_bin(d, m)])
    return ps + [py_pval(d, m, r) for d, m in deep]


def hand_histograms():
    """(name, hist, deep, r, alpha): nothing passes, everything passes, a tie group that straddles the line, deep sites mixed
    in, and random shallow libraries at three seeds"""
    out = []
    h = np.zeros(BINS, dtype=np.uint64)
    for d in range(1, 20):
        h[site_bin(d, 0)] = 50 + d
    h[site_bin(1, 1)] = 3  # p = r, far above its line
    out.append(("nothing passes", h.copy(), [], 0.05, 0.01))
    h = np.zeros(BINS, dtype=np.uint64)
    for d in range(5, 40):
        h[site_bin(d, d)] = 7
        h[site_bin(d, d - 1)] = 2
    out.append(("everything passes", h.copy(), [(200, 150), (1000, 999)], 0.01, 0.05))
    # 40 sites (2, 2), p = r^2 = 1e-4, among 1000 sites: sites 1 .. 19 of the group alone lie above their line
    # (i * 0.005 / 1000 < 1e-4 for i < 20), the group's last lies below it (40 * 0.005 / 1000 = 2e-4)
    h = np.zeros(BINS, dtype=np.uint64)
    h[site_bin(2, 2)] = 40
    h[site_bin(1, 0)] = 960
    out.append(("a tie group straddles the line", h.copy(), [], 0.01, 0.005))
    h = np.zeros(BINS, dtype=np.uint64)
    h[site_bin(127, 0)] = 300
    h[site_bin(127, 5)] = 4
    h[site_bin(127, 9)] = 2
    h[site_bin(6, 2)] = 30
    out.append(("deep sites mixed in", h.copy(), [(128, 0), (128, 6), (128, 12), (5000, 30), (5000, 60), (10000, 50), (2000, 2000)], 0.005, 0.05))
    for seed in (1, 2, 3):
        rng = random.Random(seed)
        h = np.zeros(BINS, dtype=np.uint64)
        for _ in range(3000):
            d = min(DEPTH, 1 + int(rng.expovariate(1 / 12.0)))
            level = rng.choice([0.004, 0.004, 0.3, 0.8])
            m = sum(rng.random() < level for _ in range(d))
            h[site_bin(d, m)] += 1
        deep = [(d, sum(rng.random() < 0.02 for _ in range(d))) for d in (130, 200, 300)]
        out.append(("random %d" % seed, h, deep, 0.004, 0.01))
    return out


@pytest.mark.parametrize("min_depth", [1, 5, 127])
def test_bh_over_bins_equals_the_textbook_over_sites(harness, min_depth):
    seen = set()
    for name, hist, deep, r, alpha in hand_histograms():
        ps = expand(hist, deep, r, min_depth)
        # no group's p-value within relative 1e-6 of its line: the two sides cannot disagree over a rounding
        assert bh_clearance(ps, alpha) > 1e-6, (name, min_depth)
        want = textbook_bh(ps, alpha) if ps else None
        cutoff, tested, called, table = run_context(harness, hist, deep, r, alpha, min_depth)
        assert tested == len(ps), (name, min_depth)
        assert (cutoff is None) == (want is None), (name, min_depth, cutoff, want)
        want_called = 0 if want is None else sum(p <= want for p in ps)
        assert called == want_called, (name, min_depth, called, want_called)
        if want is not None:
            assert abs(cutoff - want) <= (EXACT_TOLERANCE if not deep else large_tolerance(max(d for d, _ in deep))) * want, (name, cutoff, want)
        # the table: consistent with the p-values (monotone in m), d + 1 below min_depth and where nothing passes
        want_table = table_from_cutoffs([want] * 4, r, min_depth)[0]
        assert table[1:].tolist() == want_table[1:].tolist(), (name, min_depth)
        for d in range(1, DEPTH + 1):
            t = int(table[d])
            assert 1 <= t <= d + 1
            if d < min_depth or want is None:
                assert t == d + 1
            else:
                assert all((harness.sitecall_harness_pval(d, m, r) <= cutoff) == (m >= t) for m in range(1, d + 1)), (name, d)
        seen.add("none" if want is None else "all" if called == tested else "some")
        if name == "a tie group straddles the line" and min_depth == 1:
            assert called == 40 and sum(1 for i in range(1, 41) if 1e-4 > i * alpha / 1000) == 19
        if name == "nothing passes":
            assert want is None
        if name == "everything passes" and min_depth <= 5:
            assert called == tested > 0
        if name == "deep sites mixed in" and min_depth == 1:
            assert 0 < called < tested and table[127] in (5, 9)
    assert {"none", "some"} <= seen


def test_bh_without_a_site_and_at_rate_zero(harness):
    hist = np.zeros(BINS, dtype=np.uint64)
    cutoff, tested, called, table = run_context(harness, hist, [], 0.01, 0.05, 1)
    assert cutoff is None and tested == called == 0 and table[1:].tolist() == list(range(2, 129))
    hist[site_bin(3, 0)], hist[site_bin(3, 1)], hist[site_bin(9, 9)] = 10, 2, 1
    cutoff, tested, called, table = run_context(harness, hist, [(500, 1), (500, 0)], 0.0, 0.05, 1)
    assert cutoff == 0.0 and tested == 15 and called == 4 and table[1:].tolist() == [1] * 127  # a methylated call is impossible at r = 0


# ---------------------------------------------------------------------------
# the command line's pieces
# ---------------------------------------------------------------------------
def test_writers_and_value_parsers(harness):
    import walt_amd
    buf = ctypes.create_string_buffer(1024)
    site = np.zeros(1, dtype=walt_amd.meth_site_dtype)
    full = 0xFFFFFFFF
    for row, chrom, start, pval, want in (
            ((1234, 3, 4, ord("+"), 0, 0), "chr1", 1000, 0.000123456789, "chr1\t234\t+\tCpG\t3\t4\t0.000123457\n"),
            ((7, 5, 0, ord("-"), 2, 0), "a b", 7, 1e-30, "a b\t0\t-\tCHH\t5\t0\t1e-30\n"),
            ((full - 1, full, full, ord("-"), 3, 1), "x", 0, 0.0, "x\t4294967294\t-\tunknown\t4294967295\t4294967295\t0\n"),
            ((50, 1, 2, ord("+"), 1, 0), "chrB", 50, 0.25, "chrB\t0\t+\tCHG\t1\t2\t0.25\n")):
        site[0] = row
        n = harness.sitecall_harness_line(chrom.encode(), start, site.ctypes.data, pval, buf, 1024)
        assert buf.raw[:n].decode() == want
    tested = np.array([100, 50, 1 << 40, 0], dtype=np.uint64)
    called = np.array([7, 0, 12345, 0], dtype=np.uint64)
    has = np.array([1, 0, 1, 0], dtype=np.int32)
    cutoff = np.array([0.00123456789, 0.0, 1e-9, 0.0], dtype=np.float64)
    counts = np.array([12, 3988], dtype=np.uint64)
    n = harness.sitecall_harness_block(b"lambda", counts.ctypes.data, 1, 12 / 4000, 0.01, 1, tested.ctypes.data, called.ctypes.data,
                                       has.ctypes.data, cutoff.ctypes.data, buf, 1024)
    assert buf.raw[:n].decode() == ("control: lambda\ncontrol meth: 12\ncontrol unmeth: 3988\nnon-conversion rate: 0.003\nrule\t0.01\t1\n"
                                    "CpG\t100\t7\t0.00123457\nCHG\t50\t0\tNA\nCHH\t1099511627776\t12345\t1e-09\nunknown\t0\t0\tNA\n")
    n = harness.sitecall_harness_block(b"given", None, 1, 0.005, 0.05, 127, tested.ctypes.data, called.ctypes.data, has.ctypes.data,
                                       cutoff.ctypes.data, buf, 1024)
    assert buf.raw[:n].decode().startswith("control: given\ncontrol meth: NA\ncontrol unmeth: NA\nnon-conversion rate: 0.005\nrule\t0.05\t127\nCpG\t")
    has[:] = 0
    called[:] = 0
    n = harness.sitecall_harness_block(b"chrM", counts.ctypes.data, 0, 0.0, 0.01, 1, tested.ctypes.data, called.ctypes.data, has.ctypes.data,
                                       cutoff.ctypes.data, buf, 1024)
    assert "non-conversion rate: NA\n" in buf.raw[:n].decode() and buf.raw[:n].decode().count("\tNA\n") == 4
    # the values of -MSR (0 <= r < 1), -MSA (0 < a < 1) and -MSD (1 to 127)
    out = ctypes.c_double(7.0)
    for text, zero, want in (("0", 1, 0.0), ("0.005", 1, 0.005), ("5e-3", 1, 0.005), (".5", 0, 0.5), ("0.999999", 0, 0.999999), ("1E-2", 0, 0.01)):
        assert harness.sitecall_harness_parse_fraction(text.encode(), zero, ctypes.byref(out)) == 1 and out.value == want, text
    out.value = 7.0
    for text, zero in (("0", 0), ("0.0", 0), ("1", 1), ("1.0", 0), ("-0.1", 1), ("2", 1), ("x", 1), ("", 1), (" 0.5", 1), ("0.5 ", 1), ("nan", 1),
                       ("inf", 1), ("0x1p-3", 1), ("e-3", 1), ("0.5.5", 1), ("1e400", 1), ("+0.5", 1), ("0." + "1" * 30, 1)):
        assert harness.sitecall_harness_parse_fraction(text.encode(), zero, ctypes.byref(out)) == 0 and out.value == 7.0, text
    depth = ctypes.c_uint32(77)
    for text, want in (("1", 1), ("127", 127), ("005", 5)):
        assert harness.sitecall_harness_parse_depth(text.encode(), ctypes.byref(depth)) == 1 and depth.value == want
    depth.value = 77
    for text in ("0", "128", "-1", "", "2.5", "x", " 3"):
        assert harness.sitecall_harness_parse_depth(text.encode(), ctypes.byref(depth)) == 0 and depth.value == 77, text


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


def test_cli_parses_the_options_in_every_mode(tmp_path):
    pr = run([])
    assert pr.returncode == 0 and " -MS -MSN <name> -MSR <r> -MSA <a> -MSD <n> " in pr.stdout and " -MV " in pr.stdout, pr.stdout
    idx, out = str(tmp_path / "none.dbindex"), str(tmp_path / "o.mr")
    pair, single = ["-1", "a.fastq", "-2", "b.fastq"], ["-r", "x.fastq"]
    base = ["-i", idx, "-o", out]
    modes = [(single, []), (single, ["-A"]), (single, ["-R"]), (pair, []), (pair, ["-P"]), (pair, ["-RP"])]
    rate = ["-MSR", "0.005"]
    # the three spellings are known in every mode, alone (a consumer) and beside the others: the run gets as far as the index check
    for reads, mode in modes:
        for flag in ("-MS", "-sites", "--call-sites"):
            for extra in ([], ["-M", "-sam"], ["-MA", "-MC", "-MB", "-ML", "-ME", "-MV"], ["-D"], ["-g", "0,0"], ["-MSA", "0.05", "-MSD", "3"]):
                pr = run(base + reads + mode + extra + [flag] + rate)
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, mode, extra, pr.stdout)
    # -MS is something for -I5, -NO, the -F options, -D and -MQ to ask for
    for args in (single + ["-I5", "3"], pair + ["-NO"], single + ["-FC", "2"], single + ["-MQ", "20"], single + ["-D"]):
        pr = run(base + args + ["-MS"] + rate)
        assert pr.returncode != 0 and "index file missing" in pr.stdout, (args, pr.stdout)
    pr = run(base + single + ["-MS", "-MSN", "lambda", "-sites-alpha", "0.05", "--sites-min-depth", "127"])
    assert pr.returncode != 0 and "index file missing" in pr.stdout, pr.stdout
    # -MS wants one source of the rate
    for args, says in ((["-MS"], "-MSN"), (["-MS", "-MSA", "0.05"], "-MSR"), (["-MS", "-MSN", "lambda"] + rate, "not from both")):
        pr = run(base + single + args)
        assert pr.returncode != 0 and says in pr.stdout and "index file missing" not in pr.stdout, (args, pr.stdout)
    # the values' spellings and ranges, and that they go with -MS only
    for flags, good, bad, says in ((("-MSR", "-sites-rate", "--sites-rate"), ("0", "0.005", "0.999"), ("1", "-0.1", "x", "", "1.5"), "0 <= r < 1"),
                                   (("-MSA", "-sites-alpha", "--sites-alpha"), ("0.01", "1e-3", "0.5"), ("0", "1", "x", "", "-1"), "0 < a < 1"),
                                   (("-MSD", "-sites-min-depth", "--sites-min-depth"), ("1", "5", "127"), ("0", "128", "x", "", "2.5"), "1 to 127")):
        for flag in flags:
            with_rate = [] if flags[0] == "-MSR" else rate
            for value in good:
                pr = run(base + single + ["-MS"] + with_rate + [flag, value])
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, value, pr.stdout)
            for value in bad:
                pr = run(base + single + ["-MS"] + with_rate + [flag, value])
                assert pr.returncode != 0 and says in pr.stdout and "index file missing" not in pr.stdout, (flag, value, pr.stdout)
            for others in ([], ["-MC"], ["-M", "-ML"]):
                pr = run(base + single + others + [flag, good[1]])
                assert pr.returncode != 0 and "go with -MS" in pr.stdout and "index file missing" not in pr.stdout, (flag, others, pr.stdout)
    for flag in ("-MSN", "-sites-control", "--sites-control"):
        pr = run(base + single + ["-MC", flag, "lambda"])
        assert pr.returncode != 0 and "go with -MS" in pr.stdout, (flag, pr.stdout)
    assert not os.path.exists(out) and not os.path.exists(out + ".methsites") and not os.path.exists(out + ".sitestats")


# ---------------------------------------------------------------------------
# the libraries and the binding
# ---------------------------------------------------------------------------
def test_exports_binding_and_refusals_without_a_device():
    import walt_amd
    for pattern in (3, 5, 7):
        L = ctypes.CDLL(walt_amd.lib_path(pattern))
        for nm in NAMES:
            assert hasattr(L, nm), (pattern, nm)
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    assert "#define WALT_SITECALL_DEPTH 127u" in hdr and "#define WALT_SITECALL_BINS  8255u" in hdr
    for nm in ("depth_hist", "depth_hist_device", "call_sites", "call_sites_device"):
        assert callable(getattr(walt_amd.Pileup, nm)), nm
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm
    # no device: null objects are refused, not crashed on, and the message names the call
    E = walt_amd.WALT_EINVAL
    n = ctypes.c_uint64(0)
    assert L.walt_pileup_depth_hist(None, 0, 0, None, None) == E and b"walt_pileup_depth_hist:" in L.walt_last_error()
    assert L.walt_pileup_depth_hist_device(None, 0, 0, None, None, None) == E and b"walt_pileup_depth_hist_device:" in L.walt_last_error()
    assert L.walt_pileup_call_sites(None, 0, 0, None, None, 0, ctypes.byref(n)) == E and b"walt_pileup_call_sites:" in L.walt_last_error()
    assert L.walt_pileup_call_sites_device(None, 0, 0, None, None, 0, None, None) == E and b"walt_pileup_call_sites_device:" in L.walt_last_error()


def test_per_lane_and_host_logic_under_the_host_sanitizers(scratch):
    """tests/sitecall_sanitize_main.cpp, a stand-alone program over tests/sitecall_harness.cpp built with the host's address
    and undefined-behaviour sanitizers: the reference, the counters, the histogram, the table and the records each in a heap
    block of exactly its size -- a load or an add outside them ends the program, and so does a histogram, a record or a
    table that differs from a plain walk"""
    exe = os.path.join(scratch, "sitecall_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(refio.HERE, "sitecall_sanitize_main.cpp")] + SOURCES + ["-o", exe], check=True, timeout=300)
    pr = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert pr.returncode == 0 and pr.stdout.startswith("ok "), pr.stdout[-2000:]
