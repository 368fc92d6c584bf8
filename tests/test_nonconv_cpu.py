"""Non-converted reads (include/walt_amd.h, "non-converted reads"), the parts that need no device: what the judging kernel
runs per lane (walt_amd/csrc/nonconv_core.h), compiled with g++ (tests/nonconv_harness.cpp) and compared with the
pure-Python restatement of tests/test_gpu_nonconv.py; the <out>.filterstats writer; the exports of the three libraries,
the binding's surface and refusals without a device; and bin/walt's four options: spellings, modes and refusals."""
import ctypes
import inspect
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_nonconv import BOUNDARY_CASES, LENGTHS, expected_verdicts, fails, filterstats_text, pair_rule, tally_of

NAMES = ("walt_nonconv_batch", "walt_nonconv_batch_device", "walt_meth_nonconv_batch", "walt_meth_nonconv_batch_device",
         "walt_nonconv_pairs_batch", "walt_nonconv_pairs_batch_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")


@pytest.fixture(scope="module")
def harness(scratch):
    so = os.path.join(scratch, "libnonconv_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-I", CSRC,
                    os.path.join(refio.HERE, "nonconv_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.nonconv_harness_classes.argtypes = [vp]
    L.nonconv_harness_identity.argtypes = [vp]
    L.nonconv_harness_combine.argtypes = [vp, vp, vp]
    L.nonconv_harness_pack.argtypes = [vp, vp]
    L.nonconv_harness_scan.argtypes = [vp, u32, vp]
    L.nonconv_harness_read.argtypes = [vp, u32, u64, u64, vp]
    L.nonconv_harness_trips.argtypes = [ci, ci]
    L.nonconv_harness_trips.restype = u32
    L.nonconv_harness_fails.argtypes = [u32, u32, u32, vp]
    L.nonconv_harness_fails.restype = u32
    L.nonconv_harness_judged.argtypes = [u32, u64, u64]
    L.nonconv_harness_rule_ok.argtypes = [vp]
    L.nonconv_harness_batch.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp]
    L.nonconv_harness_batch.restype = ctypes.c_longlong
    L.nonconv_harness_pair.argtypes = [u32, vp]
    L.nonconv_harness_filter_block.argtypes = [u64, u64, vp, vp, u32]
    L.nonconv_harness_filter_block.restype = u32
    L.nonconv_harness_parse.argtypes = [ctypes.c_char_p, u32, u32, vp]
    return L


def rule_arr(rule):
    return np.array(rule, dtype=np.uint32)


# ---------------------------------------------------------------------------
# classification, the combine, the fold
# ---------------------------------------------------------------------------
def test_every_byte_value_through_the_classification(harness):
    out = np.zeros(256, dtype=np.uint8)
    harness.nonconv_harness_classes(out.ctypes.data)
    want = [1 if chr(b) in "HX" else 2 if chr(b) in "hx" else 0 for b in range(256)]
    assert out.tolist() == want and sum(want) == 6
    for b in range(256):  # and so the restatement's tally of a single byte
        assert tally_of(bytes([b])) == ((1, 1, 1) if want[b] == 1 else (0, 1, 0) if want[b] == 2 else (0, 0, 0))


def summary_of(harness, data):
    out = np.zeros(6, dtype=np.uint32)
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    harness.nonconv_harness_scan(buf.ctypes.data, len(data), out.ctypes.data)
    return out


def combine(harness, a, b):
    out = np.zeros(6, dtype=np.uint32)
    harness.nonconv_harness_combine(np.ascontiguousarray(a).ctypes.data, np.ascontiguousarray(b).ctypes.data, out.ctypes.data)
    return out


def plain_summary(data):
    """(meth, total, pre, suf, best, full) of a stretch, each by its own plain loop"""
    meth, total, best = tally_of(data)
    letters = [b for b in bytes(data) if chr(b) in "HXhx"]
    pre = next((i for i, b in enumerate(letters) if chr(b) in "hx"), len(letters))
    suf = next((i for i, b in enumerate(reversed(letters)) if chr(b) in "hx"), len(letters))
    return [meth, total, pre, suf, best, int(all(chr(b) in "HX" for b in letters))]


def test_combine_is_associative_has_an_identity_and_means_concatenation(harness):
    rng = random.Random(31)
    ident = np.zeros(6, dtype=np.uint32)
    harness.nonconv_harness_identity(ident.ctypes.data)
    assert ident.tolist() == [0, 0, 0, 0, 0, 1]
    not_commutative = 0
    for trial in range(3000):
        al = rng.choice(["HXhx", "HHHHHXh", "Hh.zZ", "H.Z", "hx."])
        parts = [bytes(ord(rng.choice(al)) for _ in range(rng.choice([0, 1, 2, 5, 16, 40]))) for _ in range(3)]
        s = [summary_of(harness, p) for p in parts]
        for p, v in zip(parts, s):
            assert v.tolist() == plain_summary(p), p
        ab_c = combine(harness, combine(harness, s[0], s[1]), s[2])
        a_bc = combine(harness, s[0], combine(harness, s[1], s[2]))
        assert ab_c.tolist() == a_bc.tolist() == plain_summary(b"".join(parts)), parts
        assert combine(harness, s[0], ident).tolist() == s[0].tolist() == combine(harness, ident, s[0]).tolist()
        not_commutative += combine(harness, s[0], s[1]).tolist() != combine(harness, s[1], s[0]).tolist()
        packed = np.zeros(6, dtype=np.uint32)  # what a cross-lane step moves: fields of at most 128
        if max(s[0]) <= 128:
            harness.nonconv_harness_pack(s[0].ctypes.data, packed.ctypes.data)
            assert packed.tolist() == s[0].tolist()
    assert not_commutative > 300


def read_through_the_fold(harness, body, lead, shift, tail=16):
    """the read behind `lead` bytes and in front of `tail` bytes of neighbours full of H, the batch at address 16 k + shift"""
    n = len(body)
    raw = np.full(lead + n + tail + 64, ord("H"), dtype=np.uint8)
    a = (-raw.ctypes.data) % 16 + shift
    raw[a + lead:a + lead + n] = np.frombuffer(bytes(body), dtype=np.uint8)
    out = np.zeros(6, dtype=np.uint32)
    harness.nonconv_harness_read(raw.ctypes.data + a + lead, n, lead, n + tail, out.ctypes.data)
    return out.tolist()


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_at_all_16_addresses_and_every_offset_between_neighbours_full_of_h(harness, length):
    rng = random.Random(length)
    bodies = [bytes(ord(rng.choice("HXhx" * 3 + "HH.Z")) for _ in range(length)), bytes(ord(rng.choice("HXhxzZuU....ACGT")) for _ in range(length)),
              b"H" * length, b"h" * length, (b"Hh" * length)[:length], b"." * length]
    for body in bodies:
        want = plain_summary(body)
        for shift in range(16):
            for lead in (range(16) if length < 1024 else [(shift * 7 + 3) % 16, 0]):
                for tail in (0, 16):
                    got = read_through_the_fold(harness, body, lead, shift, tail)
                    assert got == want, (length, shift, lead, tail, got, want)
    assert harness.nonconv_harness_trips(length, 0) == (length + 127) // 128
    assert harness.nonconv_harness_trips(length, 15) == (length + 15 + 127) // 128


def test_hand_written_boundary_cases_through_the_fold(harness):
    for text, lead, by_hand in BOUNDARY_CASES:
        assert tally_of(text.encode()) == by_hand, text[:40]
        got = read_through_the_fold(harness, text.encode(), lead, 0)
        assert (got[0], got[1], got[4]) == by_hand, (text[:40], lead, got)
        assert harness.nonconv_harness_trips(len(text), lead) == (lead + len(text) + 127) // 128


def test_batches_as_the_kernel_takes_them(harness):
    rng = random.Random(33)
    for trial in range(300):
        n = rng.randrange(1, 9)
        lens = [rng.choice([0, 1, 15, 16, 17, 31, 127, 128, 129, 1024, 1025, 40]) for _ in range(n)]
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(lens)
        if trial % 10 == 0 and n >= 3:  # a made-up offset in the middle
            offsets[n // 2] = offsets[n] + np.uint64(rng.choice([0, 1, 500]))
        total = int(max(offsets))
        al = rng.choice(["HXhx" * 3 + "HH.Z", "HXhxzZuU....ACGT"])
        raw = np.full(total + 48, ord("H"), dtype=np.uint8)
        a = (-raw.ctypes.data) % 16 + trial % 16
        calls = raw[a:a + total]
        calls[:] = np.frombuffer(bytes(ord(rng.choice(al)) for _ in range(total)), dtype=np.uint8) if total else calls
        times = [rng.choice([0, 1, 1, 1, 2]) for _ in range(n)]
        rec = np.zeros((n, 4), dtype=np.uint32)
        rec[:, 1] = times
        rule = (rng.choice([0, 3, 40]), rng.choice([0, 2, 9]), rng.choice([0, 15, 100]), rng.choice([0, 1, 5, 50]))
        filt = np.full(n, 9, dtype=np.uint8)
        tally = np.full((n, 4), 77, dtype=np.uint16)
        harness.nonconv_harness_batch(calls.ctypes.data, offsets.ctypes.data, n, rec.ctypes.data, 16, rule_arr(rule).ctypes.data,
                                      filt.ctypes.data, tally.ctypes.data)
        want_f, want_t = expected_verdicts(calls, offsets, times, rule, base=0)
        assert np.array_equal(filt, want_f) and np.array_equal(tally[:, :3].astype(np.int64), want_t) and (tally[:, 3] == 0).all(), trial


# ---------------------------------------------------------------------------
# the rule, which records are judged, the pair rule
# ---------------------------------------------------------------------------
def test_the_four_rule_boundaries(harness):
    f = lambda meth, total, run, rule: harness.nonconv_harness_fails(meth, total, run, rule_arr(rule).ctypes.data)
    # meth == min_meth fails, min_meth - 1 passes
    assert f(3, 9, 1, (3, 0, 0, 0)) == 1 and f(2, 9, 1, (3, 0, 0, 0)) == 0
    # run == min_run fails, min_run - 1 passes
    assert f(7, 9, 4, (0, 4, 0, 0)) == 1 and f(7, 9, 3, (0, 4, 0, 0)) == 0
    # 100 * meth == min_percent * total fails, one call fewer passes
    assert f(3, 20, 1, (0, 0, 15, 5)) == 1 and f(2, 20, 1, (0, 0, 15, 5)) == 0 and f(15, 100, 1, (0, 0, 15, 5)) == 1 and f(14, 100, 1, (0, 0, 15, 5)) == 0
    # total == min_total is judged, min_total - 1 is not
    assert f(5, 5, 1, (0, 0, 15, 5)) == 1 and f(4, 4, 1, (0, 0, 15, 5)) == 0
    # min_total 0 stands for 1: a read without non-CpG calls has no percentage
    assert f(0, 0, 0, (0, 0, 1, 0)) == 0 and f(1, 1, 1, (0, 0, 100, 0)) == 1 and f(0, 1, 0, (0, 0, 1, 0)) == 0
    # a field of 0 switches its test off; all zeros filter nobody; any enabled test is enough
    assert f(1024, 1024, 1024, (0, 0, 0, 0)) == 0 and f(1024, 1024, 1024, (0, 0, 0, 7)) == 0
    assert f(3, 100, 1, (3, 9, 90, 5)) == 1 and f(2, 100, 9, (3, 9, 90, 5)) == 1 and f(2, 2, 2, (3, 9, 90, 1)) == 1 and f(2, 100, 2, (3, 9, 90, 5)) == 0
    rng = random.Random(34)
    for _ in range(20000):
        total = rng.randrange(0, 1025)
        meth = rng.randrange(0, total + 1)
        run = rng.randrange(0, meth + 1)
        rule = (rng.choice([0, 1, 3, meth, meth + 1, 1024]), rng.choice([0, 1, 2, run, run + 1]), rng.choice([0, 1, 15, 50, 100]),
                rng.choice([0, 1, 5, total, total + 1]))
        assert f(meth, total, run, rule) == fails(meth, total, run, rule), (meth, total, run, rule)
    assert harness.nonconv_harness_rule_ok(rule_arr((9, 9, 100, 9)).ctypes.data) == 1
    assert harness.nonconv_harness_rule_ok(rule_arr((0, 0, 101, 0)).ctypes.data) == 0
    # judged: unique, 1 to 1024 calls, offsets in order
    j = harness.nonconv_harness_judged
    assert j(1, 10, 11) == 1 and j(1, 10, 1034) == 1 and j(1, 10, 1035) == 0 and j(1, 10, 10) == 0 and j(1, 11, 10) == 0
    assert j(0, 10, 20) == 0 and j(2, 10, 20) == 0 and j(1, 2 ** 40, 2 ** 40 + 5) == 1


def test_the_pair_rule(harness):
    for bt in (0, 1, 2, 7):
        for a in (0, 1):
            for b in (0, 1):
                f = np.array([a, b], dtype=np.uint8)
                harness.nonconv_harness_pair(bt, f.ctypes.data)
                assert f.tolist() == ([a | b, a | b] if bt == 1 else [a, b])
                assert pair_rule([[a, b]], [bt]).tolist() == [f.tolist()]


# ---------------------------------------------------------------------------
# the command line's pieces, exports, binding
# ---------------------------------------------------------------------------
def test_filterstats_writer_and_value_parser(harness):
    buf = ctypes.create_string_buffer(256)
    for records, filtered, rule in ((0, 0, (3, 0, 0, 0)), (987, 87, (3, 0, 0, 0)), (3, 1, (0, 2, 15, 5)), (2 ** 40, 2 ** 39, (1024, 1024, 100, 1024))):
        n = harness.nonconv_harness_filter_block(records, filtered, rule_arr(rule).ctypes.data, ctypes.addressof(buf), 256)
        assert buf.raw[:n].decode() == filterstats_text(records, filtered, rule)
    assert filterstats_text(0, 0, (3, 0, 0, 0)) == "records: 0\nfiltered: 0\nfilter rate: NA\nrule\t3\t0\t0\t0\n"
    assert filterstats_text(3, 1, (0, 2, 15, 5)) == "records: 3\nfiltered: 1\nfilter rate: 0.333333\nrule\t0\t2\t15\t5\n"
    out = ctypes.c_uint32(77)
    for text, lo, hi, want in (("1", 1, 1024, 1), ("1024", 1, 1024, 1024), ("007", 1, 100, 7), ("100", 1, 100, 100)):
        assert harness.nonconv_harness_parse(text.encode(), lo, hi, ctypes.byref(out)) == 1 and out.value == want, text
    for text, lo, hi in (("0", 1, 1024), ("1025", 1, 1024), ("101", 1, 100), ("", 1, 100), ("-1", 1, 100), ("abc", 1, 100), ("7x", 1, 100),
                         (" 7", 1, 100), ("+7", 1, 100), ("1e1", 1, 100), ("3.0", 1, 100), ("99999999999", 1, 1024)):
        assert harness.nonconv_harness_parse(text.encode(), lo, hi, ctypes.byref(out)) == 0, text


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert "non-converted reads" in hdr and hdr.index("ignored read ends") < hdr.index("non-converted reads") < hdr.index("---- options")


def test_binding_surface_and_refusals_without_a_device():
    import walt_amd
    for name in ("nonconv_batch", "nonconv_batch_device", "nonconv_pairs", "nonconv_pairs_device", "meth_nonconv_batch",
                 "meth_nonconv_batch_device"):
        assert callable(getattr(walt_amd.Index, name)), name
    assert walt_amd.nonconv_tally_dtype.itemsize == 8 and walt_amd.nonconv_tally_dtype.names == ("meth", "total", "run", "reserved")
    r = walt_amd.nonconv_rule(3, min_percent=15, min_total=5)
    assert r.dtype == walt_amd.nonconv_rule_dtype and r.tobytes() == np.array([3, 0, 15, 5], dtype="<u4").tobytes()
    assert walt_amd.nonconv_rule().tobytes() == bytes(16)
    for bad in (dict(min_meth=-1), dict(min_run=2 ** 32)):
        with pytest.raises(ValueError):
            walt_amd.nonconv_rule(**bad)
    # existing methods keep their signatures
    p = inspect.signature(walt_amd.Index.meth_call_batch).parameters
    assert list(p)[-6:] == ["skip", "excl", "mbias", "mbias_table", "trim5", "trim3"] and "rule" not in p
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm
    # no device: a null index is refused, not crashed on, and the message names the call
    rule, filt = walt_amd.nonconv_rule(3), np.zeros(2, dtype=np.uint8)
    E = walt_amd.WALT_EINVAL
    assert L.walt_nonconv_batch(None, None, None, 0, None, 16, rule.ctypes.data, filt.ctypes.data, 1, None) == E
    assert b"walt_nonconv_batch:" in L.walt_last_error()
    assert L.walt_nonconv_batch_device(None, None, None, 0, None, 16, rule.ctypes.data, None, 1, None, None) == E
    assert b"walt_nonconv_batch_device:" in L.walt_last_error()
    assert L.walt_nonconv_pairs_batch(None, None, 0, None) == E and b"walt_nonconv_pairs_batch:" in L.walt_last_error()
    assert L.walt_nonconv_pairs_batch_device(None, None, 0, None, None) == E and b"walt_nonconv_pairs_batch_device:" in L.walt_last_error()
    assert L.walt_meth_nonconv_batch(None, None, None, 0, None, 16, None, 0, ord("T"), None, None, rule.ctypes.data, filt.ctypes.data, 1,
                                     None) == E and b"walt_meth_nonconv_batch:" in L.walt_last_error()
    assert L.walt_meth_nonconv_batch_device(None, None, None, 0, None, 16, None, 0, ord("T"), None, None, rule.ctypes.data, None, 1, None,
                                            None) == E and b"walt_meth_nonconv_batch_device:" in L.walt_last_error()


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


SPELLINGS = {"F": ("-F", "-filter-nonconv", "--filter-nonconv", "--filter-non-conversion"),
             "FC": ("-FC", "-filter-consecutive", "--filter-consecutive"),
             "FP": ("-FP", "-filter-percent", "--filter-percent"), "FM": ("-FM", "-filter-min-count", "--filter-min-count")}


def test_cli_parses_the_options_in_every_mode_and_refuses_what_it_cannot_do(tmp_path):
    pr = run([])
    assert pr.returncode == 0 and all(" %s <" % s[0] in pr.stdout for s in SPELLINGS.values()), pr.stdout
    idx, out = str(tmp_path / "none.dbindex"), str(tmp_path / "o.mr")
    pair, single = ["-1", "a.fastq", "-2", "b.fastq"], ["-r", "x.fastq"]
    base = ["-i", idx, "-o", out]
    # every spelling is known in every mode: the run gets as far as the index check
    modes = [(single, []), (single, ["-A"]), (single, ["-R"]), (pair, []), (pair, ["-P"]), (pair, ["-RP"])]
    extras = (["-M"], ["-MC"], ["-MB"], ["-M", "-sam", "-MC", "-MB"])
    k = 0
    for reads, mode in modes:
        for key, names in SPELLINGS.items():
            for flag in names:  # (each of -M, -MC, -MB is enough: they take turns)
                k += 1
                opts = [flag, "7"] if key != "FM" else ["-FP", "20", flag, "7"]
                pr = run(base + reads + mode + extras[k % 4] + opts)
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, mode, extras[k % 4], pr.stdout)
    # any combination, beside -C, -D, -NO, the -I options and -g, the smallest and largest values
    for reads, extra in ((pair, ["-M", "-C", "AGATCGGAAGAGC"]), (pair, ["-MC", "-D"]), (pair, ["-M", "-NO"]), (single, ["-MB", "-g", "0,1"]),
                         (pair, ["-M", "-sam", "-MC", "-MB", "-D", "-NO", "-I5", "3", "-I3R2", "2"])):
        for opts in (["-F", "1", "-FC", "1024", "-FP", "100", "-FM", "1"], ["-F", "1024", "-FC", "1"], ["-FP", "1", "-FM", "1024"], ["-FC", "2", "-FP", "15"]):
            pr = run(base + reads + extra + opts)
            assert pr.returncode != 0 and "index file missing" in pr.stdout, (extra, opts, pr.stdout)
    # nothing to do without calls
    for reads, mode in modes:
        for opts, extra in ((["-F", "3"], []), (["--filter-consecutive", "2"], ["-sam"]), (["-FP", "15"], ["-D"]), (["-FP", "15", "-FM", "5"], [])):
            pr = run(base + reads + mode + extra + opts)
            assert pr.returncode != 0 and "-F" in pr.stdout and "-M" in pr.stdout and "-MC" in pr.stdout and "-MB" in pr.stdout, pr.stdout
            assert "index file missing" not in pr.stdout
    # -FM goes with -FP
    for flag in SPELLINGS["FM"]:
        for more in ([], ["-F", "3"], ["-FC", "2"]):
            pr = run(base + single + ["-M", flag, "5"] + more)
            assert pr.returncode != 0 and "-FM" in pr.stdout and "-FP" in pr.stdout and "index file missing" not in pr.stdout, pr.stdout
    # a value that is zero, negative, not a number or out of range; a missing value
    for key, names in SPELLINGS.items():
        top = "100" if key == "FP" else "1024"
        for flag in names:
            for bad in ("0", "-1", "abc", "7x", "", "+3", " 4", "1e2", str(int(top) + 1), "99999999999"):
                pr = run(base + pair + ["-M", "-FP", "20", flag, bad])
                assert pr.returncode != 0 and flag in pr.stdout and "1 to " + top in pr.stdout, (flag, bad, pr.stdout)
                assert "index file missing" not in pr.stdout
            pr = run(base + pair + ["-M", flag])
            assert pr.returncode != 0 and "missing value" in pr.stdout
    assert not os.path.exists(out) and not os.path.exists(out + ".filterstats")


def test_per_lane_logic_under_the_host_sanitizers(scratch):
    """tests/nonconv_sanitize_main.cpp, a stand-alone program over tests/nonconv_harness.cpp built with the host's address and
    undefined-behaviour sanitizers: random batches, each in a heap block that begins with the batch's first call or ends
    with its last, at every alignment -- a load outside the batch's own bytes ends the program, and so does a tally or a
    verdict that differs from a plain loop over the read's bytes"""
    exe = os.path.join(scratch, "nonconv_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(refio.HERE, "nonconv_sanitize_main.cpp"), os.path.join(refio.HERE, "nonconv_harness.cpp"), "-o", exe],
                   check=True, timeout=300)
    pr = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert pr.returncode == 0 and pr.stdout.startswith("ok "), pr.stdout[-2000:]
