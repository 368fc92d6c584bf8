"""Ignored read ends (include/walt_amd.h, "ignored read ends"), the parts that need no device: what the calling kernel and
the overlap kernel run per lane with the bounds (the new overloads of walt_amd/csrc/meth_core.h and overlap_core.h),
compiled with g++ (tests/trim_harness.cpp) and compared with the Python restatement of the contract -- the calls of
tests/test_gpu_meth.py without bounds, every letter outside [trim5, limit - trim3) replaced by '.', and a brute-force
loop over read positions for the interval; the <out>.methstats settings line; the exports of the three libraries, the
binding's surface, and bin/walt's four options: spellings, modes and refusals."""
import ctypes
import inspect
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_meth import expected_read, reference_bases
from test_gpu_overlap import counts_of, drop_letters, excluded_positions, forward_of, word_of
from test_gpu_pileup import chrom_of
from test_meth_cpu import pack_reference

NAMES = ("walt_meth_pileup_batch_trim", "walt_meth_pileup_batch_trim_device", "walt_pair_overlap_batch_trim",
         "walt_pair_overlap_batch_trim_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")


# ---------------------------------------------------------------------------
# the restatement (tests/test_gpu_trim.py uses it too)
# ---------------------------------------------------------------------------
def limit_of(n, call_len=None):
    return n if call_len is None else min(n, int(call_len))


def allowed(i, limit, trim5, trim3):
    """the contract's own sentence: read position i may get a call exactly when trim5 <= i and i + trim3 < limit"""
    return trim5 <= i and i + trim3 < limit


def trim_letters(calls, limit, trim5, trim3):
    """the calls of a read without bounds -> every letter at a position outside the bounds replaced by '.'"""
    return "".join(ch if allowed(i, limit, trim5, trim3) else "." for i, ch in enumerate(calls))


def excluded_positions_trim(start_index, genome_len, m1, m2, best_times, len1, len2, cl1=None, cl2=None, trim1=(0, 0), trim2=(0, 0)):
    """excluded_positions of tests/test_gpu_overlap.py with the bounds of both mates: mate 1's span is walked over the read
    positions it may call; mate 2's bounds only enter the count of the positions it could have been called at"""
    p1, t1, s1 = int(m1["genome_pos"]), int(m1["times"]), bytes(m1["strand"])
    p2, t2, s2 = int(m2["genome_pos"]), int(m2["times"]), bytes(m2["strand"])
    if int(best_times) != 1 or t1 != 1 or t2 != 1 or p1 >= genome_len or p2 >= genome_len or len1 > 1024 or len2 > 1024:
        return [], 0
    if chrom_of(start_index, p1)[0] != chrom_of(start_index, p2)[0]:
        return [], 0
    lim1, lim2 = limit_of(len1, cl1), limit_of(len2, cl2)
    span1 = {forward_of(start_index, p1, s1, j) for j in range(len1) if allowed(j, lim1, *trim1)} - {None}
    ex = [j for j in range(len2) if forward_of(start_index, p2, s2, j) in span1]
    return ex, sum(allowed(j, lim2, *trim2) for j in ex)


# ---------------------------------------------------------------------------
# exports, binding, command line
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_trim_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert "ignored read ends" in hdr


def test_binding_surface_and_the_form_a_call_reaches():
    import walt_amd
    for fn in (walt_amd.Index.meth_call_batch, walt_amd.Index.meth_call_batch_device, walt_amd.Pileup.add_batch,
               walt_amd.Pileup.add_batch_device):
        p = inspect.signature(fn).parameters
        assert p["trim5"].default == 0 and p["trim3"].default == 0, fn
    for fn in (walt_amd.Index.pair_overlap, walt_amd.Index.pair_overlap_device):
        p = inspect.signature(fn).parameters
        assert p["trim1"].default == (0, 0) and p["trim2"].default == (0, 0), fn
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm

    class Named:  # stands for the library: _meth_form only looks the function up by name
        def __getattr__(self, name):
            return name

    form = walt_amd._meth_form
    # a bound picks the _trim form, with a null skip, excl and bias set where the caller gave none
    assert form(Named(), False, 7, trim=(3, 0)) == ("walt_meth_pileup_batch_trim", (7,), (None, 1, None, None, 0, 3, 0))
    assert form(Named(), True, None, (5, 2), (9,), (11, 1), "excl", (0, 4)) == (
        "walt_meth_pileup_batch_trim_device", (None,), (5, 2, 9, 11, 1, 0, 4))
    # no bound: every call reaches the form it reached before
    assert walt_amd._trim_arg(0, 0) is None and walt_amd._trim_arg(0, 1) == (0, 1) and walt_amd._trim_arg(2 ** 32 - 1, 0) == (2 ** 32 - 1, 0)
    assert form(Named(), False, None, trim=None) == ("walt_meth_call_batch", (), ())
    assert form(Named(), False, 7, trim=None) == ("walt_meth_pileup_batch", (7,), ())
    assert form(Named(), True, 7, (5, 2), trim=None)[0] == "walt_meth_pileup_batch_skip_device"
    assert form(Named(), True, None, None, (9,), trim=None)[0] == "walt_meth_pileup_batch_excl_device"
    assert form(Named(), False, None, None, None, (11, 1), trim=None)[0] == "walt_meth_pileup_batch_mbias"
    for bad in ((-1, 0), (0, 2 ** 32)):
        with pytest.raises(ValueError):
            walt_amd._trim_arg(*bad)
    # no device: a null index is refused, not crashed on, and the message names the call
    assert L.walt_meth_pileup_batch_trim(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None, 1,
                                         None, None, 0, 3, 4) == walt_amd.WALT_EINVAL
    assert b"walt_meth_pileup_batch_trim:" in L.walt_last_error()
    assert L.walt_meth_pileup_batch_trim_device(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None,
                                                1, None, None, 0, 3, 4, None) == walt_amd.WALT_EINVAL
    assert b"walt_meth_pileup_batch_trim_device" in L.walt_last_error()
    assert L.walt_pair_overlap_batch_trim(None, None, None, None, 0, None, None, None, None, 1, 2, 3, 4) == walt_amd.WALT_EINVAL
    assert b"walt_pair_overlap_batch_trim:" in L.walt_last_error()
    word = np.zeros(1, dtype=np.uint32)
    assert L.walt_pair_overlap_batch_trim_device(None, None, None, None, 1, None, None, word.ctypes.data, None, 1, 2, 3, 4,
                                                 None) == walt_amd.WALT_EINVAL
    assert b"walt_pair_overlap_batch_trim_device" in L.walt_last_error()


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


SPELLINGS = {"I5": ("-I5", "-ignore", "--ignore"), "I3": ("-I3", "-ignore-3prime", "--ignore-3prime"),
             "I5R2": ("-I5R2", "-ignore-r2", "--ignore-r2"), "I3R2": ("-I3R2", "-ignore-3prime-r2", "--ignore-3prime-r2")}


def test_cli_parses_the_options_in_every_mode_and_refuses_what_it_cannot_do(tmp_path):
    pr = run([])
    assert pr.returncode == 0 and all(" %s <n>" % s[0] in pr.stdout for s in SPELLINGS.values()), pr.stdout
    idx, out = str(tmp_path / "none.dbindex"), str(tmp_path / "o.mr")
    pair, single = ["-1", "a.fastq", "-2", "b.fastq"], ["-r", "x.fastq"]
    base = ["-i", idx, "-o", out]
    # every spelling is known in every mode it applies to: the run gets as far as the index check
    modes = [(single, []), (single, ["-A"]), (single, ["-R"]), (pair, []), (pair, ["-P"]), (pair, ["-RP"])]
    extras = (["-M"], ["-MC"], ["-MB"], ["-M", "-sam", "-MC", "-MB"])
    k = 0
    for reads, mode in modes:
        for key, names in SPELLINGS.items():
            if reads is single and key.endswith("R2"):
                continue
            for flag in names:  # (each of -M, -MC, -MB is enough: they take turns)
                k += 1
                pr = run(base + reads + mode + extras[k % 4] + [flag, "7"])
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, mode, extras[k % 4], pr.stdout)
    # beside -C, -D, -NO and -g, all four at once, the values 0 and 1024
    for extra in (["-M", "-C", "AGATCGGAAGAGC"], ["-MC", "-D"], ["-M", "-NO"], ["-MB", "-g", "0,1"], ["-M", "-sam", "-MC", "-MB", "-D", "-NO"]):
        pr = run(base + pair + extra + ["-I5", "0", "-I3", "1024", "-I5R2", "10", "-I3R2", "3"])
        assert pr.returncode != 0 and "index file missing" in pr.stdout, (extra, pr.stdout)
    # nothing to do without calls
    for reads, mode in modes:
        for flag, extra in (("-I5", []), ("--ignore-3prime", ["-sam"])) + (() if reads is single else (("-I5R2", ["-D"]), ("-ignore-3prime-r2", []))):
            if True:
                pr = run(base + reads + mode + extra + [flag, "0"])
                assert pr.returncode != 0 and "-I5" in pr.stdout and "-M" in pr.stdout and "-MC" in pr.stdout and "-MB" in pr.stdout, pr.stdout
                assert "index file missing" not in pr.stdout
    # a value that is negative, not a number or above 1024; a missing value
    bads = ("-1", "abc", "1025", "7x", "", "+3", " 4", "1e2", "99999999999")
    for names in SPELLINGS.values():
        for j, flag in enumerate(names):
            for bad in bads[:3] + bads[3 + 2 * j:5 + 2 * j]:
                pr = run(base + pair + ["-M", flag, bad])
                assert pr.returncode != 0 and flag in pr.stdout and "0 to 1024" in pr.stdout, (flag, bad, pr.stdout)
                assert "index file missing" not in pr.stdout
            pr = run(base + pair + ["-M", flag])
            assert pr.returncode != 0 and "missing value" in pr.stdout
    # single-end reads have no mate 2
    for flag in SPELLINGS["I5R2"] + SPELLINGS["I3R2"]:
        for mode in ([], ["-A"], ["-R"]):
            pr = run(base + single + mode + ["-M", flag, "2"])
            assert pr.returncode != 0 and "-I5R2" in pr.stdout and "-r" in pr.stdout, pr.stdout
            assert "index file missing" not in pr.stdout
    assert not os.path.exists(out) and not os.path.exists(out + ".methstats")


# ---------------------------------------------------------------------------
# what the kernels run per lane, on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trim_harness(scratch):
    so = os.path.join(scratch, "libtrim_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-I", CSRC,
                    os.path.join(refio.HERE, "trim_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci, ll = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_longlong
    L.trim_harness_read.argtypes = [vp, u32, vp, vp, u64, u64, u64, u32, u32, u32, u32, u32, u32, u32, u32, u32, ci, vp, vp]
    L.trim_harness_read.restype = None
    L.trim_harness_flags.argtypes = [ll, ll, ll, ll, ll, u32, ll, ll, ll, vp]
    L.trim_harness_flags.restype = None
    L.trim_harness_pair.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, u32, u32, u64, u64, ci, u32, ci, u32, vp, vp]
    L.trim_harness_pair.restype = u32
    L.trim_harness_parse.argtypes = [ctypes.c_char_p, vp]
    L.trim_harness_ignore_line.argtypes = [vp, ci, vp, u32]
    L.trim_harness_ignore_line.restype = u32
    return L


COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


@pytest.fixture(scope="module")
def genome():
    """six chromosomes, C / G rich so that every context occurs often; both orientations: strand position q of a '-'
    record is forward position lo + hi - 1 - q of its chromosome"""
    rng = random.Random(2024)
    lengths = [2600, 50, 2, 1, 17, 1300]
    start = np.zeros(len(lengths) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lengths)
    fwd = "".join(rng.choice("ACGTCG") for _ in range(sum(lengths)))
    rev = "".join("".join(COMP[c] for c in reversed(fwd[int(start[k]):int(start[k + 1])])) for k in range(len(lengths)))
    R = [np.frombuffer(t.encode(), dtype=np.uint8) for t in (fwd, rev)]
    return start, (fwd, rev), R, [pack_reference(fwd), pack_reference(rev)]


def make_read(rng, text, pos, n, conv):
    """the strand genome's bases from pos on, about half of the convertible ones converted ('A' beyond the genome)"""
    frm, to = ("C", "T") if conv == "T" else ("G", "A")
    seq = [text[pos + i] if pos + i < len(text) else "A" for i in range(n)]
    return "".join(to if (ch == frm and rng.random() < 0.5) else ch for ch in seq)


def harness_read(L, ref, seq, conv, pos, lo, hi, limit, ex, trim, shift, off, tail, which=0):
    """the read between two neighbours full of callable bases, the calls array at address 16 k + shift"""
    n = len(seq)
    batch_bytes = off + n + tail
    bases = np.full(batch_bytes + 32, ord("C" if conv == "T" else "G"), dtype=np.uint8)
    bases[off:off + n] = np.frombuffer(seq.encode(), dtype=np.uint8)
    bases[batch_bytes:] = 0
    raw = np.full(batch_bytes + 64, 0x23, dtype=np.uint8)
    a16 = (-raw.ctypes.data) % 16 + shift
    counts = np.zeros(8, dtype=np.uint16)
    cmu = np.zeros(n, dtype=np.uint8)
    L.trim_harness_read(ref.ctypes.data, ref.size - 1, bases.ctypes.data, raw.ctypes.data + a16, off, n, batch_bytes, limit, pos, lo, hi,
                        1 if conv == "A" else 0, ex[0], ex[1], trim[0], trim[1], which, counts.ctypes.data, cmu.ctypes.data)
    assert (raw[:a16 + off] == 0x23).all() and (raw[a16 + off + n:] == 0x23).all(), "wrote outside the read"
    return raw[a16 + off:a16 + off + n].tobytes().decode(), counts.tolist(), cmu.tolist()


def bounds_of(n):
    vals = sorted({0, 1, 15, 16, 17, max(n - 1, 0), n, n + 1, 5000})
    pairs = {(a, b) for a in vals for b in vals}
    for a in {1, 16, n // 2, n - 1} - {-1}:  # pairs whose sum is n - 1, n and n + 1
        for s in (n - 1, n, n + 1):
            if 0 <= a <= s:
                pairs.add((a, s - a))
    return sorted(pairs)


@pytest.mark.parametrize("length", [1, 15, 16, 17, 31, 100, 1024])
def test_lengths_bounds_and_every_address_modulo_16(trim_harness, genome, length):
    """each length with trim5 and trim3 from {0, 1, 15, 16, 17, len - 1, len, len + 1, 5000} (all pairs, and pairs whose
    sum is len - 1, len, len + 1), both conversions, both strands, the calls array at every address modulo 16"""
    start, texts, R, refs = genome
    rng = random.Random(length)
    emptied = kept = partial = 0
    for conv in "TA":
        for strand in (b"+", b"-"):
            o = 1 if strand == b"-" else 0
            lo, hi = (0, int(start[1])) if length > 100 else (int(start[5]), int(start[6]))
            pos = rng.randrange(lo, hi - length)
            seq = make_read(rng, texts[o], pos, length, conv)
            plain, _ = expected_read(R, start, seq, pos, 1, strand, conv)
            assert sum(ch != "." for ch in plain) >= length // 8
            for k, (t5, t3) in enumerate(bounds_of(length)):
                want = trim_letters(plain, length, t5, t3)
                if t5 + t3 >= length:
                    assert set(want) == {"."}
                for shift in (range(16) if length < 1024 else [(k + s) % 16 for s in (0, 5, 11)]):
                    got, counts, cmu = harness_read(trim_harness, refs[o], seq, conv, pos, lo, hi, length, (0, 0), (t5, t3), shift,
                                                    off=rng.choice([0, 3, 16, 29]), tail=rng.choice([0, 1, 40]))
                    what = "len %d conv %s strand %s trim (%d, %d) shift %d" % (length, conv, strand, t5, t3, shift)
                    assert got == want, "%s\n got  %s\n want %s" % (what, got, want)
                    assert counts == counts_of(want), what
                    assert cmu == [0 if ch == "." else 1 if ch.isupper() else 2 for ch in want], what
                emptied += set(want) == {"."} and set(plain) != {"."}
                kept += want == plain
                partial += want != plain and set(want) != {"."}
    assert emptied > 20 and kept >= 4 and (partial >= 8 or length == 1), (emptied, kept, partial)


def test_clip_point_excluded_interval_and_chromosome_end(trim_harness, genome):
    """call_len below the length: trim3 counts from the clip point; an excluded interval that starts inside the ignored
    head, ends inside the ignored tail, or lies wholly inside either; a read that runs over its chromosome's end"""
    start, texts, R, refs = genome
    rng = random.Random(77)
    seen = {"clip_moves_3": 0, "ex_head": 0, "ex_tail": 0, "ex_in_head": 0, "ex_in_tail": 0, "over_end": 0, "over_end_tail": 0}
    for trial in range(2500):
        conv, strand = rng.choice("TA"), rng.choice([b"+", b"-"])
        o = 1 if strand == b"-" else 0
        c = rng.choice([0, 0, 5, 5, 1, 4])
        lo, hi = int(start[c]), int(start[c + 1])
        n = rng.choice([1, 15, 16, 17, 31, 40, 100, 150, rng.randrange(1, 200)])
        over = trial % 5 == 0
        pos = max(lo, hi - rng.randrange(1, n + 1)) if over else rng.randrange(lo, max(lo + 1, hi - n))
        seq = make_read(rng, texts[o], pos, n, conv)
        call_len = rng.choice([None, None, n // 2, max(n - 3, 0), n + 5, 0])
        limit = limit_of(n, call_len)
        t5 = rng.choice([0, 1, 5, 16, 17, n // 3, limit, 5000])
        t3 = rng.choice([0, 1, 5, 16, 17, n // 3, limit, 5000])
        kind = rng.choice(["none", "head", "tail", "in_head", "in_tail", "any"])
        top = max(limit - t3, 0)
        if kind == "head" and 0 < t5 < n:      # starts inside the ignored head, ends behind it
            ex = (rng.randrange(0, t5), rng.randrange(t5, n) + 1)
        elif kind == "tail" and 0 < top < limit:  # starts in front of the ignored tail, ends inside it
            ex = (rng.randrange(0, top), rng.randrange(top, limit) + 1)
        elif kind == "in_head" and 1 < t5 <= n:
            a = rng.randrange(0, t5 - 1)
            ex = (a, rng.randrange(a + 1, t5) + 1)
        elif kind == "in_tail" and top + 1 < limit:
            a = rng.randrange(top, limit - 1)
            ex = (a, rng.randrange(a + 1, limit) + 1)
        elif kind == "any":
            a = rng.randrange(0, n)
            ex = (a, rng.randrange(a, n + 1))
        else:
            kind, ex = "none", (0, 0)
        plain, _ = expected_read(R, start, seq, pos, 1, strand, conv, call_len)
        want = trim_letters(drop_letters(plain, range(*ex)), limit, t5, t3)
        got, counts, cmu = harness_read(trim_harness, refs[o], seq, conv, pos, lo, hi, limit, ex, (t5, t3), trial % 16,
                                        off=rng.choice([0, 1, 5, 37]), tail=rng.choice([0, 7, 64]))
        what = "trial %d conv %s strand %s pos %d [%d, %d) n %d limit %d trim (%d, %d) excl %s" % (trial, conv, strand, pos, lo, hi, n, limit, t5, t3, ex)
        assert got == want, "%s\n got  %s\n want %s" % (what, got, want)
        assert counts == counts_of(want), what
        assert cmu == [0 if ch == "." else 1 if ch.isupper() else 2 for ch in want], what
        raw_tail = trim_letters(plain, n, 0, t3)  # what counting from the raw length would leave
        seen["clip_moves_3"] += limit < n and t5 == 0 and kind == "none" and want != raw_tail
        if kind in ("in_head", "in_tail"):  # an interval inside an ignored end changes nothing
            assert want == trim_letters(plain, limit, t5, t3), what
            seen["ex_" + kind] += 1
        elif kind != "none":
            seen["ex_" + kind] = seen.get("ex_" + kind, 0) + (want != trim_letters(plain, limit, t5, t3))
        seen["over_end"] += pos + n > hi
        seen["over_end_tail"] += pos + n > hi and any(ch != "." for ch in want)
    assert all(v > 10 for v in seen.values()), seen


def test_zero_bounds_are_byte_identical_to_the_older_overloads(trim_harness, genome):
    start, texts, R, refs = genome
    rng = random.Random(9)
    for trial in range(1500):
        conv, o = rng.choice("TA"), rng.randrange(2)
        c = rng.choice([0, 5, 1, 4, 2, 3])
        lo, hi = int(start[c]), int(start[c + 1])
        n = rng.choice([1, 15, 16, 17, 31, 100, 1024, rng.randrange(1, 300)])
        pos = rng.randrange(lo, hi)
        seq = make_read(rng, texts[o], pos, n, conv)
        limit = rng.choice([n, n, n // 2, 0])
        ex = rng.choice([(0, 0), (0, 0), (n // 3, n // 2 + 1)])
        off, tail, shift = rng.choice([0, 5, 16]), rng.choice([0, 9]), trial % 16
        new = harness_read(trim_harness, refs[o], seq, conv, pos, lo, hi, limit, ex, (0, 0), shift, off, tail, which=0)
        old = harness_read(trim_harness, refs[o], seq, conv, pos, lo, hi, limit, ex, (0, 0), shift, off, tail, which=1)
        assert new == old, trial
        if ex == (0, 0):
            assert new == harness_read(trim_harness, refs[o], seq, conv, pos, lo, hi, limit, ex, (0, 0), shift, off, tail, which=2)
            assert new[:2] == harness_read(trim_harness, refs[o], seq, conv, pos, lo, hi, limit, ex, (0, 0), shift, off, tail, which=3)[:2]
    for _ in range(3000):  # the flag masks: the 5' bound is the lower end of the called range
        i0 = rng.randrange(-15, 200)
        p, lo = rng.randrange(0, 500), 0
        hi = p + rng.randrange(1, 300)
        limit, ga = rng.randrange(0, 250), rng.randrange(2)
        ex_lo, ex_hi = rng.randrange(0, 220), rng.randrange(0, 220)
        t5 = rng.choice([0, 0, 1, 16, rng.randrange(0, 260), 5000, 2 ** 32 - 1])
        out = np.zeros(6, dtype=np.uint32)
        trim_harness.trim_harness_flags(i0, p, lo, hi, limit, ga, ex_lo, ex_hi, t5, out.ctypes.data)
        mask = sum(1 << (2 * k) for k in range(16) if i0 + k >= t5)
        assert int(out[0]) == int(out[3]) & mask and out[1] == out[4] and out[2] == out[5]
        if t5 == 0:
            assert out[:3].tolist() == out[3:].tolist()


# ---------------------------------------------------------------------------
# the interval with all four bounds
# ---------------------------------------------------------------------------
REC = np.dtype([("genome_pos", "<u4"), ("times", "<u4"), ("strand", "S1")])


def rec(pos, times, strand):
    r = np.zeros(1, dtype=REC)
    r["genome_pos"], r["times"], r["strand"] = pos, times, strand
    return r[0]


def harness_pair(L, start, glen, m1, m2, bt, len1, len2, cl1, cl2, trim):
    bases = ctypes.c_uint32(0x23)
    t = None if trim is None else np.array(trim, dtype=np.uint32)
    w = L.trim_harness_pair(start.ctypes.data, start.size - 1, glen, int(m1["genome_pos"]), int(m1["times"]), m1["strand"][0],
                            int(m2["genome_pos"]), int(m2["times"]), m2["strand"][0], bt, len1, len2, cl1 is not None, cl1 or 0,
                            cl2 is not None, cl2 or 0, None if t is None else t.ctypes.data, ctypes.byref(bases))
    return w, bases.value


# one chromosome of 1,000 bases at genome position 100 (another of 100 in front).  (forward start and length of mate 1, its
# strand, the same of mate 2, call_len 1, (trim5_1, trim3_1), (trim5_2, trim3_2), the interval and the second total WRITTEN
# BY HAND).  A '-' mate at forward [a, a + n) has read position j on forward position a + n - 1 - j.
HAND = [
    # fragment of 40, shorter than a read of 60: mate 1 '+' [200, 260), mate 2 '-' [180, 240): j 0..39 of mate 2 lie on mate 1
    (200, 60, "+", 180, 60, "-", None, (0, 0), (0, 0), (0, 40), 40),
    (200, 60, "+", 180, 60, "-", None, (5, 0), (0, 0), (0, 35), 35),     # trim5_1 = 5: span [205, 260): forward 239 is j 0, 205 is j 34
    (200, 60, "+", 180, 60, "-", None, (5, 0), (3, 0), (0, 35), 32),     # ... mate 2's own bounds stay out of the word
    (200, 60, "+", 180, 60, "-", None, (0, 25), (0, 0), (5, 40), 35),    # trim3_1 = 25: span [200, 235): forward 234 is j 5
    (200, 60, "+", 180, 60, "-", None, (40, 0), (0, 0), None, 0),        # span [240, 260): behind mate 2
    # ordinary overlap: mate 1 '+' [300, 400), mate 2 '-' [380, 480): forward 380..399 = j 99..80
    (300, 100, "+", 380, 100, "-", None, (0, 0), (0, 0), (80, 100), 20),
    (300, 100, "+", 380, 100, "-", None, (0, 10), (0, 0), (90, 100), 10),  # trim3_1 = 10: span [300, 390)
    (300, 100, "+", 380, 100, "-", None, (0, 10), (0, 4), (90, 100), 6),   # trim3_2 = 4: j 96..99 could not be called anyway
    (300, 100, "+", 380, 100, "-", None, (30, 0), (0, 0), (80, 100), 20),  # trim5_1 does not reach the overlap
    (300, 100, "+", 380, 100, "-", None, (0, 20), (0, 0), None, 0),        # trim3_1 = the whole overlap
    (300, 100, "+", 380, 100, "-", 90, (0, 5), (0, 0), (95, 100), 5),      # clipped at 90, 5 more ignored: span [300, 385)
    # the other orientation: mate 1 '-' [380, 480), mate 2 '+' [300, 400): mate 1's j 0 is forward 479
    (380, 100, "-", 300, 100, "+", None, (0, 10), (0, 0), (90, 100), 10),  # trim3_1 cuts forward 380..389
    (380, 100, "-", 300, 100, "+", None, (85, 0), (95, 0), (80, 95), 0),   # trim5_1 = 85: span [380, 395); mate 2 ignores 0..94
    # mate 1 inside mate 2: mate 1 '+' [520, 560), mate 2 '-' [500, 600): forward 520..559 = j 79..40
    (520, 40, "+", 500, 100, "-", None, (0, 0), (0, 0), (40, 80), 40),
    (520, 40, "+", 500, 100, "-", None, (8, 2), (0, 0), (42, 72), 30),     # span [528, 558): j 71..42
    (520, 40, "+", 500, 100, "-", None, (8, 2), (50, 25), (42, 72), 22),   # mate 2 may call j 50..74: 50..71 of the interval
    # empty spans
    (520, 40, "+", 500, 100, "-", None, (40, 0), (0, 0), None, 0),
    (520, 40, "+", 500, 100, "-", None, (0, 40), (0, 0), None, 0),
    (520, 40, "+", 500, 100, "-", None, (20, 20), (0, 0), None, 0),
    (520, 40, "+", 500, 100, "-", None, (19, 20), (0, 0), (60, 61), 1),    # one base left: forward 539 = j 60
    (520, 40, "+", 500, 100, "-", None, (5000, 0), (0, 0), None, 0),
    (520, 40, "+", 500, 100, "-", None, (0, 2 ** 32 - 1), (0, 0), None, 0),
    (520, 40, "+", 500, 100, "-", 0, (0, 0), (0, 0), None, 0),
    # mate 1 runs 10 bases over the chromosome's end: '+' at [970, 1010), span cut at 1000; trim3 counts from the read's end
    (970, 40, "+", 940, 60, "-", None, (0, 5), (0, 0), (0, 30), 30),       # positions 0..34 allowed, 30..34 lie outside: span [970, 1000)
    (970, 40, "+", 940, 60, "-", None, (0, 15), (0, 0), (5, 30), 25),      # positions 0..24: span [970, 995): forward 994 = j 5
]


def hand_records(case):
    a1, n1, st1, a2, n2, st2 = case[:6]
    lo, hi = 100, 1100
    p1 = lo + a1 if st1 == "+" else hi - a1 - n1
    p2 = lo + a2 if st2 == "+" else hi - a2 - n2
    return rec(p1, 1, st1.encode()), rec(p2, 1, st2.encode()), n1, n2


def test_interval_on_hand_made_pairs(trim_harness):
    start = np.array([0, 100, 1100], dtype=np.uint32)
    moved5 = moved3 = 0
    for k, case in enumerate(HAND):
        m1, m2, n1, n2 = hand_records(case)
        cl1, t1, t2, by_hand, bases = case[6:]
        word = 0 if by_hand is None else by_hand[0] | (by_hand[1] << 16)
        ex, b = excluded_positions_trim(start, 1100, m1, m2, 1, n1, n2, cl1, None, t1, t2)
        assert (word_of(ex), b) == (word, bases), ("the restatement against the hand-written value", k, case)
        assert harness_pair(trim_harness, start, 1100, m1, m2, 1, n1, n2, cl1, None, t1 + t2) == (word, bases), (k, case)
        plain = harness_pair(trim_harness, start, 1100, m1, m2, 1, n1, n2, cl1, None, None)
        moved5 += t1[0] != 0 and t1[1] == 0 and word not in (0, plain[0])
        moved3 += t1[0] == 0 and t1[1] != 0 and word not in (0, plain[0])
        # every pair that is not a unique proper pair of unique mates: 0, whatever the bounds
        for bt, ta, tb in ((0, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 0)):
            assert harness_pair(trim_harness, start, 1100, rec(m1["genome_pos"], ta, m1["strand"]), rec(m2["genome_pos"], tb, m2["strand"]),
                                bt, n1, n2, cl1, None, t1 + t2) == (0, 0)
    assert moved5 >= 2 and moved3 >= 4


@pytest.mark.parametrize("seed", [1, 2])
def test_interval_equals_the_brute_force(trim_harness, seed):
    """random pairs on chromosomes of 1, 2, 17 and 300 bases, all strand combinations, reads over a chromosome's end,
    clip points, and bounds of 0, small, around the read length and beyond it on either mate"""
    rng = random.Random(seed * 104729)
    lengths = [300, 1, 17, 2, 300, 17, 1, 2]
    start = np.zeros(len(lengths) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lengths)
    glen = int(start[-1])
    seen = {"nonempty": 0, "emptied": 0, "moved": 0, "bases_less": 0, "zeros": 0, "past_end": 0}
    for trial in range(6000):
        c = rng.choice([0, 0, 4, 4, 4, rng.randrange(8)])
        lo, hi = int(start[c]), int(start[c + 1])
        L = hi - lo
        n2 = rng.choice([1, 2, 17, 40, 100, rng.randrange(1, 60)])
        a2 = rng.randrange(-3, L + 1)
        n1 = rng.choice([1, 2, 17, 40, 100, rng.randrange(1, 60)])
        a1 = a2 + rng.randrange(-n1 - 2, n2 + 3)
        st1, st2 = rng.choice([b"+", b"-"]), rng.choice([b"+", b"-"])
        p1 = lo + a1 if st1 == b"+" else hi - a1 - n1
        p2 = lo + a2 if st2 == b"+" else hi - a2 - n2
        if not (lo <= p1 < hi and lo <= p2 < hi):
            continue
        cl1 = rng.choice([None, None, 0, 1, n1, n1 // 2, n1 + 3])
        cl2 = rng.choice([None, None, 0, 1, n2, n2 // 2, n2 + 3])
        pick = lambda n: rng.choice([0, 0, 1, 3, 16, n // 2, n - 1, n, n + 1, 5000])
        t1, t2 = (pick(n1), pick(n1)), (pick(n2), pick(n2))
        if trial % 7 == 0:
            t1 = t2 = (0, 0)
        m1, m2 = rec(p1, 1, st1), rec(p2, 1, st2)
        ex, bases = excluded_positions_trim(start, glen, m1, m2, 1, n1, n2, cl1, cl2, t1, t2)
        got = harness_pair(trim_harness, start, glen, m1, m2, 1, n1, n2, cl1, cl2, t1 + t2)
        assert got == (word_of(ex), bases), (trial, (lo, hi), (p1, n1, st1, cl1, t1), (p2, n2, st2, cl2, t2), hex(got[0]), got[1], ex[:1], ex[-1:], bases)
        plain_ex, plain_bases = excluded_positions(start, glen, m1, m2, 1, n1, n2, cl1, cl2)
        old = harness_pair(trim_harness, start, glen, m1, m2, 1, n1, n2, cl1, cl2, None)
        assert old == (word_of(plain_ex), plain_bases)
        assert set(ex) <= set(plain_ex) and bases <= plain_bases
        if t1 == t2 == (0, 0):
            assert got == old
            seen["zeros"] += bool(ex)
        seen["nonempty"] += bool(ex)
        seen["emptied"] += bool(plain_ex) and not ex
        seen["moved"] += bool(ex) and ex != plain_ex
        seen["bases_less"] += ex == plain_ex and bases < plain_bases
        seen["past_end"] += p1 + n1 > hi or p2 + n2 > hi
    assert all(v > 50 for v in seen.values()), seen


@pytest.mark.parametrize("files", [("pe_1.fastq", "pe_2.fastq"), ("pe150_1.fastq", "pe150_2.fastq")])
def test_golden_libraries_bounds_move_intervals_and_mate_2_regains_letters(g1_db, trim_harness, files):
    """the golden 2 x 100 and 2 x 150 libraries on the oracle's records with trim3_1 = 10 (and bounds on mate 2): the
    interval of every pair against the brute force; some words differ from those without bounds, and where mate 1 no
    longer calls, mate 2 has its letter back"""
    from test_gpu_meth import load
    _, s1, _ = load(files[0])
    _, s2, _ = load(files[1])
    res, _, _ = refio.oracle_pe(g1_db, s1, s2)
    R = reference_bases(g1_db)
    t1, t2 = (0, 10), (4, 0)
    changed = regained = pairs = bases = plain_pairs = 0
    for i in range(len(s1)):
        args = (g1_db.start_index, g1_db.genome_len, res["m1"][i], res["m2"][i], res["best_times"][i], len(s1[i]), len(s2[i]))
        ex, b = excluded_positions_trim(*args, None, None, t1, t2)
        got = harness_pair(trim_harness, g1_db.start_index, g1_db.genome_len, res["m1"][i], res["m2"][i], int(res["best_times"][i]),
                           len(s1[i]), len(s2[i]), None, None, t1 + t2)
        assert got == (word_of(ex), b), i
        plain_ex, _ = excluded_positions(*args)
        pairs += bool(ex)
        plain_pairs += bool(plain_ex)
        bases += b
        if word_of(ex) != word_of(plain_ex):
            changed += 1
            m2 = res["m2"][i]
            calls2, _ = expected_read(R, g1_db.start_index, s2[i], m2["genome_pos"], m2["times"], bytes(m2["strand"]), "A")
            before = trim_letters(drop_letters(calls2, plain_ex), len(s2[i]), *t2)
            after = trim_letters(drop_letters(calls2, ex), len(s2[i]), *t2)
            regained += sum(x == "." and y != "." for x, y in zip(before, after))
            assert all(x == y or x == "." for x, y in zip(before, after))
    assert plain_pairs in (123, 153) and changed >= 100 and regained >= 20 and 0 < pairs <= plain_pairs and bases > 0, (
        plain_pairs, pairs, changed, regained, bases)


# ---------------------------------------------------------------------------
# the command line's pieces
# ---------------------------------------------------------------------------
def test_ignore_line_writer_and_value_parser(trim_harness):
    buf = ctypes.create_string_buffer(128)
    for v in ([0, 0], [3, 0], [0, 1024], [10, 10, 2, 0], [0, 0, 0, 7], [1024, 1024, 1024, 1024]):
        arr = np.array(v, dtype=np.uint32)
        n = trim_harness.trim_harness_ignore_line(arr.ctypes.data, len(v), ctypes.addressof(buf), 128)
        assert buf.raw[:n].decode() == "ignore\t" + "\t".join(str(x) for x in v) + "\n"
    out = ctypes.c_uint32(77)
    for text, want in (("0", 0), ("7", 7), ("0007", 7), ("1024", 1024), ("10", 10)):
        assert trim_harness.trim_harness_parse(text.encode(), ctypes.byref(out)) == 1 and out.value == want, text
    for text in ("", "-1", "1025", "9999", "10000", "4294967297", "abc", "7x", "x7", " 7", "7 ", "+7", "1e2", "0x10", "3.0"):
        assert trim_harness.trim_harness_parse(text.encode(), ctypes.byref(out)) == 0, text


def test_per_lane_logic_under_the_host_sanitizers(scratch):
    """tests/trim_sanitize_main.cpp, a stand-alone program over tests/trim_harness.cpp built with the host's address and
    undefined-behaviour sanitizers: random batches, each in a heap block that begins with the batch's first base or ends
    with its last, at every alignment, with bounds of every kind -- a load or store outside the batch's own bytes ends the
    program, and so does a call that differs from the call without bounds blanked outside them"""
    exe = os.path.join(scratch, "trim_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(refio.HERE, "trim_sanitize_main.cpp"), os.path.join(refio.HERE, "trim_harness.cpp"), "-o", exe],
                   check=True, timeout=300)
    pr = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert pr.returncode == 0 and pr.stdout.startswith("ok "), pr.stdout[-2000:]
