"""The overlap of a proper pair (include/walt_amd.h, "overlap of a pair"), the parts that need no device: what the
overlap kernel runs per lane (walt_amd/csrc/overlap_core.h) and the calling kernel's slices with an excluded interval
(the new overloads of walt_amd/csrc/meth_core.h), compiled with g++ (tests/overlap_harness.cpp) and compared with the
brute-force restatement of tests/test_gpu_overlap.py; the exports of the three libraries, the binding's surface, and
bin/walt -NO's parsing and refusals."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_meth import expected_read
from test_gpu_overlap import counts_of, drop_letters, excluded_positions, word_of
from test_meth_cpu import pack_reference

NAMES = ("walt_pair_overlap_batch", "walt_pair_overlap_batch_device", "walt_meth_pileup_batch_excl",
         "walt_meth_pileup_batch_excl_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_overlap_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert nm + "(" in hdr
    assert "overlap of a pair" in hdr and "Overlapping mates of a pair are both counted, as walt_meth_stats counts them." not in hdr


def test_binding_surface_and_null_arguments():
    import inspect

    import walt_amd
    for nm in ("pair_overlap", "pair_overlap_device"):
        assert hasattr(walt_amd.Index, nm), nm
    assert "excl" in inspect.signature(walt_amd.Index.meth_call_batch).parameters
    assert "excl" in inspect.signature(walt_amd.Pileup.add_batch).parameters
    assert "d_excl" in inspect.signature(walt_amd.Pileup.add_batch_device).parameters
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm
    # no device: a null index is refused, not crashed on, and the message names the call
    word = np.zeros(1, dtype=np.uint32)
    assert L.walt_pair_overlap_batch(None, None, None, None, 0, None, None, None, None) == walt_amd.WALT_EINVAL
    assert b"walt_pair_overlap_batch" in L.walt_last_error()
    assert L.walt_pair_overlap_batch_device(None, None, None, None, 1, None, None, word.ctypes.data, None, None) == walt_amd.WALT_EINVAL
    assert b"walt_pair_overlap_batch_device" in L.walt_last_error()
    assert L.walt_meth_pileup_batch_excl(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None, 1,
                                         None) == walt_amd.WALT_EINVAL
    assert b"walt_meth_pileup_batch_excl" in L.walt_last_error()
    assert L.walt_meth_pileup_batch_excl_device(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None,
                                                1, None, None) == walt_amd.WALT_EINVAL
    assert b"walt_meth_pileup_batch_excl_device" in L.walt_last_error()


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


def test_cli_parses_the_option_and_refuses_what_it_cannot_do(tmp_path):
    pr = run([])
    assert pr.returncode == 0 and " -NO " in pr.stdout
    idx, out = str(tmp_path / "none.dbindex"), str(tmp_path / "o.mr")
    pair = ["-1", "a.fastq", "-2", "b.fastq"]
    # every spelling is known, in every paired mode and beside -C, -D, -sam and -g: the run gets as far as the index check
    for flag in ("-NO", "-no-overlap", "--no-overlap"):
        for extra in (["-M"], ["-MC"], ["-M", "-MC", "-sam"], ["-MC", "-P"], ["-M", "-RP"], ["-MC", "-D", "-C", "AGATCGGAAGAGC"],
                      ["-M", "-g", "0,1"]):
            pr = run([flag, "-i", idx, "-o", out] + pair + extra)
            assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, extra, pr.stdout)
    # single-end reads have no mate
    for extra in (["-M"], ["-MC"], ["-M", "-R"]):
        pr = run(["-NO", "-i", idx, "-o", out, "-r", "x.fastq"] + extra)
        assert pr.returncode != 0 and "-NO" in pr.stdout and "-r" in pr.stdout and "paired-end" in pr.stdout, pr.stdout
        assert "index file missing" not in pr.stdout
    # nothing to do without calls
    for extra in ([], ["-sam"], ["-D"], ["-P"]):
        pr = run(["-NO", "-i", idx, "-o", out] + pair + extra)
        assert pr.returncode != 0 and "-NO" in pr.stdout and "-M" in pr.stdout and "-MC" in pr.stdout, pr.stdout
        assert "index file missing" not in pr.stdout
    assert not os.path.exists(out) and not os.path.exists(out + ".methstats")


# ---------------------------------------------------------------------------
# what the kernels run per lane, on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overlap_harness(scratch):
    so = os.path.join(scratch, "liboverlap_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", os.path.join(refio.ROOT, "walt_amd", "csrc"),
                    os.path.join(refio.HERE, "overlap_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci, ll = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_longlong
    L.overlap_harness_pair.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, u32, u32, u64, u64, ci, u32, ci, u32, vp]
    L.overlap_harness_pair.restype = u32
    L.overlap_harness_read.argtypes = [vp, u32, vp, vp, u64, u64, u64, u32, ci, u32, u32, u32, u32, u32, u32, ci, vp, vp]
    L.overlap_harness_read.restype = None
    L.overlap_harness_flags.argtypes = [ll, ll, ll, ll, ll, u32, ll, ll, vp]
    L.overlap_harness_flags.restype = None
    return L


REC = np.dtype([("genome_pos", "<u4"), ("times", "<u4"), ("strand", "S1")])


def rec(pos, times, strand):
    r = np.zeros(1, dtype=REC)
    r["genome_pos"], r["times"], r["strand"] = pos, times, strand
    return r[0]


def harness_pair(L, start, glen, m1, m2, bt, len1, len2, cl1, cl2):
    bases = ctypes.c_uint32(0x23)
    w = L.overlap_harness_pair(start.ctypes.data, start.size - 1, glen, int(m1["genome_pos"]), int(m1["times"]), m1["strand"][0],
                               int(m2["genome_pos"]), int(m2["times"]), m2["strand"][0], bt, len1, len2, cl1 is not None, cl1 or 0,
                               cl2 is not None, cl2 or 0, ctypes.byref(bases))
    return w, bases.value


@pytest.mark.parametrize("n_chrom", [8, 1500, 5000])
@pytest.mark.parametrize("seed", [1, 2])
def test_interval_equals_the_brute_force(overlap_harness, seed, n_chrom):
    """random pairs on chromosomes of 1, 2, 17 and 300 bases (and, for the look-up's other two paths, thousands of them):
    all four strand combinations; mate 1 before, after, inside, around and equal to mate 2; gaps of 0 and overlaps of 1;
    reads over a chromosome's end; call_len of 0, 1 and len on either mate"""
    rng = random.Random(seed * 7919 + n_chrom)
    lengths = [300, 1, 17, 2, 300, 17, 1, 2] + [rng.choice([1, 2, 17, 40, 300]) for _ in range(n_chrom - 8)]
    start = np.zeros(len(lengths) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lengths)
    glen = int(start[-1])
    seen = {"shape": set(), "strands": set(), "cl": set(), "gap0": 0, "over1": 0, "past_end": 0, "nonempty": 0}
    for trial in range(4000):
        c = rng.randrange(len(lengths)) if trial % 3 else rng.randrange(8)
        lo, hi = int(start[c]), int(start[c + 1])
        L = hi - lo
        # mate 2 as a forward interval [a2, a2 + n2) that may hang over either end of the chromosome, mate 1 placed around it
        n2 = rng.choice([1, 2, 5, 17, 40, 100, 1024, rng.randrange(1, 60)])
        a2 = rng.randrange(-3, L + 1)
        shape = rng.choice(["before", "after", "inside", "around", "equal", "gap0", "over1", "any"])
        if shape == "before":
            n1 = rng.randrange(1, 40); a1 = a2 - n1 - rng.randrange(0, 5)
        elif shape == "after":
            n1 = rng.randrange(1, 40); a1 = a2 + n2 + rng.randrange(0, 5)
        elif shape == "inside":
            n1 = rng.randrange(1, n2 + 1); a1 = a2 + rng.randrange(0, n2 - n1 + 1)
        elif shape == "around":
            a1 = a2 - rng.randrange(0, 5); n1 = (a2 - a1) + n2 + rng.randrange(0, 5)
        elif shape == "equal":
            a1, n1 = a2, n2
        elif shape == "gap0":
            n1 = rng.randrange(1, 40); a1 = rng.choice([a2 - n1, a2 + n2])
        elif shape == "over1":
            n1 = rng.randrange(1, 40); a1 = rng.choice([a2 - n1 + 1, a2 + n2 - 1])
        else:
            n1 = rng.randrange(1, 80); a1 = rng.randrange(-3, L + 1)
        st1, st2 = rng.choice([b"+", b"-"]), rng.choice([b"+", b"-"])
        # strand position of a forward interval [a, a + n): lo + a on '+', hi - a - n on '-'; it has to lie inside the
        # chromosome (a record's genome_pos does), the read may run over the end
        p1 = lo + a1 if st1 == b"+" else hi - a1 - n1
        p2 = lo + a2 if st2 == b"+" else hi - a2 - n2
        if not (lo <= p1 < hi and lo <= p2 < hi) or n1 > 1024:
            continue
        cl1 = rng.choice([None, None, 0, 1, n1, n1 // 2, n1 + 3])
        cl2 = rng.choice([None, None, 0, 1, n2, n2 // 2, n2 + 3])
        m1, m2 = rec(p1, 1, st1), rec(p2, 1, st2)
        ex, bases = excluded_positions(start, glen, m1, m2, 1, n1, n2, cl1, cl2)
        got = harness_pair(overlap_harness, start, glen, m1, m2, 1, n1, n2, cl1, cl2)
        assert got == (word_of(ex), bases), (trial, shape, (lo, hi), (p1, n1, st1, cl1), (p2, n2, st2, cl2), hex(got[0]), got[1], ex[:1], ex[-1:], bases)
        seen["shape"].add(shape); seen["strands"].add((st1, st2)); seen["cl"].add((cl1 is None, cl2 is None))
        seen["gap0"] += shape == "gap0" and not ex
        seen["over1"] += shape == "over1" and len(ex) == 1
        seen["past_end"] += p1 + n1 > hi or p2 + n2 > hi
        seen["nonempty"] += bool(ex)
        if ex and trial % 4 == 0:  # every non-eligible variant of a pair that has an interval gives 0
            other = rng.choice([k for k in range(len(lengths)) if k != c])
            for m1x, m2x, bt, l1, l2 in ((m1, m2, 0, n1, n2), (m1, m2, 2, n1, n2), (rec(p1, 0, st1), m2, 1, n1, n2),
                                         (rec(p1, 2, st1), m2, 1, n1, n2), (m1, rec(p2, 0, st2), 1, n1, n2), (m1, rec(p2, 3, st2), 1, n1, n2),
                                         (rec(glen, 1, st1), m2, 1, n1, n2), (m1, rec(glen + 7, 1, st2), 1, n1, n2),
                                         (rec(0xFFFFFFFF, 1, st1), rec(0xFFFFFFFF, 1, st2), 1, n1, n2),
                                         (m1, rec(int(start[other]), 1, st2), 1, n1, n2), (m1, m2, 1, 1025, n2), (m1, m2, 1, n1, 1025)):
                assert excluded_positions(start, glen, m1x, m2x, bt, l1, l2, cl1, cl2) == ([], 0)
                assert harness_pair(overlap_harness, start, glen, m1x, m2x, bt, l1, l2, cl1, cl2) == (0, 0), (trial, bt, l1, l2)
    assert len(seen["shape"]) == 8 and len(seen["strands"]) == 4 and len(seen["cl"]) == 4
    assert seen["gap0"] > 20 and seen["over1"] > 20 and seen["past_end"] > 100 and seen["nonempty"] > 500, seen


def random_genome(rng):
    lengths = [rng.randrange(400, 900), 50, 2, 1, 17, rng.randrange(200, 400)]
    text = "".join(rng.choice("ACGTCG") for _ in range(sum(lengths)))
    start = np.zeros(len(lengths) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lengths)
    return lengths, text, start


def harness_read(L, ref, bases, raw_addr, off, n, batch_bytes, limit, pos, lo, hi, ga, ex_lo, ex_hi, which):
    counts = np.zeros(8, dtype=np.uint16)
    cmu = np.zeros(n, dtype=np.uint8)
    L.overlap_harness_read(ref.ctypes.data, ref.size - 1, bases.ctypes.data, raw_addr, off, n, batch_bytes, limit, 1 if limit else 0,
                           pos, lo, hi, ga, ex_lo, ex_hi, which, counts.ctypes.data, cmu.ctypes.data)
    return counts, cmu


@pytest.mark.parametrize("seed", [1, 2])
def test_slice_mask_letter_by_letter(overlap_harness, seed):
    """an excluded interval at all 16 alignments of both ends, across slice boundaries and inside one slice; the old
    signatures against an empty interval"""
    rng = random.Random(40 + seed)
    lengths, text, start = random_genome(rng)
    R = np.frombuffer(text.encode(), dtype=np.uint8)
    ref = pack_reference(text)
    ends, inside_one, across, dropped = set(), 0, 0, 0
    for trial in range(1500):
        conv = rng.choice("TA")
        c = rng.choice([0, 0, 0, 5, 5, 1, 4])
        lo, hi = int(start[c]), int(start[c + 1])
        pos = rng.choice([lo, hi - 1, max(lo, hi - 17), rng.randrange(lo, hi)])
        n = rng.choice([1, 15, 16, 17, 33, 60, 100, 150, rng.randrange(1, 200)])
        if rng.random() < 0.5:
            n = max(1, min(n, hi - pos + rng.choice([0, 0, 3])))
        seq = []
        for i in range(n):
            g = text[pos + i] if pos + i < len(text) else "A"
            if conv == "T" and g == "C" and rng.random() < 0.5:
                g = "T"
            if conv == "A" and g == "G" and rng.random() < 0.5:
                g = "A"
            seq.append(g)
        seq = "".join(seq)
        call_len = rng.choice([None, None, None, n // 2, n + 5])
        limit = n if call_len is None else min(n, call_len)
        ex_lo = rng.randrange(0, n)
        ex_hi = rng.choice([ex_lo, ex_lo + 1, rng.randrange(ex_lo, n + 1), n, min(n, ex_lo + rng.randrange(1, 16))])
        if trial % 11 == 0:
            ex_lo, ex_hi = ex_hi, ex_lo  # an inverted interval is empty
        off = rng.choice([0, 1, 5, rng.randrange(0, 40)])
        batch_bytes = off + n + rng.choice([0, 1, 7, 64])
        shift = trial % 16  # alignment of the calls buffer: the slice grid
        bases = np.full(400, ord("C"), dtype=np.uint8)
        bases[off:off + n] = np.frombuffer(seq.encode(), dtype=np.uint8)
        bases[batch_bytes:] = 0
        outs = []
        for which, (e_lo, e_hi) in ((0, (ex_lo, ex_hi)), (0, (0, 0)), (1, (7, 9)), (2, (7, 9))):  # (the old forms take no interval)
            raw = np.full(400, 0x23, dtype=np.uint8)
            a16 = (-raw.ctypes.data) % 16 + shift
            counts, cmu = harness_read(overlap_harness, ref, bases, raw.ctypes.data + a16, off, n, batch_bytes, limit, pos, lo, hi,
                                       1 if conv == "A" else 0, e_lo, e_hi, which)
            assert (raw[:a16 + off] == 0x23).all() and (raw[a16 + off + n:] == 0x23).all(), "wrote outside the read"
            outs.append((raw[a16 + off:a16 + off + n].tobytes().decode(), counts.tolist(), cmu.tolist()))
        plain, _ = expected_read([R, R], start, seq, pos, 1, b"+", conv, call_len)
        want = drop_letters(plain, range(ex_lo, ex_hi))
        got, counts, cmu = outs[0]
        what = "trial %d conv %s pos %d [%d, %d) n %d limit %d excl [%d, %d) shift %d" % (trial, conv, pos, lo, hi, n, limit, ex_lo, ex_hi, shift)
        assert got == want, "%s\n got  %s\n want %s" % (what, got, want)
        assert counts == counts_of(want), what
        assert cmu == [0 if ch == "." else 1 if ch.isupper() else 2 for ch in want], what  # what the pile-up adds
        # an empty interval and both old signatures: what the calls always were
        assert outs[1][0] == plain and outs[1][1] == counts_of(plain), what
        assert outs[1] == outs[2] and outs[1][:2] == outs[3][:2], what
        if ex_lo < ex_hi:
            head = (shift + off) % 16  # slice k of the read covers read positions [16 k - head, 16 k - head + 16)
            ends.add(((ex_lo + head) % 16, (ex_hi + head) % 16))
            same = (ex_lo + head) // 16 == (ex_hi - 1 + head) // 16
            inside_one += same
            across += not same
            dropped += sum(a != b for a, b in zip(plain, want))
    assert len({e[0] for e in ends}) == 16 and len({e[1] for e in ends}) == 16
    assert inside_one > 100 and across > 100 and dropped > 1000


def test_flag_masks_old_signature_forwards(overlap_harness):
    rng = random.Random(5)
    for _ in range(3000):
        i0 = rng.randrange(-15, 200)
        p, lo = rng.randrange(0, 500), 0
        hi = p + rng.randrange(1, 300)
        limit = rng.randrange(0, 250)
        ga = rng.randrange(2)
        ex_lo, ex_hi = rng.randrange(0, 220), rng.randrange(0, 220)
        out = np.zeros(6, dtype=np.uint32)
        overlap_harness.overlap_harness_flags(i0, p, lo, hi, limit, ga, ex_lo, ex_hi, out.ctypes.data)
        call_plain = int(out[3])
        mask = 0
        for k in range(16):
            if ex_lo <= i0 + k < ex_hi:
                mask |= 1 << (2 * k)
        assert int(out[0]) == call_plain & ~mask and out[1] == out[4] and out[2] == out[5]
        empty = np.zeros(6, dtype=np.uint32)
        overlap_harness.overlap_harness_flags(i0, p, lo, hi, limit, ga, 0, 0, empty.ctypes.data)
        assert empty[:3].tolist() == empty[3:].tolist() == out[3:].tolist()


# ---------------------------------------------------------------------------
# the golden libraries on the oracle's records: how common the case is
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("files", [("pe_1.fastq", "pe_2.fastq"), ("pe150_1.fastq", "pe150_2.fastq")])
def test_golden_libraries_hold_over_100_overlapping_pairs(g1_db, overlap_harness, files):
    from test_gpu_meth import load
    from test_gpu_overlap import GOLDEN_TOTALS
    _, s1, _ = load(files[0])
    _, s2, _ = load(files[1])
    res, _, _ = refio.oracle_pe(g1_db, s1, s2)
    pairs = bases = 0
    for i in range(len(s1)):
        ex, b = excluded_positions(g1_db.start_index, g1_db.genome_len, res["m1"][i], res["m2"][i], res["best_times"][i], len(s1[i]), len(s2[i]))
        got = harness_pair(overlap_harness, g1_db.start_index, g1_db.genome_len, res["m1"][i], res["m2"][i], int(res["best_times"][i]),
                           len(s1[i]), len(s2[i]), None, None)
        assert got == (word_of(ex), b), i
        pairs += bool(ex)
        bases += b
    assert pairs >= 100 and (pairs, bases) == GOLDEN_TOTALS[files[0]]
