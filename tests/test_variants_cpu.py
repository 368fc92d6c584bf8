"""Opposite-strand evidence (include/walt_amd.h, "opposite-strand evidence"), the parts that need no device: what the
evidence kernel runs per lane and the rule (walt_amd/csrc/variants_core.h), compiled with g++ (tests/variants_harness.cpp)
and compared with the pure-Python restatement of tests/test_gpu_variants.py; the <out>.variants and <out>.variantstats
writers of hostio.h; the exports of the three libraries, the binding's surface and refusals without a device; bin/walt's
options; and a check that the golden libraries hold what the command-line tests on the device count on."""
import ctypes
import inspect
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_variants import base_letter, expected_evidence, flagged, judged
from test_meth_cpu import pack_reference
from test_pileup_cpu import random_genome

NAMES = ("walt_meth_evidence_batch", "walt_meth_evidence_batch_device", "walt_meth_pileup_batch_ev", "walt_meth_pileup_batch_ev_device",
         "walt_pileup_variants", "walt_pileup_variants_device", "walt_pileup_mask_variants", "walt_pileup_mask_variants_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")
FULL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def harness(scratch):
    so = os.path.join(scratch, "libvariants_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                    os.path.join(refio.HERE, "variants_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.variants_harness_slice.argtypes = [vp, u64, u32, u32, vp]
    L.variants_harness_slice.restype = None
    L.variants_harness_counts.argtypes = [u32, u32, u32, u32, u32, u64]
    L.variants_harness_rule.argtypes = [u32, u32, u32, u32]
    L.variants_harness_read.argtypes = [vp, u32, vp, u32, u64, u64, u64, u32, u32, u32, u32, u32, ci, vp, vp]
    L.variants_harness_read.restype = ctypes.c_longlong
    L.variants_harness_parse.argtypes = [ctypes.c_char_p, u32, u32, vp]
    L.variants_harness_line.argtypes = [ctypes.c_char_p, u32, vp, vp, u32]
    L.variants_harness_line.restype = u32
    L.variants_harness_block.argtypes = [vp, u32, u32, vp, u32]
    L.variants_harness_block.restype = u32
    return L


# ---------------------------------------------------------------------------
# what the kernel runs per lane
# ---------------------------------------------------------------------------
def test_one_slice_bit_by_bit(harness):
    """ev_slice on random slices: any 16 bytes, any reference codes, any set of positions that may be judged"""
    rng = random.Random(5)
    seen = set()
    for trial in range(4000):
        raw = bytes(rng.choice(b"ACGTACGTACGTNn.\x00\xff") if rng.random() < 0.9 else rng.randrange(256) for _ in range(16))
        rd = np.frombuffer(raw, dtype=np.uint32).copy()
        codes = [rng.randrange(4) for _ in range(32)]  # positions q0 - 2 .. q0 + 29
        ext = sum(c << (2 * k) for k, c in enumerate(codes))
        call = sum(1 << (2 * k) for k in range(16) if rng.random() < 0.7)
        for ga in (0, 1):
            out = np.zeros(2, dtype=np.uint32)
            harness.variants_harness_slice(rd.ctypes.data, ext, ga, call, out.ctypes.data)
            want_m = want_o = 0
            for k in range(16):
                ref = "ACGT"[codes[k + 2]]
                if not (call >> (2 * k)) & 1 or ref != ("C" if ga else "G"):
                    continue
                if base_letter(raw[k]) == ref:
                    want_m |= 1 << (2 * k)
                else:
                    want_o |= 1 << (2 * k)
                seen.add((ga, base_letter(raw[k]) == ref))
            assert (int(out[0]), int(out[1])) == (want_m, want_o), (trial, ga, raw, codes, call)
    assert len(seen) == 4


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_evidence_of_whole_reads_equals_the_restatement(harness, seed):
    """random genomes with chromosomes of 1, 2 and 17 bases, both strands, both conversions, all 16 slice alignments, reads
    over a chromosome's end, call_len 0, 1, 15, 16, 17 and the read's length, bytes other than A, C, G and T; the two
    planes compared over every position of the genome after every read"""
    rng = random.Random(seed)
    lengths, text, minus, start = random_genome(rng)
    assert {1, 2, 17} <= set(lengths)
    R = [np.frombuffer(text.encode(), dtype=np.uint8), np.frombuffer(minus.encode(), dtype=np.uint8)]
    refs = [pack_reference(text), pack_reference(minus)]
    glen = len(text)
    got_m, got_o = np.zeros(glen, dtype=np.uint32), np.zeros(glen, dtype=np.uint32)
    want = None
    combos, heads, limits, over, odd = set(), set(), set(), 0, 0
    recs = np.zeros(1, dtype=[("genome_pos", "<u4"), ("times", "<u4"), ("strand", "S1")])
    for trial in range(2500):
        conv = rng.choice("TA")
        strand = rng.choice([b"+", b"-"])
        G = text if strand == b"+" else minus
        c = rng.randrange(len(lengths))
        lo, hi = int(start[c]), int(start[c + 1])
        pos = rng.choice([lo, lo + 1, hi - 1, max(lo, hi - 2), max(lo, hi - 17), rng.randrange(lo, hi)])
        pos = min(max(pos, lo), hi - 1)
        n = rng.choice([1, 2, 15, 16, 17, 31, 33, 100, 128, 129, rng.randrange(1, 300), 1023, 1024])
        if rng.random() < 0.5:
            n = max(1, min(n, hi - pos + rng.choice([0, 0, 3])))  # up to, or three bases over, the chromosome's end
        over += pos + n > hi
        seq = bytearray()
        for i in range(n):
            g = G[pos + i] if pos + i < glen else "A"
            if g == ("G" if conv == "T" else "C") and rng.random() < 0.3:
                g = rng.choice("ACGT")
            if rng.random() < 0.03:
                g = rng.choice("Nn.acgt\x00\xff\x42")
                odd += 1
            seq += g.encode("latin-1")
        call_len = rng.choice([None, 0, 1, 15, 16, 17, n, n + 5])
        limit = n if call_len is None else min(n, call_len)
        limits.add(call_len if call_len in (0, 1, 15, 16, 17) else "n")
        off = rng.choice([0, 0, 1, 5, rng.randrange(0, 40)])
        batch_bytes = off + n + rng.choice([0, 0, 1, 7, 64])
        head = trial % 16  # every alignment of the slice grid
        bases = np.full(1200 + 128, ord("G"), dtype=np.uint8)
        bases[off:off + n] = np.frombuffer(bytes(seq), dtype=np.uint8)
        bases[batch_bytes:] = 0
        o = 1 if strand == b"-" else 0
        adds = harness.variants_harness_read(refs[o].ctypes.data, refs[o].size - 1, bases.ctypes.data, head, off, n, batch_bytes, limit,
                                             pos, lo, hi, 1 if conv == "A" else 0, o, got_m.ctypes.data, got_o.ctypes.data)
        assert adds >= 0
        recs["genome_pos"], recs["times"], recs["strand"] = pos, 1, strand
        want = expected_evidence(R, start, [bytes(seq)], recs, conv, None if call_len is None else [call_len], into=want)
        assert np.array_equal(got_m, want[0]) and np.array_equal(got_o, want[1]), (
            "trial %d conv %s strand %s pos %d [%d, %d) n %d off %d head %d call_len %s" % (trial, conv, strand, pos, lo, hi, n, off, head, call_len))
        combos.add((strand, conv))
        heads.add(head)
    assert len(combos) == 4 and len(heads) == 16 and limits == {0, 1, 15, 16, 17, "n"} and over > 100 and odd > 500
    assert int(want[0].sum()) > 5000 and int(want[1].sum()) > 2000
    # evidence lies on forward C and G alone
    assert not (want[0] + want[1])[~np.isin(R[0], np.frombuffer(b"CG", dtype=np.uint8))].any()


def test_which_records_count(harness):
    ok = (1, 0, 10, 100, ord("T"), 50)
    assert harness.variants_harness_counts(*ok) == 1 and harness.variants_harness_counts(1, 0, 99, 100, ord("A"), 1024) == 1
    for k, v in ((0, 0), (0, 2), (1, 1), (1, 255), (2, 100), (2, FULL), (4, ord("C")), (4, 0), (5, 0), (5, 1025), (5, 1 << 40)):
        args = list(ok)
        args[k] = v
        assert harness.variants_harness_counts(*args) == 0, (k, v)


def test_rule_at_its_boundaries(harness):
    rule = lambda m, o, d, p: harness.variants_harness_rule(m, o, d, p)
    for d in (1, 2, 5, 7, 1000, FULL):
        for p in (0, 1, 30, 50, 99):
            cases = [(0, d - 1), (d - 1, 0), (0, d), (d, 0), (d // 2, d - d // 2)]
            # 100 other == p total (not flagged), and with one more `other` (flagged)
            cases += [(100 - p, p), (100 - p, p + 1), (7 * (100 - p), 7 * p), (7 * (100 - p), 7 * p + 1)]
            cases += [(FULL, FULL), (FULL, 0), (0, FULL), (FULL - 1, FULL)]
            for m, o in cases:
                want = (1 if judged(m, o, d) else 0) | (2 if flagged(m, o, d, p) else 0)
                assert rule(m, o, d, p) == want, (m, o, d, p)
    assert rule(0, 4, 5, 0) == 0 and rule(0, 5, 5, 0) == 3          # total == min_depth - 1, total == min_depth
    assert rule(70, 30, 5, 30) == 1 and rule(70, 31, 5, 30) == 3    # 100 other == p total, one more other
    assert rule(FULL, FULL, FULL, 50) == 1 and rule(FULL, FULL, FULL, 49) == 3  # 64-bit products
    assert rule(3, 3, 5, 50) == 1 and rule(2, 3, 5, 50) == 3        # MethPipe: fewer than half show the expected base


def test_per_lane_logic_under_the_host_sanitizers(scratch):
    """tests/variants_sanitize_main.cpp, a stand-alone program over tests/variants_harness.cpp built with the host's address
    and undefined-behaviour sanitizers: bases, reference and counters each in a heap block of exactly its size -- a load or
    an add outside them ends the program, and so do adds that differ from a plain walk"""
    exe = os.path.join(scratch, "variants_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(refio.HERE, "variants_sanitize_main.cpp"), os.path.join(refio.HERE, "variants_harness.cpp"), "-o", exe],
                   check=True, timeout=300)
    pr = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert pr.returncode == 0 and pr.stdout.startswith("ok "), pr.stdout[-2000:]
    assert int(pr.stdout.split()[1]) > 50000


# ---------------------------------------------------------------------------
# exports, binding
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert hdr.index("---- four-CpG epialleles") < hdr.index("---- opposite-strand evidence") < hdr.index("---- options")
    assert "} walt_variant_site; /* 24 bytes */" in hdr


def test_binding_surface_and_refusals_without_a_device():
    import walt_amd
    for nm in ("add_evidence_batch", "add_evidence_batch_device", "variants", "variants_device", "mask_variants", "mask_variants_device"):
        assert hasattr(walt_amd.Pileup, nm), nm
    for fn in (walt_amd.Pileup.variants, walt_amd.Pileup.mask_variants):
        p = inspect.signature(fn).parameters
        assert list(p)[:2] == ["self", "ev"] and (p["pos_lo"].default, p["pos_hi"].default, p["min_depth"].default, p["max_percent"].default) == (0, None, 5, 50)
    dt = walt_amd.variant_site_dtype
    assert dt.itemsize == 24 and dt.names == ("pos", "meth", "unmeth", "strand", "context", "reserved", "match", "other")
    assert [dt.fields[f][1] for f in dt.names] == [0, 4, 8, 12, 13, 14, 16, 20]
    # evidence= is keyword-only and leaves the parameter lists as they are shown
    for fn in (walt_amd.Pileup.add_batch, walt_amd.Pileup.add_batch_device):
        assert "evidence" not in inspect.signature(fn).parameters and list(inspect.signature(fn).parameters)[-1] == "epi"

    class Index:
        def _meth_batch(self, *args):
            return ("host",) + args

        def _meth_batch_device(self, *args):
            self.last = ("device",) + args

    class Ev(walt_amd.Pileup):
        def __init__(self, h):
            self._h, self._index = h, Index()

        def close(self):
            pass

    pile, ev = Ev(11), Ev(22)
    every = ("b", "o", "r", "A", 1, False, False, 2, False, 3, 4, 5, 6, 7, 8, 9)  # bases .. trim3, pairs in its place
    handed_on = ("b", "o", "r", "A", 1, False, False, 2, False, 4, 5, 6, 7, 8, 9, 3)
    assert pile.add_batch(*every, epi="E") == ("host", 11) + handed_on + ("E", None)
    assert pile.add_batch(*every, epi="E", evidence=ev) == ("host", 11) + handed_on + ("E", 22)
    assert pile.add_batch("b", "o", "r", evidence=ev)[-1] == 22
    with pytest.raises(TypeError):
        pile.add_batch(*every, "E", ev)
    pile.add_batch_device(1, 2, 3, 4, evidence=ev, stream=9)
    got = pile._index.last
    assert got[:3] == ("device", 11, "skip") and got[-1] == 22 and got[4] == 9
    pile.add_batch_device(1, 2, 3, 4)
    assert pile._index.last[-1] is None
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm

    class Named:  # stands for the library: _meth_form only looks the function up by name
        def __getattr__(self, name):
            return name

    form = lambda **kw: walt_amd._meth_form(Named(), kw.pop("device", False), kw.pop("pile", None), **kw)
    assert form(ev=(9,)) == ("walt_meth_pileup_batch_ev", (None,), (None, 1, None, None, 0, 0, 0, None, None, 9))
    assert form(ev=(9,), epi=(4,), pairs=(7,), device=True, pile=3, skip=(5, 2), excl=(6,), mbias=(8, 1), trim=(2, 4)) == \
        ("walt_meth_pileup_batch_ev_device", (3,), (5, 2, 6, 8, 1, 2, 4, 7, 4, 9))
    # without it: the forms a call always reached
    assert form(epi=(9,)) == ("walt_meth_pileup_batch_epi", (None,), (None, 1, None, None, 0, 0, 0, None, 9))
    assert form(pile=3)[0] == "walt_meth_pileup_batch" and form()[0] == "walt_meth_call_batch"
    # no device: null objects are refused, not crashed on, and the message names the call
    E = walt_amd.WALT_EINVAL
    batch = (None, None, 0, None, 16, None, 0, ord("T"), None)
    assert L.walt_meth_evidence_batch(None, None, *batch, None, 1) == E and b"walt_meth_evidence_batch:" in L.walt_last_error()
    assert L.walt_meth_evidence_batch_device(None, None, *batch, None, 1, None) == E and b"walt_meth_evidence_batch_device:" in L.walt_last_error()
    rest = (None, None, None, None, 1, None, None, 0, 0, 0, None, None, None)
    assert L.walt_meth_pileup_batch_ev(None, None, *batch, *rest) == E and b"walt_meth_pileup_batch_ev:" in L.walt_last_error()
    assert L.walt_meth_pileup_batch_ev_device(None, None, *batch, *rest, None) == E and b"walt_meth_pileup_batch_ev_device:" in L.walt_last_error()
    n = ctypes.c_uint64(0)
    assert L.walt_pileup_variants(None, None, 0, 0, 5, 50, None, 0, ctypes.byref(n)) == E and b"walt_pileup_variants:" in L.walt_last_error()
    assert L.walt_pileup_variants_device(None, None, 0, 0, 5, 50, None, 0, None, None) == E and b"walt_pileup_variants_device:" in L.walt_last_error()
    assert L.walt_pileup_mask_variants(None, None, 0, 0, 5, 50, None) == E and b"walt_pileup_mask_variants:" in L.walt_last_error()
    assert L.walt_pileup_mask_variants_device(None, None, 0, 0, 5, 50, None, None) == E and b"walt_pileup_mask_variants_device:" in L.walt_last_error()


# ---------------------------------------------------------------------------
# the command line's pieces
# ---------------------------------------------------------------------------
def test_writers_of_variants_and_variantstats(harness):
    import walt_amd
    buf = ctypes.create_string_buffer(512)
    site = np.zeros(1, dtype=walt_amd.variant_site_dtype)
    for row, chrom, start, want in (
            ((1234, 3, 4, ord("+"), 0, 0, 0, 9), "chr1", 1000, "chr1\t234\t+\tCpG\t3\t4\t0\t9\n"),
            ((7, 0, 0, ord("-"), 2, 0, FULL, FULL), "a b", 7, "a b\t0\t-\tCHH\t0\t0\t4294967295\t4294967295\n"),
            ((FULL - 1, FULL, 1, ord("-"), 3, 0, 1, 2), "x", 0, "x\t4294967294\t-\tunknown\t4294967295\t1\t1\t2\n"),
            ((50, 1, 2, ord("+"), 1, 0, 5, 6), "chrB", 50, "chrB\t0\t+\tCHG\t1\t2\t5\t6\n")):
        site[0] = row
        n = harness.variants_harness_line(chrom.encode(), start, site.ctypes.data, buf, 512)
        assert buf.raw[:n].decode() == want
    tot = np.array([10, 4, 3, 7, 1 << 40], dtype=np.uint64)
    n = harness.variants_harness_block(tot.ctypes.data, 5, 50, buf, 512)
    assert buf.raw[:n].decode() == "judged: 10\nflagged: 4\nmasked sites: 3\nmasked meth: 7\nmasked unmeth: 1099511627776\nrule\t5\t50\n"
    tot[:] = 0
    n = harness.variants_harness_block(tot.ctypes.data, 1000000, 0, buf, 512)
    assert buf.raw[:n].decode() == "judged: 0\nflagged: 0\nmasked sites: 0\nmasked meth: 0\nmasked unmeth: 0\nrule\t1000000\t0\n"
    # the values of -MVD and -MVP
    out = ctypes.c_uint32(77)
    for text, lo, hi, want in (("1", 1, 1000000, 1), ("1000000", 1, 1000000, 1000000), ("0", 0, 99, 0), ("99", 0, 99, 99), ("007", 1, 1000000, 7)):
        assert harness.variants_harness_parse(text.encode(), lo, hi, ctypes.byref(out)) == 1 and out.value == want, text
    out.value = 77
    for text, lo, hi in (("0", 1, 1000000), ("1000001", 1, 1000000), ("100", 0, 99), ("", 0, 99), ("-1", 0, 99), ("5x", 0, 99), ("2.5", 0, 99),
                         (" 5", 0, 99), ("+5", 0, 99), ("99999999", 1, 1000000)):
        assert harness.variants_harness_parse(text.encode(), lo, hi, ctypes.byref(out)) == 0 and out.value == 77, text


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


def test_cli_parses_the_options_in_every_mode(tmp_path):
    pr = run([])
    assert pr.returncode == 0 and " -MV " in pr.stdout and " -MVD <n> " in pr.stdout and " -MVP <p> " in pr.stdout and " -ME " in pr.stdout, pr.stdout
    idx, out = str(tmp_path / "none.dbindex"), str(tmp_path / "o.mr")
    pair, single = ["-1", "a.fastq", "-2", "b.fastq"], ["-r", "x.fastq"]
    base = ["-i", idx, "-o", out]
    modes = [(single, []), (single, ["-A"]), (single, ["-R"]), (pair, []), (pair, ["-P"]), (pair, ["-RP"])]
    # the three spellings are known in every mode, alone (a consumer) and beside the others: the run gets as far as the index check
    for reads, mode in modes:
        for flag in ("-MV", "-variants", "--mask-variants"):
            for extra in ([], ["-M", "-sam"], ["-MA", "-MC", "-MB", "-ML", "-ME"], ["-D", "-C", "AGATCGGAAGAGC"], ["-I5", "3"], ["-F", "3", "-FP", "20"],
                          ["-g", "0,0"], ["-MVD", "2", "-MVP", "0"]):
                pr = run(base + reads + mode + extra + [flag])
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, mode, extra, pr.stdout)
    # -MV is something for -I5, -NO and the -F options to ask for
    for args in (single + ["-I5", "3", "-MV"], pair + ["-NO", "-MV"], single + ["-FC", "2", "-MV"]):
        pr = run(base + args)
        assert pr.returncode != 0 and "index file missing" in pr.stdout, (args, pr.stdout)
    # -MVD and -MVP: their spellings and ranges, and that they go with -MV only
    for flags, good, bad, says in ((("-MVD", "-variant-min-depth", "--variant-min-depth"), ("1", "5", "1000000"), ("0", "1000001", "-3", "x", "2.5", ""), "1 to 1000000"),
                                   (("-MVP", "-variant-max-percent", "--variant-max-percent"), ("0", "50", "99"), ("100", "-1", "x", "2.5", ""), "0 to 99")):
        for flag in flags:
            for reads, mode in modes:
                pr = run(base + reads + mode + ["-MV", flag, good[1]])
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, mode, pr.stdout)
            for value in good:
                pr = run(base + single + ["-MV", flag, value])
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, value, pr.stdout)
            for value in bad:
                pr = run(base + single + ["-MV", flag, value])
                assert pr.returncode != 0 and says in pr.stdout and "index file missing" not in pr.stdout, (flag, value, pr.stdout)
            for others in ([], ["-MC"], ["-M", "-ML"]):
                pr = run(base + single + others + [flag, good[0]])
                assert pr.returncode != 0 and "-MV" in pr.stdout and "index file missing" not in pr.stdout, (flag, others, pr.stdout)
    assert not os.path.exists(out) and not os.path.exists(out + ".variants") and not os.path.exists(out + ".variantstats")


# ---------------------------------------------------------------------------
# the golden libraries hold what the command-line tests on the device count on
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,conv,pattern", [("se_sam_au", "T", None), ("se_ag_sam_au", "A", None), ("se_sam_au", "T", 5),
                                               ("se_sam_au", "T", 7), ("se_clip_sam_au", "T", None)])
def test_golden_runs_hold_flagged_sites_with_calls(case, conv, pattern):
    """the golden SAM of a single-end run walked by the restatement at -MVD 2 -MVP 0 (ambiguous and unmapped records left
    out; the clipped library up to each read's clip point): at least 10 flagged positions that also carry calls and at
    least 1,000 unflagged covered sites, the thresholds of tests/test_gpu_variants.py's command-line tests, which run these
    libraries (seed patterns 5 and 7 and -C included)"""
    from test_gpu_cpgpairs import read_fasta
    from test_gpu_variants import D2, MIN_FLAGGED_WITH_CALLS, MIN_UNFLAGGED_COVERED, P0, enough_to_test, sam_walk
    names, seqs = read_fasta(os.path.join(refio.GOLDEN, "g1.fa"))
    R0 = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    sam = refio.golden_file(case, "out.sam", pattern)
    limit_of = None
    if case == "se_clip_sam_au":
        from test_gpu_meth import clip_point, load
        args = refio.golden_meta()["cases"][case]["args"]
        adaptor = args[args.index("-C") + 1]
        reads = dict(zip(*load("se_clip.fastq")[:2]))
        limit_of = lambda name, flag, n: clip_point(adaptor, reads[name])
    meth, unmeth, match, other, walked, undecided = sam_walk(sam, names, seqs, lambda flag: conv, limit_of)
    assert walked > 200 and undecided == 0
    with_calls, unflagged = enough_to_test(R0, meth, unmeth, match, other, D2, P0)
    print("%s, seed pattern %s: %d flagged positions with calls, %d unflagged covered sites" % (case, pattern or 3, with_calls, unflagged))
    assert with_calls >= MIN_FLAGGED_WITH_CALLS and unflagged >= MIN_UNFLAGGED_COVERED
    # a site's calls and its evidence come from reads of opposite kinds, and most evidence shows the reference base
    assert int(meth.sum()) > 0 and int(unmeth.sum()) > 0 and int(match.sum()) > 20 * int(other.sum()) > 0
