"""Genome-wide methylation levels (include/walt_amd.h, "methylation levels"), the parts that need no device: the three
libraries export the calls, the binding's struct layout and surface, null arguments and bad ranges, bin/walt -ML, the
<out>.levels writer, and what the kernel runs per lane (walt_amd/csrc/levels_core.h) compiled with g++
(tests/levels_harness.cpp) and compared with the plain restatement of tests/test_gpu_levels.py on random genomes."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_levels import (HEADER, as_dict, assert_same, classes, empty_levels, expected_levels, level_bin, level_q30,
                             levels_text)
from test_meth_cpu import pack_reference

CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")
NAMES = ("walt_pileup_levels", "walt_pileup_levels_device", "walt_pileup_read", "walt_pileup_add")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_levels_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert "} walt_level_row;" in hdr and "} walt_levels;" in hdr


def test_struct_layout_binding_surface_and_refusals():
    import walt_amd
    row, dt = walt_amd.level_row_dtype, walt_amd.levels_dtype
    assert row.itemsize == 128 and dt.itemsize == 656
    assert [row.fields[f][1] for f in ("sites", "covered", "meth", "unmeth", "max_depth", "level_sum", "hist")] == [0, 8, 16, 24, 32, 40, 48]
    assert dt.fields["row"][1] == 0 and dt.fields["offref"][1] == 640
    for nm in ("levels", "levels_device", "read", "add"):
        assert hasattr(walt_amd.Pileup, nm), nm
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm
    # no device: a null pile-up is refused, not crashed on (a range cannot be checked without one)
    out = np.zeros(1, dtype=dt)
    one = np.zeros(4, dtype=np.uint32)
    assert L.walt_pileup_levels(None, 0, 0, out.ctypes.data) == walt_amd.WALT_EINVAL
    assert b"walt_pileup_levels" in L.walt_last_error()
    assert L.walt_pileup_levels(None, 0, 0, None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_levels(None, 5, 4, out.ctypes.data) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_levels_device(None, 0, 0, None, None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_read(None, 0, 4, one.ctypes.data, one.ctypes.data) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_add(None, 0, 4, one.ctypes.data, None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_add(None, 4, 0, None, None) == walt_amd.WALT_EINVAL
    assert b"walt_pileup_add" in L.walt_last_error()
    assert not out.view(np.uint8).any()


def run_cli(args):
    pr = subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    return pr.returncode, pr.stdout


def test_cli_accepts_the_option_in_every_spelling(tmp_path):
    rc, text = run_cli([])
    assert rc == 0 and " -ML " in text
    tail = ["-i", str(tmp_path / "none.dbindex"), "-o", str(tmp_path / "o.mr")]
    for flag in ("-ML", "-levels", "--meth-levels"):
        rc, text = run_cli([flag, "-r", "x.fastq"] + tail)
        assert rc != 0 and "index file missing" in text, text  # parsed, and the index is looked at first
        assert not (tmp_path / "o.mr.levels").exists()
    # a methylation consumer: -NO, -I5 3 and -F 3 are accepted with -ML alone and still refused without one
    for opts, reads in ((["-NO"], ["-1", "a.fastq", "-2", "b.fastq"]), (["-I5", "3"], ["-r", "x.fastq"]), (["-F", "3"], ["-r", "x.fastq"])):
        rc, text = run_cli(opts + ["-ML"] + reads + tail)
        assert rc != 0 and "index file missing" in text, text
        rc, text = run_cli(opts + reads + tail)
        assert rc != 0 and "nothing for" in text and "index file missing" not in text, text


# ---------------------------------------------------------------------------
# what the kernel runs per lane, and the writer, on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(scratch):
    import walt_amd
    so = os.path.join(scratch, "liblevels_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-I", CSRC,
                    os.path.join(refio.HERE, "levels_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.levels_harness_classes.argtypes = [vp, u32, vp, u32, vp, vp]
    L.levels_harness_classes.restype = None
    L.levels_harness_q30.argtypes = [u64, u64]
    L.levels_harness_q30.restype = u64
    L.levels_harness_bin.argtypes = [u64, u64]
    L.levels_harness_bin.restype = u32
    L.levels_harness_summary.argtypes = [vp, u32, vp, u32, vp, vp, u32, u32, vp]
    L.levels_harness_summary.restype = None
    L.levels_harness_text.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
    assert walt_amd.levels_dtype.itemsize == 656
    return L


def random_genome(rng):
    """chromosomes of 1, 2, 3 and 17 bases among longer ones; CG across a chromosome boundary and at the genome's first
    and last two bases; C / G rich"""
    lengths = [rng.randrange(200, 700), 1, 2, 3, 17, rng.randrange(300, 900), 1, rng.randrange(64, 400), 2]
    seqs = [list(rng.choice("ACGTCG") for _ in range(L)) for L in lengths]
    seqs[0][:2] = "CG"
    seqs[-1][:] = "CG"
    seqs[4][-1] = "C"   # ...C | G...: no pair, and the C has no context inside its chromosome
    seqs[5][0] = "G"
    text = "".join("".join(s) for s in seqs)
    start = np.zeros(len(lengths) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lengths)
    return text, start


def harness_counters(rng, text):
    """0, 1 and 0xFFFFFFFF on both halves of the pairs (their sums need 34 bits), small counts elsewhere"""
    pick = [0, 1, 0xFFFFFFFF]
    meth = np.array([rng.choice([0, 0, 1, 2, 7, 50]) for _ in text], dtype=np.uint32)
    unmeth = np.array([rng.choice([0, 0, 1, 3, 9, 80]) for _ in text], dtype=np.uint32)
    for f in range(len(text) - 1):
        if text[f:f + 2] == "CG" and rng.random() < 0.7:
            meth[f], meth[f + 1], unmeth[f], unmeth[f + 1] = (rng.choice(pick) for _ in range(4))
    return meth, unmeth


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_class_pair_and_summary_equal_the_restatement(harness, seed):
    import walt_amd
    rng = random.Random(seed)
    text, start = random_genome(rng)
    glen = len(text)
    R0 = np.frombuffer(text.encode(), dtype=np.uint8)
    ref = pack_reference(text)
    cls, pair = classes(R0, start)
    got_cls, got_pair = np.zeros(glen, dtype=np.uint8), np.zeros(glen, dtype=np.uint8)
    harness.levels_harness_classes(ref.ctypes.data, ref.size - 1, start.ctypes.data, start.size - 1, got_cls.ctypes.data, got_pair.ctypes.data)
    assert got_cls.tolist() == [4 if c is None else c for c in cls]
    assert got_pair.tolist() == [int(p) for p in pair]
    # the planted edges: pairs at the genome's two ends, none across the boundary
    assert pair[0] and pair[glen - 2] and not pair[glen - 1]
    edge = int(start[5]) - 1
    assert text[edge:edge + 2] == "CG" and not pair[edge] and cls[edge] == 3 and cls[edge + 1] == 3
    assert {None, 0, 1, 2, 3} <= set(cls)
    meth, unmeth = harness_counters(rng, text)
    sums = {int(meth[f]) + int(meth[f + 1]) for f in range(glen) if pair[f]}
    assert 2 * 0xFFFFFFFF in sums and 0xFFFFFFFF + 1 in sums
    cuts = [0, 1, 2, int(start[5]) - 1, int(start[5]), glen // 2, glen - 2, glen - 1, glen]
    for lo, hi in [(0, glen)] + list(zip(cuts[:-1], cuts[1:])):
        out = np.zeros(1, dtype=walt_amd.levels_dtype)
        harness.levels_harness_summary(ref.ctypes.data, ref.size - 1, start.ctypes.data, start.size - 1, meth.ctypes.data,
                                       unmeth.ctypes.data, lo, hi, out.ctypes.data)
        assert_same(as_dict(out[0]), expected_levels(cls, pair, meth, unmeth, lo, hi), "[%d, %d)" % (lo, hi))


def test_level_q30_and_level_bin(harness):
    edges = [(1, 9), (2, 8), (3, 7), (4, 6), (5, 5), (6, 4), (7, 3), (8, 2), (9, 1), (10, 0), (0, 5), (99, 1), (1, 99)]
    assert [level_bin(m, u) for m, u in edges] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 0, 9, 0]
    big = [0, 1, 2, 0xFFFFFFFF, 0xFFFFFFFF + 1, 2 * 0xFFFFFFFF]
    cases = edges + [(m, u) for m in big for u in big if m + u]
    rng = random.Random(4)
    for _ in range(20000):
        bits = rng.randrange(1, 35)
        m, u = rng.randrange(0, min(1 << bits, 2 ** 33 - 1)), rng.randrange(0, min(1 << rng.randrange(1, 35), 2 ** 33 - 1))
        if m + u:
            cases.append((m, u))
    for k in range(1, 2000):  # exact multiples and their neighbours: where a rounded quotient could land on the wrong side
        d = rng.randrange(1, 2 ** 33)
        m = min(d, (d * rng.randrange(0, 11)) // 10 + rng.choice([-1, 0, 1]))
        if m >= 0:
            cases.append((m, d - m))
    for m, u in cases:
        assert harness.levels_harness_q30(m, u) == level_q30(m, u), (m, u)
        assert harness.levels_harness_bin(m, u) == level_bin(m, u), (m, u)


def test_levels_writer_text(harness):
    import walt_amd
    rec = np.zeros(1, dtype=walt_amd.levels_dtype)
    lv = empty_levels()
    lv["row"][0].update(sites=10, covered=4, meth=30, unmeth=10, max_depth=17, level_sum=3 << 30, hist=[1, 0, 0, 0, 0, 0, 0, 0, 0, 3])
    lv["row"][1].update(sites=7, covered=1, meth=0, unmeth=2 ** 33, max_depth=2 ** 33, level_sum=0, hist=[1] + [0] * 9)
    lv["row"][2].update(sites=5)                      # no site covered: NA for the two levels, 0.000000 for the others
    lv["row"][4].update(sites=5, covered=2, meth=30, unmeth=10, max_depth=30, level_sum=(1 << 30) + (1 << 29), hist=[0] * 5 + [1, 0, 0, 0, 1])
    for r in range(5):
        for k, v in lv["row"][r].items():
            rec[0]["row"][r][k] = v
    buf = ctypes.create_string_buffer(8192)
    n = harness.levels_harness_text(rec.ctypes.data, buf, 8192)
    got = buf.raw[:n].decode()
    assert got == levels_text(lv)
    lines = got.split("\n")
    assert lines[0] + "\n" == HEADER and len(lines) == 8 and lines[7] == ""
    assert lines[1] == "cytosines\t22\t5\t30\t8589934602\t8589934592\t390451574.181818\t0.227273\t0.600000\t0.000000\t2\t0\t0\t0\t0\t0\t0\t0\t0\t3"
    assert lines[2].startswith("CpG\t10\t4\t30\t10\t17\t4.000000\t0.400000\t0.750000\t0.750000\t1\t")
    assert lines[4] == "CHH\t5\t0\t0\t0\t0\t0.000000\t0.000000\tNA\tNA" + "\t0" * 10
    assert lines[5] == "unknown\t0\t0\t0\t0\t0\tNA\tNA\tNA\tNA" + "\t0" * 10
    assert lines[6].startswith("CpG_symmetric\t5\t2\t30\t10\t30\t8.000000\t0.400000\t0.750000\t0.750000\t")


def test_the_harness_under_the_sanitizers(scratch):
    """tests/levels_harness.cpp as a program of its own (-DLEVELS_HARNESS_MAIN) with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = os.path.join(scratch, "levels_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DLEVELS_HARNESS_MAIN", "-I", CSRC, os.path.join(refio.HERE, "levels_harness.cpp"), "-o", exe],
                   check=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("positions 645 pairs ") and run.stdout.rstrip().endswith(" bad 0"), run.stdout + run.stderr
