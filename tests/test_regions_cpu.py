"""Methylation levels per region (include/walt_amd.h, "methylation levels per region"), the parts that need no device:
the three libraries export the calls, the binding's struct layout and surface, null arguments, bin/walt -MR, the BED
reader and the <out>.regions writer (walt_amd/csrc/host/hostio.h), and how a call is cut into units
(walt_amd/csrc/regions_core.h) compiled with g++ (tests/regions_harness.cpp) and compared with a plain restatement."""
import bisect
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_levels import classes
from test_gpu_regions import REGIONS_HEADER, U, rec_rows, regions_text, want_record, zero_record
from test_meth_cpu import pack_reference

CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")
NAMES = ("walt_pileup_regions", "walt_pileup_regions_device", "walt_pileup_regions_workspace_bytes")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_regions_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert "} walt_region;" in hdr and "} walt_region_row;" in hdr and "} walt_region_levels;" in hdr
    L.walt_pileup_regions_workspace_bytes.restype = ctypes.c_uint64
    L.walt_pileup_regions_workspace_bytes.argtypes = [ctypes.c_uint32]
    assert L.walt_pileup_regions_workspace_bytes(0) >= 8
    assert 8 * ((1 << 22) + 1) <= L.walt_pileup_regions_workspace_bytes(1 << 22) <= 64 << 20


def test_struct_layout_binding_surface_and_refusals():
    import walt_amd
    reg, row, dt = walt_amd.region_dtype, walt_amd.region_row_dtype, walt_amd.region_levels_dtype
    assert (reg.itemsize, row.itemsize, dt.itemsize) == (8, 32, 160)
    assert [reg.fields[f][1] for f in ("lo", "hi")] == [0, 4]
    assert [row.fields[f][1] for f in ("sites", "covered", "meth", "unmeth", "level_sum")] == [0, 4, 8, 16, 24]
    assert dt.fields["row"][1] == 0 and dt["row"].shape == (5,)
    for nm in ("regions", "regions_device"):
        assert hasattr(walt_amd.Pileup, nm), nm
    assert walt_amd.regions_workspace_bytes(1000) >= 8 * 1001 and walt_amd.REGIONS_MAX == 1 << 22
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm
    # no device: a null pile-up is refused, not crashed on
    regs = np.array([(0, 4)], dtype=np.uint32)
    out = np.zeros(1, dtype=dt)
    assert L.walt_pileup_regions(None, regs.ctypes.data, 1, out.ctypes.data) == walt_amd.WALT_EINVAL
    assert b"walt_pileup_regions" in L.walt_last_error()
    assert L.walt_pileup_regions(None, None, 0, None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_regions_device(None, None, 0, None, None, None) == walt_amd.WALT_EINVAL
    assert b"walt_pileup_regions_device" in L.walt_last_error()
    assert not out.view(np.uint8).any()


def run_cli(args):
    pr = subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    return pr.returncode, pr.stdout


def test_cli_accepts_the_option_in_every_spelling(tmp_path):
    rc, text = run_cli([])
    assert rc == 0 and " -MR <bed> " in text
    bed = tmp_path / "some.bed"
    bed.write_text("chrA\t0\t10\n")
    tail = ["-i", str(tmp_path / "none.dbindex"), "-o", str(tmp_path / "o.mr")]
    for flag in ("-MR", "-regions", "--meth-regions"):
        rc, text = run_cli([flag, str(bed), "-r", "x.fastq"] + tail)
        assert rc != 0 and "index file missing" in text, text  # parsed, the BED read, and the index is looked at next
        assert not (tmp_path / "o.mr.regions").exists()
    rc, text = run_cli(["-r", "x.fastq"] + tail + ["-MR"])
    assert rc != 0 and "missing value" in text
    # the BED file is read first: a bad one is refused with its line before the index is looked at
    bad = tmp_path / "bad.bed"
    bad.write_text("chrA\t0\t10\nchrA\t7\n")
    rc, text = run_cli(["-MR", str(bad), "-r", "x.fastq"] + tail)
    assert rc != 0 and str(bad) + ":2:" in text and "index file missing" not in text, text
    rc, text = run_cli(["-MR", str(tmp_path / "absent.bed"), "-r", "x.fastq"] + tail)
    assert rc != 0 and "absent.bed" in text and "cannot open" in text and "index file missing" not in text, text
    # a methylation consumer: -NO, -I5 3 and -F 3 are accepted with -MR alone and still refused without one
    for opts, reads in ((["-NO"], ["-1", "a.fastq", "-2", "b.fastq"]), (["-I5", "3"], ["-r", "x.fastq"]), (["-F", "3"], ["-r", "x.fastq"])):
        rc, text = run_cli(opts + ["-MR", str(bed)] + reads + tail)
        assert rc != 0 and "index file missing" in text, text
        rc, text = run_cli(opts + reads + tail)
        assert rc != 0 and "nothing for" in text and "-MR" in text and "index file missing" not in text, text


# ---------------------------------------------------------------------------
# regions_core.h, the BED reader and the writer on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(scratch):
    so = os.path.join(scratch, "libregions_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                    os.path.join(refio.HERE, "regions_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci, cp = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p
    L.regions_harness_unit.restype = u32
    L.regions_harness_units.argtypes = [u32, u32, u32]
    L.regions_harness_units.restype = u32
    L.regions_harness_prefix.argtypes = [vp, u32, u32, vp]
    L.regions_harness_prefix.restype = None
    L.regions_harness_region_of_unit.argtypes = [vp, u32, u64]
    L.regions_harness_region_of_unit.restype = u32
    L.regions_harness_region_next.argtypes = [vp, u32, u32, u64]
    L.regions_harness_region_next.restype = u32
    L.regions_harness_unit_range.argtypes = [u32, u32, u32, vp, vp]
    L.regions_harness_unit_range.restype = None
    L.regions_harness_call.argtypes = [vp, u32, vp, u32, vp, vp, vp, u32, u64, vp, vp]
    L.regions_harness_call.restype = None
    L.regions_harness_parse.argtypes = [cp, u32, cp, cp, ci]
    L.regions_harness_resolve.argtypes = [cp, u32, cp, cp, vp, cp, ci]
    L.regions_harness_text.argtypes = [cp, u32, vp, u32, cp, ci]
    return L


def units_of(lo, hi, genome_len):
    return 0 if lo > hi or hi > genome_len else -(-(hi - lo) // U)


def test_units_of_a_region(harness):
    assert harness.regions_harness_unit() == U
    top = 2 ** 32 - 1
    for span in (0, 1, U - 1, U, U + 1, 2 * U + 1, top):
        want = {0: 0, 1: 1, U - 1: 1, U: 1, U + 1: 2, 2 * U + 1: 3, top: 1 << 20}[span]
        assert units_of(0, span, top) == want
        for lo in (0, 1, 77, top - span):
            if lo + span > top:
                continue
            assert harness.regions_harness_units(lo, lo + span, top) == want, (lo, span)
    # not inside the genome: no units (the device form's zero record)
    assert harness.regions_harness_units(5, 4, 100) == 0 and harness.regions_harness_units(0, 101, 100) == 0
    assert harness.regions_harness_units(0, 100, 100) == 1 and harness.regions_harness_units(100, 100, 100) == 0
    # the ranges of a region's units partition it
    for lo, hi in ((3, 3 + 2 * U + 1), (0, U), (top - U - 5, top), (9, 10)):
        at = lo
        for k in range(units_of(lo, hi, top)):
            a, b = ctypes.c_uint64(), ctypes.c_uint64()
            harness.regions_harness_unit_range(lo, hi, k, ctypes.byref(a), ctypes.byref(b))
            assert a.value == at and at < b.value <= min(hi, at + U) and (b.value == hi or b.value - a.value == U)
            at = b.value
        assert at == hi


def region_cases():
    e, one, three = (7, 7), (10, 11), (0, 2 * U + 1)
    yield "all empty", [e, e, e, (0, 0)]
    yield "empty in front, between and behind", [e, e, one, e, three, e, e, e, one, three, e]
    yield "none empty", [one, three, one, one, three]
    yield "one region", [three]
    yield "invalid ones count as empty", [(9, 8), one, (0, 10 ** 6 + 1), three, (9, 8)]
    rng = random.Random(11)
    yield "random", [rng.choice([e, e, one, three, (5, 5 + rng.randrange(0, 6 * U))]) for _ in range(300)]


def test_region_of_a_unit_steps_over_empty_regions(harness):
    genome_len = 10 ** 6
    for what, regs in region_cases():
        arr = np.array(regs, dtype=np.uint32)
        n = len(regs)
        prefix = np.zeros(n + 1, dtype=np.uint64)
        harness.regions_harness_prefix(arr.ctypes.data, n, genome_len, prefix.ctypes.data)
        units = [units_of(lo, hi, genome_len) for lo, hi in regs]
        want_prefix = [sum(units[:i]) for i in range(n + 1)]
        assert prefix.tolist() == want_prefix, what
        owner = [r for r in range(n) for _ in range(units[r])]  # the region of every unit, plainly
        assert len(owner) == want_prefix[n]
        for unit, r in enumerate(owner):
            assert units[r] > 0
            assert harness.regions_harness_region_of_unit(prefix.ctypes.data, n, unit) == r, (what, unit)
            assert bisect.bisect_right(want_prefix, unit) - 1 == r  # the last region whose prefix is not beyond the unit
            for back in {0, 1, 2, 5, unit}:  # from the region of any earlier unit
                if back <= unit:
                    assert harness.regions_harness_region_next(prefix.ctypes.data, n, owner[unit - back], unit) == r, (what, unit, back)


def harness_genome():
    """3 U + 71 bases in chromosomes of 1, 2 and many bases, C / G rich, a CG across the unit boundary of the region
    that starts at 3; counters at 0, small values and 0xFFFFFFFF"""
    rng = random.Random(12)
    lengths = [1, 2, U + 7, 61, 2 * U]
    text = list(rng.choice("ACGTCG") for _ in range(sum(lengths)))
    text[3 + U - 1:3 + U + 1] = "CG"
    text = "".join(text)
    start = np.zeros(len(lengths) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lengths)
    pick = [0, 0, 1, 2, 9, 100, 0xFFFFFFFF]
    meth = np.array([rng.choice(pick) for _ in text], dtype=np.uint32)
    unmeth = np.array([rng.choice(pick) for _ in text], dtype=np.uint32)
    return text, start, meth, unmeth


def test_a_whole_call_on_the_cpu_equals_the_walk(harness):
    import walt_amd
    text, start, meth, unmeth = harness_genome()
    glen = len(text)
    ref = pack_reference(text)
    cls, pair = classes(np.frombuffer(text.encode(), dtype=np.uint8), start)
    assert pair[3 + U - 1]
    regs = [(0, 0), (5, 5), (0, glen), (glen, glen), (3, 3 + U - 1), (3, 3 + U), (7, 7), (3, 3 + U + 1), (100, 100 + 2 * U + 1),
            (0, 3), (0, 1), (1, 3), (2, 4), (3 + U - 1, 3 + U), (3 + U, 3 + U + 1), (9, 8), (0, glen + 1), (60, 200), (60, 200), (glen, glen)]
    arr = np.array(regs, dtype=np.uint32)
    total = sum(units_of(lo, hi, glen) for lo, hi in regs)
    want = [zero_record() if units_of(lo, hi, glen) == 0 else want_record(cls, pair, meth, unmeth, lo, hi) for lo, hi in regs]
    for n_waves in (1, 2, 3, 5, total, total + 3, 8192):
        out = np.zeros(len(regs), dtype=walt_amd.region_levels_dtype)
        taken = np.zeros(total, dtype=np.uint8)
        harness.regions_harness_call(ref.ctypes.data, ref.size - 1, start.ctypes.data, start.size - 1, meth.ctypes.data, unmeth.ctypes.data,
                                     arr.ctypes.data, len(regs), n_waves, out.ctypes.data, taken.ctypes.data)
        assert (taken == 1).all(), n_waves  # every unit walked once, whatever the grid
        for i in range(len(regs)):
            assert rec_rows(out[i]) == want[i], (n_waves, i, regs[i])


def parse(harness, text, file="t.bed"):
    buf = ctypes.create_string_buffer(1 << 16)
    raw = text.encode()
    n = harness.regions_harness_parse(raw, len(raw), file.encode(), buf, 1 << 16)
    assert n >= 0
    return buf.raw[:n].decode()


def resolve(harness, text, names, start, file="t.bed"):
    buf = ctypes.create_string_buffer(1 << 16)
    raw = text.encode()
    st = np.array(start, dtype=np.uint32)
    n = harness.regions_harness_resolve(raw, len(raw), file.encode(), "\n".join(names).encode(), st.ctypes.data, buf, 1 << 16)
    assert n >= 0
    return buf.raw[:n].decode()


def test_bed_reader_accepts(harness):
    text = ("# a comment\n"
            "track name=islands\n"
            "browser position chr1:1-100\n"
            "\n"
            "   \n"
            "chr1\t0\t10\n"
            "chr1 5 5 empty\n"
            "chr2\t7\t900\tisland_1\t960\t-\tmore\n"
            "chr2   8 \t 9   spaced   out\n"
            "tracker\t1\t2\n"
            "chrUn_x\t3\t4\t.\r\n"
            "chr1\t00012\t0013\tzeros\r\n"
            "chr2\t1\t1000")
    assert parse(harness, text) == ("chr1\t0\t10\t.\t6\n" "chr1\t5\t5\tempty\t7\n" "chr2\t7\t900\tisland_1\t8\n" "chr2\t8\t9\tspaced\t9\n"
                                    "tracker\t1\t2\t.\t10\n" "chrUn_x\t3\t4\t.\t11\n" "chr1\t12\t13\tzeros\t12\n" "chr2\t1\t1000\t.\t13\n")
    # against a genome: chr1 [0, 100), chr2 [100, 1100); an unknown chromosome keeps its place as the empty range
    assert resolve(harness, text, ["chr1", "chr2"], [0, 100, 1100]) == (
        "0\t10\n" "5\t5\n" "107\t1000\n" "108\t109\n" "0\t0\n" "0\t0\n" "12\t13\n" "101\t1100\n" "unknown 2\n")
    assert parse(harness, "chr1\t0\t10") == "chr1\t0\t10\t.\t1\n"
    assert parse(harness, "chr1\t0\t10\r\n") == "chr1\t0\t10\t.\t1\n"
    assert resolve(harness, "chr1 100 100\n", ["chr1"], [0, 100]) == "100\t100\nunknown 0\n"  # the end of a chromosome is inside


def test_bed_reader_refuses_with_the_line(harness):
    for text, line, what in (("chr1\t0\t10\nchr1\t5\n", 2, "three columns"),
                             ("chr1\n", 1, "three columns"),
                             ("\n#x\nchr1\tzero\t10\n", 3, "start 'zero' is not a number"),
                             ("chr1\t0\t10\r\nchr1\t5\t1e3\r\n", 2, "end '1e3' is not a number"),
                             ("chr1\t-1\t10\n", 1, "not a number"),
                             ("chr1\t0\t+10\n", 1, "not a number"),
                             ("chr1\t0\t99999999999999999999\n", 1, "not a number"),
                             ("chr1\t0\t10\nchr1\t1\t2\nchr1\t11\t10", 3, "start 11 lies behind end 10"),
                             ("", 0, "no region"),
                             ("# only\ntrack x\n\n", 0, "no region")):
        got = parse(harness, text, "dir/my.bed")
        assert got.startswith("ERR dir/my.bed:%d: " % line) and what in got, (text, got)
    got = resolve(harness, "chr1\t0\t100\nchr2\t0\t1001\n", ["chr1", "chr2"], [0, 100, 1100], "my.bed")
    assert got == "ERR my.bed:2: end 1001 lies beyond the 1000 bases of chr2"
    assert resolve(harness, "chrX\t0\t5000000000\n", ["chr1"], [0, 100]) == "0\t0\nunknown 1\n"  # not looked at: no such chromosome


def test_regions_writer_text(harness):
    import walt_amd
    bed = "chr1\t0\t10\tfirst\nchr1 5 5\nchrNowhere\t1\t9\tlost\nchr2\t7\t900\tbig\t0\t+\n"
    rows = [("chr1", 0, 10, "first"), ("chr1", 5, 5, "."), ("chrNowhere", 1, 9, "lost"), ("chr2", 7, 900, "big")]
    recs = [zero_record() for _ in rows]
    recs[0][0].update(sites=10, covered=4, meth=30, unmeth=10, level_sum=3 << 30)
    recs[0][2].update(sites=5)                      # no site covered: NA for both levels
    recs[0][4].update(sites=5, covered=2, meth=30, unmeth=10, level_sum=(1 << 30) + (1 << 29))
    recs[3][1].update(sites=2 ** 32 - 1, covered=1, meth=0, unmeth=2 ** 33, level_sum=0)
    recs[3][3].update(sites=1, covered=1, meth=2 ** 33 - 2, unmeth=2 ** 33 - 2, level_sum=1 << 29)
    raw = np.zeros(len(rows), dtype=walt_amd.region_levels_dtype)
    for i, rec in enumerate(recs):
        for r in range(5):
            for k, v in rec[r].items():
                raw[i]["row"][r][k] = v
    buf = ctypes.create_string_buffer(1 << 16)
    text = bed.encode()
    n = harness.regions_harness_text(text, len(text), raw.ctypes.data, len(rows), buf, 1 << 16)
    assert n > 0
    got = buf.raw[:n].decode()
    assert got == regions_text(rows, recs)
    lines = got.split("\n")
    assert lines[0] + "\n" == REGIONS_HEADER and len(lines) == 6 and lines[5] == ""
    assert lines[0].split("\t")[:10] == ["chrom", "start", "end", "name", "CpG_sites", "CpG_covered", "CpG_meth", "CpG_unmeth",
                                         "CpG_mean_meth", "CpG_weighted_meth"]
    assert lines[0].split("\t")[-6:] == ["CpG_symmetric_" + c for c in ("sites", "covered", "meth", "unmeth", "mean_meth", "weighted_meth")]
    na = "\t0\t0\t0\t0\tNA\tNA"
    assert lines[1] == ("chr1\t0\t10\tfirst\t10\t4\t30\t10\t0.750000\t0.750000" + na + "\t5\t0\t0\t0\tNA\tNA" + na +
                        "\t5\t2\t30\t10\t0.750000\t0.750000")
    assert lines[2] == "chr1\t5\t5\t." + na * 5 and lines[3] == "chrNowhere\t1\t9\tlost" + na * 5  # all NA
    assert lines[4].startswith("chr2\t7\t900\tbig" + na + "\t4294967295\t1\t0\t8589934592\t0.000000\t0.000000" + na +
                               "\t1\t1\t8589934590\t8589934590\t0.500000\t0.500000")


def test_the_harness_under_the_sanitizers(scratch):
    """tests/regions_harness.cpp as a program of its own (-DREGIONS_HARNESS_MAIN) with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = os.path.join(scratch, "regions_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-DREGIONS_HARNESS_MAIN", "-I", CSRC, os.path.join(refio.HERE, "regions_harness.cpp"), "-o", exe],
                   check=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("positions 12359 regions 16 units 15 bad 0"), run.stdout + run.stderr
