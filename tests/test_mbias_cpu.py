"""Methylation bias by read position (include/walt_amd.h, "methylation bias by read position"), the parts that need no
device: what the bias kernel runs per lane (walt_amd/csrc/mbias_core.h) and the <out>.mbias block writer
(walt_amd/csrc/host/hostio.h), compiled with g++ (tests/mbias_harness.cpp) and compared with the numpy restatement of
tests/test_gpu_mbias.py; the exports of the three libraries, the binding's surface, and bin/walt -MB's parsing."""
import ctypes
import inspect
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_meth import expected_batch, load
from test_gpu_mbias import LETTERS, SHAPE, block_text, expected_table

NAMES = ("walt_mbias_create", "walt_mbias_destroy", "walt_mbias_clear", "walt_mbias_device_bytes", "walt_mbias_read",
         "walt_mbias_batch", "walt_mbias_batch_device", "walt_meth_pileup_batch_mbias", "walt_meth_pileup_batch_mbias_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
LENGTHS = (1, 15, 16, 17, 31, 127, 128, 129, 1024)


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_bias_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert "methylation bias by read position" in hdr


def test_binding_surface_and_refusals_without_a_device():
    import walt_amd
    for nm in ("add", "add_device", "read", "clear", "close"):
        assert hasattr(walt_amd.MBias, nm), nm
    for fn in (walt_amd.Index.meth_call_batch, walt_amd.Index.meth_call_batch_device, walt_amd.Pileup.add_batch,
               walt_amd.Pileup.add_batch_device):
        ps = inspect.signature(fn).parameters
        assert "mbias" in ps and "mbias_table" in ps, fn
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm
    h = ctypes.c_void_p()
    for tables in (0, 9, 1 << 31):  # outside 1..8: refused before any device is asked for
        assert L.walt_mbias_create(0, tables, ctypes.byref(h)) == walt_amd.WALT_EINVAL and not h.value
        assert b"walt_mbias_create" in L.walt_last_error() and b"1 to 8" in L.walt_last_error()
    if walt_amd.device_count() == 0:
        assert L.walt_mbias_create(0, 1, ctypes.byref(h)) == walt_amd.WALT_EHIP and not h.value
        with pytest.raises(walt_amd.WaltError) as ei:
            walt_amd.MBias()
        assert ei.value.code == walt_amd.WALT_EHIP
    one = np.zeros(8192, dtype=np.uint64)
    assert L.walt_mbias_batch(None, 0, None, None, 0, None, 16, None, 1) == walt_amd.WALT_EINVAL
    assert b"walt_mbias_batch" in L.walt_last_error() and b"null bias set" in L.walt_last_error()
    assert L.walt_mbias_batch_device(None, 0, None, None, 0, None, 16, None, 1, None) == walt_amd.WALT_EINVAL
    assert b"walt_mbias_batch_device" in L.walt_last_error()
    assert L.walt_mbias_read(None, 0, one.ctypes.data) == walt_amd.WALT_EINVAL
    assert L.walt_mbias_clear(None) == walt_amd.WALT_EINVAL
    assert L.walt_mbias_device_bytes(None) == 0
    L.walt_mbias_destroy(None)
    assert L.walt_meth_pileup_batch_mbias(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None, 1,
                                          None, None, 0) == walt_amd.WALT_EINVAL
    assert b"walt_meth_pileup_batch_mbias" in L.walt_last_error()
    assert L.walt_meth_pileup_batch_mbias_device(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None,
                                                 None, 1, None, None, 0, None) == walt_amd.WALT_EINVAL
    assert b"walt_meth_pileup_batch_mbias_device" in L.walt_last_error()


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


def test_cli_parses_the_option_in_every_mode(tmp_path):
    pr = run([])
    assert pr.returncode == 0 and " -MB " in pr.stdout
    idx, out = str(tmp_path / "none.dbindex"), str(tmp_path / "o.mr")
    pair = ["-1", "a.fastq", "-2", "b.fastq"]
    # every spelling is known, in every mode and beside every other option: the run gets as far as the index check
    for flag in ("-MB", "-mbias", "--m-bias"):
        for reads, extra in ((["-r", "x.fastq"], []), (["-r", "x.fastq"], ["-A"]), (["-r", "x.fastq"], ["-R", "-M", "-sam"]),
                             (pair, []), (pair, ["-P", "-M"]), (pair, ["-RP", "-MC"]), (pair, ["-NO"]),
                             (pair, ["-M", "-MC", "-sam", "-D", "-NO", "-C", "AGATCGGAAGAGC", "-g", "0,1"])):
            pr = run([flag, "-i", idx, "-o", out] + reads + extra)
            assert pr.returncode != 0 and "index file missing" in pr.stdout, (flag, extra, pr.stdout)
    assert not os.path.exists(out) and not os.path.exists(out + ".mbias")


# ---------------------------------------------------------------------------
# what the kernel runs per lane, on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mbias_harness(scratch):
    so = os.path.join(scratch, "libmbias_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", os.path.join(refio.HERE, "mbias_harness.cpp"),
                    "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.mbias_harness_cell.argtypes = [u32]
    L.mbias_harness_cell.restype = u32
    L.mbias_harness_batch.argtypes = [vp, vp, u32, vp, u64, vp, u64, vp]
    L.mbias_harness_batch.restype = ctypes.c_longlong
    L.mbias_harness_slice.argtypes = [vp, ci, ci, u64, u64, vp]
    L.mbias_harness_slice.restype = None
    L.mbias_harness_block.argtypes = [vp, vp, u64]
    L.mbias_harness_block.restype = ctypes.c_longlong
    return L


def harness_table(L, calls, offsets, times, skip=None, shift=0, rec_stride=16, skip_stride=1):
    """calls (uint8, indexed from offsets[0]) copied to an address that is `shift` modulo 16; records with the given times
    at rec_stride; -> (table, adds)"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    raw = np.full(calls.size + 48, ord("Z"), dtype=np.uint8)  # letters all around the batch: a slice that reads outside shows
    a = (-raw.ctypes.data) % 16 + shift
    raw[a:a + calls.size] = calls
    rec = np.zeros(max(n, 1) * rec_stride, dtype=np.uint8)
    rec.view(np.uint32)[1::rec_stride // 4][:n] = times
    sk = None
    if skip is not None:
        sk = np.full(max(n, 1) * skip_stride, 7, dtype=np.uint8)
        sk[::skip_stride][:n] = skip
    out = np.zeros(SHAPE, dtype=np.uint64)
    adds = L.mbias_harness_batch(raw.ctypes.data + a - int(offsets[0]), offsets.ctypes.data, n, rec.ctypes.data, rec_stride,
                                 None if sk is None else sk.ctypes.data, skip_stride, out.ctypes.data)
    return out, adds


def test_every_byte_value_at_a_position(mbias_harness):
    """only the eight letters count, each into its own (context, m)"""
    want_cell = {b: 2 * c + m for b, (c, m) in LETTERS.items()}
    assert len(want_cell) == 8 and sorted(want_cell.values()) == list(range(8))
    assert [want_cell[ord(ch)] for ch in "ZzXxHhUu"] == list(range(8))
    for b in range(256):
        assert mbias_harness.mbias_harness_cell(b) == want_cell.get(b, 8), b
    # ... and through the slices: a read of 256 calls holding every byte value once, at every alignment
    calls = np.arange(256, dtype=np.uint8)
    offsets = np.array([0, 256], dtype=np.uint64)
    want = expected_table(calls, offsets, [1])
    assert int(want.sum()) == 8 and all(want[c, m, b] == 1 for b, (c, m) in LETTERS.items())
    for shift in range(16):
        got, adds = harness_table(mbias_harness, calls, offsets, [1], shift=shift)
        assert adds == 8 and np.array_equal(got, want), shift


def random_calls(rng, n, dense=False):
    al = "zZxXhHuU" if dense else "zZxXhHuU" + "." * 24 + "ACGT#-"
    return np.frombuffer("".join(rng.choice(al) for _ in range(n)).encode(), dtype=np.uint8)


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_at_every_address_modulo_16(mbias_harness, length):
    """one read, and the same read between two others, with the calls array at every address modulo 16 and the read at
    every offset modulo 16: the partial first and last slice are right whether the address or the position cuts them"""
    rng = random.Random(1000 + length)
    for trial in range(3):
        body = random_calls(rng, length, dense=trial == 0)
        for lead in (0, 1, 5, 15, 16, 29):
            calls = np.concatenate([random_calls(rng, lead, True), body, random_calls(rng, 19, True)])
            offsets = np.array([0, lead, lead + length, lead + length + 19], dtype=np.uint64)
            for shift in range(16):
                for times in ([0, 1, 2], [1, 1, 1]):
                    want = expected_table(calls, offsets, times)
                    got, adds = harness_table(mbias_harness, calls, offsets, times, shift=shift)
                    assert adds == int(want.sum()) and np.array_equal(got, want), (length, lead, shift, times)
    # the loaded slice itself: 0 outside the read, the read's bytes inside -- alone in its batch (the partial slices go
    # byte by byte), with the batch's bytes all around it (one aligned load, masked), and with 3 bytes on either side
    body = random_calls(rng, length, True)
    raw = np.full(length + 64, ord("Z"), dtype=np.uint8)
    for shift in range(16):
        a = (-raw.ctypes.data) % 16 + shift + 16
        raw[:] = ord("Z")
        raw[a:a + length] = body
        for i0 in range(-shift, length, 16):
            want = [int(body[i]) if 0 <= i < length else 0 for i in range(i0, i0 + 16)]
            for before, after in ((0, length), (16, length + 16), (3, length + 3), (0, length + 16), (16, length)):
                out = np.full(16, 0x55, dtype=np.uint8)
                mbias_harness.mbias_harness_slice(raw.ctypes.data + a, length, i0, before, after, out.ctypes.data)
                assert out.tolist() == want, (length, shift, i0, before, after)


def test_records_skip_bytes_strides_and_long_reads(mbias_harness):
    rng = random.Random(77)
    lens = [40, 1025, 100, 0, 1024, 2000, 7, 33]
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    calls = random_calls(rng, int(offsets[-1]), dense=True)
    for times, skip in (([1] * 8, None), ([1, 1, 0, 1, 2, 1, 1, 3], None), ([1] * 8, [0, 0, 1, 0, 0, 0, 255, 0]),
                        ([1, 1, 1, 1, 1, 1, 0, 1], [1, 0, 0, 0, 0, 0, 0, 0])):
        want = expected_table(calls, offsets, times, skip)
        for rec_stride, skip_stride in ((16, 1), (64, 2), (20, 5)):
            got, adds = harness_table(mbias_harness, calls, offsets, times, skip, shift=3, rec_stride=rec_stride, skip_stride=skip_stride)
            assert adds == int(want.sum()) and np.array_equal(got, want), (times, skip, rec_stride)
    # the reads of 1025 and 2000 calls added nothing, their neighbours everything
    want = expected_table(calls, offsets, [1] * 8)
    assert int(want.sum()) == 40 + 100 + 1024 + 7 + 33 and want[:, :, 1023].sum() == 1
    # offsets that do not start at 0
    shifted = offsets + np.uint64(1000)
    got, _ = harness_table(mbias_harness, calls, shifted, [1] * 8)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("files", [("pe_1.fastq", "pe_2.fastq"), ("pe150_1.fastq", "pe150_2.fastq")])
def test_golden_libraries_column_sums_equal_the_totals(g1_db, mbias_harness, files):
    """the calls of the restatement of the calling (tests/test_gpu_meth.py expected_batch) on the oracle's records, both
    mates, records at the stride of a walt_pair_result: the table's column sums are that restatement's totals"""
    for k, (name, conv, mate) in enumerate(zip(files, "TA", ("m1", "m2"))):
        _, seqs, _ = load(name)
        if k == 0:
            _, s2, _ = load(files[1])
            res, _, _ = refio.oracle_pe(g1_db, seqs, s2)
        recs = res[mate]
        wcalls, _, tot = expected_batch(g1_db, seqs, recs, conv)
        calls = np.frombuffer("".join(wcalls).encode(), dtype=np.uint8)
        offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(s) for s in seqs])
        times = recs["times"].astype(np.uint32)
        got, adds = harness_table(mbias_harness, calls, offsets, times, shift=5 + k, rec_stride=64)
        assert np.array_equal(got, expected_table(calls, offsets, times))
        assert np.array_equal(got[:, 0, :].sum(axis=1).astype(np.int64), tot["meth"]), (name, got[:, 0, :].sum(axis=1), tot)
        assert np.array_equal(got[:, 1, :].sum(axis=1).astype(np.int64), tot["unmeth"]), (name, got[:, 1, :].sum(axis=1), tot)
        assert adds == int(tot["meth"].sum() + tot["unmeth"].sum()) > 1000
        longest = max(len(s) for s in seqs)
        assert got[:, :, longest:].sum() == 0 and got[:, :, :36].any(axis=(0, 1)).all()


# ---------------------------------------------------------------------------
# the <out>.mbias block writer
# ---------------------------------------------------------------------------
def harness_block(L, table):
    table = np.ascontiguousarray(table, dtype=np.uint64)
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.mbias_harness_block(table.ctypes.data, buf, len(buf))
    assert n >= 0
    return buf.raw[:n].decode()


def test_block_writer(mbias_harness):
    empty = np.zeros(SHAPE, dtype=np.uint64)
    assert harness_block(mbias_harness, empty) == "" == block_text(empty)  # L = 0: no line
    last = empty.copy()
    last[3, 1, 1023] = 1  # the only count at position 1024: every context has 1024 lines, all but one NA
    text = harness_block(mbias_harness, last)
    assert text == block_text(last)
    lines = text.splitlines()
    assert len(lines) == 4 * 1024 and lines[0] == "CpG\t1\t0\t0\tNA" and lines[-1] == "unknown\t1024\t0\t1\t0.000000"
    assert sum(l.endswith("\tNA") for l in lines) == 4 * 1024 - 1
    big = empty.copy()
    big[0, 0, 0] = (1 << 32) + 5  # above 2^32
    big[0, 1, 0] = 3
    big[2, 1, 2] = (1 << 40)
    big[1, 0, 1] = 1
    big[1, 1, 1] = 2
    text = harness_block(mbias_harness, big)
    assert text == block_text(big)
    lines = text.splitlines()
    assert len(lines) == 12 and lines[0] == "CpG\t1\t4294967301\t3\t%.6f" % (4294967301 / 4294967304)
    assert lines[4] == "CHG\t2\t1\t2\t0.333333" and lines[8] == "CHH\t3\t0\t1099511627776\t0.000000" and lines[9] == "unknown\t1\t0\t0\tNA"
    rng = np.random.default_rng(3)
    rnd = empty.copy()
    rnd[:, :, :151] = rng.integers(0, 50, size=(4, 2, 151))
    rnd[:, :, 150] = 0
    rnd[1, 0, 150] = 9
    assert harness_block(mbias_harness, rnd) == block_text(rnd)



def test_per_lane_logic_under_the_host_sanitizers(scratch):
    """tests/mbias_sanitize_main.cpp, a stand-alone program over tests/mbias_harness.cpp built with the host's address and
    undefined-behaviour sanitizers: random batches, each in a heap block that begins with the batch's first call and ends
    with its last, at every alignment -- a load outside the batch's own bytes ends the program"""
    exe = os.path.join(scratch, "mbias_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(refio.HERE, "mbias_sanitize_main.cpp"), os.path.join(refio.HERE, "mbias_harness.cpp"), "-o", exe],
                   check=True, timeout=300)
    pr = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert pr.returncode == 0 and pr.stdout.startswith("ok "), pr.stdout[-2000:]
