"""Methylation calls (include/walt_amd.h, "methylation calls"), the parts that need no device: the three libraries
export the calls, the binding's struct layouts, bin/walt -M, and the per-slice classification of
walt_amd/csrc/meth_core.h -- the functions the HIP kernel runs per lane -- compiled with g++ (tests/meth_harness.cpp)
and compared with the plain restatement of the contract in tests/test_gpu_meth.py on random genomes."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_meth import expected_read

NAMES = ("walt_index_enable_reference", "walt_index_has_reference", "walt_meth_call_batch", "walt_meth_call_batch_device")


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_meth_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert nm + "(" in hdr
    assert "#define WALT_WITH_REFERENCE 16u" in hdr


def test_struct_sizes_and_binding_surface():
    import walt_amd
    assert walt_amd.meth_counts_dtype.itemsize == 16 and walt_amd.meth_stats_dtype.itemsize == 72
    assert walt_amd.meth_counts_dtype.fields["unmeth"][1] == 8
    assert walt_amd.meth_stats_dtype.fields["meth"][1] == 8 and walt_amd.meth_stats_dtype.fields["unmeth"][1] == 40
    assert walt_amd.WITH_REFERENCE == 16
    for nm in ("has_reference", "enable_reference", "meth_call_batch", "meth_call_batch_device"):
        assert hasattr(walt_amd.Index, nm), nm
    # no device: has_reference of no index is 0, and the calls refuse a null index instead of crashing
    L = walt_amd.lib()
    assert L.walt_index_has_reference(None) == 0
    assert L.walt_index_enable_reference(None) == walt_amd.WALT_EINVAL
    assert L.walt_meth_call_batch(None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None) == walt_amd.WALT_EINVAL


def test_cli_lists_the_option_and_checks_the_index_first(tmp_path):
    walt = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
    pr = subprocess.run([walt], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert pr.returncode == 0 and " -M " in pr.stdout
    for flag in ("-M", "-meth", "--meth-calls"):
        pr = subprocess.run([walt, flag, "-i", str(tmp_path / "none.dbindex"), "-r", "x.fastq", "-o", str(tmp_path / "o.mr")],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert pr.returncode != 0 and "index file missing" in pr.stdout, pr.stdout
    assert not (tmp_path / "o.mr.methstats").exists()


# ---------------------------------------------------------------------------
# the per-slice classification on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meth_harness(scratch):
    so = os.path.join(scratch, "libmeth_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", os.path.join(refio.ROOT, "walt_amd", "csrc"),
                    os.path.join(refio.HERE, "meth_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.meth_harness_read.argtypes = [vp, u32, vp, vp, u64, u64, u64, u32, ctypes.c_int, u32, u32, u32, u32, vp]
    L.meth_harness_read.restype = None
    return L


CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def pack_reference(text, pad_words=16):
    codes = np.array([CODE[c] for c in text], dtype=np.uint32)
    nwords = (len(text) + 15) // 16
    full = np.zeros(nwords * 16, dtype=np.uint32)
    full[:codes.size] = codes
    words = (full.reshape(nwords, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([words, np.zeros(pad_words, dtype=np.uint32)])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_slice_classification_equals_the_restatement(meth_harness, seed):
    rng = random.Random(seed)
    # several chromosomes, one shorter than 64 bases, one of 1 base; C / G rich so that every context occurs often
    lengths = [rng.randrange(200, 2500), 50, rng.randrange(1100, 3000), 1, 17, rng.randrange(64, 400)]
    text = "".join(rng.choice("ACGTCG") for _ in range(sum(lengths)))
    start = np.zeros(len(lengths) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lengths)
    R = np.frombuffer(text.encode(), dtype=np.uint8)
    ref = pack_reference(text)
    seen = set()
    buf_len = 1200
    for trial in range(1500):
        conv = rng.choice("TA")
        c = rng.randrange(len(lengths))
        lo, hi = int(start[c]), int(start[c + 1])
        # positions near both chromosome ends as often as in the middle; reads may run over the chromosome's end
        pos = rng.choice([lo, lo + 1, lo + 2, hi - 1, max(lo, hi - 2), max(lo, hi - 17), rng.randrange(lo, hi)])
        pos = min(max(pos, lo), hi - 1)
        n = rng.choice([1, 2, 15, 16, 17, 31, 33, 100, 101, rng.randrange(1, 300), 1023, 1024])
        if rng.random() < 0.5:
            n = min(n, hi - pos + rng.choice([0, 0, 3]))
        n = max(1, n)
        seq = []
        for i in range(n):  # the reference with conversions, a few mismatches
            g = text[pos + i] if pos + i < len(text) else "A"
            if conv == "T" and g == "C" and rng.random() < 0.5:
                g = "T"
            if conv == "A" and g == "G" and rng.random() < 0.5:
                g = "A"
            if rng.random() < 0.05:
                g = rng.choice("ACGT")
            seq.append(g)
        seq = "".join(seq)
        call_len = rng.choice([None, None, 0, n // 2, n, n + 5])
        limit = n if call_len is None else min(n, call_len)
        off = rng.choice([0, 0, 1, 5, rng.randrange(0, 40)])
        # the batch ends right behind the read, or further on: whole 16-byte loads stay inside [0, batch_bytes)
        batch_bytes = off + n + rng.choice([0, 0, 1, 7, 64])
        shift = rng.randrange(0, 16)  # alignment of the calls buffer
        bases = np.full(buf_len + 128, ord("C"), dtype=np.uint8)
        bases[off:off + n] = np.frombuffer(seq.encode(), dtype=np.uint8)
        bases[batch_bytes:] = 0  # nothing behind the batch may matter
        raw = np.full(buf_len + 96, 0x23, dtype=np.uint8)
        base_addr = raw.ctypes.data
        a16 = (-base_addr) % 16 + shift
        counts = np.zeros(8, dtype=np.uint16)
        meth_harness.meth_harness_read(ref.ctypes.data, ref.size - 1, bases.ctypes.data, base_addr + a16, off, n, batch_bytes, limit,
                                       1 if limit else 0, pos, lo, hi, 1 if conv == "A" else 0, counts.ctypes.data)
        want, wcounts = expected_read([R, R], start, seq, pos, 1, b"+", conv, call_len)
        got = raw[a16 + off:a16 + off + n].tobytes().decode()
        assert got == want, "trial %d conv %s pos %d [%d, %d) n %d off %d shift %d\n got  %s\n want %s" % (
            trial, conv, pos, lo, hi, n, off, shift, got, want)
        assert counts.tolist() == wcounts, (trial, counts, wcounts)
        assert (raw[:a16 + off] == 0x23).all() and (raw[a16 + off + n:] == 0x23).all(), "wrote outside the read"
        seen |= set(want)
    assert set("zZxXhHuU.") <= seen
