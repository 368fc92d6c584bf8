"""Per-cytosine methylation pile-up (include/walt_amd.h, "methylation pile-up"), the parts that need no device: the
three libraries export the calls, the binding's struct layout and surface, null arguments, bin/walt -MC, and what the
kernels run per lane (walt_amd/csrc/pileup_core.h on top of meth_core.h) compiled with g++ (tests/pileup_harness.cpp)
and compared with the plain restatement of the contract in tests/test_gpu_pileup.py on random genomes."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_pileup import expected_counts, site_class
from test_meth_cpu import pack_reference

NAMES = ("walt_pileup_create", "walt_pileup_destroy", "walt_pileup_clear", "walt_pileup_device_bytes",
         "walt_meth_pileup_batch", "walt_meth_pileup_batch_device", "walt_pileup_extract", "walt_pileup_extract_device")


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_pileup_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert nm + "(" in hdr
    assert "} walt_meth_site;" in hdr and "typedef struct walt_pileup walt_pileup;" in hdr


def test_struct_layout_and_binding_surface():
    import walt_amd
    dt = walt_amd.meth_site_dtype
    assert dt.itemsize == 16
    assert [dt.fields[f][1] for f in ("pos", "meth", "unmeth", "strand", "context", "reserved")] == [0, 4, 8, 12, 13, 14]
    assert hasattr(walt_amd.Index, "pileup")
    for nm in ("add_batch", "add_batch_device", "extract", "extract_device", "clear", "device_bytes", "close"):
        assert hasattr(walt_amd.Pileup, nm), nm
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm
    # no device: null handles are refused, not crashed on
    out = ctypes.c_void_p()
    n = ctypes.c_uint64(7)
    assert L.walt_pileup_create(None, ctypes.byref(out)) == walt_amd.WALT_EINVAL and not out.value
    assert L.walt_pileup_create(None, None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_clear(None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_device_bytes(None) == 0
    L.walt_pileup_destroy(None)
    assert L.walt_pileup_extract(None, 0, 0, None, 0, ctypes.byref(n), None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_extract_device(None, 0, 0, None, 0, None, None, None) == walt_amd.WALT_EINVAL
    assert L.walt_meth_pileup_batch(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None) == walt_amd.WALT_EINVAL
    assert L.walt_meth_pileup_batch_device(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None,
                                           None) == walt_amd.WALT_EINVAL
    assert b"walt_meth_pileup_batch_device" in L.walt_last_error()


def test_cli_lists_the_option_and_checks_the_index_first(tmp_path):
    walt = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
    pr = subprocess.run([walt], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert pr.returncode == 0 and " -MC " in pr.stdout
    for flag in ("-MC", "-methcounts", "--meth-counts"):
        pr = subprocess.run([walt, flag, "-i", str(tmp_path / "none.dbindex"), "-r", "x.fastq", "-o", str(tmp_path / "o.mr")],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert pr.returncode != 0 and "index file missing" in pr.stdout, pr.stdout
        assert not (tmp_path / "o.mr.methcounts").exists()


# ---------------------------------------------------------------------------
# what the kernels run per lane, on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pileup_harness(scratch):
    so = os.path.join(scratch, "libpileup_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", os.path.join(refio.ROOT, "walt_amd", "csrc"),
                    os.path.join(refio.HERE, "pileup_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.pileup_harness_read.argtypes = [vp, u32, vp, u32, u64, u64, u64, u32, ci, u32, u32, u32, u32, ci, vp, vp]
    L.pileup_harness_read.restype = None
    L.pileup_harness_site.argtypes = [vp, u32, u32, u32, u32, vp, vp]
    return L


def random_genome(rng):
    """several chromosomes, among them ones of 1, 2 and 17 bases; C / G rich so that every context occurs often"""
    lengths = [rng.randrange(200, 2500), 50, 2, rng.randrange(1100, 3000), 1, 17, rng.randrange(64, 400), 1]
    text = "".join(rng.choice("ACGTCG") for _ in range(sum(lengths)))
    start = np.zeros(len(lengths) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lengths)
    # the '-' genome: every chromosome reverse-complemented in place
    minus = "".join(refio.revcomp(text[int(start[c]):int(start[c + 1])]) for c in range(len(lengths)))
    return lengths, text, minus, start


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_slice_adds_equal_the_restatement(pileup_harness, seed):
    rng = random.Random(seed)
    lengths, text, minus, start = random_genome(rng)
    R = [np.frombuffer(text.encode(), dtype=np.uint8), np.frombuffer(minus.encode(), dtype=np.uint8)]
    refs = [pack_reference(text), pack_reference(minus)]
    glen = len(text)
    got_m, got_u = np.zeros(glen, dtype=np.uint32), np.zeros(glen, dtype=np.uint32)
    want = None
    combos, heads, cut, over = set(), set(), 0, 0
    for trial in range(2500):
        conv = rng.choice("TA")
        strand = rng.choice([b"+", b"-"])
        G = text if strand == b"+" else minus
        c = rng.randrange(len(lengths))
        lo, hi = int(start[c]), int(start[c + 1])
        pos = rng.choice([lo, lo + 1, lo + 2, hi - 1, max(lo, hi - 2), max(lo, hi - 17), rng.randrange(lo, hi)])
        pos = min(max(pos, lo), hi - 1)
        n = rng.choice([1, 2, 15, 16, 17, 31, 33, 100, 101, rng.randrange(1, 300), 1023, 1024])
        if rng.random() < 0.5:
            n = min(n, hi - pos + rng.choice([0, 0, 3]))  # up to, or three bases over, the chromosome's end
        n = max(1, n)
        over += pos + n > hi
        seq = []
        for i in range(n):
            g = G[pos + i] if pos + i < glen else "A"
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
        cut += limit < n
        off = rng.choice([0, 0, 1, 5, rng.randrange(0, 40)])
        batch_bytes = off + n + rng.choice([0, 0, 1, 7, 64])
        head = trial % 16  # every alignment of the slice grid
        bases = np.full(1200 + 128, ord("C"), dtype=np.uint8)
        bases[off:off + n] = np.frombuffer(seq.encode(), dtype=np.uint8)
        bases[batch_bytes:] = 0
        o = 1 if strand == b"-" else 0
        pileup_harness.pileup_harness_read(refs[o].ctypes.data, refs[o].size - 1, bases.ctypes.data, head, off, n, batch_bytes, limit,
                                           1 if limit else 0, pos, lo, hi, 1 if conv == "A" else 0, o, got_m.ctypes.data,
                                           got_u.ctypes.data)
        recs = np.zeros(1, dtype=[("genome_pos", "<u4"), ("times", "<u4"), ("strand", "S1")])
        recs["genome_pos"], recs["times"], recs["strand"] = pos, 1, strand
        # (the restatement asserts that every letter's context is its site's, and its strand the site's)
        want = expected_counts(R, start, [seq], recs, conv, None if call_len is None else [call_len], into=want)
        assert np.array_equal(got_m, want[0]) and np.array_equal(got_u, want[1]), (
            "trial %d conv %s strand %s pos %d [%d, %d) n %d off %d head %d" % (trial, conv, strand, pos, lo, hi, n, off, head))
        combos.add((strand, conv))
        heads.add(head)
    assert len(combos) == 4 and len(heads) == 16 and cut > 100 and over > 100
    assert int(want[0].sum()) > 5000 and int(want[1].sum()) > 5000


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_site_classifier_at_every_position(pileup_harness, seed):
    rng = random.Random(100 + seed)
    lengths, text, minus, start = random_genome(rng)
    R0 = np.frombuffer(text.encode(), dtype=np.uint8)
    ref = pack_reference(text)
    seen = set()
    for c in range(len(lengths)):
        lo, hi = int(start[c]), int(start[c + 1])
        for f in range(lo, hi):
            strand, ctx = ctypes.c_uint8(0), ctypes.c_uint8(0)
            rc = pileup_harness.pileup_harness_site(ref.ctypes.data, ref.size - 1, f, lo, hi, ctypes.byref(strand), ctypes.byref(ctx))
            want = site_class(R0, start, f)
            got = (chr(strand.value), ctx.value) if rc else None
            assert got == want, (f, lo, hi, text[max(lo, f - 2):f + 3], got, want)
            seen.add(want)
    assert {None} | {(s, k) for s in "+-" for k in range(4)} <= seen
