"""The dense verifiers' mismatch count with the read aligned to the record grid once (walt_amd/csrc/core.h align_read,
count_mismatch_aligned, aligned_header_word) against the count that shifts every window word (count_mismatch_regs),
compiled with g++ for the seed patterns 3, 5 and 7 (tests/align_harness.cpp: kWinLead 2, 4, 6) -- no device; and the
same harness as a stand-alone program under the host's sanitizers (tests/align_sanitize_main.cpp).

A read of seed shift seed_i meets a record sh / 2 = kWinLead - seed_i bases in.  A window is the NW + 1 record words;
the read's words rd[NW] hold base k at bits 2 k, 2 k + 1, the mask bit 2 k.  Lengths 16 NW - kWinLead - 3 .. 16 NW: on
either side of the length from which the last base falls into word NW, at every shift."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import refio

CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")
PATTERNS = [3, 5, 7]
NWS = [7, 8]


@pytest.fixture(scope="module", params=PATTERNS)
def harness(request, scratch):
    pat = request.param
    so = os.path.join(scratch, "libalign_harness_sp%d.so" % pat)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                    "-DWALT_SEEDPATTERN=%d" % pat, "-I", CSRC, os.path.join(refio.HERE, "align_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name in ("pat", "lead", "max_len1"):
        getattr(L, "align_harness_" + name).restype = u32
    L.align_harness_tail_mask.argtypes = [u32, u32, u32]
    L.align_harness_tail_mask.restype = u32
    L.align_harness_regs.argtypes = [u32, vp, u32, vp, vp]
    L.align_harness_regs.restype = u32
    L.align_harness_aligned.argtypes = [u32, vp, u32, vp, vp, vp, vp, vp]
    L.align_harness_aligned.restype = u32
    L.align_harness_count.argtypes = [u32, vp, vp, vp, u32]
    L.align_harness_count.restype = u32
    L.align_harness_header.argtypes = [u32, vp, u32, vp]
    L.align_harness_header.restype = None
    assert L.align_harness_pat() == pat and L.align_harness_lead() == pat - 1
    assert L.align_harness_max_len1() == 112 - (pat - 1)
    return L


def words(value, n):
    return np.array([(value >> (32 * w)) & 0xFFFFFFFF for w in range(n)], dtype=np.uint32)


def both(L, nw, g, sh, rd, mk):
    """-> (count_mismatch_regs, count_mismatch_aligned, top, rd_a, mk_a); nothing is written behind the arrays' words"""
    rd_a = np.full(nw + 2, 0xDEADBEEF, dtype=np.uint32)
    mk_a = np.full(nw + 2, 0xDEADBEEF, dtype=np.uint32)
    top = ctypes.c_uint32(7)
    old = L.align_harness_regs(nw, g.ctypes.data, sh, rd.ctypes.data, mk.ctypes.data)
    new = L.align_harness_aligned(nw, g.ctypes.data, sh, rd.ctypes.data, mk.ctypes.data, rd_a.ctypes.data, mk_a.ctypes.data, ctypes.byref(top))
    assert rd_a[nw + 1] == 0xDEADBEEF and mk_a[nw + 1] == 0xDEADBEEF and top.value in (0, 1)
    return old, new, top.value, rd_a[:nw + 1], mk_a[:nw + 1]


def cases(L, nw):
    lead = L.align_harness_lead()
    for seed_i in range(L.align_harness_pat()):
        for length in range(16 * nw - lead - 3, 16 * nw + 1):
            yield seed_i, length, 2 * (lead - seed_i)


def all_bases(L, nw, length):
    return np.array([L.align_harness_tail_mask(w, 0, length) for w in range(nw)], dtype=np.uint32)


def read_of(rng, length):
    return rng.getrandbits(2 * length)  # (the bits beyond the read's last base are zero, as pack_read leaves them)


@pytest.mark.parametrize("nw", NWS)
def test_equal_on_random_windows_reads_and_masks(harness, nw):
    rng = random.Random(100 * harness.align_harness_pat() + nw)
    seen = set()
    for seed_i, length, sh in cases(harness, nw):
        for trial in range(24):
            g = words(rng.getrandbits(32 * (nw + 1)), nw + 1)
            rd = words(read_of(rng, length) if trial % 2 else rng.getrandbits(32 * nw), nw)  # (also reads with bits beyond their length)
            if trial % 3 == 0:
                mk = all_bases(harness, nw, length)
            else:  # some of the bases, the last one among them (every mask source ends with the tail [.., length))
                m = sum(1 << (2 * k) for k in range(length) if rng.random() < 0.6 or k == length - 1)
                mk = words(m, nw)
            old, new, top, rd_a, mk_a = both(harness, nw, g, sh, rd, mk)
            assert old == new, "nw %d seed_i %d length %d: %d from count_mismatch_regs, %d aligned" % (nw, seed_i, length, old, new)
            assert (int(rd_a[0]) | int(mk_a[0])) & ((1 << sh) - 1) == 0  # the low bits are zero-filled
            seen.add(old)
    assert len(seen) > 20  # (the counts vary: random windows differ from the reads in three bases of four)


@pytest.mark.parametrize("nw", NWS)
def test_one_differing_base_counts_once(harness, nw):
    rng = random.Random(200 * harness.align_harness_pat() + nw)
    for seed_i, length, sh in cases(harness, nw):
        read = read_of(rng, length)
        rd, mk = words(read, nw), all_bases(harness, nw, length)
        # the window that holds the read sh / 2 bases in, anything in front of it and behind it
        frame = rng.getrandbits(sh) | (read << sh) | (rng.getrandbits(32 * (nw + 1)) >> (sh + 2 * length) << (sh + 2 * length))
        old, new, top, _, _ = both(harness, nw, words(frame, nw + 1), sh, rd, mk)
        assert (old, new) == (0, 0)
        for j in range(length):
            g = words(frame ^ (rng.choice([1, 2, 3]) << (sh + 2 * j)), nw + 1)
            old, new, top, _, _ = both(harness, nw, g, sh, rd, mk)
            assert (old, new) == (1, 1), "nw %d seed_i %d length %d base %d: %d, %d" % (nw, seed_i, length, j, old, new)


@pytest.mark.parametrize("nw", NWS)
def test_top_word_is_compared_exactly_when_the_read_reaches_it(harness, nw):
    rng = random.Random(300 * harness.align_harness_pat() + nw)
    lead = harness.align_harness_lead()
    tops = set()
    for seed_i, length, sh in cases(harness, nw):
        read = read_of(rng, length)
        rd, mk = words(read, nw), all_bases(harness, nw, length)
        frame = (read << sh) ^ (1 << (sh + 2 * (length - 1)))  # differs in the read's LAST base alone
        g = words(frame, nw + 1)
        old, new, top, rd_a, mk_a = both(harness, nw, g, sh, rd, mk)
        reaches = length + lead - seed_i > 16 * nw
        assert top == (1 if reaches else 0), "nw %d seed_i %d length %d: top %d" % (nw, seed_i, length, top)
        assert (old, new) == (1, 1)
        # a count that leaves the top word out misses that base exactly there
        cut = harness.align_harness_count(nw, g.ctypes.data, rd_a.ctypes.data, mk_a.ctypes.data, 0)
        assert cut == (0 if reaches else 1)
        tops.add((reaches, top))
    assert tops == {(False, 0), (True, 1)}
    # the 7-word records end where the longest read they take ends: no read routed to them has a top word
    if nw == 7:
        for seed_i in range(harness.align_harness_pat()):
            length = harness.align_harness_max_len1()
            _, _, top, _, _ = both(harness, 7, words(0, 8), 2 * (lead - seed_i), words(read_of(rng, length), 7), all_bases(harness, 7, length))
            assert top == 0


@pytest.mark.parametrize("nw", NWS)
def test_header_lanes_aligned_in_place(harness, nw):
    """aligned_header_word over the 32 words of one read's lanes: the first eight stay, rd_a / mk_a stand where rd / mk
    stood, the two top words behind them, everything else stays"""
    rng = random.Random(400 * harness.align_harness_pat() + nw)
    for seed_i, length, sh in cases(harness, nw):
        rd = words(read_of(rng, length), nw)
        mk = all_bases(harness, nw, length)
        hdr = np.array([rng.getrandbits(32) for _ in range(32)], dtype=np.uint32)
        hdr[8:8 + nw], hdr[8 + nw:8 + 2 * nw] = rd, mk
        out = np.zeros(33, dtype=np.uint32)
        out[32] = 0xDEADBEEF
        harness.align_harness_header(nw, hdr.ctypes.data, sh, out.ctypes.data)
        _, _, _, rd_a, mk_a = both(harness, nw, words(0, nw + 1), sh, rd, mk)
        assert out[32] == 0xDEADBEEF and np.array_equal(out[:8], hdr[:8])
        assert np.array_equal(out[8:8 + nw], rd_a[:nw]) and np.array_equal(out[8 + nw:8 + 2 * nw], mk_a[:nw])
        assert out[8 + 2 * nw] == rd_a[nw] and out[8 + 2 * nw + 1] == mk_a[nw]
        assert np.array_equal(out[8 + 2 * nw + 2:32], hdr[8 + 2 * nw + 2:])


@pytest.mark.parametrize("pat", PATTERNS)
def test_the_harness_under_the_sanitizers(scratch, pat):
    """tests/align_sanitize_main.cpp: the same harness as a program of its own with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = os.path.join(scratch, "align_sanitize_sp%d" % pat)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                    "-DWALT_SEEDPATTERN=%d" % pat, "-I", CSRC, os.path.join(refio.HERE, "align_sanitize_main.cpp"),
                    os.path.join(refio.HERE, "align_harness.cpp"), "-o", exe], check=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr
