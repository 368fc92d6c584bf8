"""What the four host-buffer mapping calls do with a caller's offsets array before anything reaches the device
(walt_amd/csrc/batch_host.h: scan_offsets, rebase_offsets), compiled with g++ (tests/batch_host_harness.cpp): the
refusals (a decreasing pair, a read above 1024 bases) with their messages, the running maximum over one or two read
sets, and the offsets relative to the first read.  The harness is built twice, plain and with
-fsanitize=address,undefined, and keeps every offsets array in a heap block of exactly n + 1 words, so the second build
also pins that nothing beyond offsets[n] is read.

The same header holds what the host forms of the methylation-side calls share (meth.hip, mbias.hip, dedup.hip): a strided
array packed into a dense one, the stride and conversion refusals, and the per-read checks of the calling call in the
order a caller sees them.  The harness drives those from its command line, under both builds."""
import os
import subprocess

import numpy as np
import pytest

import refio

DECREASING = "offsets not non-decreasing"
TOO_LONG = "read length above 1024 is not supported"


@pytest.fixture(scope="module", params=["plain", "sanitised"])
def batch_host(request, scratch):
    exe = os.path.join(scratch, "batch_host_harness_" + request.param)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] if request.param == "sanitised" else []
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I", os.path.join(refio.ROOT, "walt_amd", "csrc"),
                    os.path.join(refio.HERE, "batch_host_harness.cpp"), "-o", exe], check=True, timeout=300)
    if request.param == "sanitised":
        assert b"__asan_report_load8" in open(exe, "rb").read(), "the sanitised build carries no address checks"
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    serial = [0]

    def run(*sets):
        """one call's read sets (offset lists) -> per set (message or None, running max_len, own array back, rebased offsets)"""
        serial[0] += 1
        fin, fout = (os.path.join(scratch, "batch_host_%s_%d.%s" % (request.param, serial[0], x)) for x in ("in", "out"))
        with open(fin, "wb") as f:
            f.write(np.array([len(sets)], dtype="<u8").tobytes())
            for offsets in sets:
                f.write(np.array([len(offsets) - 1] + list(offsets), dtype="<u8").tobytes())
        pr = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
        assert pr.returncode == 0, "batch_host_harness (%s) exit %d:\n%s" % (request.param, pr.returncode, pr.stdout[-4000:])
        res = []
        for line in open(fout).read().splitlines():
            f = line.split("\t")
            if f[0] == "ok":
                res.append((None, int(f[1]), f[2] == "1", [int(x) for x in f[3].split()]))
            else:
                res.append((f[0], int(f[1]), None, None))
        os.remove(fin)
        os.remove(fout)
        return res

    def piece(*args):
        """the harness's command-line modes (pack, refuse, reads) -> the line it printed"""
        pr = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
        assert pr.returncode == 0, "batch_host_harness (%s) %s exit %d:\n%s" % (request.param, args, pr.returncode, pr.stdout[-4000:])
        return pr.stdout.rstrip("\n")

    run.piece = piece
    return run


def offsets_of(lengths, first=0):
    return [first + int(x) for x in np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)])]


def test_no_reads(batch_host):
    assert batch_host([0]) == [(None, 0, True, [0])]
    assert batch_host([777]) == [(None, 0, False, [0])]


def test_one_read(batch_host):
    assert batch_host([0, 100]) == [(None, 100, True, [0, 100])]
    assert batch_host([5, 5]) == [(None, 0, False, [0, 0])]


@pytest.mark.parametrize("first", [0, 12345])
def test_lengths_0_1_1024(batch_host, first):
    lengths = [0, 1, 1024, 1, 0, 0, 1024, 7]
    off = offsets_of(lengths, first)
    (msg, max_len, own, rel), = batch_host(off)
    assert msg is None and max_len == 1024
    assert own == (first == 0)
    assert rel == offsets_of(lengths)
    # each of the three lengths alone is the maximum it should be
    for l in (0, 1, 1024):
        assert batch_host(offsets_of([l], first))[0][:2] == (None, l)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_length_1025_is_refused(batch_host, where):
    lengths = [100] * 9
    lengths[{"first": 0, "middle": 4, "last": 8}[where]] = 1025
    (msg, _, _, _), = batch_host(offsets_of(lengths, 3))
    assert msg == TOO_LONG


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_decreasing_offsets_are_refused(batch_host, where):
    off = offsets_of([100] * 9, 50)
    i = {"first": 0, "middle": 4, "last": 8}[where]
    off[i + 1] = off[i] - 1  # read i ends before it starts (the pair behind it is 201 apart: in order, not above 1024)
    (msg, _, _, _), = batch_host(off)
    assert msg == DECREASING


def test_order_is_checked_before_length(batch_host):
    """read by read, the order first: an over-long read in front is reported before a decreasing pair behind it, and
    the other way round"""
    assert batch_host([0, 1025, 1000])[0][0] == TOO_LONG
    assert batch_host([10, 5, 2000])[0][0] == DECREASING


def test_own_array_comes_back_when_it_starts_at_zero(batch_host):
    (_, _, own, rel), = batch_host(offsets_of([3, 0, 150], 0))
    assert own and rel == [0, 3, 3, 153]


def test_rebased_to_the_first_read(batch_host):
    lengths = list(np.random.RandomState(5).randint(0, 1025, size=300))
    off = offsets_of(lengths, 12345)
    (msg, max_len, own, rel), = batch_host(off)
    assert msg is None and not own and max_len == max(lengths)
    assert len(rel) == len(off) == 301 and rel == [x - 12345 for x in off]


def test_two_mates_share_the_maximum(batch_host):
    m1, m2 = offsets_of([100, 90, 100]), offsets_of([100, 151, 30], 12345)
    r1, r2 = batch_host(m1, m2)
    assert r1 == (None, 100, True, m1)
    assert r2 == (None, 151, False, offsets_of([100, 151, 30]))
    # ... and a maximum in the first mate stays
    r1, r2 = batch_host(m2, m1)
    assert (r1[1], r2[1]) == (151, 151)
    # a refusal in the second mate ends the call there
    res = batch_host(m1, [0, 100, 99, 200])
    assert [r[0] for r in res] == [None, DECREASING]


# ---------------------------------------------------------------------------
# what the methylation-side host forms share
# ---------------------------------------------------------------------------
RECORD_STRIDE = "record stride %d is smaller than a walt_best_match (16) or not a multiple of 4"
CONV_STRIDE = "conv stride 0 is smaller than its element (1)"
SKIP_STRIDE = "skip stride 0 is smaller than its element (1)"
CONVERSION = "conversion %d is neither 'T' nor 'A'"
T, A, C = ord("T"), ord("A"), ord("C")


@pytest.mark.parametrize("n", [0, 1, 3])
@pytest.mark.parametrize("elem,stride", [(16, 16), (16, 20), (16, 64), (1, 1), (1, 2), (1, 64)])
def test_strided_packing_reads_the_element_and_no_more(batch_host, elem, stride, n):
    """the source is a heap block that ends with the last element: the sanitised build reports a read of `stride` bytes
    there; the harness compares the packed output element by element"""
    assert batch_host.piece("pack", elem, stride, n) == "ok"


def test_each_shared_refusal_alone_and_its_accepted_neighbours(batch_host):
    piece = batch_host.piece
    for stride in (8, 12, 18):
        assert piece("refuse", "record", stride) == RECORD_STRIDE % stride
    assert piece("refuse", "record", 16) == "ok" and piece("refuse", "record", 20) == "ok"
    # a conv / skip stride of 0 with an array; without one the stride is not looked at
    assert piece("refuse", "conv", 1, 0, T) == CONV_STRIDE and piece("refuse", "conv", 1, 1, T) == "ok"
    assert piece("refuse", "skip", 1, 0) == SKIP_STRIDE and piece("refuse", "skip", 1, 1) == "ok"
    assert piece("refuse", "skip", 0, 0) == "ok"
    # a batch-wide conversion with no array; with one the batch-wide value is not looked at
    assert piece("refuse", "conv", 0, 0, C) == CONVERSION % C
    assert piece("refuse", "conv", 0, 0, T) == "ok" and piece("refuse", "conv", 0, 0, A) == "ok"
    assert piece("refuse", "conv", 1, 1, C) == "ok"


@pytest.mark.parametrize("stride", [1, 2])
def test_several_faults_in_one_batch_report_the_first_by_read_then_by_check(batch_host, stride):
    """read i's order, then its length, then its conversion byte, before anything of read i + 1"""
    piece = batch_host.piece
    bad_conv = "who: conversion %d of read %%d is neither 'T' nor 'A'" % C
    # a bad conversion byte at read 0, 1,025 bases at read 1
    assert piece("reads", stride, 3, 0, 5, 1030, 1035, C, T, T) == bad_conv % 0
    # 1,025 bases and a bad conversion byte, both at read 0
    assert piece("reads", stride, 3, 0, 1025, 1030, 1035, C, T, T) == TOO_LONG
    # a decreasing pair at read 1, a bad conversion byte at read 2
    assert piece("reads", stride, 3, 0, 50, 40, 1035, T, T, C) == DECREASING
    # each alone, the last read included; none; no conversions at all; no reads
    assert piece("reads", stride, 3, 0, 50, 100, 150, T, A, C) == bad_conv % 2
    assert piece("reads", stride, 3, 0, 50, 100, 1125, T, A, T) == TOO_LONG
    assert piece("reads", stride, 3, 0, 50, 100, 99, T, A, T) == DECREASING
    assert piece("reads", stride, 3, 0, 50, 100, 1124, T, A, T) == "ok"
    assert piece("reads", stride, 3, 0, 50, 100, 150) == "ok" and piece("reads", stride, 0, 7) == "ok"
