"""Grouping of the dense verifier's work items by region (walt_amd/csrc/group_core.h), the parts that need no device:
key, bucket and the unit cutter, compiled with g++ (tests/group_harness.cpp) and compared with a plain Python
restatement on synthetic item headers; and the same harness as a stand-alone program under the host's sanitizers
(tests/group_sanitize_main.cpp)."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import refio

CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")
BIG_FIRST = 1024
MULT = 0x9E3779B97F4A7C15
RS = [2, 4, 8, 64]


@pytest.fixture(scope="module")
def harness(scratch):
    so = os.path.join(scratch, "libgroup_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", CSRC,
                    os.path.join(refio.HERE, "group_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.group_harness_buckets.restype = u32
    L.group_harness_slice.restype = u32
    L.group_harness_key.argtypes = [u32, u32]
    L.group_harness_key.restype = u64
    L.group_harness_bucket.argtypes = [u64]
    L.group_harness_bucket.restype = u32
    L.group_harness_cut.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp]
    L.group_harness_cut.restype = u32
    return L


# ---------------------------------------------------------------------------
# the plain restatement
# ---------------------------------------------------------------------------
def key_of(item):
    ident, size, rec0, tail = item
    return ((ident >> 31) << 32) | rec0


def bucket_of(key):
    return ((key * MULT) & (2 ** 64 - 1)) >> 48


def plain_units(items, r):
    """-> (order, units): the items by bucket (in item order), every 64 places of that order regrouped by first
    appearance of (key, size) -- a tail item alone -- and every group cut into units of at most r; units = (first place,
    items, big)"""
    by_bucket = {}
    for i, it in enumerate(items):
        by_bucket.setdefault(bucket_of(key_of(it)), []).append(i)
    order, units = [], []
    members = [i for b in sorted(by_bucket) for i in by_bucket[b]]
    for s in range(0, len(members), 64):
        sl = members[s:s + 64]
        groups = []
        for i in sl:
            ident, size, rec0, tail = items[i]
            for g in groups:
                j = g[0]
                if tail == 0 and items[j][3] == 0 and key_of(items[j]) == key_of(items[i]) and items[j][1] == size:
                    g.append(i)
                    break
            else:
                groups.append([i])
        for g in groups:
            for u in range(0, len(g), r):
                units.append((len(order) + u, len(g[u:u + r]), items[g[0]][1] > BIG_FIRST))
            order += g
    return order, units


def cut(harness, items, r):
    n = len(items)
    cols = [np.array([it[c] for it in items] + [0], dtype=np.uint32) for c in range(4)]
    order = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32)
    first = np.zeros(n + 1, dtype=np.uint32)
    cnt = np.zeros(n + 1, dtype=np.uint32)
    big = np.zeros(n + 1, dtype=np.uint8)
    k = harness.group_harness_cut(cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data, cols[3].ctypes.data, n, r, BIG_FIRST,
                                  order.ctypes.data, first.ctypes.data, cnt.ctypes.data, big.ctypes.data)
    assert order[n] == 0xFFFFFFFF and cnt[n] == 0  # nothing behind the arrays' n entries
    return order[:n].tolist(), [(int(first[u]), int(cnt[u]), bool(big[u])) for u in range(k)]


def check(harness, items, r):
    """the harness equals the restatement; every item in exactly one unit; no unit mixes keys or sizes, exceeds r or
    holds a tail item beside another"""
    order, units = cut(harness, items, r)
    want_order, want_units = plain_units(items, r)
    assert order == want_order
    assert sorted(units) == sorted(want_units)
    assert sorted(order) == list(range(len(items)))
    seen = [0] * len(items)
    for first, n, big in units:
        assert 1 <= n <= r
        members = [items[order[p]] for p in range(first, first + n)]
        for p in range(first, first + n):
            seen[p] += 1
        assert len({(key_of(m), m[1]) for m in members}) == 1
        assert n == 1 or all(m[3] == 0 for m in members)
        assert big == (members[0][1] > BIG_FIRST)
    assert seen == [1] * len(items)
    return order, units


def keys_in_bucket(harness, bucket, count, start=0):
    """`count` record numbers whose '+' key falls into `bucket`"""
    found = []
    lo = start
    while len(found) < count:
        rec = np.arange(lo, lo + (1 << 22), dtype=np.uint64)
        b = (rec * np.uint64(MULT)) >> np.uint64(48)
        found += rec[b == np.uint64(bucket)].tolist()
        lo += 1 << 22
    found = [int(v) for v in found[:count]]
    assert all(harness.group_harness_bucket(v) == bucket for v in found)
    return found


# ---------------------------------------------------------------------------
def test_key_and_bucket_equal_the_restatement(harness):
    assert harness.group_harness_buckets() == 1 << 16 and harness.group_harness_slice() == 64
    rng = random.Random(3)
    for _ in range(4000):
        ident, rec0 = rng.getrandbits(32), rng.getrandbits(32)
        k = harness.group_harness_key(ident, rec0)
        assert k == key_of((ident, 0, rec0, 0)) and k >> 33 == 0
        assert harness.group_harness_bucket(k) == bucket_of(k) < 1 << 16
    # the chunk position of an item is no part of its key, its strand is
    assert harness.group_harness_key(5, 77) == harness.group_harness_key(900, 77) != harness.group_harness_key(5 | 1 << 31, 77)


@pytest.mark.parametrize("r", RS)
def test_runs_of_every_length(harness, r):
    rng = random.Random(r)
    for run in sorted({1, 2, r - 1, r, r + 1, 2 * r + 1, 64, 65, 130}):
        if run < 1:
            continue
        items = [(rng.randrange(1 << 20), 300, 123456, 0) for _ in range(run)]  # one region, `run` reads
        items += [(rng.randrange(1 << 20), rng.choice([40, 2000]), 10 ** 6 + 7 * k, 0) for k in range(50)]  # background
        rng.shuffle(items)
        order, units = check(harness, items, r)
        mine = sorted(n for first, n, big in units if items[order[first]][2] == 123456)
        # a run is cut at the borders of the order's slices of 64 and into units of r: no fewer units than ceil(run / r), and at
        # most one more per border it crosses
        assert sum(mine) == run and len(mine) >= -(-run // r)
        assert len(mine) <= -(-run // r) + (run + 62) // 64 + 1


@pytest.mark.parametrize("r", RS)
def test_strands_sizes_and_tail_items_are_kept_apart(harness, r):
    plus, minus = 10, 10 | 1 << 31
    items = [(plus + k, 500, 4242, 0) for k in range(5)] + [(minus + k, 500, 4242, 0) for k in range(5)]  # equal rec0, two strands
    items += [(plus + 20 + k, 700, 4242, 0) for k in range(5)]  # equal rec0, another size
    items += [(plus + 40 + k, 500, 4242, 1) for k in range(3)] + [(plus + 50, 500, 4242, 2)]  # tail items inside the run
    random.Random(9).shuffle(items)
    order, units = check(harness, items, r)
    got = sorted((items[order[first]][0] >> 31, items[order[first]][1], items[order[first]][3], n) for first, n, big in units)
    cutn = lambda n: [r] * (n // r) + ([n % r] if n % r else [])
    want = [(0, 500, 0, n) for n in cutn(5)] + [(1, 500, 0, n) for n in cutn(5)] + [(0, 700, 0, n) for n in cutn(5)]
    want += [(0, 500, 1, 1)] * 3 + [(0, 500, 2, 1)]
    assert got == sorted(want)


@pytest.mark.parametrize("r", RS)
def test_every_key_in_one_bucket_and_every_key_in_its_own(harness, r):
    rng = random.Random(40 + r)
    recs = keys_in_bucket(harness, 777, 30)
    items = []
    for k, rec in enumerate(recs):  # 30 regions of 1 .. 9 reads each, all in bucket 777: 150 items, three slices
        items += [(rng.randrange(1 << 20), 100 + k, rec, 0) for _ in range(1 + k % 9)]
    rng.shuffle(items)
    check(harness, items, r)
    # the other extreme: no two keys share a bucket
    items, used = [], set()
    rec = 0
    while len(items) < 300:
        rec += 1
        b = bucket_of(rec)
        if b in used:
            continue
        used.add(b)
        items += [(rng.randrange(1 << 20), 64, rec, 0) for _ in range(rng.choice([1, 1, 2, r + 1]))]
    rng.shuffle(items)
    order, units = check(harness, items, r)
    least = sum(-(-n // r) for n in np.unique([it[2] for it in items], return_counts=True)[1])
    assert least <= len(units) <= least + len(items) // 64 + 1  # (a slice border may cut a run once more)


@pytest.mark.parametrize("r", RS)
def test_zero_items_and_random_mixtures(harness, r):
    assert cut(harness, [], r) == ([], [])
    rng = random.Random(1000 + r)
    for trial in range(40):
        regions = [(rng.randrange(1 << 31), rng.choice([17, 64, 1024, 1025, 5000]), rng.getrandbits(1)) for _ in range(rng.choice([1, 5, 60]))]
        items = []
        for _ in range(rng.choice([1, 63, 64, 65, 700])):
            rec, size, strand = rng.choice(regions)
            size = size if rng.random() < 0.9 else size + 1
            items.append((rng.randrange(1 << 20) | strand << 31, size, rec, 1 if rng.random() < 0.05 else 0))
        check(harness, items, r)


def test_the_harness_under_the_sanitizers(scratch):
    """tests/group_sanitize_main.cpp: the same harness as a program of its own with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = os.path.join(scratch, "group_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(refio.HERE, "group_sanitize_main.cpp"), os.path.join(refio.HERE, "group_harness.cpp"), "-o", exe],
                   check=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr
