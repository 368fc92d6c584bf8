"""The long-slot search whose first fence round takes the keys of its A pivots from core.h fence_first_keys -- what the
heavy and staged kernels do with the keys map_common.h probe_entries_first fetches beside the directory pair -- compiled
with g++ (tests/fence_prefetch_harness.cpp) and compared with slot_fence_search and std::equal_range.

The harness draws sorted key arrays with the fence levels of k_make_fences (every 16th, 256th, 4096th and 65536th key),
slots of 5, 16, 17, 31, 32, 255, 256, 257, 4095, 4097, 8200 and 70,003 entries at first entries that are and are not
multiples of 16, masks of 1 .. 32 key characters, and targets that are absent, below every key, above every key, an equal
run over a pivot and an equal run that is the whole slot.  It asserts (1) the same [a, u] and found / not found from the
three searches, (2) that the addresses fence_first_keys names are those the first round of slot_fence_bounds reads
(fence_plan + fence_ptr of the whole slot) and lie inside their arrays.  It is a program of its own, built plain and
with -fsanitize=address,undefined; every array is a heap block of exactly its words, so the second build also reports
any key read beyond one.  The tests here check that the run was clean and that no class of inputs was empty."""
import os
import subprocess

import pytest

import refio

SIZES = [5, 16, 17, 31, 32, 255, 256, 257, 4095, 4097, 8200, 70003]


@pytest.fixture(scope="module", params=["plain", "sanitised"])
def harness_counts(request, scratch):
    exe = os.path.join(scratch, "fence_prefetch_harness_" + request.param)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] if request.param == "sanitised" else []
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-I", os.path.join(refio.ROOT, "walt_amd", "csrc"),
                    os.path.join(refio.HERE, "fence_prefetch_harness.cpp"), "-o", exe], check=True, timeout=300)
    if request.param == "sanitised":
        assert b"__asan_report_load4" in open(exe, "rb").read(), "the sanitised build carries no address checks"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    total = {}
    for seed in (1, 2, 3):
        pr = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
        assert pr.returncode == 0, "fence_prefetch_harness (%s, seed %d) exit %d:\n%s" % (request.param, seed, pr.returncode, pr.stdout[-4000:])
        words = pr.stdout.split()
        assert len(words) % 2 == 0 and words[0] == "cases", pr.stdout[-2000:]
        for name, value in zip(words[::2], words[1::2]):
            total[name] = total.get(name, 0) + int(value)
    return total


def test_searches_agree_on_every_class(harness_counts):
    """exit 0 of the fixture's runs = the three searches agreed and every address check held; here: nothing was left out"""
    c = harness_counts
    assert c["cases"] > 30000 and 0 < c["found"] < c["cases"]
    for size in SIZES:
        for al in ("aligned", "unaligned"):
            assert c["size_%d_%s" % (size, al)] >= 3, (size, al)
    for nk in range(1, 33):
        assert c["nk_%d" % nk] > 0, nk
    for t in ("absent", "below", "above", "run_over_pivot", "run_is_slot"):
        assert c["target_" + t] > 0, t


def test_every_first_plan_occurs(harness_counts):
    """the first round's plan: entries (fewer than 16 of them too) and each of the four fence levels"""
    c = harness_counts
    assert c["few_pivots"] > 0
    for sh in (0, 4, 8, 12, 16):
        assert c["sh_%d" % sh] > 0, sh
