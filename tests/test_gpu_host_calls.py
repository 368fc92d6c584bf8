"""The four host-buffer mapping calls (walt_map_se_batch, walt_map_se_rpbat_batch, walt_map_pe_batch,
walt_map_pe_rpbat_batch) share one host-side driver: the offset scan and rebase (walt_amd/csrc/batch_host.h), the
grow-only device buffers of the index, and the index's busy locks.  On the golden g1 index: a slice of a larger
batch maps like the same reads packed on their own; the buffers the single-end and paired-end forms share keep every
form exact while they grow and shrink between calls; and a second concurrent call of a form is refused with
WALT_EINVAL -- or runs after the first -- but never races it."""
import os
import threading

import numpy as np
import pytest

import refio
import test_gpu_rpbat as se_rule
import test_pe_rpbat_cpu as pe_rule
from test_harness_cpu import assert_best_equal

pytestmark = pytest.mark.gpu

PAIR_FIELDS = ("best_times", "frag_len", "best_i", "best_j", "pair_mm")


def load(name, n=10 ** 7):
    return next(refio.load_fastq_batches(os.path.join(refio.GOLDEN, name), n))[1]


@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "host_calls_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
    yield refio.DbIndex(path), idx
    idx.close()


def assert_pairs(got, want, what):
    for f in PAIR_FIELDS:
        assert np.array_equal(got[f], want[f]), "%s field %s" % (what, f)
    assert_best_equal(got["m1"], want["m1"], what + " m1")
    assert_best_equal(got["m2"], want["m2"], what + " m2")


def test_a_slice_maps_like_its_reads_alone(g1):
    """offsets[100 .. 400] of a batch of 600 (the first entry is not 0) with the whole batch's bases: every form gives
    the records, conversion bytes and statistics of reads 100-399 packed on their own"""
    import walt_amd
    _, idx = g1
    lo, hi = 100, 400
    se, p1, p2 = load("se_ct.fastq", 600), load("pe_1.fastq", 600), load("pe_2.fastq", 600)
    assert len(se) == len(p1) == len(p2) == 600
    whole = {k: walt_amd.pack_reads(v) for k, v in (("se", se), ("p1", p1), ("p2", p2))}
    alone = {k: walt_amd.pack_reads(v[lo:hi]) for k, v in (("se", se), ("p1", p1), ("p2", p2))}

    def sliced(k):
        bases, offsets = whole[k]
        assert int(offsets[lo]) > 0
        return bases, offsets[lo:hi + 1]

    got, st = idx.map_se_batch(*sliced("se"))
    want, wst = idx.map_se_batch(*alone["se"])
    assert got.tobytes() == want.tobytes() and st.tobytes() == wst.tobytes() and int(wst["probes"]) > 0

    got, conv, st = idx.map_se_rpbat_batch(*sliced("se"))
    want, wconv, wst = idx.map_se_rpbat_batch(*alone["se"])
    assert got.tobytes() == want.tobytes() and np.array_equal(conv, wconv) and st.tobytes() == wst.tobytes()
    assert set(np.unique(wconv)) <= {ord("T"), ord("A")} and (want["times"] > 0).sum() > 200

    got, st = idx.map_pe_batch(*sliced("p1"), *sliced("p2"))
    want, wst = idx.map_pe_batch(*alone["p1"], *alone["p2"])
    assert_pairs(got, want, "paired-end slice")
    assert st.tobytes() == wst.tobytes() and (want["best_times"] > 0).sum() > 200

    got, conv, st = idx.map_pe_rpbat_batch(*sliced("p1"), *sliced("p2"))
    want, wconv, wst = idx.map_pe_rpbat_batch(*alone["p1"], *alone["p2"])
    assert_pairs(got, want, "paired-end random PBAT slice")
    assert np.array_equal(conv, wconv) and st.tobytes() == wst.tobytes()
    assert (want["best_times"] > 0).sum() > 200


def test_forms_share_growing_buffers(g1):
    """single-end, paired-end, single-end random PBAT, paired-end random PBAT, single-end on one index with 64, 600,
    64, 600, 64 reads: the slots the forms share grow under one form and are reused by the next"""
    import walt_amd
    db, idx = g1
    se, p1, p2 = load("se_ct.fastq", 600), load("pe_1.fastq", 600), load("pe_2.fastq", 600)

    def single_end(n):
        got, st = idx.map_se_batch(*walt_amd.pack_reads(se[:n]))
        want, work = refio.oracle_se(db, se[:n])
        assert_best_equal(got, want, "single-end n=%d" % n)
        assert int(st["too_short"]) == int(work["too_short"])

    single_end(64)
    got, _ = idx.map_pe_batch(*walt_amd.pack_reads(p1), *walt_amd.pack_reads(p2))
    assert_pairs(got, refio.oracle_pe(db, p1, p2)[0], "paired-end n=600")
    got, conv, st = idx.map_se_rpbat_batch(*walt_amd.pack_reads(se[:64]))
    want, wconv, _, short = se_rule.oracle_rpbat(db, se[:64])
    se_rule.assert_records(got, conv, want, wconv, "single-end random PBAT n=64")
    assert int(st["too_short"]) == short
    got, conv, st = idx.map_pe_rpbat_batch(*walt_amd.pack_reads(p1), *walt_amd.pack_reads(p2))
    want, wconv, _, short = pe_rule.oracle_pe_rpbat(db, p1, p2)
    pe_rule.compare(got, conv, want, wconv, "paired-end random PBAT n=600")
    assert (int(st[0]["too_short"]), int(st[1]["too_short"])) == short
    single_end(64)


@pytest.mark.parametrize("form", ["map_se_batch", "map_pe_batch"])
def test_a_second_call_is_refused_never_raced(g1, form):
    """two threads, four calls each of one form on one index: every call returns the single-threaded result or is
    refused (WALT_EINVAL, "another ... call is running"); whether a refusal happens is a matter of timing"""
    import walt_amd
    _, idx = g1
    if form == "map_se_batch":
        args = walt_amd.pack_reads(load("se_ct.fastq") * 3)
    else:
        args = walt_amd.pack_reads(load("pe_1.fastq") * 4) + walt_amd.pack_reads(load("pe_2.fastq") * 4)
    assert args[1].size - 1 >= 3000
    call = getattr(idx, form)
    same = assert_best_equal if form == "map_se_batch" else assert_pairs
    want, want_st = call(*args)
    assert ((want["times"] if form == "map_se_batch" else want["best_times"]) > 0).sum() > 2000
    barrier = threading.Barrier(2)
    results = [[], []]

    def worker(k):
        barrier.wait(60)
        for _ in range(4):
            try:
                results[k].append(call(*args))
            except BaseException as e:  # judged in the main thread
                results[k].append(e)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    done = results[0] + results[1]
    assert len(done) == 8
    ok = 0
    for r in done:
        if isinstance(r, BaseException):
            assert isinstance(r, walt_amd.WaltError), repr(r)
            assert r.code == walt_amd.WALT_EINVAL and "another" in str(r), str(r)
        else:
            same(r[0], want, "a call beside another one")
            assert r[1].tobytes() == want_st.tobytes()
            ok += 1
    assert ok >= 1
    got, st = call(*args)
    same(got, want, "a call after the threads")
    assert st.tobytes() == want_st.tobytes()
