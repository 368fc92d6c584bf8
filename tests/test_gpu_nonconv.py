"""Non-converted reads on the GPU (include/walt_amd.h, "non-converted reads"): walt_nonconv_batch, walt_nonconv_pairs_batch
and walt_meth_nonconv_batch through walt_amd.Index, host and device forms, and bin/walt -F / -FC / -FP / -FM, all against
one pure-Python restatement of the contract (tally_of, fails, expected_verdicts, pair_rule below: plain loops over the
bytes, which never use the code under test).  tests/test_nonconv_cpu.py imports the restatement."""
import os
import random
import subprocess

import numpy as np
import pytest

import refio

LENGTHS = (1, 15, 16, 17, 31, 127, 128, 129, 1024)
WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
# the three settings of the command-line cases: (options, rule as min_meth, min_run, min_percent, min_total)
SETTINGS = {"F3": (["-F", "3"], (3, 0, 0, 0)), "FC2": (["-FC", "2"], (0, 2, 0, 0)), "FP15": (["-FP", "15", "-FM", "5"], (0, 0, 15, 5))}


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def tally_of(calls):
    """calls: the bytes of one read in read order -> (meth, total, run)"""
    meth = total = run = cur = 0
    for b in bytes(calls):
        if b in (ord("H"), ord("X")):
            meth += 1
            total += 1
            cur += 1
            run = max(run, cur)
        elif b in (ord("h"), ord("x")):
            total += 1
            cur = 0
    return meth, total, run


def fails(meth, total, run, rule):
    """the contract's three sentences; rule = (min_meth, min_run, min_percent, min_total)"""
    min_meth, min_run, min_percent, min_total = rule
    if min_meth > 0 and meth >= min_meth:
        return 1
    if min_run > 0 and run >= min_run:
        return 1
    if min_percent > 0 and total >= max(min_total, 1) and 100 * meth >= min_percent * total:
        return 1
    return 0


def expected_verdicts(calls, offsets, times, rule, base=None):
    """calls: uint8 array whose element 0 is byte `base` (default offsets[0]) of what the offsets index.  A record is
    judged when times == 1, it has 1 to 1024 calls and its offsets lie inside [offsets[0], offsets[n]); every other one
    gets zeros.  -> (filt uint8[n], tally int array [n, 3])"""
    calls = np.asarray(calls, dtype=np.uint8)
    offsets = [int(v) for v in offsets]
    base = offsets[0] if base is None else base
    n = len(offsets) - 1
    filt, tally = np.zeros(n, dtype=np.uint8), np.zeros((n, 3), dtype=np.int64)
    for r in range(n):
        lo, hi = offsets[r], offsets[r + 1]
        if int(times[r]) != 1 or not 1 <= hi - lo <= 1024 or lo < offsets[0] or hi > offsets[n]:
            continue
        tally[r] = tally_of(calls[lo - base:hi - base].tobytes())
        filt[r] = fails(*tally[r], rule)
    return filt, tally


def pair_rule(filt, best_times):
    """filt [n, 2] -> a copy with both bytes of a pair with best_times == 1 set to their OR"""
    out = np.array(filt, dtype=np.uint8).reshape(-1, 2).copy()
    for i in range(out.shape[0]):
        if int(best_times[i]) == 1:
            out[i, :] = out[i, 0] | out[i, 1]
    return out


def filterstats_text(records, filtered, rule):
    return "records: %d\nfiltered: %d\nfilter rate: %s\nrule\t%d\t%d\t%d\t%d\n" % (
        (records, filtered, "%.6f" % (filtered / records) if records else "NA") + tuple(rule))


def calls_list_to_array(calls_list):
    return np.frombuffer("".join(calls_list).encode("latin-1"), dtype=np.uint8)


def se_outcome(recs, filt, dup=None):
    """-> (records, filtered) of <out>.filterstats for single records"""
    keep = (recs["times"] == 1) & ((dup == 0) if dup is not None else True)
    return int(keep.sum()), int((filt[keep] != 0).sum())


def pe_outcome(res, filt, dup=None):
    """filt, dup: [n, 2] in the records' order -> (records, filtered): unique pairs once, lone unique mates each"""
    records = filtered = 0
    for j in range(res.size):
        if int(res["best_times"][j]) == 1:
            owners = [0]
        else:
            owners = [k for k in (0, 1) if int(res["m%d" % (k + 1)]["times"][j]) == 1]
        for k in owners:
            if dup is not None and dup[j, k]:
                continue
            records += 1
            filtered += int(filt[j, k] != 0)
    return records, filtered


def random_calls(rng, n, dense=False):
    al = "HXhx" * 3 + "HH.Z" if dense else "HXhxzZuU" + "H" * 4 + "." * 20 + "ACGT#-"
    return np.frombuffer("".join(rng.choice(al) for _ in range(n)).encode(), dtype=np.uint8)


def records(times, stride=16):
    import walt_amd
    rec = np.zeros(len(times), dtype=walt_amd.best_match_dtype if stride == 16 else walt_amd.pair_result_dtype)
    if stride == 16:
        rec["times"] = times
        return rec
    rec["m2"]["times"] = times  # the second mate of a walt_pair_result array: stride 64, base + 16
    rec["m1"]["times"] = 1 - np.minimum(np.asarray(times), 1)  # (the other mate's would be wrong)
    return rec["m2"]


def tally_array(tally):
    return np.stack([tally["meth"], tally["total"], tally["run"]], axis=1).astype(np.int64)


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "nonconv_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    return refio.DbIndex(path), path


@pytest.fixture(scope="module")
def g1_all(g1):
    import walt_amd
    idx = walt_amd.Index.open(g1[1], device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def g1_ct(g1):
    """any strands will do, with or without the reference: the hand-made batches run on the C->T strands alone"""
    import walt_amd
    idx = walt_amd.Index.open(g1[1], device=0, strands=walt_amd.STRANDS_CT)
    yield idx
    idx.close()


def hand_batch(rng, lens, dense=False):
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    return random_calls(rng, int(offsets[-1]), dense), offsets


def lengths_at_every_offset():
    """every length behind reads of 0 .. 15 calls: each length at every offset modulo 16"""
    lens = []
    for L in LENGTHS:
        for lead in range(16):
            lens += [lead, L]
    return lens + [40] * 5


RULES = ((3, 0, 0, 0), (0, 2, 0, 0), (0, 0, 15, 5), (40, 7, 60, 1), (0, 0, 0, 0), (1024, 1024, 100, 1024))


# ---------------------------------------------------------------------------
# 1. hand-made batches
# ---------------------------------------------------------------------------
def test_host_form_lengths_alignments_records_strides_and_n(wa, g1_ct):
    rng = random.Random(21)
    lens = lengths_at_every_offset()
    assert len(lens) == 293
    for dense in (False, True):
        calls, offsets = hand_batch(rng, lens, dense)
        times = [rng.choice([0, 1, 1, 1, 2]) for _ in lens]
        assert {0, 1, 2} <= set(times)
        for rule in RULES:
            want_f, want_t = expected_verdicts(calls, offsets, times, rule)
            filt, tally = g1_ct.nonconv_batch(calls, offsets, records(times), wa.nonconv_rule(*rule))
            assert filt.dtype == np.uint8 and tally.dtype == wa.nonconv_tally_dtype
            assert np.array_equal(tally_array(tally), want_t) and (tally["reserved"] == 0).all(), rule
            assert np.array_equal(filt, want_f), rule
            if rule == (0, 0, 0, 0):
                assert not filt.any()
            elif rule[0] == 3:
                assert 20 < int(filt.sum()) < int((np.asarray(times) == 1).sum()) - 5
        assert want_t[:, 2].max() >= (10 if dense else 3)  # (the inputs hold runs worth the name)
    # offsets that do not start at 0, records at stride 64, a filt stride of 2, no tally: the C call itself
    rule = (3, 2, 0, 0)
    want_f, want_t = expected_verdicts(calls, offsets, times, rule)
    moved = offsets + np.uint64(12345)
    rec = records(times, 64)
    filt2 = np.full((len(lens), 2), 7, dtype=np.uint8)
    r = wa.nonconv_rule(*rule)
    L = wa.lib()
    rc = L.walt_nonconv_batch(g1_ct.handle, calls.ctypes.data - 12345, moved.ctypes.data, len(lens), rec.ctypes.data, 64, r.ctypes.data,
                              filt2.ctypes.data + 1, 2, None)
    assert rc == 0, L.walt_last_error()
    assert np.array_equal(filt2[:, 1], want_f) and (filt2[:, 0] == 7).all()
    filt, tally = g1_ct.nonconv_batch(calls, moved, rec, r)
    assert np.array_equal(filt, want_f) and np.array_equal(tally_array(tally), want_t)
    assert g1_ct.nonconv_batch(calls, moved, rec, r, want_tally=False)[1] is None
    # n = 0 and n = 1
    filt, tally = g1_ct.nonconv_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), records([]), r)
    assert filt.size == 0 and tally.size == 0
    filt, tally = g1_ct.nonconv_batch(np.frombuffer(b"HxH.HHh", dtype=np.uint8), [0, 7], records([1]), r)
    assert filt.tolist() == [1] and tally_array(tally).tolist() == [[4, 6, 3]]  # (the '.' between H and HH does not end the run)


def to_device(torch, dev, calls, offsets, rec, shift=0, pad=64):
    """calls at a device address that is `shift` modulo 16, with 'H' around it (a slice that reads outside the reads
    shows in the tally)"""
    d_raw = torch.full((calls.size + pad + 32,), ord("H"), dtype=torch.uint8, device=dev)
    a = (-d_raw.data_ptr()) % 16 + shift
    d_raw[a:a + calls.size] = torch.from_numpy(np.ascontiguousarray(calls)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(dev)
    stride = rec.strides[0] if rec.size > 1 else rec.dtype.itemsize
    flat = np.zeros(max(rec.size, 1) * stride + 64, dtype=np.uint8)
    for i in range(rec.size):
        flat[i * stride:i * stride + 16] = np.frombuffer(rec[i].tobytes(), dtype=np.uint8)
    d_rec = torch.from_numpy(flat).to(dev)
    return d_raw, d_raw.data_ptr() + a, d_off, d_rec, stride


def device_verdicts(wa, idx, torch, dev, calls, offsets, rec, rule, shift=0, stream=None, filt_stride=1, tally=True):
    n = len(offsets) - 1
    keep, d_calls, d_off, d_rec, stride = to_device(torch, dev, calls, offsets, rec, shift)
    d_filt = torch.full((max(n, 1) * filt_stride + 1,), 7, dtype=torch.uint8, device=dev)
    d_tally = torch.full((max(n, 1), 4), -1, dtype=torch.int16, device=dev) if tally else None
    torch.cuda.synchronize()
    idx.nonconv_batch_device(d_calls, d_off.data_ptr(), n, d_rec.data_ptr(), wa.nonconv_rule(*rule), d_filt.data_ptr(), stride,
                             filt_stride, d_tally.data_ptr() if tally else None, stream.cuda_stream if stream is not None else 0)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    f = d_filt.cpu().numpy()
    assert (f[n * filt_stride:] == 7).all()
    others = np.delete(f[:n * filt_stride].reshape(n, filt_stride), 0, axis=1) if n and filt_stride > 1 else np.zeros(0)
    assert (others == 7).all()
    t = d_tally.cpu().numpy().view(np.uint16)[:n] if tally else None
    return f[:n * filt_stride:filt_stride], t


def test_device_form_every_alignment_on_a_stream_of_its_own(wa, g1_ct):
    import torch
    rng = random.Random(22)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    lens = lengths_at_every_offset()
    calls, offsets = hand_batch(rng, lens, dense=True)
    times = [rng.choice([0, 1, 1, 1, 2]) for _ in lens]
    rule = (30, 6, 55, 4)
    want_f, want_t = expected_verdicts(calls, offsets, times, rule)
    assert 20 < int(want_f.sum()) < int((np.asarray(times) == 1).sum()) - 20
    for shift in range(16):
        stride = 64 if shift % 3 == 0 else 16
        f, t = device_verdicts(wa, g1_ct, torch, dev, calls, offsets, records(times, stride), rule, shift, stream,
                               filt_stride=2 if shift % 2 else 1)
        assert np.array_equal(t[:, :3].astype(np.int64), want_t) and (t[:, 3] == 0).all(), shift
        assert np.array_equal(f, want_f), shift
    f, t = device_verdicts(wa, g1_ct, torch, dev, calls, offsets, records(times), rule, 5, None, tally=False)
    assert np.array_equal(f, want_f) and t is None
    # n = 0 with null arrays is fine; n = 1
    g1_ct.nonconv_batch_device(None, None, 0, None, wa.nonconv_rule(*rule), None)
    f, t = device_verdicts(wa, g1_ct, torch, dev, np.frombuffer(b"xHHHHHHx", dtype=np.uint8), [0, 8], records([1]), rule, 9, stream)
    assert f.tolist() == [1] and t[0, :3].tolist() == [6, 8, 6]


def one_read(text, lead=0):
    """-> (calls, offsets, times) of one read behind `lead` bytes of a neighbour full of H (and one in front of another)"""
    body = np.frombuffer(text.encode(), dtype=np.uint8)
    calls = np.concatenate([np.full(lead, ord("H"), dtype=np.uint8), body, np.full(16, ord("H"), dtype=np.uint8)])
    return calls, [0, lead, lead + body.size, lead + body.size + 16], [1, 1, 1]


# (the read, the bytes of the neighbour in front of it = its head misalignment when the batch is 16-byte aligned, the tally
# WRITTEN BY HAND).  Slices are cut at the 16-byte boundaries of the array: read position i sits in slice (lead + i) // 16,
# a trip of a group is eight slices.
BOUNDARY_CASES = [
    ("h" + "." * 14 + "HH" + "." * 14 + "h", 0, (2, 4, 2)),                  # H at positions 15 and 16: a run over a slice boundary
    ("x" + "." * 126 + "XH" + "." * 10 + "x", 0, (2, 4, 2)),                # positions 127 and 128: over the group's trip boundary
    ("x" + "." * 118 + "XH" + "." * 10 + "x", 8, (2, 4, 2)),                # the same boundary with a head of 8 (positions 119, 120)
    ("h" + "." * 126 + "HH" + "h", 5, (2, 4, 2)),                            # 130 calls behind a head of 5: nine slices, two trips
    ("hH" + "." * 20 + "Z" * 20 + "." * 8 + "Hh", 14, (2, 4, 2)),            # a run carried through two slices of only '.' and 'Z'
    ("H" * 16 + "h" + "H" * 15 + "H" * 15 + "h" + "H" * 16, 0, (62, 64, 30)),  # an h as the first and as the last byte of a slice
    ("H" * 1024, 0, (1024, 1024, 1024)),
    ("H" * 1024, 3, (1024, 1024, 1024)),
    ("Hh" * 512, 0, (512, 1024, 1)),
    ("hH" * 512, 7, (512, 1024, 1)),
    ("zZuU.ACGT#" * 10, 1, (0, 0, 0)),
    ("H", 15, (1, 1, 1)),
    ("h" + "H" * 300 + "x" + "X" * 299 + "z" + "H" * 2, 11, (601, 603, 301)),  # a run over three trips; z does not end one
]


def test_runs_across_slice_and_trip_boundaries_host_and_device(wa, g1_ct):
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for text, lead, by_hand in BOUNDARY_CASES:
        assert tally_of(text.encode()) == by_hand, ("the restatement against the hand-written value", text[:40])
        calls, offsets, times = one_read(text, lead)
        rule = (0, by_hand[2], 0, 0)  # run == min_run fails
        f, t = device_verdicts(wa, g1_ct, torch, dev, calls, offsets, records(times), rule, 0, stream)
        assert t[1, :3].tolist() == list(by_hand), (text[:40], lead, t[1])
        assert t[0, :3].tolist() == [lead] * 3 and t[2, :3].tolist() == [16] * 3
        assert f[1] == (1 if by_hand[2] else 0)
        rule = (0, by_hand[2] + 1, 0, 0)  # one more passes
        f, _ = device_verdicts(wa, g1_ct, torch, dev, calls, offsets, records(times), rule, 0, stream)
        assert f[1] == 0
        # the host form stages the calls at an aligned address: the read's head is `lead` there too
        filt, tally = g1_ct.nonconv_batch(calls, offsets, records(times), wa.nonconv_rule(by_hand[0], 0, 0, 0))
        assert tally_array(tally)[1].tolist() == list(by_hand) and filt[1] == (1 if by_hand[0] else 0)


def test_a_read_of_1025_calls_and_made_up_offsets_between_judged_reads(wa, g1_ct):
    import torch
    rng = random.Random(23)
    dev = torch.device("cuda", 0)
    # a read of 1025 calls among the lengths: it gets zeros, its neighbours everything
    lens = [100, 1025, 129, 16, 1024, 1025, 1025, 17, 0, 31]
    calls, offsets = hand_batch(rng, lens, dense=True)
    times = [1] * len(lens)
    rule = (1, 0, 0, 0)
    want_f, want_t = expected_verdicts(calls, offsets, times, rule)
    assert want_f.tolist() == [1, 0, 1, 1, 1, 0, 0, 1, 0, 1] and (want_t[[1, 5, 6, 8]] == 0).all()
    for shift in (0, 7):
        f, t = device_verdicts(wa, g1_ct, torch, dev, calls, offsets, records(times), rule, shift)
        assert np.array_equal(f, want_f) and np.array_equal(t[:, :3].astype(np.int64), want_t)
    filt, tally = g1_ct.nonconv_batch(calls, offsets, records(times), wa.nonconv_rule(*rule))  # the host form does not refuse it
    assert np.array_equal(filt, want_f) and np.array_equal(tally_array(tally), want_t)
    # made-up offsets: read 1 ends behind the batch's last call, read 2 runs backwards; reads 0 and 3 are right
    calls = random_calls(rng, 300, dense=True)
    offsets = np.array([0, 100, 700, 200, 300], dtype=np.uint64)
    want_f, want_t = expected_verdicts(calls, offsets, [1, 1, 1, 1], rule)
    assert want_f.tolist() == [1, 0, 0, 1] and want_t[0, 0] > 0 and want_t[3, 0] > 0
    f, t = device_verdicts(wa, g1_ct, torch, dev, calls, offsets, records([1, 1, 1, 1]), rule, 3)
    assert np.array_equal(f, want_f) and np.array_equal(t[:, :3].astype(np.int64), want_t)


def test_more_reads_than_the_grid_takes_in_one_trip(wa, g1_ct):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # a block of nonconv.hip's kernel takes kBlock / kNonconvGroup = 256 / 8 reads per trip and at most
    # kNonconvBlocksPerCu = 8 blocks per compute unit are launched.  If those constants change, change these with them, or
    # the batch stops exceeding one trip of the grid.
    n = 8 * cus * (256 // 8) + 1237
    L = 40
    rng = np.random.default_rng(6)
    al = np.frombuffer(b"HXhxzZ" + b"H" * 2 + b"." * 12, dtype=np.uint8)
    calls = al[rng.integers(0, al.size, size=n * L)]
    times = rng.integers(0, 3, size=n).astype(np.uint32)
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    rule = (9, 4, 70, 5)
    rows = calls.reshape(n, L)
    up, low = (rows == ord("H")) | (rows == ord("X")), (rows == ord("h")) | (rows == ord("x"))
    meth, total = up.sum(axis=1), (up | low).sum(axis=1)
    # the restatement on a slice, and its meth / total columns vectorised over all reads of one length
    small_f, small_t = expected_verdicts(calls[:300 * L], offsets[:301], times[:300], rule)
    judged = times == 1
    assert np.array_equal(small_t[:, 0], np.where(judged, meth, 0)[:300]) and np.array_equal(small_t[:, 1], np.where(judged, total, 0)[:300])
    rec = np.zeros(n, dtype=wa.best_match_dtype)
    rec["times"] = times
    filt, tally = g1_ct.nonconv_batch(calls, offsets, rec, wa.nonconv_rule(*rule))
    assert np.array_equal(tally["meth"], np.where(judged, meth, 0)) and np.array_equal(tally["total"], np.where(judged, total, 0))
    assert np.array_equal(filt[:300], small_f) and np.array_equal(tally_array(tally)[:300], small_t)
    # every read of the batch: the verdict from the kernel's own tally equals the rule, and the last reads equal the restatement
    assert all(int(filt[i]) == fails(int(tally["meth"][i]), int(tally["total"][i]), int(tally["run"][i]), rule) for i in range(n))
    tail_f, tail_t = expected_verdicts(calls[(n - 300) * L:], offsets[n - 300:] - offsets[n - 300], times[n - 300:], rule)
    assert np.array_equal(filt[n - 300:], tail_f) and np.array_equal(tally_array(tally)[n - 300:], tail_t)
    assert 1000 < int(filt.sum()) < int(judged.sum()) - 1000 and not filt[~judged].any()


def test_refusals_name_their_cause(wa, g1_ct, g1_all):
    import torch
    dev = torch.device("cuda", 0)
    L = wa.lib()
    EINVAL = wa.WALT_EINVAL
    calls = np.frombuffer(b"HxH.HHh" * 3, dtype=np.uint8).copy()
    off = np.array([0, 21], dtype=np.uint64)
    rec = records([1])
    rule = wa.nonconv_rule(3)
    bad_rule = wa.nonconv_rule(0, 0, 101, 0)
    filt = np.zeros(2, dtype=np.uint8)
    h = g1_ct.handle
    host = [((None, calls.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, rule.ctypes.data, filt.ctypes.data, 1, None), "null index"),
            ((h, calls.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, None, filt.ctypes.data, 1, None), "null rule"),
            ((h, calls.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, bad_rule.ctypes.data, filt.ctypes.data, 1, None), "min_percent 101"),
            ((h, calls.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 12, rule.ctypes.data, filt.ctypes.data, 1, None), "stride 12"),
            ((h, calls.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 18, rule.ctypes.data, filt.ctypes.data, 1, None), "stride 18"),
            ((h, calls.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, rule.ctypes.data, filt.ctypes.data, 0, None), "filt stride 0"),
            ((h, calls.ctypes.data, None, 1, rec.ctypes.data, 16, rule.ctypes.data, filt.ctypes.data, 1, None), "null"),
            ((h, calls.ctypes.data, off.ctypes.data, 1, None, 16, rule.ctypes.data, filt.ctypes.data, 1, None), "null"),
            ((h, calls.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, rule.ctypes.data, None, 1, None), "null"),
            ((h, None, off.ctypes.data, 1, rec.ctypes.data, 16, rule.ctypes.data, filt.ctypes.data, 1, None), "null"),
            ((h, calls.ctypes.data, off[::-1].copy().ctypes.data, 1, rec.ctypes.data, 16, rule.ctypes.data, filt.ctypes.data, 1, None), "non-decreasing")]
    for args, word in host:
        assert L.walt_nonconv_batch(*args) == EINVAL, word
        msg = L.walt_last_error().decode()
        assert "walt_nonconv_batch:" in msg and word in msg, (word, msg)
    keep, d_calls, d_off, d_rec, _ = to_device(torch, dev, calls, off, rec, 0)
    d_filt = torch.zeros(8, dtype=torch.uint8, device=dev)
    d_tally = torch.zeros(8, dtype=torch.int64, device=dev)
    dc, do, dr, df, dt = d_calls, d_off.data_ptr(), d_rec.data_ptr(), d_filt.data_ptr(), d_tally.data_ptr()
    device = [((None, dc, do, 1, dr, 16, rule.ctypes.data, df, 1, dt, None), "null index"),
              ((h, dc, do, 1, dr, 16, None, df, 1, dt, None), "null rule"),
              ((h, dc, do, 1, dr, 16, bad_rule.ctypes.data, df, 1, dt, None), "min_percent 101"),
              ((h, dc, do, 1, dr, 8, rule.ctypes.data, df, 1, dt, None), "stride 8"),
              ((h, dc, do, 1, dr, 16, rule.ctypes.data, df, 0, dt, None), "filt stride 0"),
              ((h, None, do, 1, dr, 16, rule.ctypes.data, df, 1, dt, None), "null"),
              ((h, dc, None, 1, dr, 16, rule.ctypes.data, df, 1, dt, None), "null"),
              ((h, dc, do, 1, None, 16, rule.ctypes.data, df, 1, dt, None), "null"),
              ((h, dc, do, 1, dr, 16, rule.ctypes.data, None, 1, dt, None), "null"),
              ((h, dc, do + 4, 1, dr, 16, rule.ctypes.data, df, 1, dt, None), "aligned"),
              ((h, dc, do, 1, dr + 2, 16, rule.ctypes.data, df, 1, dt, None), "aligned"),
              ((h, dc, do, 1, dr, 16, rule.ctypes.data, df, 1, dt + 4, None), "aligned")]
    for args, word in device:
        assert L.walt_nonconv_batch_device(*args) == EINVAL, word
        msg = L.walt_last_error().decode()
        assert "walt_nonconv_batch_device:" in msg and word in msg, (word, msg)
    torch.cuda.synchronize()
    assert not d_filt.cpu().numpy().any() and not d_tally.cpu().numpy().any()
    # the pair rule
    pairs = np.zeros(1, dtype=wa.pair_result_dtype)
    for args, word in (((None, pairs.ctypes.data, 1, filt.ctypes.data), "null index"), ((h, None, 1, filt.ctypes.data), "null"),
                       ((h, pairs.ctypes.data, 1, None), "null")):
        assert L.walt_nonconv_pairs_batch(*args) == EINVAL and "walt_nonconv_pairs_batch:" in L.walt_last_error().decode(), word
        assert word in L.walt_last_error().decode()
    for args, word in (((None, dr, 1, df, None), "null index"), ((h, None, 1, df, None), "null"), ((h, dr, 1, None, None), "null"),
                       ((h, dr + 2, 1, df, None), "aligned")):
        assert L.walt_nonconv_pairs_batch_device(*args) == EINVAL and "walt_nonconv_pairs_batch_device:" in L.walt_last_error().decode(), word
        assert word in L.walt_last_error().decode()
    # calling and judging in one step: what the calling call refuses, what the rule's forms refuse, and calls to judge
    bases = np.frombuffer(b"ACGTTGCATTGACCGTAGCAT", dtype=np.uint8).copy()
    for idx, kw, word in ((g1_ct, {}, "holds no reference"), (g1_all, dict(rule=bad_rule), "min_percent 101"),
                          (g1_all, dict(conv="X"), "neither 'T' nor 'A'")):
        with pytest.raises(wa.WaltError) as ei:
            idx.meth_nonconv_batch(bases, off, rec, kw.get("rule", rule), conv=kw.get("conv", "T"))
        assert ei.value.code == EINVAL and word in str(ei.value) and "walt_meth_nonconv_batch:" in str(ei.value), word
    gh = g1_all.handle
    assert L.walt_meth_nonconv_batch(gh, bases.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, None, 1, ord("T"), None, None,
                                     rule.ctypes.data, None, 1, None) == EINVAL and "null filt" in L.walt_last_error().decode()
    assert L.walt_meth_nonconv_batch(gh, bases.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, None, 1, ord("T"), None, None,
                                     None, filt.ctypes.data, 1, None) == EINVAL and "null rule" in L.walt_last_error().decode()
    d_bases = torch.from_numpy(bases).to(dev)
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_nonconv_batch_device(d_bases.data_ptr(), do, 1, dr, rule, None, df)
    assert ei.value.code == EINVAL and "d_calls" in str(ei.value) and "made from the calls" in str(ei.value)
    assert "walt_meth_nonconv_batch_device:" in str(ei.value)
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_nonconv_batch_device(d_bases.data_ptr(), do, 1, dr, rule, dc, df, d_tally=dt + 4)
    assert ei.value.code == EINVAL and "tally" in str(ei.value)
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_nonconv_batch_device(d_bases.data_ptr(), do, 1, dr, rule, dc, df, filt_stride=0)
    assert ei.value.code == EINVAL and "filt stride 0" in str(ei.value)
    torch.cuda.synchronize()
    assert not d_filt.cpu().numpy().any()


# ---------------------------------------------------------------------------
# 2. the pair rule
# ---------------------------------------------------------------------------
def test_pair_rule_on_hand_made_pairs(wa, g1_ct):
    import torch
    dev = torch.device("cuda", 0)
    rows = [(bt, a, b) for bt in (0, 1, 2, 3) for a in (0, 1) for b in (0, 1)]
    rows = rows * 40 + [(1, 1, 0)]  # more than one block's worth of lanes is not needed: several wavefronts, an odd count
    pairs = np.zeros(len(rows), dtype=wa.pair_result_dtype)
    pairs["best_times"] = [r[0] for r in rows]
    filt = np.array([[r[1], r[2]] for r in rows], dtype=np.uint8)
    want = pair_rule(filt, pairs["best_times"])
    by_hand = {(1, 1, 0): (1, 1), (1, 0, 1): (1, 1), (1, 0, 0): (0, 0), (1, 1, 1): (1, 1), (0, 1, 0): (1, 0), (2, 0, 1): (0, 1), (3, 1, 0): (1, 0)}
    for i, r in enumerate(rows):
        assert tuple(want[i]) == by_hand.get(r, (r[1], r[2])), r
    got = g1_ct.nonconv_pairs(pairs, filt.copy())
    assert np.array_equal(got, want)
    flat = g1_ct.nonconv_pairs(pairs, filt.reshape(-1).copy())
    assert np.array_equal(flat.reshape(-1, 2), want)
    assert g1_ct.nonconv_pairs(pairs[:0], np.zeros(0, dtype=np.uint8)).size == 0
    stream = torch.cuda.Stream(device=dev)
    d_pairs = torch.from_numpy(pairs.view(np.uint8).reshape(-1, 64)).to(dev)
    d_filt = torch.from_numpy(np.concatenate([filt.reshape(-1), np.full(5, 7, dtype=np.uint8)])).to(dev)
    torch.cuda.synchronize()
    g1_ct.nonconv_pairs_device(d_pairs.data_ptr(), len(rows), d_filt.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    out = d_filt.cpu().numpy()
    assert np.array_equal(out[:-5].reshape(-1, 2), want) and (out[-5:] == 7).all()
    g1_ct.nonconv_pairs_device(None, 0, None)


# ---------------------------------------------------------------------------
# 3. calling and judging in one step, on the golden libraries
# ---------------------------------------------------------------------------
def golden_case(g1_all, case):
    """-> list of (seqs, records (a strided view for pairs), conv) of a golden library mapped through the binding"""
    import walt_amd
    from test_gpu_meth import cli_records_se, load
    if case in ("se_ct", "se_ga"):
        _, seqs, _ = load(case + ".fastq")
        recs, conv = cli_records_se(g1_all, seqs, "A" if case == "se_ga" else "T")
        return [(seqs, recs, conv)]
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    res, _ = g1_all.map_pe_batch(*walt_amd.pack_reads(s1), *walt_amd.pack_reads(s2))
    return [(s1, res["m1"], "T"), (s2, res["m2"], "A")]


@pytest.mark.parametrize("case", ["se_ct", "se_ga", "pe"])
def test_meth_nonconv_batch_on_the_golden_libraries(wa, g1, g1_all, case):
    import torch
    from test_gpu_meth import expected_batch
    db, _ = g1
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for seqs, recs, conv in golden_case(g1_all, case):
        bases, offs = wa.pack_reads(seqs)
        want_calls = calls_list_to_array(expected_batch(db, seqs, recs, conv)[0])
        plain = g1_all.meth_call_batch(bases, offs, recs, conv, want_counts=False, want_stats=False)[0]
        assert plain.tobytes() == want_calls.tobytes()
        n = len(seqs)
        for rule in ((3, 0, 0, 0), (0, 2, 0, 0), (0, 0, 15, 5)):
            want_f, want_t = expected_verdicts(want_calls, offs, recs["times"], rule)
            assert int(want_f.sum()) >= 20 and int((recs["times"] == 1).sum()) - int(want_f.sum()) >= 20
            filt, tally, calls = g1_all.meth_nonconv_batch(bases, offs, recs, wa.nonconv_rule(*rule), conv, want_calls=True)
            assert np.array_equal(filt, want_f) and np.array_equal(tally_array(tally), want_t), (case, rule)
            assert calls.tobytes() == plain.tobytes()
            filt, tally, calls = g1_all.meth_nonconv_batch(bases, offs, recs, wa.nonconv_rule(*rule), conv, want_tally=False)
            assert np.array_equal(filt, want_f) and tally is None and calls is None
        # the device form on a stream of its own: records in place (stride 16 or 64), the calls at an odd address
        rule = (0, 2, 15, 5)
        want_f, want_t = expected_verdicts(want_calls, offs, recs["times"], rule)
        stride = recs.strides[0]
        raw = np.zeros(n * stride, dtype=np.uint8)
        raw.reshape(n, stride)[:, :16] = np.ascontiguousarray(recs).view(np.uint8).reshape(n, 16)
        d_rec = torch.from_numpy(raw).to(dev)
        d_bases = torch.from_numpy(bases).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_calls = torch.full((bases.size + 48,), 0x23, dtype=torch.uint8, device=dev)
        d_filt = torch.full((2 * n + 1,), 7, dtype=torch.uint8, device=dev)
        d_tally = torch.zeros((n, 4), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        g1_all.meth_nonconv_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_rec.data_ptr(), wa.nonconv_rule(*rule),
                                         d_calls.data_ptr() + 3, d_filt.data_ptr() + 1, record_stride=stride, conversion=conv,
                                         filt_stride=2, d_tally=d_tally.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        got_calls = d_calls.cpu().numpy()
        assert got_calls[3:3 + bases.size].tobytes() == plain.tobytes() and (got_calls[:3] == 0x23).all() and (got_calls[3 + bases.size:] == 0x23).all()
        f = d_filt.cpu().numpy()
        assert np.array_equal(f[1::2], want_f) and (f[0::2] == 7).all()
        assert np.array_equal(d_tally.cpu().numpy().view(np.uint16)[:, :3].astype(np.int64), want_t)


def test_call_len_bounds_the_verdict_and_nothing_else_does(wa, g1, g1_all):
    """the verdict is made from the whole read up to call_len"""
    from test_gpu_meth import expected_batch
    db, _ = g1
    (seqs, recs, conv), = golden_case(g1_all, "se_ct")
    bases, offs = wa.pack_reads(seqs)
    rng = random.Random(4)
    call_len = np.array([rng.choice([len(s), len(s), len(s) // 2, 10, 0]) for s in seqs], dtype=np.uint32)
    want_calls = calls_list_to_array(expected_batch(db, seqs, recs, conv, call_len)[0])
    rule = (2, 0, 0, 0)
    want_f, want_t = expected_verdicts(want_calls, offs, recs["times"], rule)
    full_f, _ = expected_verdicts(calls_list_to_array(expected_batch(db, seqs, recs, conv)[0]), offs, recs["times"], rule)
    assert int(want_f.sum()) >= 20 and int(full_f.sum()) - int(want_f.sum()) >= 20
    filt, tally, _ = g1_all.meth_nonconv_batch(bases, offs, recs, wa.nonconv_rule(*rule), conv, call_len=call_len)
    assert np.array_equal(filt, want_f) and np.array_equal(tally_array(tally), want_t)


# ---------------------------------------------------------------------------
# 4. command line
# ---------------------------------------------------------------------------
def run_walt(args, binary=WALT_BIN, timeout=600):
    pr = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert pr.returncode == 0, pr.stdout[-2000:]
    return pr.stdout


def sam_flags(path):
    return [int(l.split("\t")[1]) for l in open(path) if not l.startswith("@")]


def sam_without_0x200(path):
    out = []
    for l in open(path):
        if not l.startswith("@"):
            p = l.split("\t")
            p[1] = str(int(p[1]) & ~0x200)
            l = "\t".join(p)
        out.append(l)
    return out


def loaded(fq, adaptor=""):
    seqs = []
    for _, sq, _ in refio.load_fastq_batches(fq, 10 ** 7, adaptor):
        seqs += sq
    return seqs


def write_mixed(scratch):
    from test_gpu_rpbat import mixed_library
    names, seqs, scores = mixed_library()
    fq = os.path.join(scratch, "nonconv_mixed.fastq")
    if not os.path.exists(fq):
        with open(fq, "w") as f:
            for nm, s, q in zip(names, seqs, scores):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
    return fq


def mode_library(wa, g1_all, scratch, mode):
    """-> (the run's read options, [(seqs, records, conv)] in the USER's order: one part for single-end, two for pairs,
    the pair records in the user's order or None)"""
    from test_gpu_meth import cli_records_se, load
    from test_gpu_overlap import cli_library
    if mode in ("r", "A", "R"):
        fq = write_mixed(scratch) if mode == "R" else os.path.join(refio.GOLDEN, "se_ga.fastq" if mode == "A" else "se_ct.fastq")
        seqs = loaded(fq)
        recs, conv = cli_records_se(g1_all, seqs, mode if mode != "r" else "T")
        return ["-r", fq] + ({"A": ["-A"], "R": ["-R"]}.get(mode, [])), [(seqs, recs, conv)], None
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    u1, u2, res, cv1, cv2 = cli_library(g1_all, mode, s1, s2)
    reads = ["-1", f2, "-2", f1, "-P"] if mode == "P" else ["-1", f1, "-2", f2] + (["-RP"] if mode == "RP" else [])
    return reads, [(u1, res["m1"], cv1), (u2, res["m2"], cv2)], res


def restated_verdicts(wa, g1_all, parts, res, rule, call_lens=None):
    """the restatement over the binding's calls: -> filt [n, parts] in the user's order, the pair rule applied"""
    cols = []
    for k, (seqs, recs, conv) in enumerate(parts):
        bases, offs = wa.pack_reads(seqs)
        calls = g1_all.meth_call_batch(bases, offs, recs, conv, None if call_lens is None else call_lens[k], want_counts=False,
                                       want_stats=False)[0]
        cols.append(expected_verdicts(calls, offs, recs["times"], rule)[0])
    filt = np.stack(cols, axis=1)
    return pair_rule(filt, res["best_times"]) if res is not None else filt


def expected_outputs(wa, g1, g1_all, parts, filt, dup=None, call_lens=None, excl=None, trims=None, heads=None):
    """the binding's calling call with the verdicts (ORed with the duplicates' bytes) as skip bytes -> the texts of
    <out>.methstats (its blocks), <out>.methcounts and <out>.mbias"""
    from test_gpu_mbias import block_text
    from test_gpu_meth import methstats_text
    from test_gpu_pileup import counts_text
    db, _ = g1
    pile = g1_all.pileup()
    mb = wa.MBias(0, len(parts))
    blocks = []
    for k, (seqs, recs, conv) in enumerate(parts):
        bases, offs = wa.pack_reads(seqs)
        skip = np.ascontiguousarray(filt[:, k] | (dup[:, k] if dup is not None else 0)).astype(np.uint8)
        t5, t3 = trims[k] if trims else (0, 0)
        st = pile.add_batch(bases, offs, recs, conv, None if call_lens is None else call_lens[k], want_calls=False, want_counts=False,
                            skip=skip, excl=excl if (excl is not None and k == 1) else None, mbias=mb, mbias_table=k, trim5=t5, trim3=t3)[2]
        blocks.append(((heads or [None, None])[k] if len(parts) == 2 else None, {f: st[f][0] for f in ("reads", "meth", "unmeth")}))
    sites, _ = pile.extract()
    bias = "".join(("" if len(parts) == 1 else "mate%d\n" % (k + 1)) + block_text(mb.read(k)) for k in range(len(parts)))
    pile.close()
    mb.close()
    return methstats_text(blocks), counts_text(db, sites), bias


_plain_runs = {}


def plain_run(scratch, path, mode, reads):
    """the run without the option, once per mode: SAM with -M -MC -MB, and the .mr file"""
    if mode not in _plain_runs:
        out = os.path.join(scratch, "nonconv_plain_" + mode)
        run_walt(["-i", path] + reads + ["-o", out, "-a", "-u", "-sam", "-M", "-MC", "-MB"])
        run_walt(["-i", path] + reads + ["-o", out + ".mr", "-a", "-u", "-M"])
        _plain_runs[mode] = out
    return _plain_runs[mode]


def mr_owners(parts, res):
    """(read, part) of every line of the main .mr file, in file order"""
    if res is None:
        return [(j, 0) for j in range(len(parts[0][0])) if int(parts[0][1]["times"][j]) == 1]
    owners = []
    for j in range(res.size):
        if int(res["best_times"][j]) == 1:
            owners.append((j, 0))
        else:
            owners += [(j, k) for k in (0, 1) if int(res["m%d" % (k + 1)]["times"][j]) == 1]
    return owners


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", ["r", "A", "R", "pe", "P", "RP"])
def test_cli_modes_and_settings(wa, g1, g1_all, scratch, mode, setting):
    _, path = g1
    opts, rule = SETTINGS[setting]
    reads, parts, res = mode_library(wa, g1_all, scratch, mode)
    filt = restated_verdicts(wa, g1_all, parts, res, rule)
    records_n, filtered_n = se_outcome(parts[0][1], filt[:, 0]) if res is None else pe_outcome(res, filt)
    # the condition on the inputs, on the restatement alone: both outcomes occur
    assert filtered_n >= 20 and records_n - filtered_n >= 20, (mode, setting, records_n, filtered_n)
    plain = plain_run(scratch, path, mode, reads)
    out = os.path.join(scratch, "nonconv_cli_%s_%s" % (mode, setting))
    run_walt(["-i", path] + reads + ["-o", out, "-a", "-u", "-sam", "-M", "-MC", "-MB"] + opts)
    # 0x200 on exactly the filtered records' lines, and nothing else changes on any line
    flags = sam_flags(out)
    assert len(flags) == filt.size and [(f >> 9) & 1 for f in flags] == filt.reshape(-1).tolist()
    assert sam_without_0x200(out) == open(plain).readlines()
    assert "XM:Z:" in open(out).read()
    assert open(out + ".mapstats").read() == open(plain + ".mapstats").read()
    # the counts leave the filtered records out
    stats, counts, bias = expected_outputs(wa, g1, g1_all, parts, filt, heads=["mate1", "mate2"])
    assert open(out + ".methstats").read() == stats and open(out + ".methstats").read() != open(plain + ".methstats").read()
    assert open(out + ".methcounts").read() == counts and open(out + ".mbias").read() == bias
    assert open(out + ".filterstats").read() == filterstats_text(records_n, filtered_n, rule)
    assert not os.path.exists(plain + ".filterstats") and not os.path.exists(out + ".dupstats")
    # .mr lacks exactly the filtered records' lines (a filtered pair's one fragment line)
    run_walt(["-i", path] + reads + ["-o", out + ".mr", "-a", "-u", "-M"] + opts)
    owners = mr_owners(parts, res)
    lines = open(plain + ".mr").readlines()
    assert len(lines) == len(owners)
    assert open(out + ".mr").readlines() == [l for l, (j, k) in zip(lines, owners) if not filt[j, k]]
    for sfx in (".mapstats",) + (("_ambiguous", "_unmapped") if res is None else ("_1_ambiguous", "_2_unmapped")):
        assert open(out + ".mr" + sfx).read() == open(plain + ".mr" + sfx).read(), sfx
    assert open(out + ".mr.methstats").read() == stats and open(out + ".mr.filterstats").read() == filterstats_text(records_n, filtered_n, rule)


def test_cli_beside_duplicates_and_two_shares(wa, g1, g1_all, scratch):
    """-F beside -D: duplicates are judged like any read, a filtered read still enters the duplicate set; .dupstats is the
    run's without the option; the verdict does not depend on -N or -g"""
    from test_dedup_cpu import DupRule, expect_single
    from test_gpu_dedup import doubled, dupstats_text
    from test_gpu_meth import cli_records_se
    _, path = g1
    (_, fq), = doubled(scratch, "nonconv", [os.path.join(refio.GOLDEN, "se_ct.fastq")])
    seqs = loaded(fq)
    recs, conv = cli_records_se(g1_all, seqs, "T")
    dup = expect_single(DupRule(), recs, conv)
    opts, rule = SETTINGS["F3"]
    parts = [(seqs, recs, conv)]
    filt = restated_verdicts(wa, g1_all, parts, None, rule)
    records_n, filtered_n = se_outcome(recs, filt[:, 0], dup)
    assert filtered_n >= 20 and records_n - filtered_n >= 20 and int((dup & filt[:, 0]).sum()) >= 20
    out = os.path.join(scratch, "nonconv_cli_D")
    run_walt(["-i", path, "-r", fq, "-o", out, "-a", "-u", "-sam", "-M", "-MC", "-MB", "-D"] + opts)
    flags = sam_flags(out)
    assert [(f >> 9) & 1 for f in flags] == filt[:, 0].tolist() and [(f >> 10) & 1 for f in flags] == dup.tolist()
    stats, counts, bias = expected_outputs(wa, g1, g1_all, parts, filt, dup=dup.reshape(-1, 1))
    assert open(out + ".methstats").read() == stats and open(out + ".methcounts").read() == counts and open(out + ".mbias").read() == bias
    assert open(out + ".filterstats").read() == filterstats_text(records_n, filtered_n, rule)
    assert open(out + ".dupstats").read() == dupstats_text(int((recs["times"] == 1).sum()), int(dup.sum()))
    for name, extra in (("N64", ["-N", "64"]), ("g", ["-g", "0,1" if wa.device_count() >= 2 else "0,0"])):
        run_walt(["-i", path, "-r", fq, "-o", out + name, "-a", "-u", "-sam", "-M", "-MC", "-MB", "-D"] + opts + extra)
        for sfx in ("", ".mapstats", ".methstats", ".methcounts", ".mbias", ".dupstats", ".filterstats"):
            assert open(out + name + sfx, "rb").read() == open(out + sfx, "rb").read(), (name, sfx)
    # .mr: neither the duplicates' nor the filtered records' lines
    run_walt(["-i", path, "-r", fq, "-o", out + ".mr", "-a", "-u", "-MC", "-D", "--filter-non-conversion", "3"])
    run_walt(["-i", path, "-r", fq, "-o", out + "_plain.mr", "-a", "-u"])
    owners = mr_owners(parts, None)
    lines = open(out + "_plain.mr").readlines()
    assert open(out + ".mr").readlines() == [l for l, (j, _) in zip(lines, owners) if not filt[j, 0] and not dup[j]]
    assert open(out + ".mr.methcounts").read() == counts


def test_cli_beside_overlap_ignored_ends_and_the_pile_up_alone(wa, g1, g1_all, scratch):
    """-FC beside -NO and the -I options, with -MC alone (no -M): the verdict is made from the whole read, whatever the
    other options take out of the counts"""
    _, path = g1
    opts, rule = SETTINGS["FC2"]
    reads, parts, res = mode_library(wa, g1_all, scratch, "pe")
    filt = restated_verdicts(wa, g1_all, parts, res, rule)
    records_n, filtered_n = pe_outcome(res, filt)
    assert filtered_n >= 20 and records_n - filtered_n >= 20
    trims = [(5, 3), (7, 2)]
    _, o1 = wa.pack_reads(parts[0][0])
    _, o2 = wa.pack_reads(parts[1][0])
    excl, _ = g1_all.pair_overlap(res, o1, o2, trim1=trims[0], trim2=trims[1])
    stats, counts, bias = expected_outputs(wa, g1, g1_all, parts, filt, excl=excl, trims=trims, heads=["mate1", "mate2"])
    out = os.path.join(scratch, "nonconv_cli_NO_I")
    run_walt(["-i", path] + reads + ["-o", out, "-a", "-u", "-MC", "-MB", "-NO", "-I5", "5", "-I3", "3", "-I5R2", "7", "-I3R2", "2",
                                     "--filter-consecutive", "2"])
    assert open(out + ".methcounts").read() == counts and open(out + ".mbias").read() == bias
    assert open(out + ".filterstats").read() == filterstats_text(records_n, filtered_n, rule)
    assert not os.path.exists(out + ".methstats")
    run_walt(["-i", path] + reads + ["-o", out + "_M", "-a", "-u", "-M", "-NO", "-I5", "5", "-I3", "3", "-I5R2", "7", "-I3R2", "2", "-v"] + opts)
    text = open(out + "_M.methstats").read()
    assert text.startswith(stats) and "overlap\t" in text and text.endswith("ignore\t5\t3\t7\t2\n")


def test_cli_beside_clipping(wa, g1, g1_all, scratch):
    """-FP -FM beside -C: the verdict is made from the read up to its clip point"""
    from test_gpu_meth import cli_records_se, clip_point
    _, path = g1
    args = refio.golden_meta()["cases"]["se_clip_sam_au"]["args"]
    adaptor = args[args.index("-C") + 1]
    fq = os.path.join(refio.GOLDEN, "se_clip.fastq")
    seqs = loaded(fq, adaptor)
    raw = [l.rstrip(b"\n") for l in open(fq, "rb").readlines()[1::4]]
    call_len = np.array([clip_point(adaptor.encode(), bytearray(r)) for r in raw], dtype=np.uint32)
    recs, conv = cli_records_se(g1_all, seqs, "T")
    parts = [(seqs, recs, conv)]
    rule = (0, 0, 10, 3)
    filt = restated_verdicts(wa, g1_all, parts, None, rule, [call_len])
    records_n, filtered_n = se_outcome(recs, filt[:, 0])
    assert filtered_n >= 20 and records_n - filtered_n >= 20
    out = os.path.join(scratch, "nonconv_cli_C")
    text = run_walt(["-i", path, "-r", fq, "-o", out, "-a", "-u", "-sam", "-M", "-MC", "-C", adaptor, "-filter-percent", "10",
                     "-filter-min-count", "3", "-v"])
    assert [(f >> 9) & 1 for f in sam_flags(out)] == filt[:, 0].tolist()
    stats, counts, _ = expected_outputs(wa, g1, g1_all, parts, filt, call_lens=[call_len])
    assert open(out + ".methstats").read() == stats and open(out + ".methcounts").read() == counts
    assert open(out + ".filterstats").read() == filterstats_text(records_n, filtered_n, rule)
    assert filterstats_text(records_n, filtered_n, rule) in text  # -v prints the same lines


@pytest.mark.parametrize("pattern", [5, 7])
def test_cli_seed_patterns_5_and_7(wa, scratch, pattern):
    binary = os.path.join(refio.ROOT, "walt_amd", "bin", "walt_sp%d" % pattern)
    path = os.path.join(scratch, "nonconv_g1_sp%d.dbindex" % pattern)
    old = wa.PATTERN
    wa.set_pattern(pattern)
    try:
        wa.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
        idx = wa.Index.open(path, device=0, strands=wa.STRANDS_CT | wa.WITH_REFERENCE)
    finally:
        wa.set_pattern(old)
    fq = os.path.join(refio.GOLDEN, "sp_se_ct.fastq")
    seqs = loaded(fq)
    bases, offs = wa.pack_reads(seqs)
    recs, _ = idx.map_se_batch(bases, offs)
    calls = idx.meth_call_batch(bases, offs, recs, "T", want_counts=False, want_stats=False)[0]
    opts, rule = SETTINGS["F3"]
    filt, _ = expected_verdicts(calls, offs, recs["times"], rule)
    records_n, filtered_n = se_outcome(recs, filt)
    assert filtered_n >= 20 and records_n - filtered_n >= 20
    got, _, _ = idx.meth_nonconv_batch(bases, offs, recs, wa.nonconv_rule(*rule), "T")
    idx.close()
    assert np.array_equal(got, filt)
    out = os.path.join(scratch, "nonconv_cli_sp%d" % pattern)
    run_walt(["-i", path, "-r", fq, "-o", out, "-a", "-u", "-sam", "-M"] + opts, binary=binary)
    assert [(f >> 9) & 1 for f in sam_flags(out)] == filt.tolist()
    assert open(out + ".filterstats").read() == filterstats_text(records_n, filtered_n, rule)


def test_nonconv_soak_slice():
    """a few random genomes and libraries through tools/soak.py's slice"""
    import sys
    sys.path.insert(0, os.path.join(refio.ROOT, "tools"))
    import soak
    line = soak.run_soak_nonconv(range(1, 4), pattern=3)
    assert line.startswith("soak ok: nonconv")
