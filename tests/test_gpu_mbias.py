"""Methylation bias by read position on the GPU (include/walt_amd.h, "methylation bias by read position"): walt_mbias_*
through walt_amd.MBias, the composition with the calling (mbias= on Index.meth_call_batch / Pileup.add_batch and their
device forms) and bin/walt -MB, all against one numpy restatement of the contract (expected_table below, which never
uses the code under test)."""
import os
import random
import subprocess

import numpy as np
import pytest

import refio

SHAPE = (4, 2, 1024)
CONTEXTS = ("CpG", "CHG", "CHH", "unknown")
# call letter -> (context, m): z / Z CpG, x / X CHG, h / H CHH, u / U unknown; upper case is methylated (m = 0)
LETTERS = {ord(ch): (k, 0 if ch.isupper() else 1) for k, pair in enumerate(("zZ", "xX", "hH", "uU")) for ch in pair}
LENGTHS = (1, 15, 16, 17, 31, 127, 128, 129, 1024)
WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def expected_table(calls, offsets, times, skip=None, base=None, into=None):
    """calls: uint8 array whose element 0 is byte `base` (default offsets[0]) of what the offsets index.  A record adds
    when times == 1, its skip byte (if any) is 0 and it has at most 1024 calls."""
    calls = np.asarray(calls, dtype=np.uint8)
    offsets = [int(v) for v in offsets]
    base = offsets[0] if base is None else base
    t = np.zeros(SHAPE, dtype=np.uint64) if into is None else into
    for r in range(len(offsets) - 1):
        lo, hi = offsets[r] - base, offsets[r + 1] - base
        if int(times[r]) != 1 or (skip is not None and int(skip[r]) != 0) or hi - lo > 1024 or hi <= lo:
            continue
        seg = calls[lo:hi]
        for b, (c, m) in LETTERS.items():
            t[c, m, np.nonzero(seg == b)[0]] += np.uint64(1)  # (a position holds one letter: the indices are distinct)
    return t


def block_text(table):
    """one block of <out>.mbias"""
    table = np.asarray(table)
    nz = np.nonzero(table.reshape(8, 1024).any(axis=0))[0]
    L = int(nz[-1]) + 1 if nz.size else 0
    out = []
    for c, name in enumerate(CONTEXTS):
        for i in range(L):
            m, u = int(table[c, 0, i]), int(table[c, 1, i])
            out.append("%s\t%d\t%d\t%d\t%s\n" % (name, i + 1, m, u, "%.6f" % (m / (m + u)) if m + u else "NA"))
    return "".join(out)


def parse_mbias(text):
    """-> list of (head or None, table) in file order; a block ends where the position runs backwards within a context
    that was already seen or a head line comes"""
    blocks, head, table, seen = [], None, None, None

    def close():
        nonlocal table
        if table is not None:
            blocks.append((head, table))
        table = None

    for line in text.splitlines():
        parts = line.split("\t")
        if len(parts) == 1:
            close()
            head, table, seen = parts[0], np.zeros(SHAPE, dtype=np.uint64), set()
            continue
        ctx, pos, m, u, level = parts
        c, i = CONTEXTS.index(ctx), int(pos) - 1
        if table is None or (c, i) in seen:
            close()
            head = None if table is None and not blocks else head
            table, seen = np.zeros(SHAPE, dtype=np.uint64), set()
        seen.add((c, i))
        table[c, 0, i], table[c, 1, i] = int(m), int(u)
        assert level == ("%.6f" % (int(m) / (int(m) + int(u))) if int(m) + int(u) else "NA"), line
    close()
    return blocks


def methstats_counts(text):
    """-> list of (meth[4], unmeth[4]) per block of <out>.methstats"""
    out = []
    for line in text.splitlines():
        p = line.split("\t")
        if p[0] == "reads":
            out.append((np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)))
        elif p[0] in CONTEXTS:
            out[-1][0][CONTEXTS.index(p[0])], out[-1][1][CONTEXTS.index(p[0])] = int(p[1]), int(p[2])
    return out


def column_sums(table):
    return table[:, 0, :].sum(axis=1), table[:, 1, :].sum(axis=1)


def random_calls(rng, n, dense=False):
    al = "zZxXhHuU" if dense else "zZxXhHuU" + "." * 24 + "ACGT#-"
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


# ---------------------------------------------------------------------------
# 1. hand-made batches
# ---------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


def hand_batch(rng, lens, dense=False):
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    return random_calls(rng, int(offsets[-1]), dense), offsets


def test_host_form_lengths_alignments_records_and_skip(wa):
    rng = random.Random(11)
    mb = wa.MBias(0, 2)
    assert mb.device_bytes == 2 * 8 * 65536 and mb.read(0).shape == SHAPE and mb.read(1).dtype == np.uint64
    # every length at every offset modulo 16 (each length follows reads of 0 .. 15 calls), times 0 / 1 / 2
    lens = []
    for L in LENGTHS:
        for lead in range(16):
            lens += [lead, L]
    lens += [40] * 5
    calls, offsets = hand_batch(rng, lens)
    times = [rng.choice([0, 1, 1, 1, 2]) for _ in lens]
    assert {0, 1, 2} <= set(times) and len(lens) % 32 != 0  # (32 reads per block: the last trip is partial)
    want = expected_table(calls, offsets, times)
    assert want[:, :, 1023].sum() > 0
    mb.add(calls, offsets, records(times))
    assert np.array_equal(mb.read(0), want) and mb.read(1).sum() == 0
    # offsets that do not start at 0; skip bytes at stride 2; records at stride 64; into table 1
    skip = np.full((len(lens), 2), 9, dtype=np.uint8)
    skip[:, 1] = [rng.choice([0, 0, 1, 200]) for _ in lens]
    want1 = expected_table(calls, offsets, times, skip[:, 1])
    assert 0 < want1.sum() < want.sum()
    mb.add(calls, offsets + np.uint64(12345), records(times, 64), skip=skip[:, 1], table=1)
    assert np.array_equal(mb.read(1), want1) and np.array_equal(mb.read(0), want)
    # n = 0 and n = 1
    mb.add(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), records([]))
    one = random_calls(rng, 37, True)
    mb.add(one, [0, 37], records([1]))
    want = expected_table(one, [0, 37], [1], into=want)
    assert np.array_equal(mb.read(0), want)
    # the host form rejects a read of 1025 calls, and adds nothing of that batch
    with pytest.raises(wa.WaltError) as ei:
        mb.add(random_calls(rng, 1025 + 10, True), [0, 1025, 1035], records([1, 1]))
    assert ei.value.code == wa.WALT_EINVAL and "1024" in str(ei.value)
    assert np.array_equal(mb.read(0), want)
    # refusals name their cause
    for kw, word in ((dict(table=2), "table 2"), (dict(table=8), "table 8")):
        with pytest.raises(wa.WaltError) as ei:
            mb.add(one, [0, 37], records([1]), **kw)
        assert ei.value.code == wa.WALT_EINVAL and word in str(ei.value)
    L = wa.lib()
    rec = records([1])
    off = np.array([0, 37], dtype=np.uint64)
    for args, word in (((mb.handle, 0, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 12, None, 1), "stride 12"),
                       ((mb.handle, 0, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 18, None, 1), "stride 18"),
                       ((mb.handle, 0, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, one.ctypes.data, 0), "skip stride 0"),
                       ((mb.handle, 0, one.ctypes.data, None, 1, rec.ctypes.data, 16, None, 1), "null"),
                       ((mb.handle, 0, one.ctypes.data, off.ctypes.data, 1, None, 16, None, 1), "null")):
        assert L.walt_mbias_batch(*args) == wa.WALT_EINVAL and word in L.walt_last_error().decode(), word
    mb.clear()
    assert mb.read(0).sum() == 0 and mb.read(1).sum() == 0
    mb.close()
    for tables in (0, 9):
        with pytest.raises(wa.WaltError) as ei:
            wa.MBias(0, tables)
        assert ei.value.code == wa.WALT_EINVAL
    with pytest.raises(wa.WaltError) as ei:
        wa.MBias(wa.device_count() + 3, 1)
    assert ei.value.code == wa.WALT_EINVAL


def to_device(torch, dev, calls, offsets, rec, shift=0, pad=64):
    """calls at a device address that is `shift` modulo 16, with '#'... no: with 'Z' around it (a slice that reads outside
    the reads shows in the table)"""
    d_raw = torch.full((calls.size + pad + 32,), ord("Z"), dtype=torch.uint8, device=dev)
    a = (-d_raw.data_ptr()) % 16 + shift
    d_raw[a:a + calls.size] = torch.from_numpy(np.ascontiguousarray(calls)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(dev)
    stride = rec.strides[0] if rec.size > 1 else rec.dtype.itemsize
    flat = np.zeros(max(rec.size, 1) * stride + 64, dtype=np.uint8)
    for i in range(rec.size):
        flat[i * stride:i * stride + 16] = np.frombuffer(rec[i].tobytes(), dtype=np.uint8)
    d_rec = torch.from_numpy(flat).to(dev)
    return d_raw, d_raw.data_ptr() + a, d_off, d_rec, stride


def test_device_form_alignments_strides_and_a_read_of_1025(wa):
    import torch
    rng = random.Random(12)
    dev = torch.device("cuda", 0)
    mb = wa.MBias(0, 1)
    stream = torch.cuda.Stream(device=dev)
    # a read of 1025 calls between two counted reads, among the lengths: it adds nothing, its neighbours everything
    lens = [100, 1025, 129, 16, 1024, 1025, 1025, 17, 0, 31]
    calls, offsets = hand_batch(rng, lens, dense=True)
    times = [1] * len(lens)
    want = expected_table(calls, offsets, times)
    assert int(want.sum()) == 100 + 129 + 16 + 1024 + 17 + 31
    for shift in (0, 1, 7, 15):
        for stride in (16, 64):
            rec = records(times, stride)
            keep, d_calls, d_off, d_rec, st = to_device(torch, dev, calls, offsets, rec, shift)
            assert st == stride
            torch.cuda.synchronize()
            mb.clear()
            mb.add_device(d_calls, d_off.data_ptr(), len(lens), d_rec.data_ptr(), stride, stream=stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(mb.read(), want), (shift, stride)
    # skip bytes at stride 2, times 0 / 1 / 2, sparse calls
    lens = [rng.choice(LENGTHS + (40, 100, 150)) for _ in range(333)]
    calls, offsets = hand_batch(rng, lens)
    times = [rng.choice([0, 1, 1, 1, 2]) for _ in lens]
    skip = np.full((len(lens), 2), 1, dtype=np.uint8)
    skip[:, 0] = [rng.choice([0, 0, 0, 3]) for _ in lens]
    keep, d_calls, d_off, d_rec, _ = to_device(torch, dev, calls, offsets, records(times), 5)
    d_skip = torch.from_numpy(skip).to(dev)
    torch.cuda.synchronize()
    mb.clear()
    mb.add_device(d_calls, d_off.data_ptr(), len(lens), d_rec.data_ptr(), 16, d_skip.data_ptr(), 2)
    assert np.array_equal(mb.read(), expected_table(calls, offsets, times, skip[:, 0]))
    # n = 0 with null arrays is fine; refusals
    mb.add_device(None, None, 0, None)
    for kw, word in ((dict(record_stride=8), "stride 8"), (dict(skip_stride=0, d_skip=d_skip.data_ptr()), "skip stride 0"),
                     (dict(table=1), "table 1")):
        args = dict(d_calls=d_calls, d_offsets=d_off.data_ptr(), n=len(lens), d_records=d_rec.data_ptr())
        args.update(kw)
        with pytest.raises(wa.WaltError) as ei:
            mb.add_device(**args)
        assert ei.value.code == wa.WALT_EINVAL and word in str(ei.value), word
    for args, word in (((d_calls, d_off.data_ptr() + 4, 1, d_rec.data_ptr()), "aligned"), ((d_calls, d_off.data_ptr(), 1, d_rec.data_ptr() + 2), "aligned"),
                       ((None, d_off.data_ptr(), 1, d_rec.data_ptr()), "null"), ((d_calls, None, 1, d_rec.data_ptr()), "null"),
                       ((d_calls, d_off.data_ptr(), 1, None), "null")):
        with pytest.raises(wa.WaltError) as ei:
            mb.add_device(*args)
        assert ei.value.code == wa.WALT_EINVAL and word in str(ei.value), word
    assert np.array_equal(mb.read(), expected_table(calls, offsets, times, skip[:, 0]))
    mb.close()


# ---------------------------------------------------------------------------
# 2. contention, the grid-stride loop, accumulation
# ---------------------------------------------------------------------------
def test_contention_whole_wavefronts_on_one_counter(wa):
    mb = wa.MBias(0, 2)
    n, L = 4096, 100
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    mb.add(np.full(n * L, ord("Z"), dtype=np.uint8), offsets, records([1] * n))
    got = mb.read(0)
    assert (got[0, 0, :L] == n).all() and got.sum() == n * L
    # the eight letters cycling by read: the reads of a wavefront hold different letters at the same position
    letters = np.frombuffer(b"ZzXxHhUu", dtype=np.uint8)
    calls = np.repeat(letters[np.arange(n) % 8], L)
    mb.add(calls, offsets, records([1] * n), table=1)
    got = mb.read(1)
    assert (got[:, :, :L] == n // 8).all() and got.sum() == n * L
    assert np.array_equal(got, expected_table(calls, offsets, [1] * n))
    mb.close()


def test_grid_stride_loop_more_reads_than_the_grid_takes_at_once(wa):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # a block of mbias.hip's kernel takes kBlock / kMbiasGroup = 256 / 8 reads per trip and at most kMbiasBlocksPerCu = 4
    # blocks per compute unit are launched: 8 per unit leaves room for a grid twice as large.  If those constants change,
    # change these with them, or the batch stops exceeding one trip of the grid.
    reads_per_block = 256 // 8
    n = 8 * cus * reads_per_block + 1237  # more than any grid of up to 8 blocks per compute unit takes in one trip
    L = 40
    rng = np.random.default_rng(5)
    al = np.frombuffer(b"zZxXhHuU" + b"." * 24, dtype=np.uint8)
    calls = al[rng.integers(0, al.size, size=n * L)]
    times = rng.integers(0, 3, size=n).astype(np.uint32)
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    # the restatement, vectorised over reads of one length (the same rule as expected_table)
    rows = calls.reshape(n, L)[times == 1]
    want = np.zeros(SHAPE, dtype=np.uint64)
    for b, (c, m) in LETTERS.items():
        want[c, m, :L] = (rows == b).sum(axis=0)
    small = expected_table(calls[:200 * L], offsets[:201], times[:200])
    rows200 = calls.reshape(n, L)[:200][times[:200] == 1]
    assert all(np.array_equal(small[c, m, :L], (rows200 == b).sum(axis=0)) for b, (c, m) in LETTERS.items())
    mb = wa.MBias(0, 1)
    rec = np.zeros(n, dtype=wa.best_match_dtype)
    rec["times"] = times
    mb.add(calls, offsets, rec)
    assert np.array_equal(mb.read(), want)
    mb.close()


def test_accumulation_across_calls_tables_and_streams(wa):
    import torch
    rng = random.Random(14)
    dev = torch.device("cuda", 0)
    mb = wa.MBias(0, 2)
    batches = []
    for k in range(3):
        lens = [rng.choice([36, 100, 150, 151]) for _ in range(500 + 37 * k)]
        calls, offsets = hand_batch(rng, lens)
        times = [rng.choice([0, 1, 1, 2]) for _ in lens]
        batches.append((calls, offsets, times))
    mb.add(batches[0][0], batches[0][1], records(batches[0][2]), table=0)
    mb.add(batches[1][0], batches[1][1], records(batches[1][2]), table=0)
    mb.add(batches[2][0], batches[2][1], records(batches[2][2]), table=1)
    want0 = expected_table(*batches[0])
    want0 = expected_table(*batches[1], into=want0)
    assert np.array_equal(mb.read(0), want0) and np.array_equal(mb.read(1), expected_table(*batches[2]))
    mb.clear()
    assert mb.read(0).sum() == 0 and mb.read(1).sum() == 0
    # two streams feed table 0 at the same time, several calls each
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    staged = [to_device(torch, dev, b[0], b[1], records(b[2]), shift=3 * k) for k, b in enumerate(batches[:2])]
    torch.cuda.synchronize()
    reps = 6
    for _ in range(reps):
        for k in range(2):
            _, d_calls, d_off, d_rec, _ = staged[k]
            mb.add_device(d_calls, d_off.data_ptr(), len(batches[k][2]), d_rec.data_ptr(), stream=streams[k].cuda_stream)
    for s in streams:
        s.synchronize()
    assert np.array_equal(mb.read(0), want0 * np.uint64(reps)) and mb.read(1).sum() == 0
    mb.close()


# ---------------------------------------------------------------------------
# 3. the composition with the calling
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "mbias_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    return refio.DbIndex(path), path


@pytest.fixture(scope="module")
def g1_all(g1):
    import walt_amd
    idx = walt_amd.Index.open(g1[1], device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def g1_pairs(g1_all):
    import walt_amd
    from test_gpu_meth import load
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    excl, _ = g1_all.pair_overlap(res, o1, o2)
    return (b1, o1, b2, o2), res, excl


def same_outputs(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.tobytes() == y.tobytes()


def stats_sums(stats):
    return stats["meth"][0].astype(np.uint64), stats["unmeth"][0].astype(np.uint64)


def test_composition_host_form(wa, g1_all, g1_pairs):
    (b1, o1, b2, o2), res, excl = g1_pairs
    n = res.size
    rng = np.random.default_rng(8)
    skip = (rng.integers(0, 4, size=(n, 2)) == 0).astype(np.uint8)
    assert (excl != 0).sum() >= 100
    mb = wa.MBias(0, 2)
    for with_pile in (False, True):
        for use_skip, use_excl in ((False, False), (True, False), (False, True), (True, True)):
            kw = dict(skip=skip[:, 1] if use_skip else None, excl=excl if use_excl else None)
            piles = [g1_all.pileup(), g1_all.pileup()] if with_pile else [None, None]
            call = [p.add_batch if p is not None else g1_all.meth_call_batch for p in piles]
            plain = call[0](b2, o2, res["m2"], "A", **kw)
            mb.clear()
            got = call[1](b2, o2, res["m2"], "A", mbias=mb, mbias_table=1, **kw)
            same_outputs(plain, got)
            if with_pile:
                s0, s1 = piles[0].extract(), piles[1].extract()
                assert s0[0].tobytes() == s1[0].tobytes() and s0[0].size > 1000 and np.array_equal(s0[1], s1[1])
                for p in piles:
                    p.close()
            table = mb.read(1)
            assert np.array_equal(table, expected_table(got[0], o2, res["m2"]["times"], kw["skip"])) and table.sum() > 1000
            m, u = column_sums(table)
            assert np.array_equal(m, stats_sums(got[2])[0]) and np.array_equal(u, stats_sums(got[2])[1])
            assert mb.read(0).sum() == 0
    # the caller's calls NULL: the host form allocates the device array for itself
    mb.clear()
    full = g1_all.meth_call_batch(b1, o1, res["m1"], "T")
    none = g1_all.meth_call_batch(b1, o1, res["m1"], "T", want_calls=False, want_counts=False, want_stats=False, mbias=mb)
    assert none == (None, None, None)
    assert np.array_equal(mb.read(0), expected_table(full[0], o1, res["m1"]["times"]))
    # refusals: a table the set has not
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_call_batch(b1, o1, res["m1"], "T", mbias=mb, mbias_table=2)
    assert ei.value.code == wa.WALT_EINVAL and "table 2" in str(ei.value)
    mb.close()


def test_composition_device_form(wa, g1_all, g1_pairs):
    import torch
    (b1, o1, b2, o2), res, excl = g1_pairs
    n = res.size
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    skip = (rng.integers(0, 4, size=n) == 0).astype(np.uint8)
    d_bases = torch.from_numpy(b2).to(dev)
    d_offs = torch.from_numpy(o2.view(np.int64)).to(dev)
    d_pairs = torch.from_numpy(res.view(np.uint8).reshape(n, 64)).to(dev)
    d_skip = torch.from_numpy(skip).to(dev)
    d_excl = torch.from_numpy(excl.view(np.int32)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    mb = wa.MBias(0, 1)
    total = int(o2[-1])
    for with_pile in (False, True):
        for use_skip, use_excl in ((False, False), (True, True)):
            outs = []
            for with_mb in (False, True):
                d_calls = torch.full((total + 48,), 0x23, dtype=torch.uint8, device=dev)
                d_counts = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
                d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
                pile = g1_all.pileup() if with_pile else None
                torch.cuda.synchronize()
                mb.clear()
                args = (d_bases.data_ptr(), d_offs.data_ptr(), n, d_pairs.data_ptr() + 16, 64, None, 1, "A", None,
                        d_calls.data_ptr() + 3, d_counts.data_ptr(), d_stats.data_ptr())
                kw = dict(stream=stream.cuda_stream, d_skip=d_skip.data_ptr() if use_skip else None, skip_stride=1,
                          d_excl=d_excl.data_ptr() if use_excl else None)
                if with_mb:
                    kw.update(mbias=mb, mbias_table=0)
                if pile is not None:
                    pile.add_batch_device(*args, **kw)
                else:
                    g1_all.meth_call_batch_device(*args, **kw)
                stream.synchronize()
                sites = pile.extract()[0].tobytes() if pile is not None else b""
                if pile is not None:
                    pile.close()
                outs.append((d_calls.cpu().numpy(), d_counts.cpu().numpy(), d_stats.cpu().numpy(), sites))
            for x, y in zip(outs[0], outs[1]):
                assert (x == y) if isinstance(x, bytes) else np.array_equal(x, y)
            calls = outs[1][0]
            assert (calls[:3] == 0x23).all() and (calls[3 + total:] == 0x23).all()
            table = mb.read()
            assert np.array_equal(table, expected_table(calls[3:3 + total], o2, res["m2"]["times"], skip if use_skip else None))
            m, u = column_sums(table)
            st = outs[1][2].view(np.uint64)
            assert np.array_equal(m, st[1:5]) and np.array_equal(u, st[5:9]) and m.sum() > 500
    # d_calls NULL with a set: refused, and the message says why
    before = mb.read()
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_call_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_pairs.data_ptr() + 16, 64, None, 1, "A", None,
                                      None, None, None, mbias=mb)
    assert ei.value.code == wa.WALT_EINVAL and "d_calls" in str(ei.value) and "counted from the calls" in str(ei.value)
    assert np.array_equal(mb.read(), before)
    if wa.device_count() >= 2:  # a set on another device than the index
        other = wa.MBias(1, 1)
        with pytest.raises(wa.WaltError) as ei:
            g1_all.meth_call_batch(b2, o2, res["m2"], "A", mbias=other)
        assert ei.value.code == wa.WALT_EINVAL and "device" in str(ei.value)
        other.close()
    mb.close()


# ---------------------------------------------------------------------------
# 4. command line
# ---------------------------------------------------------------------------
def run_walt(args, binary=WALT_BIN, timeout=600):
    pr = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert pr.returncode == 0, pr.stdout[-2000:]
    return pr.stdout


def check_against_methstats(out, heads):
    blocks = parse_mbias(open(out + ".mbias").read())
    stats = methstats_counts(open(out + ".methstats").read())
    assert [h for h, _ in blocks] == heads and len(stats) == len(blocks)
    for (_, table), (m, u) in zip(blocks, stats):
        cm, cu = column_sums(table)
        assert np.array_equal(cm, m) and np.array_equal(cu, u) and cm.sum() + cu.sum() > 100
    return blocks


@pytest.mark.parametrize("mode", ["r", "A", "R"])
def test_cli_single_end(wa, g1, g1_all, scratch, mode):
    from test_gpu_meth import cli_records_se, load
    from test_gpu_rpbat import mixed_library
    _, path = g1
    if mode == "R":
        names, seqs, scores = mixed_library()
        fq = os.path.join(scratch, "mbias_mixed.fastq")
        with open(fq, "w") as f:
            for nm, s, q in zip(names, seqs, scores):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
        extra = ["-R"]
    else:
        fq, extra = os.path.join(refio.GOLDEN, "se_ga.fastq" if mode == "A" else "se_ct.fastq"), ["-A"] if mode == "A" else []
    out = os.path.join(scratch, "mbias_cli_se_" + mode)
    base = ["-i", path, "-r", fq, "-a", "-u"] + extra
    run_walt(base + ["-o", out, "-MB", "-M", "-sam"])
    (head, table), = check_against_methstats(out, [None])
    loaded = []
    for _, sq, _ in refio.load_fastq_batches(fq, 10 ** 7, ""):
        loaded += sq
    recs, conv = cli_records_se(g1_all, loaded, mode if mode != "r" else "T")
    bases, offs = wa.pack_reads(loaded)
    calls, _, _ = g1_all.meth_call_batch(bases, offs, recs, conv)
    want = expected_table(calls, offs, recs["times"])
    assert np.array_equal(table, want) and open(out + ".mbias").read() == block_text(want)
    # without -MB: no .mbias, and SAM and .methstats byte-identical
    run_walt(base + ["-o", out + "_plain", "-M", "-sam"])
    assert not os.path.exists(out + "_plain.mbias")
    for sfx in ("", ".methstats", ".mapstats"):
        assert open(out + sfx, "rb").read() == open(out + "_plain" + sfx, "rb").read(), sfx
    # -MB alone (the other spellings): the same table, no .methstats, the .mr file of a run without it
    run_walt(base + ["-o", out + "_alone", "-mbias"])
    run_walt(base + ["-o", out + "_mr"])
    assert open(out + "_alone.mbias", "rb").read() == open(out + ".mbias", "rb").read()
    assert not os.path.exists(out + "_alone.methstats") and not os.path.exists(out + "_mr.mbias")
    assert open(out + "_alone", "rb").read() == open(out + "_mr", "rb").read()
    if mode == "r":
        # two shares of the batch on two sets (the same device twice), and small batches: the same file
        run_walt(base + ["-o", out + "_g00", "--m-bias", "-M", "-sam", "-g", "0,0", "-N", "1000"])
        assert open(out + "_g00.mbias", "rb").read() == open(out + ".mbias", "rb").read()
        # two read files that share an output name: one table after another, the set cleared in between
        run_walt(["-i", path, "-r", fq + "," + fq, "-o", out + "_two," + out + "_two", "-MB"])
        assert open(out + "_two.mbias").read() == 2 * block_text(want)


@pytest.mark.parametrize("mode", ["pe", "P", "RP"])
def test_cli_paired_end(wa, g1, g1_all, scratch, mode):
    from test_gpu_meth import load
    from test_gpu_overlap import cli_library
    _, path = g1
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    u1, u2, res, cv1, cv2 = cli_library(g1_all, mode, s1, s2)
    reads = ["-1", f2, "-2", f1, "-P"] if mode == "P" else ["-1", f1, "-2", f2] + (["-RP"] if mode == "RP" else [])
    out = os.path.join(scratch, "mbias_cli_pe_" + mode)
    base = ["-i", path] + reads + ["-a", "-u"]
    run_walt(base + ["-o", out, "-MB", "-M", "-sam"])
    blocks = check_against_methstats(out, ["mate1", "mate2"])
    want = []
    for seqs, mate, cv in ((u1, "m1", cv1), (u2, "m2", cv2)):
        bases, offs = wa.pack_reads(seqs)
        calls, _, _ = g1_all.meth_call_batch(bases, offs, res[mate], cv)
        want.append(expected_table(calls, offs, res[mate]["times"]))
    assert np.array_equal(blocks[0][1], want[0]) and np.array_equal(blocks[1][1], want[1])
    assert open(out + ".mbias").read() == "mate1\n" + block_text(want[0]) + "mate2\n" + block_text(want[1])
    assert not np.array_equal(want[0], want[1])
    run_walt(base + ["-o", out + "_plain", "-M", "-sam"])
    assert not os.path.exists(out + "_plain.mbias")
    for sfx in ("", ".methstats", ".mapstats"):
        assert open(out + sfx, "rb").read() == open(out + "_plain" + sfx, "rb").read(), sfx
    run_walt(base + ["-o", out + "_alone", "-MB"])
    assert open(out + "_alone.mbias", "rb").read() == open(out + ".mbias", "rb").read()
    assert not os.path.exists(out + "_alone.methstats")


@pytest.mark.parametrize("case", ["D", "NO", "C", "MC_D_NO"])
def test_cli_with_duplicates_overlap_clipping(wa, g1, scratch, case):
    """-MB beside -D, -NO, -C: the same file with and without -M, column sums equal to that run's .methstats, and a
    different table than the run without the option"""
    from test_gpu_dedup import doubled
    _, path = g1
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    extra = {"D": ["-D"], "NO": ["-NO"], "C": [], "MC_D_NO": ["-MC", "-D", "-NO"]}[case]
    if "-D" in extra:
        (_, f1), (_, f2) = doubled(scratch, "mbias_" + case, [f1, f2])
    if case == "C":
        args = refio.golden_meta()["cases"]["pe_clip_sam_au"]["args"]
        extra = ["-C", args[args.index("-C") + 1]]
        f1, f2 = os.path.join(refio.GOLDEN, "pe_clip_1.fastq"), os.path.join(refio.GOLDEN, "pe_clip_2.fastq")
    out = os.path.join(scratch, "mbias_cli_" + case)
    base = ["-i", path, "-1", f1, "-2", f2, "-a", "-u"]
    run_walt(base + ["-o", out + "_M", "-MB", "-M", "-sam"] + extra)
    blocks = check_against_methstats(out + "_M", ["mate1", "mate2"])
    run_walt(base + ["-o", out + "_alone", "-MB"] + extra)
    assert open(out + "_alone.mbias", "rb").read() == open(out + "_M.mbias", "rb").read()
    run_walt(base + ["-o", out + "_without", "-MB"] + [e for e in extra if e == "-MC"])
    without = parse_mbias(open(out + "_without.mbias").read())
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(blocks, without))
    if case != "C":  # -D and -NO only take calls away (clipping also lets more reads map)
        assert all((a[1] <= b[1]).all() for a, b in zip(blocks, without))
    if "-MC" in extra:
        run_walt(base + ["-o", out + "_noMB", "-M", "-sam"] + extra)
        for sfx in ("", ".methstats", ".methcounts", ".dupstats"):
            assert open(out + "_M" + sfx, "rb").read() == open(out + "_noMB" + sfx, "rb").read(), sfx


@pytest.mark.parametrize("pattern", [5, 7])
def test_cli_seed_patterns_5_and_7(wa, scratch, pattern):
    binary = os.path.join(refio.ROOT, "walt_amd", "bin", "walt_sp%d" % pattern)
    path = os.path.join(scratch, "mbias_g1_sp%d.dbindex" % pattern)
    old = wa.PATTERN
    wa.set_pattern(pattern)
    try:
        wa.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    finally:
        wa.set_pattern(old)
    out = os.path.join(scratch, "mbias_cli_sp%d" % pattern)
    run_walt(["-i", path, "-r", os.path.join(refio.GOLDEN, "sp_se_ct.fastq"), "-o", out, "-MB", "-M", "-sam"], binary=binary)
    check_against_methstats(out, [None])


def test_cli_two_devices_give_the_file_of_one(wa, g1, scratch):
    if wa.device_count() < 2:
        pytest.skip("one device")
    _, path = g1
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    out = os.path.join(scratch, "mbias_cli_g")
    run_walt(["-i", path, "-1", f1, "-2", f2, "-o", out + "_1", "-MB", "-M"])
    run_walt(["-i", path, "-1", f1, "-2", f2, "-o", out + "_2", "-MB", "-M", "-g", "0,1"])
    assert open(out + "_1.mbias", "rb").read() == open(out + "_2.mbias", "rb").read()


def test_mbias_soak_slice():
    """a few dozen random genomes and libraries through tools/soak.py's slice"""
    import sys
    sys.path.insert(0, os.path.join(refio.ROOT, "tools"))
    import soak
    line = soak.run_soak_mbias(range(1, 25), pattern=3)
    assert line.startswith("soak ok: mbias")
