"""Ignored read ends (include/walt_amd.h, "ignored read ends") on the device: walt_meth_pileup_batch_trim[_device],
walt_pair_overlap_batch_trim[_device] and bin/walt -I5 -I3 -I5R2 -I3R2.  The expected values come from the Python
restatement alone: the calls of tests/test_gpu_meth.py without bounds, every letter at a position outside
[trim5, limit - trim3) replaced by '.', and counts, totals, the pile-up and the bias table recomputed from the letters
that remain; the interval from a brute-force loop over read positions (tests/test_trim_cpu.py)."""
import os
import random

import numpy as np
import pytest

import refio
from test_gpu_mbias import block_text, column_sums
from test_gpu_mbias import expected_table as bias_table
from test_gpu_meth import cli_records_se, clip_point, load, methstats_text, planted, reference_bases, run_walt, strip_xm
from test_gpu_overlap import (assert_mate, cli_library, counts_of, expected_mate, hand_batch, overlap_line, pile_letters, word_of)
from test_gpu_pileup import assert_table, counts_text, expected_table
from test_trim_cpu import excluded_positions_trim, limit_of, trim_letters

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def want_mate(R, start_index, seqs, recs, conv, call_len=None, ex=None, skip=None, trim=(0, 0)):
    """expected_mate of tests/test_gpu_overlap.py (no bounds), then the letters outside the bounds replaced by '.' and the
    counts and totals recomputed from what remains; `reads` stays -> (calls, counts [n, 8], totals)"""
    plain, _, tot0 = expected_mate(R, start_index, seqs, recs, conv, call_len, ex, skip)
    glen = len(R[0])
    calls = [trim_letters(c, limit_of(len(c), None if call_len is None else call_len[i]), *trim) for i, c in enumerate(plain)]
    counts = np.array([counts_of(c) for c in calls], dtype=np.int64).reshape(len(calls), 8)
    tot = {"reads": tot0["reads"], "meth": np.zeros(4, dtype=np.int64), "unmeth": np.zeros(4, dtype=np.int64)}
    for i in range(len(calls)):
        cv = conv if isinstance(conv, str) else chr(int(conv[i]))
        if int(recs["times"][i]) == 1 and int(recs["genome_pos"][i]) < glen and cv in ("T", "A") and not (skip is not None and skip[i]):
            tot["meth"] += counts[i, :4]
            tot["unmeth"] += counts[i, 4:]
    return calls, counts, tot


def want_table(calls, offsets, recs, skip=None, into=None):
    text = np.frombuffer("".join(calls).encode(), dtype=np.uint8)
    return bias_table(text, offsets, recs["times"], skip, base=int(offsets[0]), into=into)


def want_words(start_index, glen, res, s1, s2, cl1, cl2, t1, t2):
    ex, bases = [], 0
    for i in range(len(s1)):
        e, b = excluded_positions_trim(start_index, glen, res["m1"][i], res["m2"][i], res["best_times"][i], len(s1[i]), len(s2[i]),
                                       None if cl1 is None else cl1[i], None if cl2 is None else cl2[i], t1, t2)
        ex.append(e)
        bases += b
    words = np.array([word_of(e) for e in ex], dtype=np.uint32)
    return ex, words, [int((words != 0).sum()), bases]


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def planted_idx(wa, scratch):
    fa, _, _, _ = planted(scratch)
    path = os.path.join(scratch, "trim_planted.dbindex")
    wa.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    idx = wa.Index.open(path, device=0, strands=wa.STRANDS_ALL | wa.WITH_REFERENCE)
    yield db, idx, reference_bases(db)
    idx.close()


@pytest.fixture(scope="module")
def g1(wa, scratch):
    path = os.path.join(scratch, "trim_g1.dbindex")
    wa.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    return refio.DbIndex(path), path


@pytest.fixture(scope="module")
def g1_all(wa, g1):
    idx = wa.Index.open(g1[1], device=0, strands=wa.STRANDS_ALL | wa.WITH_REFERENCE)
    yield idx
    idx.close()


# ---------------------------------------------------------------------------
# 1. hand-made batches through the host forms, at the three kPile paths, composed with skip, excl and a bias set
# ---------------------------------------------------------------------------
BOUNDS = [((5, 7), (3, 20)), ((16, 0), (0, 16)), ((0, 1), (17, 0)), ((59, 0), (0, 59)), ((30, 30), (31, 30)), ((0, 5000), (5000, 0)),
          ((1, 15), (15, 1))]


def check_host(wa, idx, R, start_index, seqs, recs, conv, cl, words, ex, skip, trim, mb, table, what, index_options=None):
    """one mate through Index.meth_call_batch, Pileup.add_batch and Pileup.add_batch under pile_rows: calls, counts,
    totals, the pile-up and the bias table against the restatement"""
    glen = len(R[0])
    bases, offs = wa.pack_reads(seqs)
    want = want_mate(R, start_index, seqs, recs, conv, cl, ex, skip, trim)
    kw = dict(call_len=cl, skip=skip, excl=words, trim5=trim[0], trim3=trim[1])
    for path in ("calls", "pile", "pile_rows"):
        index_options(idx, pile_rows=1 if path == "pile_rows" else 0)
        pile = idx.pileup() if path != "calls" else None
        try:
            if mb is not None:
                mb.clear()
            call = pile.add_batch if pile is not None else idx.meth_call_batch
            got = call(bases, offs, recs, conv, mbias=mb, mbias_table=table, **kw)
            assert_mate(got, want, "%s %s" % (what, path))
            if pile is not None:
                m, u = pile_letters(start_index, glen, want[0], recs, skip)
                assert_table(pile.extract(), R[0], start_index, m, u, "%s %s" % (what, path))
            if mb is not None:
                tab = mb.read(table)
                assert np.array_equal(tab, want_table(want[0], offs, recs, skip)), (what, path)
                cm, cu = column_sums(tab)  # the table's column sums are the returned totals
                assert np.array_equal(cm, got[2]["meth"][0].astype(np.uint64)) and np.array_equal(cu, got[2]["unmeth"][0].astype(np.uint64))
                if trim[0] < 1024:
                    assert tab[:, :, :trim[0]].sum() == 0
        finally:
            if pile is not None:
                pile.close()
    return want


@pytest.mark.parametrize("n", [0, 1, 293])
def test_hand_made_batches_host_forms(wa, planted_idx, index_options, n):
    db, idx, R = planted_idx
    s1, s2, res, cl1, cl2, _ = hand_batch(db, R, n)
    rng = random.Random(n)
    skip = np.array([[rng.random() < 0.2, rng.random() < 0.2] for _ in range(n)], dtype=np.uint8).reshape(n, 2)
    mb = wa.MBias(0, 2)
    try:
        blanked = kept = 0
        for k, (t1, t2) in enumerate(BOUNDS if n else BOUNDS[:2]):
            use_cl, use_skip = k % 2 == 0, k % 3 != 0
            c1, c2 = (cl1, cl2) if use_cl else (None, None)
            ex, words, totals = want_words(db.start_index, db.genome_len, res, s1, s2, c1, c2, t1, t2)
            got_words, got_totals = idx.pair_overlap(res, *(wa.pack_reads(s)[1] for s in (s1, s2)), c1, c2, trim1=t1, trim2=t2)
            assert got_words.tolist() == words.tolist() and got_totals.tolist() == totals, (n, t1, t2)
            w1 = check_host(wa, idx, R, db.start_index, s1, res["m1"], "T", c1, None, None, skip[:, 0] if use_skip else None, t1, mb, 0,
                            "n=%d mate 1 %s" % (n, t1), index_options)
            w2 = check_host(wa, idx, R, db.start_index, s2, res["m2"], "A", c2, words, ex, skip[:, 1] if use_skip else None, t2,
                            mb if k % 2 else None, 1, "n=%d mate 2 %s" % (n, t2), index_options)
            plain = expected_mate(R, db.start_index, s1, res["m1"], "T", c1)[0]
            blanked += sum(a != b for a, b in zip("".join(plain), "".join(w1[0])))
            kept += sum(ch != "." for ch in "".join(w1[0]) + "".join(w2[0]))
        if n == 293:
            assert blanked > 1000 and kept > 1000
    finally:
        mb.close()


def test_more_reads_than_one_trip_of_the_grid(wa, planted_idx, index_options):
    """256-thread blocks of 32 groups, at most 8 blocks per compute unit (meth.hip meth_launch): the hand-made batch tiled
    beyond that, the restatement computed once"""
    import torch
    db, idx, R = planted_idx
    s1, _, res, cl1, _, _ = hand_batch(db, R, 293)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    times = -(-(8 * cus * 32 + 1237) // 293)
    trim = (6, 9)
    one = want_mate(R, db.start_index, s1, res["m1"], "T", cl1, None, None, trim)
    seqs, recs, cl = s1 * times, np.tile(res["m1"], times), cl1 * times
    assert len(seqs) > 8 * cus * 32
    bases, offs = wa.pack_reads(seqs)
    m1, u1 = pile_letters(db.start_index, db.genome_len, one[0], res["m1"])
    for rows in (1,):  # (the trips over the grid are the same loop at every kPile; pile_rows needs every lane in each)
        index_options(idx, pile_rows=rows)
        pile = idx.pileup()
        try:
            calls, counts, stats = pile.add_batch(bases, offs, recs, "T", call_len=cl, trim5=trim[0], trim3=trim[1])
            assert calls.tobytes().decode() == "".join(one[0]) * times
            gc = np.concatenate([counts["meth"].astype(np.int64), counts["unmeth"].astype(np.int64)], axis=1)
            assert np.array_equal(gc, np.tile(one[1], (times, 1)))
            assert int(stats["reads"][0]) == times * one[2]["reads"]
            assert np.array_equal(stats["meth"][0].astype(np.int64), times * one[2]["meth"])
            assert np.array_equal(stats["unmeth"][0].astype(np.int64), times * one[2]["unmeth"])
            assert_table(pile.extract(), R[0], db.start_index, times * m1, times * u1, "tiled rows=%d" % rows)
        finally:
            pile.close()


# ---------------------------------------------------------------------------
# 2. the golden library: zeros, the device form on a stream, the overlap call
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1_pairs(wa, g1_all):
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    s1, s2 = s1[:600], s2[:600]
    b1, o1 = wa.pack_reads(s1)
    b2, o2 = wa.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    return (s1, s2), (b1, o1, b2, o2), res


def test_zero_bounds_through_the_trim_forms_are_byte_identical_to_the_bias_forms(wa, g1_all, g1_pairs, index_options):
    _, (b1, o1, b2, o2), res = g1_pairs
    n = res.size
    L = wa.lib()
    excl, totals = g1_all.pair_overlap(res, o1, o2)
    skip = (np.arange(n) % 3 == 0).astype(np.uint8)
    rec = np.ascontiguousarray(res["m2"])
    mb = wa.MBias(0, 2)
    try:
        for rows in (0, 1):
            index_options(g1_all, pile_rows=rows)
            for with_pile in (False, True):
                outs = []
                for form in (L.walt_meth_pileup_batch_mbias, L.walt_meth_pileup_batch_trim):
                    pile = g1_all.pileup() if with_pile else None
                    calls = np.full(b2.size, 0x23, dtype=np.uint8)
                    counts = np.zeros(n, dtype=wa.meth_counts_dtype)
                    stats = np.zeros(1, dtype=wa.meth_stats_dtype)
                    mb.clear()
                    tail = (0, 0) if form is L.walt_meth_pileup_batch_trim else ()
                    rc = form(g1_all.handle, pile.handle if pile is not None else None, b2.ctypes.data, o2.ctypes.data, n, rec.ctypes.data, 16,
                              None, 0, ord("A"), None, calls.ctypes.data, counts.ctypes.data, stats.ctypes.data, skip.ctypes.data, 1,
                              excl.ctypes.data, mb.handle, 1, *tail)
                    assert rc == 0, L.walt_last_error()
                    sites = pile.extract()[0].tobytes() if pile is not None else b""
                    if pile is not None:
                        pile.close()
                    outs.append((calls.tobytes(), counts.tobytes(), stats.tobytes(), sites, mb.read(1).tobytes()))
                assert outs[0] == outs[1] and b"Z" in outs[0][0]
        # the binding: zeros reach the forms they always reached (tests/test_gpu_meth_refusals.py pins the names) and give the same
        plain = g1_all.meth_call_batch(b2, o2, res["m2"], "A", skip=skip, excl=excl)
        same = g1_all.meth_call_batch(b2, o2, res["m2"], "A", skip=skip, excl=excl, trim5=0, trim3=0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, same))
        # the overlap call with all zeros equals the older call
        w = np.zeros(n, dtype=np.uint32)
        t = np.zeros(2, dtype=np.uint64)
        pr = np.ascontiguousarray(res)
        assert L.walt_pair_overlap_batch_trim(g1_all.handle, pr.ctypes.data, o1.ctypes.data, o2.ctypes.data, n, None, None, w.ctypes.data,
                                              t.ctypes.data, 0, 0, 0, 0) == 0
        assert w.tobytes() == excl.tobytes() and t.tolist() == totals.tolist() and int(t[0]) > 20
    finally:
        mb.close()


def test_device_forms_on_a_stream(wa, g1, g1_all, g1_pairs, index_options):
    """the overlap kernel with bounds enqueued in front of mate 2's bounded call on one stream, into a pile-up and a
    bias set; everything against the restatement"""
    import torch
    db, _ = g1
    R = reference_bases(db)
    (s1, s2), (b1, o1, b2, o2), res = g1_pairs
    n = res.size
    rng = random.Random(4)
    cl1 = np.array([rng.choice([len(s), len(s), len(s) // 2, 0, len(s) + 3]) for s in s1], dtype=np.uint32)
    cl2 = np.array([rng.choice([len(s), len(s), len(s) // 2, 0, len(s) + 3]) for s in s2], dtype=np.uint32)
    skip = (np.arange(n) % 5 == 0).astype(np.uint8)
    t1, t2 = (2, 10), (7, 3)
    ex, words, totals = want_words(db.start_index, db.genome_len, res, s1, s2, cl1, cl2, t1, t2)
    plain_words = want_words(db.start_index, db.genome_len, res, s1, s2, cl1, cl2, (0, 0), (0, 0))[1]
    assert totals[0] > 20 and (words != plain_words).sum() > 10
    want = want_mate(R, db.start_index, s2, res["m2"], "A", cl2, ex, skip, t2)
    dev = torch.device("cuda", 0)
    d_res = torch.from_numpy(res.view(np.uint8).reshape(n, 64)).to(dev)
    d_o1, d_o2 = torch.from_numpy(o1.view(np.int64)).to(dev), torch.from_numpy(o2.view(np.int64)).to(dev)
    d_cl1, d_cl2 = torch.from_numpy(cl1.view(np.int32)).to(dev), torch.from_numpy(cl2.view(np.int32)).to(dev)
    d_b2, d_skip = torch.from_numpy(b2).to(dev), torch.from_numpy(skip).to(dev)
    st = torch.cuda.Stream(device=dev)
    mb = wa.MBias(0, 2)
    try:
        for path in ("calls", "pile", "pile_rows"):
            index_options(g1_all, pile_rows=1 if path == "pile_rows" else 0)
            pile = g1_all.pileup() if path != "calls" else None
            d_excl = torch.full((n,), 0x23232323, dtype=torch.int32, device=dev)
            d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
            d_calls = torch.full((b2.size + 48,), 0x23, dtype=torch.uint8, device=dev)
            d_counts = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
            d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
            mb.clear()
            torch.cuda.synchronize()
            try:
                g1_all.pair_overlap_device(d_res.data_ptr(), d_o1.data_ptr(), d_o2.data_ptr(), n, d_excl.data_ptr(), d_cl1.data_ptr(),
                                           d_cl2.data_ptr(), d_tot.data_ptr(), stream=st.cuda_stream, trim1=t1, trim2=t2)
                args = (d_b2.data_ptr(), d_o2.data_ptr(), n, d_res.data_ptr() + 16, 64, None, 1, "A", d_cl2.data_ptr(),
                        d_calls.data_ptr() + 5, d_counts.data_ptr(), d_stats.data_ptr())
                kw = dict(stream=st.cuda_stream, d_skip=d_skip.data_ptr(), d_excl=d_excl.data_ptr(), mbias=mb, mbias_table=1,
                          trim5=t2[0], trim3=t2[1])
                (pile.add_batch_device if pile is not None else g1_all.meth_call_batch_device)(*args, **kw)
                st.synchronize()
                assert d_excl.cpu().numpy().view(np.uint32).tolist() == words.tolist()
                assert d_tot.cpu().numpy().tolist() == totals
                calls = d_calls.cpu().numpy()
                assert (calls[:5] == 0x23).all() and (calls[5 + b2.size:] == 0x23).all()
                got = (calls[5:5 + b2.size], d_counts.cpu().numpy().reshape(-1).view(wa.meth_counts_dtype),
                       d_stats.cpu().numpy().view(wa.meth_stats_dtype))
                assert_mate(got, want, "device " + path)
                assert np.array_equal(mb.read(1), want_table(want[0], o2, res["m2"], skip)) and mb.read(0).sum() == 0
                if pile is not None:
                    m, u = pile_letters(db.start_index, db.genome_len, want[0], res["m2"], skip)
                    assert_table(pile.extract(), R[0], db.start_index, m, u, "device " + path)
            finally:
                if pile is not None:
                    pile.close()
        # the new forms refuse what the bias forms refuse, under their own names
        L = wa.lib()
        rc = L.walt_meth_pileup_batch_trim_device(g1_all.handle, None, d_b2.data_ptr(), d_o2.data_ptr(), n, d_res.data_ptr() + 16, 64, None,
                                                  1, ord("A"), None, None, None, None, None, 1, None, mb.handle, 0, 1, 1, None)
        assert rc == wa.WALT_EINVAL and b"walt_meth_pileup_batch_trim_device" in L.walt_last_error() and b"d_calls" in L.walt_last_error()
        rc = L.walt_pair_overlap_batch_trim_device(g1_all.handle, d_res.data_ptr() + 2, d_o1.data_ptr(), d_o2.data_ptr(), n, None, None,
                                                   d_excl.data_ptr(), None, 1, 1, 1, 1, None)
        assert rc == wa.WALT_EINVAL and b"walt_pair_overlap_batch_trim_device" in L.walt_last_error() and b"aligned" in L.walt_last_error()
    finally:
        mb.close()


def test_an_index_without_reference_serves_the_bounded_overlap(wa, g1, g1_all, g1_pairs):
    db, path = g1
    (s1, s2), (b1, o1, b2, o2), res = g1_pairs
    idx = wa.Index.open(path, device=0, strands=wa.STRANDS_CT)
    try:
        assert not idx.has_reference
        for t1, t2 in (((0, 10), (0, 0)), ((12, 0), (4, 4)), ((0, 0), (0, 30))):
            _, words, totals = want_words(db.start_index, db.genome_len, res, s1, s2, None, None, t1, t2)
            got, tot = idx.pair_overlap(res, o1 + np.uint64(7), o2, trim1=t1, trim2=t2)
            assert got.tolist() == words.tolist() and tot.tolist() == totals and totals[0] > 20, (t1, t2)
    finally:
        idx.close()


# ---------------------------------------------------------------------------
# 3. command line
# ---------------------------------------------------------------------------
def ignore_line(v):
    return "ignore\t" + "\t".join(str(x) for x in v) + "\n"


def check_xm(rows, recs, calls, what):
    n_xm = 0
    for i, ml in enumerate(rows):
        _, xm = strip_xm(ml)
        assert (xm is not None) == (int(recs["times"][i]) >= 1), (what, ml)
        if xm is not None:
            n_xm += 1
            exp = calls[i][::-1] if bytes(recs["strand"][i]) == b"-" else calls[i]
            assert xm == exp, "%s line %d\n got  %s\n want %s" % (what, i, xm, exp)
    return n_xm


def mbias_zero_at_ignored(text, bounds):
    """every block of <out>.mbias has zero counts with level NA at its mate's first trim5 positions"""
    blocks = [b for b in text.replace("mate2\n", "\x00").replace("mate1\n", "").split("\x00")]
    assert len(blocks) == len(bounds)
    for block, (t5, _) in zip(blocks, bounds):
        rows = [l.split("\t") for l in block.splitlines()]
        head = [r for r in rows if int(r[1]) <= t5]
        assert len(head) == 4 * t5 and all(r[2:] == ["0", "0", "NA"] for r in head) and len(rows) > len(head)


@pytest.mark.parametrize("mode", ["r", "A", "R"])
def test_cli_single_end(wa, g1, g1_all, scratch, mode):
    from test_gpu_rpbat import mixed_library
    db, path = g1
    R = reference_bases(db)
    if mode == "R":
        names, seqs, scores = mixed_library()
        fq = os.path.join(scratch, "trim_mixed.fastq")
        with open(fq, "w") as f:
            for nm, s, q in zip(names, seqs, scores):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
        extra = ["-R"]
    else:
        fq, extra = os.path.join(refio.GOLDEN, "se_ga.fastq" if mode == "A" else "se_ct.fastq"), ["-A"] if mode == "A" else []
    loaded = []
    for _, sq, _ in refio.load_fastq_batches(fq, 10 ** 7, ""):
        loaded += sq
    recs, conv = cli_records_se(g1_all, loaded, mode if mode != "r" else "T")
    _, offs = wa.pack_reads(loaded)
    trim = (6, 11)
    out = os.path.join(scratch, "trim_cli_se_" + mode)
    base = ["-i", path, "-r", fq, "-a", "-u", "-M", "-sam", "-MC", "-MB"] + extra
    log = run_walt(base + ["-o", out, "-I5", "6", "--ignore-3prime", "11", "-v"])
    for tag, t in ((out, trim), (out + "_plain", (0, 0))):
        if t == (0, 0):
            run_walt(base + ["-o", tag])
        want = want_mate(R, db.start_index, loaded, recs, conv, None, None, None, t)
        rows = [l for l in open(tag) if not l.startswith("@")]
        assert check_xm(rows, recs, want[0], tag) > 100
        assert open(tag + ".methstats").read() == methstats_text([(None, want[2])]) + (ignore_line(t) if any(t) else "")
        m, u = pile_letters(db.start_index, db.genome_len, want[0], recs)
        assert open(tag + ".methcounts").read() == counts_text(db, expected_table(R[0], db.start_index, m, u)[0])
        assert open(tag + ".mbias").read() == block_text(want_table(want[0], offs, recs))
    assert ignore_line(trim) in log
    mbias_zero_at_ignored(open(out + ".mbias").read(), [trim])
    # zeros given on the command line: the run without the options, byte for byte
    run_walt(base + ["-o", out + "_zero", "-ignore", "0", "-I3", "0"])
    for sfx in ("", ".methstats", ".methcounts", ".mbias", ".mapstats"):
        assert open(out + "_zero" + sfx, "rb").read() == open(out + "_plain" + sfx, "rb").read(), sfx
    # nothing but the calls differs: the lines without XM:Z: and the mapping statistics
    assert [strip_xm(l)[0] for l in open(out)] == [strip_xm(l)[0] for l in open(out + "_plain")]
    assert open(out + ".mapstats").read() == open(out + "_plain.mapstats").read()
    if mode == "r":
        # two shares of small batches, and two read files into one output: one part after the other, each with its line
        run_walt(base + ["-o", out + "_g00", "-I5", "6", "-I3", "11", "-g", "0,0", "-N", "1000"])
        for sfx in ("", ".methstats", ".methcounts", ".mbias"):
            assert open(out + "_g00" + sfx, "rb").read() == open(out + sfx, "rb").read(), sfx
        run_walt(["-i", path, "-r", fq + "," + fq, "-o", out + "_two," + out + "_two", "-M", "-MB", "-I5", "6", "-I3", "11"])
        assert open(out + "_two.methstats").read() == 2 * open(out + ".methstats").read()
        assert open(out + "_two.mbias").read() == 2 * open(out + ".mbias").read()


def expect_pe(wa, db, R, u1, u2, res, cv1, cv2, t1, t2, cl1=None, cl2=None, skip=None, no_overlap=False):
    """the four outputs of a paired run in the user's order -> dict"""
    ex = words = totals = None
    if no_overlap:
        ex, words, totals = want_words(db.start_index, db.genome_len, res, u1, u2, cl1, cl2, t1, t2)
    w1 = want_mate(R, db.start_index, u1, res["m1"], cv1, cl1, None, None if skip is None else skip[:, 0], t1)
    w2 = want_mate(R, db.start_index, u2, res["m2"], cv2, cl2, ex, None if skip is None else skip[:, 1], t2)
    pile = pile_letters(db.start_index, db.genome_len, w1[0], res["m1"], None if skip is None else skip[:, 0])
    pile = pile_letters(db.start_index, db.genome_len, w2[0], res["m2"], None if skip is None else skip[:, 1], into=pile)
    stats = methstats_text([("mate1", w1[2]), ("mate2", w2[2])]) + (overlap_line(totals) if no_overlap else "")
    stats += ignore_line(t1 + t2) if any(t1 + t2) else ""
    tabs = [want_table(w[0], wa.pack_reads(u)[1], res[m], None if skip is None else skip[:, k])
            for k, (w, u, m) in enumerate(((w1, u1, "m1"), (w2, u2, "m2")))]
    return {"w1": w1, "w2": w2, "stats": stats, "counts": counts_text(db, expected_table(R[0], db.start_index, *pile)[0]),
            "mbias": "mate1\n" + block_text(tabs[0]) + "mate2\n" + block_text(tabs[1]), "words": words, "totals": totals}


def check_pe_outputs(out, want, res, what):
    rows = [l for l in open(out) if not l.startswith("@")]
    assert len(rows) == 2 * res.size
    assert check_xm(rows[0::2], res["m1"], want["w1"][0], what + " mate 1") + check_xm(rows[1::2], res["m2"], want["w2"][0], what + " mate 2") > 500
    assert open(out + ".methstats").read() == want["stats"], what
    assert open(out + ".methcounts").read() == want["counts"], what
    assert open(out + ".mbias").read() == want["mbias"], what


@pytest.mark.parametrize("mode", ["pe", "P", "RP"])
def test_cli_paired_end_with_and_without_no_overlap(wa, g1, g1_all, scratch, mode):
    db, path = g1
    R = reference_bases(db)
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    u1, u2, res, cv1, cv2 = cli_library(g1_all, mode, s1, s2)
    reads = ["-1", f2, "-2", f1, "-P"] if mode == "P" else ["-1", f1, "-2", f2] + (["-RP"] if mode == "RP" else [])
    base = ["-i", path] + reads + ["-a", "-u", "-M", "-sam", "-MC", "-MB"]
    t1, t2 = (3, 10), (8, 2)  # the user's mate 1 and mate 2
    opts = ["-I5", "3", "-I3", "10", "-I5R2", "8", "-I3R2", "2"]
    out = os.path.join(scratch, "trim_cli_pe_" + mode)
    log = run_walt(base + ["-o", out] + opts + ["-v"])
    want = expect_pe(wa, db, R, u1, u2, res, cv1, cv2, t1, t2)
    check_pe_outputs(out, want, res, mode)
    assert ignore_line(t1 + t2) in log
    mbias_zero_at_ignored(open(out + ".mbias").read(), [t1, t2])
    # beside -NO: the interval comes from mate 1's bounded span, mate 2 keeps its calls where mate 1 is ignored
    run_walt(base + ["-o", out + "_NO", "-NO", "--ignore", "3", "-ignore-3prime", "10", "--ignore-r2", "8", "-ignore-3prime-r2", "2"])
    want_no = expect_pe(wa, db, R, u1, u2, res, cv1, cv2, t1, t2, no_overlap=True)
    check_pe_outputs(out + "_NO", want_no, res, mode + " -NO")
    unbounded = want_words(db.start_index, db.genome_len, res, u1, u2, None, None, (0, 0), (0, 0))[1]
    assert (want_no["words"] != unbounded).sum() >= 100 and want_no["totals"][0] >= 100
    # without the four options: today's output
    run_walt(base + ["-o", out + "_plain"])
    check_pe_outputs(out + "_plain", expect_pe(wa, db, R, u1, u2, res, cv1, cv2, (0, 0), (0, 0)), res, mode + " plain")
    assert "ignore" not in open(out + "_plain.methstats").read()
    assert [strip_xm(l)[0] for l in open(out)] == [strip_xm(l)[0] for l in open(out + "_plain")]
    assert open(out + ".mapstats").read() == open(out + "_plain.mapstats").read()


def test_cli_beside_clipping_duplicates_and_small_batches_on_two_shares(wa, g1, g1_all, scratch):
    from test_dedup_cpu import DupRule, expect_pairs
    from test_gpu_dedup import doubled, loaded
    db, path = g1
    R = reference_bases(db)
    t1, t2 = (2, 12), (9, 4)
    opts = ["-I5", "2", "-I3", "12", "-I5R2", "9", "-I3R2", "4"]
    # -C: trim3 counts back from the clip point
    args = refio.golden_meta()["cases"]["pe_clip_sam_au"]["args"]
    adaptor = args[args.index("-C") + 1]
    ap = adaptor.split(":") if ":" in adaptor else [adaptor, adaptor]
    f1, f2 = os.path.join(refio.GOLDEN, "pe_clip_1.fastq"), os.path.join(refio.GOLDEN, "pe_clip_2.fastq")
    seqs, cls = [], []
    for fq, ad in ((f1, ap[0]), (f2, ap[1])):
        got = []
        for _, sq, _ in refio.load_fastq_batches(fq, 10 ** 7, ad):
            got += sq
        raw = [l.rstrip(b"\n") for l in open(fq, "rb").readlines()[1::4]]
        seqs.append(got)
        cls.append([clip_point(ad.encode(), bytearray(r)) for r in raw])
    assert sum(c < len(s) for c, s in zip(cls[0], seqs[0])) > 10
    res, _ = g1_all.map_pe_batch(*wa.pack_reads(seqs[0]), *wa.pack_reads(seqs[1]))
    out = os.path.join(scratch, "trim_cli_clip")
    run_walt(["-i", path, "-1", f1, "-2", f2, "-o", out, "-a", "-u", "-M", "-sam", "-MC", "-MB", "-NO", "-C", adaptor] + opts)
    want = expect_pe(wa, db, R, seqs[0], seqs[1], res, "T", "A", t1, t2, cls[0], cls[1], no_overlap=True)
    check_pe_outputs(out, want, res, "-C")
    raw_end = expect_pe(wa, db, R, seqs[0], seqs[1], res, "T", "A", t1, t2, None, None, no_overlap=True)
    assert raw_end["stats"] != want["stats"]
    # -D -NO, in one batch and in batches of 64 on two shares: the restatement, and each other
    (g1f, d1), (g2f, d2) = doubled(scratch, "trim", [os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")])
    s1, s2 = loaded(d1), loaded(d2)
    res, _ = g1_all.map_pe_batch(*wa.pack_reads(s1), *wa.pack_reads(s2))
    dup = expect_pairs(DupRule(), res, "T")
    assert int(dup.sum()) > 200
    a = os.path.join(scratch, "trim_cli_dup")
    run_walt(["-i", path, "-1", d1, "-2", d2, "-o", a, "-a", "-u", "-M", "-sam", "-MC", "-MB", "-D", "-NO"] + opts)
    check_pe_outputs(a, expect_pe(wa, db, R, s1, s2, res, "T", "A", t1, t2, skip=dup, no_overlap=True), res, "-D -NO")
    s1, s2 = loaded(g1f), loaded(g2f)
    b, c = os.path.join(scratch, "trim_cli_one"), os.path.join(scratch, "trim_cli_n64")
    common = ["-i", path, "-1", g1f, "-2", g2f, "-a", "-u", "-M", "-sam", "-MC", "-MB", "-NO"] + opts
    run_walt(common + ["-o", b])
    run_walt(common + ["-o", c, "-N", "64", "-g", "0,0"])
    res, _ = g1_all.map_pe_batch(*wa.pack_reads(s1), *wa.pack_reads(s2))
    check_pe_outputs(c, expect_pe(wa, db, R, s1, s2, res, "T", "A", t1, t2, no_overlap=True), res, "-N 64 -g 0,0")
    for sfx in ("", ".methcounts", ".methstats", ".mbias", ".mapstats"):
        assert open(b + sfx, "rb").read() == open(c + sfx, "rb").read(), sfx


@pytest.mark.parametrize("pattern", [5, 7])
def test_cli_seed_patterns_5_and_7(wa, scratch, pattern):
    from test_gpu_mbias import methstats_counts, parse_mbias
    binary = os.path.join(refio.ROOT, "walt_amd", "bin", "walt_sp%d" % pattern)
    path = os.path.join(scratch, "trim_g1_sp%d.dbindex" % pattern)
    old = wa.PATTERN
    wa.set_pattern(pattern)
    try:
        wa.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    finally:
        wa.set_pattern(old)
    out = os.path.join(scratch, "trim_cli_sp%d" % pattern)
    import subprocess
    for tag, opts in (("", ["-I5", "4", "-I3", "9"]), ("_plain", [])):
        pr = subprocess.run([binary, "-i", path, "-r", os.path.join(refio.GOLDEN, "sp_se_ct.fastq"), "-o", out + tag, "-MB", "-M", "-sam"] + opts,
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert pr.returncode == 0, pr.stdout[-2000:]
    # every XM:Z: of the bounded run is the plain run's with the ends blanked, in the order of the read as sequenced
    n_xm = 0
    for pl, tl in zip(open(out + "_plain"), open(out)):
        (rest_p, xm_p), (rest_t, xm_t) = strip_xm(pl), strip_xm(tl)
        assert rest_p == rest_t
        if xm_p is not None:
            minus = int(pl.split("\t")[1]) & 0x10
            seq_order = xm_p[::-1] if minus else xm_p
            exp = trim_letters(seq_order, len(seq_order), 4, 9)
            assert xm_t == (exp[::-1] if minus else exp)
            n_xm += 1
    assert n_xm > 100
    assert open(out + ".methstats").read().endswith(ignore_line((4, 9)))
    (_, table), = parse_mbias(open(out + ".mbias").read())
    (m, u), = methstats_counts(open(out + ".methstats").read())
    cm, cu = column_sums(table)
    assert np.array_equal(cm, m) and np.array_equal(cu, u) and cm.sum() + cu.sum() > 100 and table[:, :, :4].sum() == 0


# ---------------------------------------------------------------------------
# 4. a soak slice
# ---------------------------------------------------------------------------
def test_trim_soak_slice():
    import sys
    sys.path.insert(0, os.path.join(refio.ROOT, "tools"))
    import soak
    line = soak.run_soak_trim(range(1, 6), pattern=3)
    assert line.startswith("soak ok: trim")
