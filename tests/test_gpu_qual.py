"""Minimum base quality (include/walt_amd.h, "minimum base quality") on the device: walt_meth_pileup_batch_qual[_device],
walt_meth_nonconv_batch_qual[_device] and bin/walt -MQ -MQO.  The expected values come from the Python restatement alone:
the calls of tests/test_gpu_trim.py without qualities, every letter at a position whose quality byte is below the floor
replaced by '.', and counts, totals, the pile-up and the tables recomputed from the letters that remain; the evidence from a
plain walk that leaves those positions out.  The command-line runs are checked against their own SAM."""
import os
import random

import numpy as np
import pytest

import refio
from test_gpu_cpgpairs import expected_table as pair_table
from test_gpu_cpgpairs import find_pairs, mode_args, run_walt, sites_list, sites_of
from test_gpu_epialleles import epi_list, epi_sites_of, expected_epi
from test_gpu_mbias import block_text
from test_gpu_meth import load, methstats_text, reference_bases, strip_xm
from test_gpu_meth_contigs import Genome, build_index, remove_index
from test_gpu_nonconv import expected_verdicts, fails, tally_of
from test_gpu_overlap import assert_mate, counts_of, pile_letters
from test_gpu_pileup import assert_table, chrom_of
from test_gpu_trim import g1, g1_all, planted_idx, wa, want_mate, want_table  # noqa: F401  (fixtures among them)
from test_gpu_variants import SAM_SKIP, assert_planes, base_letter, cli_texts
from test_trim_cpu import make_read

pytestmark = pytest.mark.gpu

LENGTHS = (1, 15, 16, 17, 33, 100, 128)
FLOORS = (1, 35, 53, 127)


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def qual_letters(calls, quals, min_qual):
    """the calls of a read without qualities -> every letter at a position whose quality byte is below the floor replaced by '.'"""
    return "".join(ch if int(q) >= min_qual else "." for ch, q in zip(calls, bytes(quals)))


def want_mate_q(R, start_index, seqs, recs, conv, quals, min_qual, call_len=None, ex=None, skip=None, trim=(0, 0)):
    """want_mate of tests/test_gpu_trim.py (no qualities), then the letters below the floor replaced by '.' and the counts and
    totals recomputed from what remains; `reads` stays -> (calls, counts [n, 8], totals)"""
    plain, _, tot0 = want_mate(R, start_index, seqs, recs, conv, call_len, ex, skip, trim)
    glen = len(R[0])
    calls = [qual_letters(c, q, min_qual) for c, q in zip(plain, quals)]
    counts = np.array([counts_of(c) for c in calls], dtype=np.int64).reshape(len(calls), 8)
    tot = {"reads": tot0["reads"], "meth": np.zeros(4, dtype=np.int64), "unmeth": np.zeros(4, dtype=np.int64)}
    for i in range(len(calls)):
        cv = conv if isinstance(conv, str) else chr(int(conv[i]))
        if int(recs["times"][i]) == 1 and int(recs["genome_pos"][i]) < glen and cv in ("T", "A") and not (skip is not None and skip[i]):
            tot["meth"] += counts[i, :4]
            tot["unmeth"] += counts[i, 4:]
    return calls, counts, tot


def expected_evidence_q(R, start_index, seqs, recs, conv, quals, min_qual, call_len=None, skip=None, into=None):
    """expected_evidence of tests/test_gpu_variants.py with the positions below the floor left out (quals None: all kept)"""
    glen = len(R[0])
    match, other = into if into is not None else (np.zeros(glen, dtype=np.int64), np.zeros(glen, dtype=np.int64))
    for i, s in enumerate(seqs):
        s = s.encode("latin-1") if isinstance(s, str) else bytes(s)
        cv = conv if isinstance(conv, str) else chr(int(conv[i]))
        pos, strand = int(recs["genome_pos"][i]), bytes(recs["strand"][i])
        if int(recs["times"][i]) != 1 or (skip is not None and int(skip[i])) or pos >= glen or cv not in "TA" or not 1 <= len(s) <= 1024:
            continue
        _, lo, hi = chrom_of(start_index, pos)
        G = R[1 if strand == b"-" else 0]
        want = "G" if cv == "T" else "C"
        limit = len(s) if call_len is None else min(len(s), int(call_len[i]))
        for k in range(limit):
            q = pos + k
            if q >= hi:
                break
            if chr(G[q]) != want or (quals is not None and int(bytes(quals[i])[k]) < min_qual):
                continue
            f = lo + hi - 1 - q if strand == b"-" else q
            (match if base_letter(s[k]) == want else other)[f] += 1
    return match, other


def qual_pool(t):
    return [0, max(t - 1, 0), t, min(t + 1, 255), 127, 128, 255]


def made_batch(R, start_index, seed, t, reps=3):
    """reads of every length of LENGTHS on both strands under both conversions, a third of the opposite-strand bases changed,
    quality bytes from {0, t - 1, t, t + 1, 127, 128, 255}; a few records that are not unique
    -> seqs, quals (bytes), recs, conv, call_len, ex (positions per read), words, skip"""
    import walt_amd
    rng = random.Random(seed)
    texts = [R[0].tobytes().decode("latin-1"), R[1].tobytes().decode("latin-1")]
    starts = [int(v) for v in start_index]
    rows = []
    for n in LENGTHS:
        for strand in (b"+", b"-"):
            for cv in "TA":
                for rep in range(reps):
                    c = rng.choice([k for k in range(len(starts) - 1) if starts[k + 1] - starts[k] >= n])
                    lo, hi = starts[c], starts[c + 1]
                    pos = hi - n if rep == 1 and rng.random() < 0.3 else rng.randrange(lo, hi - n + 1)
                    seq = list(make_read(rng, texts[1 if strand == b"-" else 0], pos, n, cv))
                    for k, ch in enumerate(seq):  # evidence of both kinds
                        if ch == ("G" if cv == "T" else "C") and rng.random() < 0.33:
                            seq[k] = rng.choice("ACGT")
                    times = 1 if rng.random() < 0.9 else rng.choice([0, 2])
                    rows.append(("".join(seq), bytes(rng.choice(qual_pool(t)) for _ in range(n)), pos, times, strand, cv))
    rng.shuffle(rows)
    n = len(rows)
    recs = np.zeros(n, dtype=walt_amd.best_match_dtype)
    recs["genome_pos"], recs["times"], recs["strand"] = [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows]
    conv = np.array([ord(r[5]) for r in rows], dtype=np.uint8)
    seqs, quals = [r[0] for r in rows], [r[1] for r in rows]
    call_len = [rng.choice([len(s), len(s), len(s) // 2, 0, len(s) + 3]) for s in seqs]
    ex = []
    for s in seqs:
        a = rng.randrange(0, len(s))
        ex.append(list(range(a, rng.randrange(a + 1, len(s) + 1))) if rng.random() < 0.3 else [])
    words = np.array([(e[0] | ((e[-1] + 1) << 16)) if e else 0 for e in ex], dtype=np.uint32)
    skip = np.array([rng.random() < 0.2 for _ in range(n)], dtype=np.uint8)
    return seqs, quals, recs, conv, call_len, ex, words, skip


# ---------------------------------------------------------------------------
# 1. hand-made batches through the host forms: the three kPile paths, alone and composed
# ---------------------------------------------------------------------------
def check_host_q(wa, idx, R, start_index, batch, t, composed, what, index_options):
    seqs, quals, recs, conv, call_len, ex, words, skip = batch
    glen = len(R[0])
    bases, offs = wa.pack_reads(seqs)
    q = wa.pack_quals(quals)
    assert q.size == bases.size and {0, 128, 255} <= set(q.tolist())
    if composed:
        kw = dict(call_len=call_len, skip=skip, excl=words, trim5=5, trim3=7)
        want = want_mate_q(R, start_index, seqs, recs, conv, quals, t, call_len, ex, skip, (5, 7))
        want_ev = expected_evidence_q(R, start_index, seqs, recs, conv, quals, t, call_len, skip)
    else:
        kw, skip = {}, None
        want = want_mate_q(R, start_index, seqs, recs, conv, quals, t)
        want_ev = expected_evidence_q(R, start_index, seqs, recs, conv, quals, t)
    plain = want_mate(R, start_index, seqs, recs, conv, kw.get("call_len"), ex if composed else None, skip, (5, 7) if composed else (0, 0))
    lost = sum(a != b for a, b in zip("".join(plain[0]), "".join(want[0])))
    mb = wa.MBias(0, 2) if composed else None
    try:
        for path in ("calls", "pile", "pile_rows"):
            index_options(idx, pile_rows=1 if path == "pile_rows" else 0)
            pile = idx.pileup() if path != "calls" else None
            ev = idx.pileup() if path != "calls" else None
            try:
                if mb is not None:
                    mb.clear()
                extra = dict(mbias=mb, mbias_table=1) if mb is not None else {}
                if pile is not None:
                    got = pile.add_batch(bases, offs, recs, conv, quals=q, min_qual=t, evidence=ev, **extra, **kw)
                else:
                    got = idx.meth_call_batch(bases, offs, recs, conv, quals=q, min_qual=t, **extra, **kw)
                assert_mate(got, want, "%s %s" % (what, path))
                if pile is not None:
                    m, u = pile_letters(start_index, glen, want[0], recs, skip)
                    assert_table(pile.extract(), R[0], start_index, m, u, "%s %s" % (what, path))
                    assert_planes(ev, want_ev[0], want_ev[1], "%s %s fused evidence" % (what, path))
                    ev.clear()
                    ev.add_evidence_batch(bases, offs, recs, conv, call_len=kw.get("call_len"), skip=skip, quals=q, min_qual=t)
                    assert_planes(ev, want_ev[0], want_ev[1], "%s %s evidence alone" % (what, path))
                if mb is not None:
                    assert np.array_equal(mb.read(1), want_table(want[0], offs, recs, skip)) and mb.read(0).sum() == 0, (what, path)
            finally:
                for p in (pile, ev):
                    if p is not None:
                        p.close()
    finally:
        if mb is not None:
            mb.close()
    return lost, sum(ch != "." for ch in "".join(want[0])), int(want_ev[0].sum() + want_ev[1].sum())


@pytest.mark.parametrize("t", FLOORS)
@pytest.mark.parametrize("genome", ["planted", "g1"])
def test_hand_made_batches_host_forms(wa, planted_idx, g1, g1_all, index_options, genome, t):
    if genome == "planted":
        db, idx, R = planted_idx
    else:
        db, idx, R = g1[0], g1_all, reference_bases(g1[0])
    batch = made_batch(R, db.start_index, 100 + t, t)
    for composed in (False, True):
        lost, kept, evidence = check_host_q(wa, idx, R, db.start_index, batch, t, composed, "%s t=%d composed=%d" % (genome, t, composed),
                                            index_options)
        assert lost > 50 and kept > 50 and evidence > 50, (lost, kept, evidence)


# ---------------------------------------------------------------------------
# 2. identities
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_se(wa, g1_all):
    _, seqs, scores = load("se_ct.fastq")
    seqs, scores = seqs[:700], scores[:700]
    bases, offs = wa.pack_reads(seqs)
    recs, _ = g1_all.map_se_batch(bases, offs)
    assert int((recs["times"] == 1).sum()) > 300
    return seqs, scores, bases, offs, recs


def test_floor_zero_is_byte_identical_and_floor_127_over_126_empties(wa, g1_all, golden_se, index_options):
    seqs, scores, bases, offs, recs = golden_se
    n = recs.size
    L = wa.lib()
    q = wa.pack_quals(scores)
    skip = (np.arange(n) % 4 == 0).astype(np.uint8)
    rec = np.ascontiguousarray(recs)

    def run(form, tail, with_pile):
        pile = g1_all.pileup() if with_pile else None
        calls = np.full(bases.size, 0x23, dtype=np.uint8)
        counts = np.zeros(n, dtype=wa.meth_counts_dtype)
        stats = np.zeros(1, dtype=wa.meth_stats_dtype)
        rc = form(g1_all.handle, pile.handle if pile is not None else None, bases.ctypes.data, offs.ctypes.data, n, rec.ctypes.data, 16,
                  None, 0, ord("T"), None, calls.ctypes.data, counts.ctypes.data, stats.ctypes.data, skip.ctypes.data, 1, None, None, 0,
                  0, 0, None, None, None, *tail)
        assert rc == 0, L.walt_last_error()
        sites = pile.extract()[0].tobytes() if pile is not None else b""
        if pile is not None:
            pile.close()
        return calls.tobytes(), counts.tobytes(), stats.tobytes(), sites

    for rows in (0, 1):
        index_options(g1_all, pile_rows=rows)
        for with_pile in (False, True):
            old = run(L.walt_meth_pileup_batch_ev, (), with_pile)
            new = run(L.walt_meth_pileup_batch_qual, (q.ctypes.data, 0), with_pile)
            null = run(L.walt_meth_pileup_batch_qual, (None, 0), with_pile)
            assert old == new == null and b"Z" in old[0] and (not with_pile or len(old[3]) > 1000)
            # every byte 126 under a floor of 127: no call anywhere, `reads` as it was
            q126 = np.full(bases.size, 126, dtype=np.uint8)
            calls, counts, stats, sites = run(L.walt_meth_pileup_batch_qual, (q126.ctypes.data, 127), with_pile)
            assert set(calls) == {ord(".")} and not any(counts) and sites == b""
            st, st_old = np.frombuffer(stats, dtype=wa.meth_stats_dtype), np.frombuffer(old[2], dtype=wa.meth_stats_dtype)
            assert int(st["reads"][0]) == int(st_old["reads"][0]) > 200 and not st["meth"].any() and not st["unmeth"].any()
            assert run(L.walt_meth_pileup_batch_qual, (q126.ctypes.data, 126), with_pile) == old
    # the binding: the same through the methods, and the evidence likewise
    plain = g1_all.meth_call_batch(bases, offs, recs, "T", skip=skip)
    same = g1_all.meth_call_batch(bases, offs, recs, "T", skip=skip, quals=q, min_qual=0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, same))
    ev, ev_q = g1_all.pileup(), g1_all.pileup()
    ev.add_evidence_batch(bases, offs, recs, "T")
    ev_q.add_evidence_batch(bases, offs, recs, "T", quals=q, min_qual=0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ev.read(), ev_q.read())) and int(ev.read()[0].sum()) > 1000
    ev.close()
    ev_q.close()


# ---------------------------------------------------------------------------
# 3. device forms: the quality array at every kind of address
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_device_forms_with_the_qualities_at_any_address(wa, g1, g1_all, index_options, shift):
    import torch
    db = g1[0]
    R = reference_bases(db)
    t = 53
    seqs, quals, recs, conv, call_len, ex, words, skip = made_batch(R, db.start_index, 7, t, reps=2)
    n = recs.size
    bases, offs = wa.pack_reads(seqs)
    q = wa.pack_quals(quals)
    cl = np.array(call_len, dtype=np.uint32)
    want = want_mate_q(R, db.start_index, seqs, recs, conv, quals, t, call_len, ex, skip, (2, 3))
    want_ev = expected_evidence_q(R, db.start_index, seqs, recs, conv, quals, t, call_len, skip)
    dev = torch.device("cuda", 0)
    d_bases, d_offs = torch.from_numpy(bases).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(n, 16).copy()).to(dev)
    d_conv, d_cl = torch.from_numpy(conv).to(dev), torch.from_numpy(cl.view(np.int32)).to(dev)
    d_skip, d_excl = torch.from_numpy(skip).to(dev), torch.from_numpy(words.view(np.int32)).to(dev)
    d_qraw = torch.zeros(bases.size + 48, dtype=torch.uint8, device=dev)
    at = (-d_qraw.data_ptr()) % 16 + shift
    d_qraw[at:at + bases.size] = torch.from_numpy(q).to(dev)
    assert (d_qraw.data_ptr() + at) % 16 == shift and d_bases.data_ptr() % 16 == 0
    st = torch.cuda.Stream(device=dev)
    for path in ("calls", "pile", "pile_rows"):
        index_options(g1_all, pile_rows=1 if path == "pile_rows" else 0)
        pile = g1_all.pileup() if path != "calls" else None
        ev = g1_all.pileup()
        d_calls = torch.full((bases.size + 48,), 0x23, dtype=torch.uint8, device=dev)
        c_at = (-d_calls.data_ptr()) % 16 + 5
        d_counts = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        try:
            args = (d_bases.data_ptr(), d_offs.data_ptr(), n, d_recs.data_ptr(), 16, d_conv.data_ptr(), 1, "T", d_cl.data_ptr(),
                    d_calls.data_ptr() + c_at, d_counts.data_ptr(), d_stats.data_ptr())
            kw = dict(stream=st.cuda_stream, d_skip=d_skip.data_ptr(), d_excl=d_excl.data_ptr(), trim5=2, trim3=3,
                      quals=d_qraw.data_ptr() + at, min_qual=t)
            if pile is not None:
                pile.add_batch_device(*args, evidence=ev, **kw)
            else:
                g1_all.meth_call_batch_device(*args, **kw)
                ev.add_evidence_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_recs.data_ptr(), 16, d_conv.data_ptr(), 1, "T",
                                             d_cl.data_ptr(), d_skip.data_ptr(), 1, stream=st.cuda_stream, quals=d_qraw.data_ptr() + at,
                                             min_qual=t)
            st.synchronize()
            calls = d_calls.cpu().numpy()
            assert (calls[:c_at] == 0x23).all() and (calls[c_at + bases.size:] == 0x23).all()
            got = (calls[c_at:c_at + bases.size], d_counts.cpu().numpy().reshape(-1).view(wa.meth_counts_dtype),
                   d_stats.cpu().numpy().view(wa.meth_stats_dtype))
            assert_mate(got, want, "device %s shift %d" % (path, shift))
            assert_planes(ev, want_ev[0], want_ev[1], "device %s shift %d" % (path, shift))
            if pile is not None:
                m, u = pile_letters(db.start_index, db.genome_len, want[0], recs, skip)
                assert_table(pile.extract(), R[0], db.start_index, m, u, "device %s shift %d" % (path, shift))
        finally:
            for p in (pile, ev):
                if p is not None:
                    p.close()
    # the verdict's device form, the calls it leaves on the device judged by the restatement
    rule = wa.nonconv_rule(min_meth=2)
    d_calls = torch.full((bases.size + 16,), 0x23, dtype=torch.uint8, device=dev)
    d_filt = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g1_all.meth_nonconv_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_recs.data_ptr(), rule, d_calls.data_ptr(), d_filt.data_ptr(),
                                     d_conv=d_conv.data_ptr(), d_call_len=d_cl.data_ptr(), stream=st.cuda_stream,
                                     quals=d_qraw.data_ptr() + at, min_qual=t)
    st.synchronize()
    unbounded = want_mate_q(R, db.start_index, seqs, recs, conv, quals, t, call_len)
    text = np.frombuffer("".join(unbounded[0]).encode(), dtype=np.uint8)
    assert d_calls.cpu().numpy()[:bases.size].tobytes() == text.tobytes()
    assert d_filt.cpu().numpy().tolist() == expected_verdicts(text, offs, recs["times"], (2, 0, 0, 0))[0].tolist()


# ---------------------------------------------------------------------------
# 4., 5., 6. a genome made for it: five neighbouring CpGs, three CHH cytosines, one C for a planted change
# ---------------------------------------------------------------------------
FIVE = "CGATT" * 5            # five neighbouring pairs, their C's five bases apart
CHH = "TTATTCATTATTCATTATTCATTATTATT"  # three cytosines in CHH context, no other C or G
QUIET = "AT" * 12


def qual_genome():
    rng = random.Random(404)
    rnd = lambda n, al="ACGT": "".join(rng.choice(al) for _ in range(n))
    where = {}
    c0 = rnd(211)
    for name, seg in (("five", FIVE), ("chh", CHH), ("site", "TTATTATTCATTATTATT")):
        c0 += QUIET
        where[name] = len(c0)
        c0 += seg
    c0 += QUIET + rnd(900)
    return Genome(["q0", "q1"], [c0, rnd(777)]), where


@pytest.fixture(scope="module")
def made(wa, scratch):
    g, where = qual_genome()
    db, path, idx = build_index(g, scratch, "qual_made")
    try:
        yield {"g": g, "where": where, "idx": idx, "db": db}
    finally:
        idx.close()
        remove_index(path)


def one_record(wa, pos, strand=b"+", n=1):
    recs = np.zeros(n, dtype=wa.best_match_dtype)
    recs["genome_pos"], recs["times"], recs["strand"] = pos, 1, strand
    return recs


def test_a_masked_cpg_breaks_the_run_for_the_pair_and_window_tables(wa, made):
    g, idx, at = made["g"], made["idx"], made["where"]["five"]
    pairs = find_pairs(g.text, g.start_index)
    lead = 7
    seq = g.text[at - lead:at + len(FIVE) + 4]  # a '+' read under conversion 'T', every C kept: five Z
    recs = one_record(wa, at - lead)
    bases, offs = wa.pack_reads([seq])
    cs = [lead + 5 * k for k in range(5)]
    for masked in ([], [cs[2]], [cs[0]], [cs[1], cs[3]]):
        q = np.full(len(seq), 73, dtype=np.uint8)
        q[masked] = 40
        ap, ep = idx.cpg_pairs(), idx.epialleles()
        try:
            calls, counts, _ = idx.meth_call_batch(bases, offs, recs, "T", pairs=ap, epi=ep, quals=q, min_qual=53)
            want = "".join("Z" if (i in cs and i not in masked) else "." for i in range(len(seq)))
            assert calls.tobytes().decode() == want
            assert int(counts["meth"][0][0]) == 5 - len(masked)
            args = (g.text, g.start_index, calls, offs, recs["genome_pos"], recs["times"], [b"+"])
            want_pairs = sites_of(pair_table(*args), pairs)
            want_epi = epi_sites_of(expected_epi(*args), pairs)
            assert sites_list(ap.extract()) == want_pairs and epi_list(ep.extract()) == want_epi
            # the middle one masked: a couple on either side, none across it, and no window at all
            assert (len(want_pairs), len(want_epi)) == {0: (4, 2), 1: (2, 0) if masked == [cs[2]] else (3, 1), 2: (0, 0)}[len(masked)]
        finally:
            ap.close()
            ep.close()


def test_a_planted_change_is_flagged_only_while_its_reads_pass_the_floor(wa, made):
    g, idx = made["g"], made["idx"]
    f = made["where"]["site"] + 8  # the segment's only C
    assert g.text[f] == "C" and "C" not in g.text[f - 8:f] + g.text[f + 1:f + 10]
    # '+' records under conversion 'A' are evidence at forward C; theirs shows T there
    seqs, quals = [], []
    for lead in (3, 9, 16, 20):
        s = list(g.text[f - lead:f + 12])
        s[lead] = "T"
        seqs.append("".join(s))
        quals.append(bytes(40 if k == lead else 73 for k in range(len(s))))
    recs = one_record(wa, 0, n=4)
    recs["genome_pos"] = [f - lead for lead in (3, 9, 16, 20)]
    bases, offs = wa.pack_reads(seqs)
    q = wa.pack_quals(quals)
    pile = idx.pileup()
    for t, flagged in ((53, False), (41, False), (40, True), (0, True)):
        ev = idx.pileup()
        ev.add_evidence_batch(bases, offs, recs, "A", quals=q, min_qual=t)
        want = expected_evidence_q(g.R, g.start_index, seqs, recs, "A", quals, t)
        assert_planes(ev, want[0], want[1], "floor %d" % t)
        match, other = ev.read()
        assert (int(match[f]), int(other[f])) == ((0, 4) if flagged else (0, 0))
        sites = pile.variants(ev, 0, g.genome_len, min_depth=1, max_percent=50)
        assert (f in [int(p) for p in sites["pos"]]) == flagged, (t, sites)
        ev.close()
    pile.close()


def test_the_verdict_is_made_from_the_masked_calls(wa, made):
    g, idx, at = made["g"], made["idx"], made["where"]["chh"]
    seq = g.text[at:at + len(CHH)]  # every C kept: three H
    hs = [i for i, ch in enumerate(seq) if ch == "C"]
    assert len(hs) == 3
    recs = one_record(wa, at)
    bases, offs = wa.pack_reads([seq])
    rule = wa.nonconv_rule(min_meth=3)
    filt, tally, calls = idx.meth_nonconv_batch(bases, offs, recs, rule, want_calls=True)
    assert filt.tolist() == [1] and calls.tobytes().decode() == "".join("H" if i in hs else "." for i in range(len(seq)))
    for k in range(3):
        q = np.full(len(seq), 60, dtype=np.uint8)
        q[hs[k]] = 52
        filt, tally, calls = idx.meth_nonconv_batch(bases, offs, recs, rule, want_calls=True, quals=q, min_qual=53)
        assert filt.tolist() == [0] and calls.tobytes().decode().count("H") == 2 and calls[hs[k]] == ord(".")
        assert tally_of(calls.tobytes())[0] == 2 and not fails(*tally_of(calls.tobytes()), (3, 0, 0, 0))
        filt, _, _ = idx.meth_nonconv_batch(bases, offs, recs, rule, quals=q, min_qual=52)
        assert filt.tolist() == [1]


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals(wa, g1_all, golden_se):
    seqs, scores, bases, offs, recs = golden_se
    n = recs.size
    L = wa.lib()
    q = wa.pack_quals(scores)
    rec = np.ascontiguousarray(recs)
    calls = np.zeros(bases.size, dtype=np.uint8)
    filt = np.zeros(n, dtype=np.uint8)
    rule = wa.nonconv_rule(min_meth=3)

    def pile_form(quals, min_qual):
        return L.walt_meth_pileup_batch_qual(g1_all.handle, None, bases.ctypes.data, offs.ctypes.data, n, rec.ctypes.data, 16, None, 0,
                                             ord("T"), None, calls.ctypes.data, None, None, None, 1, None, None, 0, 0, 0, None, None, None,
                                             quals, min_qual)

    def rule_form(quals, min_qual):
        return L.walt_meth_nonconv_batch_qual(g1_all.handle, bases.ctypes.data, offs.ctypes.data, n, rec.ctypes.data, 16, None, 0, ord("T"),
                                              None, None, rule.ctypes.data, filt.ctypes.data, 1, None, quals, min_qual)

    for form, name in ((pile_form, b"walt_meth_pileup_batch_qual"), (rule_form, b"walt_meth_nonconv_batch_qual")):
        assert form(q.ctypes.data, 127) == 0, L.walt_last_error()
        assert form(q.ctypes.data, 128) == wa.WALT_EINVAL and name in L.walt_last_error() and b"min_qual 128" in L.walt_last_error()
        assert form(None, 1) == wa.WALT_EINVAL and name in L.walt_last_error() and b"without quals" in L.walt_last_error()
        assert form(None, 0) == 0
    rc = L.walt_meth_pileup_batch_qual_device(g1_all.handle, None, None, None, n, None, 16, None, 0, ord("T"), None, None, None, None, None, 1,
                                              None, None, 0, 0, 0, None, None, None, None, 200, None)
    assert rc == wa.WALT_EINVAL and b"walt_meth_pileup_batch_qual_device" in L.walt_last_error()
    # the binding: an array of another size, another type, and a floor that is no floor
    for bad in (q[:-1], np.concatenate([q, q[:1]]), q.astype(np.uint16), q.reshape(1, -1)):
        with pytest.raises(ValueError, match="quals"):
            g1_all.meth_call_batch(bases, offs, recs, "T", quals=bad, min_qual=20)
        with pytest.raises(ValueError, match="quals"):
            g1_all.meth_nonconv_batch(bases, offs, recs, rule, quals=bad, min_qual=20)
    with pytest.raises(wa.WaltError):
        g1_all.meth_call_batch(bases, offs, recs, "T", quals=q, min_qual=128)
    with pytest.raises(wa.WaltError):
        g1_all.meth_call_batch(bases, offs, recs, "T", min_qual=5)
    # a refused call leaves nothing behind: the next call without qualities is the old one
    assert g1_all.meth_call_batch(bases, offs, recs, "T")[0].tobytes() == g1_all.meth_call_batch(bases, offs, recs, "T", quals=q)[0].tobytes()


# ---------------------------------------------------------------------------
# 8. command line: every run against the plain run's SAM and against its own
# ---------------------------------------------------------------------------
MQ = 20  # (tests/test_qual_cpu.py: at this floor every golden library loses between 10 % and 90 % of its letters)


def masked_xm(xm, qual, min_qual, offset=33):
    """XM:Z: and QUAL of one SAM record, both in SEQ order -> the XM:Z: of the run with the floor"""
    return "".join(ch if ord(qc) - offset >= min_qual else "." for ch, qc in zip(xm, qual))


def qual_sam_walk(sam_text, plain_text, names, seqs, min_qual, offset=33):
    """What a -M -sam run with a floor implies, from its own records (tests/test_gpu_variants.py sam_walk, plus the floor
    under the evidence and the tables by read position): per mate block of .methstats (single-end: one block) the totals and
    the bias table, and over forward positions meth, unmeth, match, other.  A record calls forward C's -- and is evidence at
    forward G's -- when the reference base under its first call letter is C; the floor may leave a record without a letter,
    so that letter is looked up in the same line of the run without the floor (plain_text).  -> (blocks, the four planes,
    records that have no letter there either)"""
    text = "".join(seqs)
    starts = [0]
    for s in seqs:
        starts.append(starts[-1] + len(s))
    glen = len(text)
    meth, unmeth, match, other = (np.zeros(glen, dtype=np.int64) for _ in range(4))
    blocks = {}
    undecided = 0
    lines, plain_lines = sam_text.splitlines(), plain_text.splitlines()
    assert len(lines) == len(plain_lines)
    for line, plain_line in zip(lines, plain_lines):
        if line.startswith("@"):
            continue
        p = line.split("\t")
        flag = int(p[1])
        if flag & SAM_SKIP:
            continue
        q = plain_line.split("\t")
        assert (q[0], q[2], q[3], q[9]) == (p[0], p[2], p[3], p[9])  # the same record
        mate = 1 if flag & 0x80 else 0
        b = blocks.setdefault(mate, {"reads": 0, "meth": np.zeros(4, dtype=np.int64), "unmeth": np.zeros(4, dtype=np.int64),
                                     "table": np.zeros((4, 2, 1024), dtype=np.uint64)})
        b["reads"] += 1
        xm = [t[5:] for t in p[11:] if t.startswith("XM:Z:")][0]
        c = names.index(p[2])
        pos0, seq, qual, hi = starts[c] + int(p[3]) - 1, p[9], p[10], starts[c + 1]
        n, rev = len(seq), bool(flag & 0x10)
        for k, ch in enumerate(xm):
            if ch == ".":
                continue
            ctx, m = "zxhu".index(ch.lower()), ch.isupper()
            b["meth" if m else "unmeth"][ctx] += 1
            b["table"][ctx, 0 if m else 1, n - 1 - k if rev else k] += 1
            (meth if m else unmeth)[pos0 + k] += 1
        plain_xm = strip_xm(plain_line)[1]
        letters = [k for k, ch in enumerate(plain_xm) if ch != "."]
        if not letters:
            undecided += 1
            continue
        opp = "G" if text[pos0 + letters[0]] == "C" else "C"
        for k in range(n):
            f = pos0 + k
            if starts[c] <= f < hi and text[f] == opp and ord(qual[k]) - offset >= min_qual:
                (match if base_letter(ord(seq[k])) == opp else other)[f] += 1
    return blocks, (meth, unmeth, match, other), undecided


def tables_text(cli, blocks, planes, paired):
    """-> (.methstats without its settings lines, .methcounts, .mbias) as the run writes them"""
    heads = ["mate1", "mate2"] if paired else [None]
    stats = methstats_text([(h, blocks[k]) for k, h in enumerate(heads)])
    counts = cli_texts(cli["names"], cli["R0"], cli["db"].start_index, planes[0], planes[1], 0 * planes[0], 0 * planes[0], 1, 0)[2]
    mbias = "".join((h + "\n" if h else "") + block_text(blocks[k]["table"]) for k, h in enumerate(heads))
    return stats, counts, mbias


@pytest.fixture(scope="module")
def cli(wa, scratch):
    from test_gpu_cpgpairs import read_fasta
    path = os.path.join(scratch, "qual_cli_g1.dbindex")
    wa.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    db = refio.DbIndex(path)
    names, seqs = read_fasta(os.path.join(refio.GOLDEN, "g1.fa"))
    R0 = reference_bases(db)[0]
    text = R0.tobytes().decode()
    starts = [int(v) for v in db.start_index]
    return {"db": db, "path": path, "names": names, "seqs": [text[starts[k]:starts[k + 1]] for k in range(len(names))], "R0": R0}


def check_against_the_plain_run(out, plain, min_qual, offset=33):
    """every line of the run is the plain run's but for XM:Z:, which is the plain one with '.' where QUAL is below the floor
    -> (letters kept, letters lost)"""
    kept = lost = 0
    rows, plain_rows = open(out).readlines(), open(plain).readlines()
    assert len(rows) == len(plain_rows)
    for a, b in zip(rows, plain_rows):
        (rest_a, xm_a), (rest_b, xm_b) = strip_xm(a), strip_xm(b)
        assert rest_a == rest_b
        assert (xm_a is None) == (xm_b is None)
        if xm_a is not None:
            want = masked_xm(xm_b, a.split("\t")[10], min_qual, offset)
            assert xm_a == want, "%s\n got  %s\n want %s" % (a.split("\t")[0], xm_a, want)
            kept += sum(ch != "." for ch in want)
            lost += sum(x != y for x, y in zip(want, xm_b))
    return kept, lost


@pytest.mark.parametrize("mode", ["r", "A", "pe", "P", "R", "RP"])
def test_cli_every_mode(cli, scratch, mode):
    out = os.path.join(scratch, "qual_cli_" + mode)
    paired = mode in ("pe", "P", "RP")
    base = ["-i", cli["path"]] + mode_args(scratch, mode) + ["-a", "-u", "-sam", "-M", "-MC", "-MB"]
    spelling = {"r": ["-MQ", str(MQ)], "A": ["-min-qual", str(MQ)], "pe": ["--min-base-quality", str(MQ)]}.get(mode, ["-MQ", str(MQ)])
    extra = {"A": ["-MV", "-MVD", "1", "-MVP", "0"]}.get(mode, [])
    log = run_walt(base + ["-o", out, "-v"] + spelling + extra)
    run_walt(base + ["-o", out + "-plain"] + extra)
    kept, lost = check_against_the_plain_run(out, out + "-plain", MQ)
    print("%s: %d letters kept, %d lost" % (mode, kept, lost))
    assert kept > 1000 and lost > 1000
    blocks, planes, undecided = qual_sam_walk(open(out).read(), open(out + "-plain").read(), cli["names"], cli["seqs"], MQ)
    stats, counts, mbias = tables_text(cli, blocks, planes, paired)
    line = "minqual\t%d\t33\n" % MQ
    assert open(out + ".methstats").read() == stats + line and line in log
    assert "minqual" not in open(out + "-plain.methstats").read()
    assert open(out + ".mbias").read() == mbias
    if not extra:
        assert open(out + ".methcounts").read() == counts
    else:  # -MV: the flagged positions, the totals and the masked counts of the masked evidence walk
        assert undecided == 0
        variants, vstats, masked_counts, (_, _, tot, rows) = cli_texts(cli["names"], cli["R0"], cli["db"].start_index, *planes, 1, 0)
        assert open(out + ".variants").read() == variants and open(out + ".variantstats").read() == vstats
        assert open(out + ".methcounts").read() == masked_counts and len(rows) >= 10
        # the floor acts on the evidence: the plain run judges more positions
        assert int(open(out + "-plain.variantstats").read().split()[1]) > tot[0] > 0
    # nothing but the calls differs
    for sfx in (".mapstats",):
        assert open(out + sfx, "rb").read() == open(out + "-plain" + sfx, "rb").read()


def test_cli_offset_64_filter_and_two_shares(cli, scratch):
    fq = os.path.join(refio.GOLDEN, "se_ct.fastq")
    out = os.path.join(scratch, "qual_cli_more")
    base = ["-i", cli["path"], "-a", "-u", "-sam", "-M", "-MC", "-MB"]
    run_walt(base + ["-r", fq, "-o", out, "-MQ", str(MQ)])
    # a copy with every quality byte raised by 31 is a Phred+64 file
    fq64 = os.path.join(scratch, "qual_se_ct_64.fastq")
    with open(fq64, "wb") as f:
        for k, l in enumerate(open(fq, "rb")):
            f.write(bytes(b + 31 for b in l.rstrip(b"\n")) + b"\n" if k % 4 == 3 else l)
    run_walt(base + ["-r", fq64, "-o", out + "-64", "-MQ", str(MQ), "--quality-offset", "64"])
    for sfx in (".methcounts", ".mbias", ".mapstats"):
        assert open(out + "-64" + sfx, "rb").read() == open(out + sfx, "rb").read(), sfx
    assert open(out + "-64.methstats").read() == open(out + ".methstats").read().replace("minqual\t%d\t33\n" % MQ, "minqual\t%d\t64\n" % MQ)
    assert [strip_xm(l)[1] for l in open(out + "-64")] == [strip_xm(l)[1] for l in open(out)]
    # two shares of small batches on one device named twice: the same files
    run_walt(base + ["-r", fq, "-o", out + "-g00", "-MQ", str(MQ), "-g", "0,0", "-N", "1000"])
    for sfx in ("", ".methstats", ".methcounts", ".mbias"):
        assert open(out + "-g00" + sfx, "rb").read() == open(out + sfx, "rb").read(), sfx
    # -F 3: the verdict is made from the masked calls -- a record is marked exactly when its own XM:Z: fails the rule -- and
    # the tables are those of the records that are left
    run_walt(base + ["-r", fq, "-o", out + "-F", "-MQ", str(MQ), "-F", "3"])
    run_walt(base + ["-r", fq, "-o", out + "-Fplain", "-F", "3"])
    marked = judged = 0
    for l in open(out + "-F"):
        p = l.split("\t")
        if l.startswith("@") or int(p[1]) & (0x4 | 0x100 | 0x400):
            continue
        xm = strip_xm(l)[1]
        judged += 1
        assert bool(int(p[1]) & 0x200) == bool(fails(*tally_of(xm.encode()), (3, 0, 0, 0))), l
        marked += bool(int(p[1]) & 0x200)
    plain_marked = sum(1 for l in open(out + "-Fplain") if not l.startswith("@") and int(l.split("\t")[1]) & 0x200)
    print("-F 3: %d of %d records marked, %d without the floor" % (marked, judged, plain_marked))
    assert 0 < marked < plain_marked
    blocks, planes, _ = qual_sam_walk(open(out + "-F").read(), open(out + "-Fplain").read(), cli["names"], cli["seqs"], MQ)
    stats, counts, mbias = tables_text(cli, blocks, planes, False)
    assert open(out + "-F.methstats").read() == stats + "minqual\t%d\t33\n" % MQ
    assert open(out + "-F.methcounts").read() == counts and open(out + "-F.mbias").read() == mbias


def test_cli_refusals(cli, scratch):
    import subprocess
    from test_gpu_cpgpairs import WALT_BIN
    fq = os.path.join(refio.GOLDEN, "se_ct.fastq")
    out = os.path.join(scratch, "qual_cli_refused")

    def refused(args, *words):
        pr = subprocess.run([WALT_BIN, "-i", cli["path"], "-o", out] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert pr.returncode != 0, args
        for w in words:
            assert w in pr.stdout, (args, w, pr.stdout[-500:])

    refused(["-r", fq, "-MQ", "20"], "-MQ", "nothing for it to do")
    refused(["-r", fq, "-M", "-MQ", "0"], "from 1 to 93")
    refused(["-r", fq, "-M", "-MQ", "94"], "from 1 to 93")
    refused(["-r", fq, "-M", "-MQ", "x"], "from 1 to 93")
    refused(["-r", fq, "-M", "-MQ", "20", "-MQO", "50"], "33 or 64")
    refused(["-r", fq, "-M", "-MQO", "64"], "-MQO", "goes with -MQ")
    refused(["-r", fq, "-M", "-MQ", "64", "-MQO", "64"], "127")
    # one quality line a character short: the message names the file and the read
    lines = open(fq).read().split("\n")
    lines[4 * 10 + 3] = lines[4 * 10 + 3][:-1]
    short = os.path.join(scratch, "qual_short.fastq")
    with open(short, "w") as f:
        f.write("\n".join(lines))
    refused(["-r", short, "-M", "-MQ", "20"], short, lines[4 * 10][1:].split(" ")[0], "quality line")
    # without -MQ the same file maps as it always did
    run_walt(["-i", cli["path"], "-r", short, "-o", out, "-M"])
