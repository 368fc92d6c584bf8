"""The overlap of a proper pair counted once (walt_pair_overlap_batch, walt_meth_pileup_batch_excl, bin/walt -NO; the
contract is in include/walt_amd.h, "overlap of a pair").

The expected values come from the restatement below.  It does not know the interval formula: for every read position
j of mate 2 it computes the forward position and asks whether that position is one mate 1 is called at -- a membership
test in a set -- and drops the letter `expected_read` of tests/test_gpu_meth.py gives there.  The interval word, the
totals, the calls, the per-read counts, the batch totals and the pile-up all follow from those dropped letters.  The
hand-made pairs carry their intervals written by hand as well."""
import os
import random

import numpy as np
import pytest

import refio
from test_gpu_meth import clip_point, expected_read, load, methstats_text, planted, reference_bases, run_walt, strip_xm
from test_gpu_pileup import assert_table, chrom_of, context_sums, counts_text, expected_counts, expected_table

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def forward_of(start_index, pos, strand, j):
    """forward position of read position j of a record at `pos`; None beyond its chromosome's end"""
    _, lo, hi = chrom_of(start_index, pos)
    q = pos + j
    if q >= hi:
        return None
    return lo + hi - 1 - q if strand in (b"-", "-") else q


def excluded_positions(start_index, genome_len, m1, m2, best_times, len1, len2, cl1=None, cl2=None):
    """-> (the read positions of mate 2 whose forward position is one of mate 1's called span, ascending; how many of
    them lie below mate 2's own call limit).  Nothing for a pair that is not a unique proper pair of unique mates on one
    chromosome."""
    p1, t1, s1 = int(m1["genome_pos"]), int(m1["times"]), bytes(m1["strand"])
    p2, t2, s2 = int(m2["genome_pos"]), int(m2["times"]), bytes(m2["strand"])
    if int(best_times) != 1 or t1 != 1 or t2 != 1 or p1 >= genome_len or p2 >= genome_len or len1 > 1024 or len2 > 1024:
        return [], 0
    if chrom_of(start_index, p1)[0] != chrom_of(start_index, p2)[0]:
        return [], 0
    lim1 = len1 if cl1 is None else min(len1, int(cl1))
    span1 = {forward_of(start_index, p1, s1, j) for j in range(lim1)} - {None}
    ex = [j for j in range(len2) if forward_of(start_index, p2, s2, j) in span1]
    lim2 = len2 if cl2 is None else min(len2, int(cl2))
    return ex, sum(j < lim2 for j in ex)


def word_of(ex):
    if not ex:
        return 0
    assert ex == list(range(ex[0], ex[-1] + 1)), "the excluded positions are one interval"
    return ex[0] | ((ex[-1] + 1) << 16)


def drop_letters(calls, ex):
    out = list(calls)
    for j in ex:
        out[j] = "."
    return "".join(out)


def counts_of(calls):
    c = [0] * 8
    for ch in calls:
        if ch != ".":
            c["zxhu".index(ch.lower()) + (0 if ch.isupper() else 4)] += 1
    return c


def expected_mate(R, start_index, seqs, recs, conv, call_len=None, ex=None, skip=None):
    """expected_batch of tests/test_gpu_meth.py with the letters at ex[i] dropped and the records with skip[i] left out
    of the totals -> (calls, counts [n, 8], totals)."""
    glen = len(R[0])
    calls, counts = [], np.zeros((len(seqs), 8), dtype=np.int64)
    tot = {"reads": 0, "meth": np.zeros(4, dtype=np.int64), "unmeth": np.zeros(4, dtype=np.int64)}
    for i, s in enumerate(seqs):
        cv = conv if isinstance(conv, str) else chr(int(conv[i]))
        c, _ = expected_read(R, start_index, s, recs["genome_pos"][i], recs["times"][i], bytes(recs["strand"][i]), cv,
                             None if call_len is None else call_len[i])
        if ex is not None:
            c = drop_letters(c, ex[i])
        calls.append(c)
        counts[i] = counts_of(c)
        if int(recs["times"][i]) == 1 and int(recs["genome_pos"][i]) < glen and cv in ("T", "A") and not (skip is not None and skip[i]):
            tot["reads"] += 1
            tot["meth"] += counts[i, :4]
            tot["unmeth"] += counts[i, 4:]
    return calls, counts, tot


def pile_letters(start_index, glen, calls, recs, skip=None, into=None):
    """every letter of every record with times == 1 (and no skip byte) walked to its forward position"""
    meth, unmeth = into if into is not None else (np.zeros(glen, dtype=np.int64), np.zeros(glen, dtype=np.int64))
    for i, c in enumerate(calls):
        if int(recs["times"][i]) != 1 or (skip is not None and skip[i]):
            continue
        for k, ch in enumerate(c):
            if ch != ".":
                f = forward_of(start_index, int(recs["genome_pos"][i]), bytes(recs["strand"][i]), k)
                (meth if ch.isupper() else unmeth)[f] += 1
    return meth, unmeth


def expected_pairs(R, start_index, s1, s2, res, conv1="T", conv2="A", cl1=None, cl2=None, skip=None):
    """-> dict: words (uint32[n]), totals [pairs, bases], ex (the positions per pair), w1 / w2 (expected_mate of each
    mate, mate 2's with the overlap dropped), pile (meth, unmeth of both mates)."""
    glen = len(R[0])
    ex, bases = [], 0
    for i in range(len(s1)):
        e, b = excluded_positions(start_index, glen, res["m1"][i], res["m2"][i], res["best_times"][i], len(s1[i]), len(s2[i]),
                                  None if cl1 is None else cl1[i], None if cl2 is None else cl2[i])
        ex.append(e)
        bases += b
    words = np.array([word_of(e) for e in ex], dtype=np.uint32)
    sk1 = None if skip is None else skip[:, 0]
    sk2 = None if skip is None else skip[:, 1]
    w1 = expected_mate(R, start_index, s1, res["m1"], conv1, cl1, None, sk1)
    w2 = expected_mate(R, start_index, s2, res["m2"], conv2, cl2, ex, sk2)
    pile = pile_letters(start_index, glen, w1[0], res["m1"], sk1)
    pile = pile_letters(start_index, glen, w2[0], res["m2"], sk2, into=pile)
    return {"words": words, "totals": [int((words != 0).sum()), bases], "ex": ex, "w1": w1, "w2": w2, "pile": pile}


def assert_mate(got, want, what):
    """got: (calls, counts, stats) of meth_call_batch / add_batch; want: expected_mate's"""
    calls, counts, stats = got
    text = calls.tobytes().decode("latin-1")
    at = 0
    for i, w in enumerate(want[0]):
        g = text[at:at + len(w)]
        assert g == w, "%s read %d calls differ:\n got  %s\n want %s" % (what, i, g, w)
        at += len(w)
    assert at == len(text)
    gc = np.concatenate([counts["meth"].astype(np.int64), counts["unmeth"].astype(np.int64)], axis=1)
    bad = np.nonzero((gc != want[1]).any(axis=1))[0]
    assert bad.size == 0, "%s counts differ at %s: got %s want %s" % (what, bad[:5], gc[bad[:5]], want[1][bad[:5]])
    assert int(stats["reads"][0]) == want[2]["reads"], (what, stats, want[2])
    assert np.array_equal(stats["meth"][0].astype(np.int64), want[2]["meth"]), (what, stats, want[2])
    assert np.array_equal(stats["unmeth"][0].astype(np.int64), want[2]["unmeth"]), (what, stats, want[2])


def run_pairs(idx, R, start_index, s1, s2, res, conv1="T", conv2="A", cl1=None, cl2=None, skip=None, what=""):
    """pair_overlap, then mate 1 as always and mate 2 with the interval, both into one pile-up; everything compared with
    expected_pairs.  -> (expected_pairs' dict, excl)"""
    import walt_amd
    want = expected_pairs(R, start_index, s1, s2, res, conv1, conv2, cl1, cl2, skip)
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    excl, totals = idx.pair_overlap(res, o1, o2, cl1, cl2)
    assert excl.dtype == np.uint32 and excl.tolist() == want["words"].tolist(), (
        what, [(i, hex(int(g)), hex(int(w))) for i, (g, w) in enumerate(zip(excl, want["words"])) if g != w][:5])
    assert totals.tolist() == want["totals"], (what, totals, want["totals"])
    pile = idx.pileup()
    try:
        got1 = pile.add_batch(b1, o1, res["m1"], conv1, call_len=cl1, skip=None if skip is None else skip[:, 0])
        got2 = pile.add_batch(b2, o2, res["m2"], conv2, call_len=cl2, skip=None if skip is None else skip[:, 1], excl=excl)
        assert_mate(got1, want["w1"], what + " mate 1")
        assert_mate(got2, want["w2"], what + " mate 2")
        # without a pile-up: the same per-read outputs
        alone = idx.meth_call_batch(b2, o2, res["m2"], conv2, call_len=cl2, skip=None if skip is None else skip[:, 1], excl=excl)
        assert all(a.tobytes() == g.tobytes() for a, g in zip(alone, got2)), what
        sites = assert_table(pile.extract(), R[0], start_index, want["pile"][0], want["pile"][1], what)
    finally:
        pile.close()
    want["sites"], want["stats"] = sites, (got1[2], got2[2])
    return want, excl


# ---------------------------------------------------------------------------
# 1. hand-made pairs on the planted genome
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_idx(scratch):
    import walt_amd
    fa, _, _, _ = planted(scratch)
    path = os.path.join(scratch, "overlap_planted.dbindex")
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield db, idx, reference_bases(db)
    idx.close()


# (chromosome, forward start of mate 1 inside it, length, strand, the same of mate 2, best_times, times 1, times 2,
#  call_len 1, call_len 2, the interval WRITTEN BY HAND or None).  A '-' mate 2 at forward [a, a + n) has read
#  position j on forward position a + n - 1 - j.  chrP1 has 1,580 bases, chrS 50.
HAND = [
    (0, 100, 60, "+", 160, 60, "-", 1, 1, 1, None, None, None),        # abutting: overlap of 0
    (0, 100, 60, "+", 159, 60, "-", 1, 1, 1, None, None, (59, 60)),    # overlap of 1: forward 159 = j 59
    (0, 325, 22, "+", 300, 60, "-", 1, 1, 1, None, None, (13, 35)),    # mate 1 strictly inside mate 2; across slice boundaries
    (0, 500, 100, "+", 520, 60, "-", 1, 1, 1, None, None, (0, 60)),    # mate 2 wholly inside mate 1
    (0, 600, 60, "-", 570, 60, "+", 1, 1, 1, None, None, (30, 60)),    # the other orientation
    (0, 725, 22, "-", 700, 60, "+", 1, 1, 1, None, None, (25, 47)),    # ... mate 1 inside mate 2
    (0, 830, 60, "+", 800, 60, "-", 1, 1, 1, None, None, (0, 30)),     # dovetail: mate 2 starts in front of mate 1
    (0, 900, 60, "+", 910, 60, "-", 1, 1, 1, 30, None, (40, 60)),      # mate 1 clipped at 30: its span is [900, 930)
    (0, 1000, 60, "-", 990, 60, "+", 1, 1, 1, 20, None, (50, 60)),     # a '-' mate 1 clipped at 20: its span is [1040, 1060)
    (0, 1100, 100, "+", 1120, 60, "-", 1, 1, 1, None, 45, (0, 60)),    # mate 2 clipped at 45: the interval stays, 45 bases
    (0, 1250, 60, "+", 1260, 60, "-", 1, 1, 1, 0, None, None),         # mate 1 clipped at 0: no span
    (1, 20, 40, "+", 5, 45, "-", 1, 1, 1, None, None, (0, 30)),        # mate 1 runs 10 bases over chrS's end: span [20, 50)
    (1, 0, 50, "-", 30, 40, "+", 1, 1, 1, None, None, (0, 20)),        # mate 2 runs 20 bases over the end
    (0, 1300, 100, "+", 1320, 60, "-", 0, 1, 1, None, None, None),     # no proper pair: everything counted
    (0, 1300, 100, "+", 1320, 60, "-", 2, 1, 1, None, None, None),     # an ambiguous pair: everything counted
    (0, 1300, 100, "+", 1320, 60, "-", 1, 2, 1, None, None, None),     # a made-up record: mate 1 not unique
    (0, 1300, 100, "+", 1320, 60, "-", 1, 1, 0, None, None, None),     # ... mate 2 unmapped
    (0, 1400, 60, "+", 1430, 60, "+", 1, 1, 1, None, None, (0, 30)),   # equal strands: the same formula
    (0, 1400, 60, "-", 1430, 60, "-", 1, 1, 1, None, None, (30, 60)),
    (0, 100, 60, "+", 100, 60, "-", 1, 1, 1, None, None, (0, 60)),     # the same span
]


def hand_pair(db, R, k, case):
    """-> (mate 1's read, mate 2's read, the pair's record fields) of one HAND row; the reads are the strand genome
    under the mate's conversion, about half of the C / G kept (deterministic per row)"""
    rng = random.Random(1000 + k)
    c, a1, n1, st1, a2, n2, st2, bt, t1, t2 = case[:10]
    lo, hi = int(db.start_index[c]), int(db.start_index[c + 1])
    out = []
    for a, n, st, frm, to in ((a1, n1, st1, "C", "T"), (a2, n2, st2, "G", "A")):
        p = lo + a if st == "+" else hi - a - n
        G = R[1 if st == "-" else 0]
        seq = "".join(chr(G[p + i]) if p + i < len(G) else "A" for i in range(n))
        out.append((p, "".join(to if (ch == frm and rng.random() < 0.5) else ch for ch in seq)))
    return out[0][1], out[1][1], (out[0][0], t1, st1.encode(), out[1][0], t2, st2.encode(), bt)


def hand_batch(db, R, n):
    import walt_amd
    s1, s2 = [], []
    res = np.zeros(n, dtype=walt_amd.pair_result_dtype)
    cl1, cl2, by_hand = [], [], []
    for i in range(n):
        k = (i + n) % len(HAND)
        r1, r2, (p1, t1, st1, p2, t2, st2, bt) = hand_pair(db, R, k, HAND[k])
        s1.append(r1)
        s2.append(r2)
        res["m1"]["genome_pos"][i], res["m1"]["times"][i], res["m1"]["strand"][i] = p1, t1, st1
        res["m2"]["genome_pos"][i], res["m2"]["times"][i], res["m2"]["strand"][i] = p2, t2, st2
        res["best_times"][i] = bt
        cl1.append(len(r1) if HAND[k][10] is None else HAND[k][10])
        cl2.append(len(r2) if HAND[k][11] is None else HAND[k][11])
        by_hand.append(0 if HAND[k][12] is None else HAND[k][12][0] | (HAND[k][12][1] << 16))
    return s1, s2, res, cl1, cl2, by_hand


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_hand_made_pairs(planted_idx, n):
    db, idx, R = planted_idx
    assert [int(db.start_index[c + 1] - db.start_index[c]) for c in (0, 1)] == [1580, 50]
    s1, s2, res, cl1, cl2, by_hand = hand_batch(db, R, n)
    want, excl = run_pairs(idx, R, db.start_index, s1, s2, res, "T", "A", cl1, cl2, what="hand-made n=%d" % n)
    assert excl.tolist() == by_hand
    if n >= len(HAND):
        # mate 2 clipped at 45 inside an interval of 60: 45 bases; every letter of a mate 2 inside mate 1 is gone
        k = [(i + n) % len(HAND) for i in range(n)]
        i9, i3 = k.index(9), k.index(3)
        assert excluded_positions(db.start_index, db.genome_len, res["m1"][i9], res["m2"][i9], 1, 100, 60, None, 45)[1] == 45
        assert set(want["w2"][0][i3]) == {"."} and want["w2"][1][i3].sum() == 0
        assert want["totals"][0] == sum(w != 0 for w in by_hand) and want["totals"][1] > want["totals"][0]
        # the rows that leave everything counted have letters in their overlap on both mates
        both = 0
        for i in range(len(HAND)):
            if HAND[k[i]][7] != 1:
                both += sum(ch != "." for ch in want["w2"][0][i][:40])
        assert both > 0


def test_pair_outside_the_genome_and_on_two_chromosomes(planted_idx):
    import walt_amd
    db, idx, R = planted_idx
    res = np.zeros(4, dtype=walt_amd.pair_result_dtype)
    res["best_times"] = 1
    res["m1"]["times"] = res["m2"]["times"] = 1
    res["m1"]["strand"], res["m2"]["strand"] = b"+", b"-"
    e0 = int(db.start_index[1])
    res["m1"]["genome_pos"] = [db.genome_len + 5, 100, e0 - 30, 0xFFFFFFFF]
    res["m2"]["genome_pos"] = [100, db.genome_len, e0 + 1, 0xFFFFFFFF]  # (the third: mate 1 ends chrP1, mate 2 lies on chrS)
    s1, s2 = ["ACGT" * 15] * 4, ["TGCA" * 10] * 4
    want, excl = run_pairs(idx, R, db.start_index, s1, s2, res, what="outside")
    assert excl.tolist() == [0, 0, 0, 0] and want["totals"] == [0, 0]


# ---------------------------------------------------------------------------
# 2. the golden libraries
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "overlap_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    return refio.DbIndex(path), path


@pytest.fixture(scope="module")
def g1_all(g1):
    import walt_amd
    idx = walt_amd.Index.open(g1[1], device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield idx
    idx.close()


# pairs with a non-empty interval and mate-2 bases excluded, counted on the oracle's records (tests/test_overlap_cpu.py
# counts them again without a device)
GOLDEN_TOTALS = {"pe_1.fastq": (123, 5092), "pe150_1.fastq": (153, 11637)}


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("files", [("pe_1.fastq", "pe_2.fastq"), ("pe150_1.fastq", "pe150_2.fastq")])
def test_golden_pairs_count_their_overlap_once(g1, g1_all, index_options, files, rows):
    import walt_amd
    db, _ = g1
    R = reference_bases(db)
    index_options(g1_all, pile_rows=rows)
    _, s1, _ = load(files[0])
    _, s2, _ = load(files[1])
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    want, excl = run_pairs(g1_all, R, db.start_index, s1, s2, res, what=files[0])
    assert want["totals"][0] >= 100
    assert tuple(want["totals"]) == GOLDEN_TOTALS[files[0]]
    # the per-context sums of the one table equal the two mates' totals
    m, u = context_sums(want["sites"])
    st1, st2 = want["stats"]
    assert np.array_equal(m, (st1["meth"][0] + st2["meth"][0]).astype(np.int64))
    assert np.array_equal(u, (st1["unmeth"][0] + st2["unmeth"][0]).astype(np.int64))
    # for every unique proper pair, no forward position receives a call from both mates -- from the GPU's own letters
    c1 = g1_all.meth_call_batch(b1, o1, res["m1"], "T")[0].tobytes().decode()
    c2 = g1_all.meth_call_batch(b2, o2, res["m2"], "A", excl=excl)[0].tobytes().decode()
    plain2 = g1_all.meth_call_batch(b2, o2, res["m2"], "A")[0].tobytes().decode()
    shared_before = checked = 0
    for i in np.nonzero(res["best_times"] == 1)[0]:
        f1 = {forward_of(db.start_index, int(res["m1"]["genome_pos"][i]), bytes(res["m1"]["strand"][i]), k)
              for k, ch in enumerate(c1[int(o1[i]):int(o1[i + 1])]) if ch != "."}
        at = lambda text: {forward_of(db.start_index, int(res["m2"]["genome_pos"][i]), bytes(res["m2"]["strand"][i]), k)
                           for k, ch in enumerate(text[int(o2[i]):int(o2[i + 1])]) if ch != "."}
        assert not (f1 & at(c2)), (files[0], int(i))
        shared_before += len(f1 & at(plain2))
        checked += 1
    assert checked > 300 and shared_before > 100  # (without the interval they did share positions)
    # both counted: what tests/test_gpu_pileup.py expects, and more calls than with the interval
    acc = expected_counts(R, db.start_index, s1, res["m1"], "T")
    acc = expected_counts(R, db.start_index, s2, res["m2"], "A", into=acc)
    assert int(acc[0].sum() + acc[1].sum()) > int(want["pile"][0].sum() + want["pile"][1].sum())


def test_excl_none_is_byte_identical_to_the_older_entry_points(g1, g1_all):
    import walt_amd
    db, _ = g1
    _, s2, _ = load("pe_2.fastq")
    _, s1, _ = load("pe_1.fastq")
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    n = len(s2)
    zeros = np.zeros(n, dtype=np.uint32)
    skip = (np.arange(n) % 3 == 0).astype(np.uint8)
    plain = g1_all.meth_call_batch(b2, o2, res["m2"], "A")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, g1_all.meth_call_batch(b2, o2, res["m2"], "A", excl=zeros)))
    skipped = g1_all.meth_call_batch(b2, o2, res["m2"], "A", skip=skip)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(skipped, g1_all.meth_call_batch(b2, o2, res["m2"], "A", skip=skip, excl=zeros)))
    tables = []
    for kw in ({}, {"excl": zeros}, {"skip": np.zeros(n, dtype=np.uint8)}, {"skip": np.zeros(n, dtype=np.uint8), "excl": zeros}):
        pile = g1_all.pileup()
        try:
            got = pile.add_batch(b2, o2, res["m2"], "A", **kw)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, got)), kw.keys()
            tables.append(pile.extract()[0].tobytes())
        finally:
            pile.close()
    assert len(set(tables)) == 1 and len(tables[0]) > 16 * 100


def test_skip_and_excl_together(g1, g1_all):
    import walt_amd
    db, _ = g1
    R = reference_bases(db)
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    s1, s2 = s1[:500] + s1[:500], s2[:500] + s2[:500]  # every pair twice: the second copies are duplicates
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    dd = walt_amd.Dedup(initial_slots=64)
    try:
        dup = dd.add_pairs(res, "T")
    finally:
        dd.close()
    assert int(dup[500:, 0].sum()) > 250 and int(dup[:500].sum()) == 0
    want, excl = run_pairs(g1_all, R, db.start_index, s1, s2, res, skip=dup, what="skip and excl")
    # the totals of the overlap kernel count the duplicates too: twice the first half's
    first = expected_pairs(R, db.start_index, s1[:500], s2[:500], res[:500])
    assert want["totals"] == [2 * first["totals"][0], 2 * first["totals"][1]] and first["totals"][0] > 50
    # ... while the pile-up holds the first copies only
    assert np.array_equal(want["pile"][0], first["pile"][0]) and np.array_equal(want["pile"][1], first["pile"][1])


def test_device_form_on_a_stream(g1, g1_all):
    """the overlap kernel enqueued in front of mate 2's call on one stream; totals accumulate; refusals"""
    import torch
    import walt_amd
    db, _ = g1
    _, s1, _ = load("pe150_1.fastq")
    _, s2, _ = load("pe150_2.fastq")
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    n = len(s1)
    rng = random.Random(3)
    cl1 = np.array([rng.choice([len(s), len(s), len(s) // 2, 0, len(s) + 3]) for s in s1], dtype=np.uint32)
    cl2 = np.array([rng.choice([len(s), len(s), len(s) // 2, 0, len(s) + 3]) for s in s2], dtype=np.uint32)
    excl, totals = g1_all.pair_overlap(res, o1, o2, cl1, cl2)
    host_pile, pile = g1_all.pileup(), g1_all.pileup()
    try:
        host = host_pile.add_batch(b2, o2, res["m2"], "A", call_len=cl2, excl=excl)
        want_sites, _ = host_pile.extract()
        dev = torch.device("cuda", 0)
        d_res = torch.from_numpy(res.view(np.uint8).reshape(n, 64)).to(dev)
        d_o1, d_o2 = torch.from_numpy(o1.view(np.int64)).to(dev), torch.from_numpy(o2.view(np.int64)).to(dev)
        d_cl1, d_cl2 = torch.from_numpy(cl1.view(np.int32)).to(dev), torch.from_numpy(cl2.view(np.int32)).to(dev)
        d_b2 = torch.from_numpy(b2).to(dev)
        d_excl = torch.full((n,), 0x23232323, dtype=torch.int32, device=dev)
        d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
        d_calls = torch.zeros(b2.size + 32, dtype=torch.uint8, device=dev)
        d_counts = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        for _ in range(2):  # (totals are accumulated into)
            g1_all.pair_overlap_device(d_res.data_ptr(), d_o1.data_ptr(), d_o2.data_ptr(), n, d_excl.data_ptr(), d_cl1.data_ptr(),
                                       d_cl2.data_ptr(), d_tot.data_ptr(), stream=st.cuda_stream)
        pile.add_batch_device(d_b2.data_ptr(), d_o2.data_ptr(), n, d_res.data_ptr() + 16, 64, None, 1, "A", d_cl2.data_ptr(),
                              d_calls.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(), stream=st.cuda_stream,
                              d_excl=d_excl.data_ptr())
        st.synchronize()
        assert d_excl.cpu().numpy().view(np.uint32).tolist() == excl.tolist()
        assert d_tot.cpu().numpy().tolist() == [2 * int(totals[0]), 2 * int(totals[1])] and int(totals[0]) > 100
        assert d_calls.cpu().numpy()[:b2.size].tobytes() == host[0].tobytes()
        assert d_counts.cpu().numpy().tobytes() == host[1].tobytes() and d_stats.cpu().numpy().tobytes() == host[2].tobytes()
        assert pile.extract()[0].tobytes() == want_sites.tobytes()
        # no call_len, no totals
        d_excl.fill_(0x23232323)
        g1_all.pair_overlap_device(d_res.data_ptr(), d_o1.data_ptr(), d_o2.data_ptr(), n, d_excl.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert d_excl.cpu().numpy().view(np.uint32).tolist() == g1_all.pair_overlap(res, o1, o2)[0].tolist()
        # refusals name the call
        L = walt_amd.lib()
        rc = L.walt_pair_overlap_batch_device(g1_all.handle, d_res.data_ptr() + 2, d_o1.data_ptr(), d_o2.data_ptr(), n, None, None,
                                              d_excl.data_ptr(), None, None)
        assert rc == walt_amd.WALT_EINVAL and b"walt_pair_overlap_batch_device" in L.walt_last_error() and b"aligned" in L.walt_last_error()
        rc = L.walt_pair_overlap_batch_device(g1_all.handle, d_res.data_ptr(), d_o1.data_ptr(), d_o2.data_ptr(), n, None, None,
                                              d_excl.data_ptr(), d_tot.data_ptr() + 4, None)
        assert rc == walt_amd.WALT_EINVAL and b"aligned" in L.walt_last_error()
        rc = L.walt_pair_overlap_batch_device(g1_all.handle, None, d_o1.data_ptr(), d_o2.data_ptr(), n, None, None, d_excl.data_ptr(),
                                              None, None)
        assert rc == walt_amd.WALT_EINVAL
        rc = L.walt_meth_pileup_batch_excl_device(g1_all.handle, None, d_b2.data_ptr(), d_o2.data_ptr(), n, d_res.data_ptr() + 16, 64,
                                                  None, 1, ord("A"), None, d_calls.data_ptr(), None, None, None, 1,
                                                  d_excl.data_ptr() + 2, None)
        assert rc == walt_amd.WALT_EINVAL and b"excl" in L.walt_last_error()
        assert (d_excl.cpu().numpy().view(np.uint32) == g1_all.pair_overlap(res, o1, o2)[0]).all()  # (nothing was enqueued)
    finally:
        pile.close()
        host_pile.close()


def test_an_index_without_reference_serves_the_overlap(g1, g1_all):
    import walt_amd
    db, path = g1
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    s1, s2 = s1[:300], s2[:300]
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT)
    try:
        assert not idx.has_reference
        excl, totals = idx.pair_overlap(res, o1 + np.uint64(7), o2)  # (only the differences of the offsets matter)
        want = [word_of(excluded_positions(db.start_index, db.genome_len, res["m1"][i], res["m2"][i], res["best_times"][i],
                                           len(s1[i]), len(s2[i]))[0]) for i in range(len(s1))]
        assert excl.tolist() == want and int(totals[0]) == sum(w != 0 for w in want) > 20
        assert excl.tolist() == g1_all.pair_overlap(res, o1, o2)[0].tolist()
    finally:
        idx.close()


# ---------------------------------------------------------------------------
# 3. command line
# ---------------------------------------------------------------------------
def cli_library(g1_all, mode, s_a, s_b):
    """the records of a run on files (a, b) = (pe_1, pe_2) in `mode`, put into USER order (the read of file -1 first)
    -> (user's mate 1 reads, mate 2 reads, records in user order, conv of mate 1, conv of mate 2)"""
    import walt_amd
    b1, o1 = walt_amd.pack_reads(s_a)
    b2, o2 = walt_amd.pack_reads(s_b)
    if mode == "RP":
        res, conv, _ = g1_all.map_pe_rpbat_batch(b1, o1, b2, o2)
        return s_a, s_b, res, conv[:, 0], conv[:, 1]
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    if mode == "pe":
        return s_a, s_b, res, "T", "A"
    # -P: the run gets -1 pe_2 -2 pe_1; the user's mate 1 is the A-rich read, the second record of the mapping call
    user = res.copy()
    user["m1"], user["m2"] = res["m2"], res["m1"]
    return s_b, s_a, user, "A", "T"


def overlap_line(totals):
    return "overlap\t%d\t%d\n" % (totals[0], totals[1])


def check_sam_xm(path, u1, u2, res, want):
    """every line's XM:Z: against the restatement; lines come in user order (mate 1, then mate 2)"""
    rows = [l for l in open(path) if not l.startswith("@")]
    assert len(rows) == 2 * len(u1)
    n_xm = dotted = 0
    for k, ml in enumerate(rows):
        _, xm = strip_xm(ml)
        i, mate = k // 2, k % 2
        rec = res["m2" if mate else "m1"][i]
        exp = want["w2" if mate else "w1"][0][i]
        assert (xm is not None) == (int(rec["times"]) >= 1), ml
        if xm is not None:
            n_xm += 1
            assert xm == (exp[::-1] if bytes(rec["strand"]) == b"-" else exp), (k, ml)
            if mate and want["ex"][i]:
                assert set(exp[want["ex"][i][0]:want["ex"][i][-1] + 1]) == {"."}
                dotted += 1
    assert n_xm > 1000 and dotted > 100


@pytest.mark.parametrize("mode", ["pe", "P", "RP"])
def test_cli_no_overlap(g1, g1_all, scratch, mode):
    db, path = g1
    R = reference_bases(db)
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    u1, u2, res, cv1, cv2 = cli_library(g1_all, mode, s1, s2)
    want = expected_pairs(R, db.start_index, u1, u2, res, cv1, cv2)
    assert want["totals"][0] >= 100
    sites, off = expected_table(R[0], db.start_index, *want["pile"])
    assert sites.size > 1000 and off == [0, 0]
    text = counts_text(db, sites)
    stats = methstats_text([("mate1", want["w1"][2]), ("mate2", want["w2"][2])]) + overlap_line(want["totals"])
    reads = ["-1", f2, "-2", f1, "-P"] if mode == "P" else ["-1", f1, "-2", f2] + (["-RP"] if mode == "RP" else [])
    out = os.path.join(scratch, "overlap_cli_" + mode)
    # -sam -M
    run_walt(["-i", path] + reads + ["-o", out + "_M", "-a", "-u", "-sam", "-M", "-NO"])
    assert open(out + "_M.methstats").read() == stats
    assert not os.path.exists(out + "_M.methcounts")
    check_sam_xm(out + "_M", u1, u2, res, want)
    # -MC alone (.mr lines), under the second spelling
    log = run_walt(["-i", path] + reads + ["-o", out + "_MC", "-a", "-u", "-MC", "-no-overlap", "-v"])
    assert open(out + "_MC.methcounts").read() == text
    assert not os.path.exists(out + "_MC.methstats") and overlap_line(want["totals"]) in log
    # both, under the third spelling
    run_walt(["-i", path] + reads + ["-o", out + "_both", "-a", "-u", "-sam", "-M", "-MC", "--no-overlap"])
    assert open(out + "_both.methcounts").read() == text and open(out + "_both.methstats").read() == stats
    assert open(out + "_both", "rb").read() == open(out + "_M", "rb").read()
    # the same command without -NO: both mates counted, as tests/test_gpu_pileup.py expects; nothing else differs
    run_walt(["-i", path] + reads + ["-o", out + "_plain", "-a", "-u", "-sam", "-M", "-MC"])
    acc = expected_counts(R, db.start_index, u1, res["m1"], cv1)
    acc = expected_counts(R, db.start_index, u2, res["m2"], cv2, into=acc)
    both_sites, _ = expected_table(R[0], db.start_index, *acc)
    assert open(out + "_plain.methcounts").read() == counts_text(db, both_sites) != text
    plain_stats = open(out + "_plain.methstats").read()
    assert "overlap" not in plain_stats
    assert plain_stats == methstats_text([("mate1", expected_mate(R, db.start_index, u1, res["m1"], cv1)[2]),
                                          ("mate2", expected_mate(R, db.start_index, u2, res["m2"], cv2)[2])])
    assert open(out + "_plain.mapstats").read() == open(out + "_both.mapstats").read()
    assert [strip_xm(l)[0] for l in open(out + "_plain")] == [strip_xm(l)[0] for l in open(out + "_both")]


def test_cli_no_overlap_in_small_batches_on_two_shares(g1, g1_all, scratch):
    import walt_amd
    from test_gpu_dedup import doubled, loaded
    db, path = g1
    R = reference_bases(db)
    # (records without N: the loader's draw for an N depends on the record's place in its -N batch)
    (f1, _), (f2, _) = doubled(scratch, "overlap_n64", [os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")])
    s1, s2 = loaded(f1), loaded(f2)
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    want = expected_pairs(R, db.start_index, s1, s2, res)
    assert want["totals"][0] >= 100
    sites, _ = expected_table(R[0], db.start_index, *want["pile"])
    text = counts_text(db, sites)
    stats = methstats_text([("mate1", want["w1"][2]), ("mate2", want["w2"][2])]) + overlap_line(want["totals"])
    a, b = os.path.join(scratch, "overlap_cli_one"), os.path.join(scratch, "overlap_cli_n64")
    common = ["-i", path, "-1", f1, "-2", f2, "-a", "-u", "-sam", "-M", "-MC", "-NO"]
    run_walt(common + ["-o", a])
    run_walt(common + ["-o", b, "-N", "64", "-g", "0,0"])
    for out in (b, a):  # each run against the restatement, then against each other
        assert open(out + ".methcounts").read() == text, out
        assert open(out + ".methstats").read() == stats, out
        check_sam_xm(out, s1, s2, res, want)
    for sfx in ("", ".methcounts", ".methstats", ".mapstats"):
        assert open(a + sfx, "rb").read() == open(b + sfx, "rb").read(), sfx


def test_cli_no_overlap_with_clipping(g1, g1_all, scratch):
    import walt_amd
    db, path = g1
    R = reference_bases(db)
    args = refio.golden_meta()["cases"]["se_clip_sam_au"]["args"]
    adaptor = args[args.index("-C") + 1]
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    seqs, cls = [], []
    for fq in (f1, f2):
        got = []
        for _, sq, _ in refio.load_fastq_batches(fq, 10 ** 7, adaptor):
            got += sq
        raw = [l.rstrip(b"\n") for l in open(fq, "rb").readlines()[1::4]]
        seqs.append(got)
        cls.append([clip_point(adaptor.encode(), bytearray(r)) for r in raw])
    b1, o1 = walt_amd.pack_reads(seqs[0])
    b2, o2 = walt_amd.pack_reads(seqs[1])
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    want = expected_pairs(R, db.start_index, seqs[0], seqs[1], res, "T", "A", cls[0], cls[1])
    sites, _ = expected_table(R[0], db.start_index, *want["pile"])
    out = os.path.join(scratch, "overlap_cli_clip")
    run_walt(["-i", path, "-1", f1, "-2", f2, "-o", out, "-a", "-u", "-M", "-MC", "-NO", "-C", adaptor])
    assert open(out + ".methcounts").read() == counts_text(db, sites)
    assert open(out + ".methstats").read() == (methstats_text([("mate1", want["w1"][2]), ("mate2", want["w2"][2])]) +
                                               overlap_line(want["totals"]))
    # the same through the library, clip points given
    got, _ = run_pairs(g1_all, R, db.start_index, seqs[0], seqs[1], res, "T", "A", cls[0], cls[1], what="clipped")
    assert got["totals"] == want["totals"]


def test_cli_no_overlap_with_duplicates(g1, g1_all, scratch):
    import walt_amd
    from test_dedup_cpu import DupRule, expect_pairs
    from test_gpu_dedup import doubled, loaded
    db, path = g1
    R = reference_bases(db)
    (_, f1), (_, f2) = doubled(scratch, "overlap", [os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")])
    s1, s2 = loaded(f1), loaded(f2)
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    dup = expect_pairs(DupRule(), res, "T")
    assert int(dup.sum()) > 200
    want = expected_pairs(R, db.start_index, s1, s2, res, skip=dup)
    sites, _ = expected_table(R[0], db.start_index, *want["pile"])
    out = os.path.join(scratch, "overlap_cli_dup")
    run_walt(["-i", path, "-1", f1, "-2", f2, "-o", out, "-a", "-u", "-sam", "-M", "-MC", "-D", "-NO"])
    assert open(out + ".methcounts").read() == counts_text(db, sites)
    # the overlap line counts every unique proper pair, duplicates included
    assert open(out + ".methstats").read() == (methstats_text([("mate1", want["w1"][2]), ("mate2", want["w2"][2])]) +
                                               overlap_line(want["totals"]))
    check_sam_xm(out, s1, s2, res, want)


# ---------------------------------------------------------------------------
# 4. a soak slice
# ---------------------------------------------------------------------------
def test_overlap_soak_slice():
    import sys
    sys.path.insert(0, os.path.join(refio.ROOT, "tools"))
    import soak
    line = soak.run_soak_overlap(range(1, 3), pattern=3)
    assert line.startswith("soak ok: overlap")
