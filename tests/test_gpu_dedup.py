"""PCR-duplicate marking on the device (walt_dedup_*, walt_meth_pileup_batch_skip, bin/walt -D; the contract is in
include/walt_amd.h, "duplicates").

The expected verdicts come from the restatement in tests/test_dedup_cpu.py (a Python dict: the first record fed with a key
wins); the expected methylation tables from the restatement in tests/test_gpu_pileup.py applied to the records that are
not duplicates.  Everything runs on the golden genome g1."""
import os
import random

import numpy as np
import pytest

import refio
from test_dedup_cpu import DupRule, expect_pairs, expect_single
from test_gpu_meth import cli_records_se, load, reference_bases, run_walt
from test_gpu_pileup import assert_sums_equal_stats, assert_table, counts_text, expected_counts, expected_table

pytestmark = pytest.mark.gpu

T, A = ord("T"), ord("A")
DEFAULT_BYTES = 16 * (1 << 25) + 16


@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "dedup_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    return refio.DbIndex(path), path


@pytest.fixture(scope="module")
def g1_all(g1):
    import walt_amd
    idx = walt_amd.Index.open(g1[1], device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def dd():
    """one set of the default size for the tests that do not care about capacity; cleared before each use"""
    import walt_amd
    d = walt_amd.Dedup()
    yield d
    d.close()


def records(rows):
    """rows: (genome_pos, times, strand) -> best_match_dtype array"""
    import walt_amd
    r = np.zeros(len(rows), dtype=walt_amd.best_match_dtype)
    for i, (pos, times, strand) in enumerate(rows):
        r["genome_pos"][i], r["times"][i], r["strand"][i] = pos, times, strand
    return r


def pairs_of(rows):
    """rows: (m1 (pos, times, strand), m2 (...), best_times, frag_len) -> pair_result_dtype array"""
    import walt_amd
    p = np.zeros(len(rows), dtype=walt_amd.pair_result_dtype)
    for i, (m1, m2, bt, fl) in enumerate(rows):
        for nm, m in (("m1", m1), ("m2", m2)):
            p[nm]["genome_pos"][i], p[nm]["times"][i], p[nm]["strand"][i] = m
        p["best_times"][i], p["frag_len"][i] = bt, fl
    return p


def stream_of(n, n_keys, seed):
    """n records over at most n_keys distinct keys (position, strand, conversion), some ineligible"""
    rng = random.Random(seed)
    pool = [(rng.choice([0, 1, 0xFFFFFFFE]) if rng.random() < 0.05 else rng.randrange(1 << 32), rng.choice([b"+", b"-"]), rng.choice([T, A]))
            for _ in range(n_keys)]
    rows, conv = [], []
    for _ in range(n):
        pos, strand, cv = rng.choice(pool)
        rows.append((pos, rng.choice([1, 1, 1, 1, 0, 2]), strand))
        conv.append(cv)
    return records(rows), np.array(conv, dtype=np.uint8)


# ---------------------------------------------------------------------------
# 1. hand-made record arrays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_within_one_call_the_lowest_index_wins(dd, n):
    dd.clear()
    recs, conv = stream_of(n, 16, n)
    got = dd.add_batch(recs, conv)
    want = expect_single(DupRule(), recs, conv)
    assert got.dtype == np.uint8 and got.tolist() == want.tolist()
    if n >= 63:
        assert 0 < int(got.sum()) and int(got.sum()) >= int((recs["times"] == 1).sum()) - 16
    seen = set()
    for i in range(n):  # said once more without the dict: the first eligible record of each key is no duplicate, every later one is
        if int(recs["times"][i]) != 1:
            assert got[i] == 0
            continue
        k = (int(recs["genome_pos"][i]), bytes(recs["strand"][i]), int(conv[i]))
        assert got[i] == (1 if k in seen else 0), i
        seen.add(k)
    assert dd.count() == (len(seen), n)


def test_cutting_the_stream_into_calls_changes_nothing(dd):
    recs, conv = stream_of(4097, 16, 99)
    dd.clear()
    whole = dd.add_batch(recs, conv)
    assert whole.tolist() == expect_single(DupRule(), recs, conv).tolist()
    for cut in (1, 7, 1000):
        dd.clear()
        parts = [dd.add_batch(recs[a:a + cut], conv[a:a + cut]) for a in range(0, len(recs), cut)]
        assert np.concatenate(parts).tolist() == whole.tolist(), cut
        assert dd.count()[1] == len(recs)


def test_growth_from_64_slots_changes_nothing(dd):
    import walt_amd
    recs, conv = stream_of(6000, 5000, 7)
    dd.clear()
    assert dd.device_bytes == DEFAULT_BYTES
    small = walt_amd.Dedup(initial_slots=64)
    try:
        assert small.device_bytes == 16 * 64 + 16
        assert walt_amd.Dedup(initial_slots=1).device_bytes == 16 * 64 + 16 and walt_amd.Dedup(initial_slots=65).device_bytes == 16 * 128 + 16
        got_small, got_big = [], []
        for a in range(0, len(recs), 500):
            got_small.append(small.add_batch(recs[a:a + 500], conv[a:a + 500]))
            got_big.append(dd.add_batch(recs[a:a + 500], conv[a:a + 500]))
        assert np.concatenate(got_small).tolist() == np.concatenate(got_big).tolist() == expect_single(DupRule(), recs, conv).tolist()
        keys, fed = small.count()
        assert (keys, fed) == dd.count() and keys > 2000 and fed == 6000
        assert small.device_bytes >= 16 * 64 * 2 ** 6 + 16  # doubled at least six times
        assert dd.device_bytes == DEFAULT_BYTES
        # reserve alone grows too, and keeps what the set holds
        before = small.device_bytes
        small.reserve(40000)
        assert small.device_bytes >= 16 * 2 * (keys + 40000) and small.device_bytes > before and small.count() == (keys, fed)
        assert small.add_batch(recs[:500], conv[:500]).tolist() == [1 if t == 1 else 0 for t in recs["times"][:500]]
    finally:
        small.close()


def test_ineligible_records_get_zero(dd):
    dd.clear()
    rows = [(10, 0, b"+"), (10, 2, b"+"), (10, 3, b"-"), (0xFFFFFFFF, 1, b"+"), (10, 1, b"+"), (10, 1, b"+")]
    conv = np.array([T, T, T, T, ord("N"), 0], dtype=np.uint8)
    for _ in range(3):  # fed again and again: never a duplicate, never a key
        assert dd.add_batch(records(rows), conv).tolist() == [0] * 6
    assert dd.count() == (0, 18)
    assert dd.add_batch(records(rows[:4]), "A").tolist() == [0] * 4
    # the same through pairs: a unique pair without a position or letter for mate 1, mates that are not unique
    p = pairs_of([((0xFFFFFFFF, 1, b"+"), (5, 1, b"-"), 1, 100), ((7, 0, b"+"), (8, 2, b"-"), 0, 0), ((7, 2, b"+"), (8, 0, b"-"), 2, 0)])
    for _ in range(2):
        assert dd.add_pairs(p, "T").tolist() == [[0, 0]] * 3
    bad = np.array([[ord("N"), A]] * 3, dtype=np.uint8)
    assert dd.add_pairs(pairs_of([((7, 1, b"+"), (8, 1, b"-"), 1, 100)] * 3), bad).tolist() == [[0, 0]] * 3
    assert dd.count()[0] == 0


def test_keys_that_differ_in_one_field_are_distinct(dd):
    dd.clear()
    base = [(100, 1, b"+")]
    assert dd.add_batch(records(base), "T", kind=0).tolist() == [0]
    assert dd.add_batch(records(base), "A", kind=0).tolist() == [0]             # conv
    assert dd.add_batch(records([(100, 1, b"-")]), "T", kind=0).tolist() == [0]  # strand
    assert dd.add_batch(records(base), "T", kind=1).tolist() == [0]             # kind
    assert dd.add_batch(records(base), "T", kind=2).tolist() == [0]
    assert dd.add_batch(records([(101, 1, b"+")]), "T", kind=0).tolist() == [0]  # pos
    pr = [((100, 1, b"+"), (300, 1, b"-"), 1, 250), ((100, 1, b"+"), (300, 1, b"-"), 1, 251)]  # aux (and kind 3)
    assert dd.add_pairs(pairs_of(pr), "T").tolist() == [[0, 0], [0, 0]]
    assert dd.count() == (8, 8)
    # every one of them again: all duplicates
    assert dd.add_batch(records(base), "T", kind=0).tolist() == [1]
    assert dd.add_batch(records(base), "A", kind=0).tolist() == [1]
    assert dd.add_batch(records([(100, 1, b"-")]), "T", kind=0).tolist() == [1]
    assert dd.add_batch(records(base), "T", kind=1).tolist() == [1]
    assert dd.add_batch(records(base), "T", kind=2).tolist() == [1]
    assert dd.add_batch(records([(101, 1, b"+")]), "T", kind=0).tolist() == [1]
    assert dd.add_pairs(pairs_of(pr), "T").tolist() == [[1, 1], [1, 1]]
    assert dd.count() == (8, 16)


def test_many_copies_of_one_key_clear_and_count(dd):
    import walt_amd
    dd.clear()
    recs = records([(123456, 1, b"-")] * 4096)
    got = dd.add_batch(recs, "A")
    assert got[0] == 0 and int(got.sum()) == 4095
    assert dd.count() == (1, 4096)
    assert dd.add_batch(recs[:3], "A").tolist() == [1, 1, 1]
    dd.clear()  # forgets, and numbers from 0 again
    assert dd.count() == (0, 0)
    assert dd.add_batch(recs[:3], "A").tolist() == [0, 1, 1]
    assert dd.count() == (1, 3)
    # strided records and conversions are read in place
    wide = np.zeros(8, dtype=walt_amd.pair_result_dtype)
    wide["m2"]["genome_pos"], wide["m2"]["times"], wide["m2"]["strand"] = [5, 6, 5, 6, 7, 5, 6, 7], 1, b"+"
    conv = np.zeros((8, 2), dtype=np.uint8)
    conv[:, 1] = [T, T, T, A, T, A, T, T]
    dd.clear()
    assert dd.add_batch(wide["m2"], conv[:, 1], kind=2).tolist() == [0, 0, 1, 0, 0, 0, 1, 1]
    with pytest.raises(walt_amd.WaltError) as ei:
        dd.add_batch(recs[:3], "A", kind=3)
    assert ei.value.code == walt_amd.WALT_EINVAL and "kind" in str(ei.value)
    with pytest.raises(walt_amd.WaltError) as ei:
        dd.add_batch(recs[:3], "N")
    assert ei.value.code == walt_amd.WALT_EINVAL and "conversion" in str(ei.value)


# ---------------------------------------------------------------------------
# 2. pairs
# ---------------------------------------------------------------------------
def test_pairs(dd):
    dd.clear()
    uniq = ((100, 1, b"+"), (300, 1, b"-"), 1, 250)
    lone1 = ((100, 1, b"+"), (0, 0, b"+"), 0, 0)          # mate 1 alone at 100 '+'
    lone2 = ((0, 0, b"+"), (100, 1, b"+"), 0, 0)          # mate 2 alone at the same place
    both = ((100, 1, b"+"), (100, 1, b"+"), 2, 0)         # no unique pair, both mates unique
    p = pairs_of([uniq, uniq, lone1, lone2, both, uniq, lone1])
    got = dd.add_pairs(p, "T")
    # a duplicate unique pair marks both mates; lone mates are deduplicated per mate number, never against the pair
    assert got.tolist() == [[0, 0], [1, 1], [0, 0], [0, 0], [1, 1], [1, 1], [1, 0]]
    assert got.tolist() == expect_pairs(DupRule(), p, "T").tolist()
    # (under the scalar T every mate 2 has conversion A: `both`'s mates repeat the keys of `lone1` and `lone2`)
    assert dd.count() == (3, 7)
    # a lone mate never collides with a single-end key at the same position, strand and conversion
    dd.clear()
    assert dd.add_batch(records([(100, 1, b"+")]), "T", kind=0).tolist() == [0]
    assert dd.add_pairs(pairs_of([lone1]), "T").tolist() == [[0, 0]]
    assert dd.add_pairs(pairs_of([lone2]), "A").tolist() == [[0, 0]]  # (mate 2 then has conversion T)
    assert dd.add_batch(records([(100, 1, b"+")]), "T", kind=0).tolist() == [1]
    # conv[2n] and the scalar agree, on a random stream, against the dict
    rng = random.Random(3)
    rows = []
    for _ in range(3000):
        m1 = (rng.choice([10, 20, 30]), rng.choice([0, 1, 1, 2]), rng.choice([b"+", b"-"]))
        m2 = (rng.choice([10, 20, 30]), rng.choice([0, 1, 1, 2]), rng.choice([b"+", b"-"]))
        bt = rng.choice([0, 1, 1, 2])
        rows.append((m1, m2, bt, rng.choice([200, 201, -5]) if bt == 1 else 0))
    p = pairs_of(rows)
    for letter, other in (("T", "A"), ("A", "T")):
        dd.clear()
        scalar = dd.add_pairs(p, letter)
        dd.clear()
        arr = np.array([[ord(letter), ord(other)]] * len(p), dtype=np.uint8)
        assert dd.add_pairs(p, arr).tolist() == scalar.tolist() == expect_pairs(DupRule(), p, letter).tolist()
        assert 500 < int(scalar.sum()) < 2 * len(p)
    # mixed conversions per pair, cut into calls
    conv = np.array([[rng.choice([T, A]), rng.choice([T, A])] for _ in rows], dtype=np.uint8)
    dd.clear()
    parts = [dd.add_pairs(p[a:a + 700], conv[a:a + 700]) for a in range(0, len(p), 700)]
    assert np.concatenate(parts).tolist() == expect_pairs(DupRule(), p, conv).tolist()


# ---------------------------------------------------------------------------
# 3. device forms
# ---------------------------------------------------------------------------
def test_device_forms_stream_reserve_refusal(dd):
    import torch
    import walt_amd
    recs, conv = stream_of(5000, 300, 21)
    dd.clear()
    want = dd.add_batch(recs, conv)
    dev = torch.device("cuda", 0)
    n = len(recs)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(n, 16)).to(dev)
    d_conv = torch.from_numpy(conv).to(dev)
    d_dup = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    s1 = torch.cuda.Stream(device=dev)
    small = walt_amd.Dedup(initial_slots=64)
    try:
        torch.cuda.synchronize()
        with pytest.raises(walt_amd.WaltError) as ei:  # a device form cannot grow the table
            small.add_batch_device(d_recs.data_ptr(), n, d_dup.data_ptr(), 16, d_conv.data_ptr(), 1, stream=s1.cuda_stream)
        assert ei.value.code == walt_amd.WALT_EINVAL and "walt_dedup_reserve" in str(ei.value)
        assert small.count() == (0, 0) and bool((d_dup == 9).all())  # nothing was enqueued
        small.reserve(n)
        assert small.device_bytes >= 16 * 2 * n
        half = 2048  # two calls on one stream: the second call's inserts come after the first call's marks
        small.add_batch_device(d_recs.data_ptr(), half, d_dup.data_ptr(), 16, d_conv.data_ptr(), 1, stream=s1.cuda_stream)
        small.add_batch_device(d_recs.data_ptr() + 16 * half, n - half, d_dup.data_ptr() + half, 16, d_conv.data_ptr() + half, 1,
                               stream=s1.cuda_stream)
        s1.synchronize()
        assert d_dup.cpu().numpy().tolist() == want.tolist()
        # the bound is the host's: keys at the last count plus everything enqueued since (a count reads the real number)
        with pytest.raises(walt_amd.WaltError):
            small.add_batch_device(d_recs.data_ptr(), n, d_dup.data_ptr(), 16, d_conv.data_ptr(), 1, stream=s1.cuda_stream)
        assert small.count() == dd.count()
        # pairs: the records as mates of pairs without a unique pair, against the host form
        rng = random.Random(8)
        rows = [((rng.choice([10, 20]), 1, b"+"), (rng.choice([10, 20, 30]), rng.choice([1, 2]), b"-"), rng.choice([0, 1]), 0) for _ in range(1500)]
        rows = [(m1, m2, bt, rng.choice([100, 101]) if bt else 0) for m1, m2, bt, _ in rows]
        p = pairs_of(rows)
        dd.clear()
        want_p = dd.add_pairs(p, "T")
        assert want_p.tolist() == expect_pairs(DupRule(), p, "T").tolist()
        small.clear()
        small.reserve(2 * len(p))
        d_pairs = torch.from_numpy(p.view(np.uint8).reshape(len(p), 64)).to(dev)
        d_dup2 = torch.full((len(p), 2), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        small.add_pairs_device(d_pairs.data_ptr(), len(p), d_dup2.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        assert d_dup2.cpu().numpy().tolist() == want_p.tolist()
        with pytest.raises(walt_amd.WaltError) as ei:
            small.add_pairs_device(d_pairs.data_ptr() + 4, 1, d_dup2.data_ptr())
        assert "aligned" in str(ei.value)
    finally:
        small.close()


# ---------------------------------------------------------------------------
# 4. skip: duplicates kept out of the pile-up and the totals
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def se_library(g1_all):
    import walt_amd
    _, seqs, _ = load("se_ct.fastq")
    bases, offs = walt_amd.pack_reads(seqs)
    recs, _ = g1_all.map_se_batch(bases, offs)
    return seqs, bases, offs, recs


def test_skip_all_zero_is_the_plain_pileup(g1, g1_all, se_library):
    seqs, bases, offs, recs = se_library
    plain, skipped = g1_all.pileup(), g1_all.pileup()
    try:
        want = plain.add_batch(bases, offs, recs, "T")
        got = skipped.add_batch(bases, offs, recs, "T", skip=np.zeros(len(seqs), dtype=np.uint8))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        a, b = plain.extract(), skipped.extract()
        assert a[0].tobytes() == b[0].tobytes() and a[0].size > 100 and a[1].tolist() == b[1].tolist()
    finally:
        plain.close()
        skipped.close()


@pytest.mark.parametrize("rows", [0, 1])
def test_skip_random_mask(g1, g1_all, se_library, index_options, rows):
    db, _ = g1
    R = reference_bases(db)
    seqs, bases, offs, recs = se_library
    rng = np.random.default_rng(5 + rows)
    mask = (rng.random(len(seqs)) < 0.4).astype(np.uint8) * rng.integers(1, 256, len(seqs)).astype(np.uint8)  # any non-zero byte skips
    assert 100 < int((mask != 0).sum()) < len(seqs) - 100
    kept = recs.copy()
    kept["times"][mask != 0] = 0  # the restatement piles up records with times == 1
    meth, unmeth = expected_counts(R, db.start_index, seqs, kept, "T")
    plain = g1_all.meth_call_batch(bases, offs, recs, "T")
    index_options(g1_all, pile_rows=rows)
    pile = g1_all.pileup()
    try:
        calls, counts, stats = pile.add_batch(bases, offs, recs, "T", skip=mask)
        assert calls.tobytes() == plain[0].tobytes() and counts.tobytes() == plain[1].tobytes()  # written as before
        sites = assert_table(pile.extract(), R[0], db.start_index, meth, unmeth, "skip, pile_rows=%d" % rows)
        assert_sums_equal_stats(sites, pile.extract()[1], stats, "skip")
        assert int(stats["reads"][0]) == int(((recs["times"] == 1) & (mask == 0)).sum()) < int(plain[2]["reads"][0])
        # a null pile-up: the calls and the totals alone
        got = g1_all.meth_call_batch(bases, offs, recs, "T", skip=mask)
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes() and got[2].tobytes() == stats.tobytes()
        assert pile.extract()[0].tobytes() == sites.tobytes()
    finally:
        pile.close()


def test_skip_strided_over_the_mates_of_pairs(g1, g1_all):
    import walt_amd
    db, _ = g1
    R = reference_bases(db)
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    s1, s2 = s1[:600] + s1[:600], s2[:600] + s2[:600]  # every pair twice: the second copies are duplicates
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    out, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    dd = walt_amd.Dedup(initial_slots=64)
    pile = g1_all.pileup()
    try:
        dup = dd.add_pairs(out, "T")
        assert dup.tolist() == expect_pairs(DupRule(), out, "T").tolist()
        assert int(dup[600:, 0].sum()) > 300 and dup.strides == (2, 1)
        acc = None
        for k, (seqs, b, o, cv) in enumerate(((s1, b1, o1, "T"), (s2, b2, o2, "A"))):
            m = out["m%d" % (k + 1)]
            pile.add_batch(b, o, m, cv, skip=dup[:, k], want_calls=False, want_counts=False, want_stats=False)
            kept = np.ascontiguousarray(m).copy()
            kept["times"][dup[:, k] != 0] = 0
            acc = expected_counts(R, db.start_index, seqs, kept, cv, into=acc)
        assert_table(pile.extract(), R[0], db.start_index, acc[0], acc[1], "pairs with skip")
    finally:
        pile.close()
        dd.close()


# ---------------------------------------------------------------------------
# 5. command line
# ---------------------------------------------------------------------------
def doubled(scratch, tag, files):
    """-> per read file (original, doubled): the file without the records that hold anything but ACGT in either mate (the
    loader fills such a base with a draw that depends on the record's place in its -N batch, so a copy would not be a copy), and that file
    followed by a shuffled copy of itself (the same shuffle for both mates)"""
    recs = []
    for fq in files:
        lines = open(fq).read().split("\n")
        lines = lines[:len(lines) // 4 * 4]
        recs.append([lines[i:i + 4] for i in range(0, len(lines), 4)])
    keep = [i for i in range(len(recs[0])) if all(set(r[i][1]) <= set("ACGT") for r in recs)]
    assert len(keep) > 0.9 * len(recs[0])
    order = list(keep)
    random.Random(17).shuffle(order)
    out = []
    for k, r in enumerate(recs):
        text = ["\n".join(x) + "\n" for x in r]
        orig = os.path.join(scratch, "dedup_%s_orig_%d.fastq" % (tag, k + 1))
        path = os.path.join(scratch, "dedup_%s_%d.fastq" % (tag, k + 1))
        with open(orig, "w") as f:
            f.write("".join(text[i] for i in keep))
        with open(path, "w") as f:
            f.write("".join(text[i] for i in keep) + "".join(text[i] for i in order))
        out.append((orig, path))
    return out


def loaded(fq):
    seqs = []
    for _, sq, _ in refio.load_fastq_batches(fq, 10 ** 7):
        seqs += sq
    return seqs


def sam_flags(path):
    return [int(l.split("\t")[1]) for l in open(path) if not l.startswith("@")]


def sam_without_flag_bit(path):
    out = []
    for l in open(path):
        if not l.startswith("@"):
            p = l.split("\t")
            p[1] = str(int(p[1]) & ~0x400)
            l = "\t".join(p)
        out.append(l)
    return out


def dupstats_text(records, duplicates):
    return "records: %d\nduplicates: %d\nduplication rate: %s\n" % (records, duplicates, "%.6f" % (duplicates / records) if records else "NA")


def all_outputs(out):
    d, base = os.path.dirname(out), os.path.basename(out)
    return {f[len(base):]: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith(base)}


def se_case(scratch, g1, g1_all, tag, src, mode):
    """-> (original fastq, doubled fastq, seqs, recs, conv, dup, eligible records, methcounts text of the records that
    are no duplicates) of a doubled single-end library"""
    db, _ = g1
    R = reference_bases(db)
    (orig, fq), = doubled(scratch, tag, [src])
    seqs = loaded(fq)
    recs, conv = cli_records_se(g1_all, seqs, mode)
    dup = expect_single(DupRule(), recs, conv)
    eligible = int((recs["times"] == 1).sum())
    assert int(dup.sum()) >= 100 and eligible - int(dup.sum()) >= 100  # (the test cannot pass vacuously)
    kept = recs.copy()
    kept["times"][dup != 0] = 0
    meth, unmeth = expected_counts(R, db.start_index, seqs, kept, conv)
    sites, off = expected_table(R[0], db.start_index, meth, unmeth)
    assert sites.size > 100 and off == [0, 0]
    return orig, fq, seqs, recs, conv, dup, eligible, counts_text(db, sites)


def test_cli_single_end(g1, g1_all, scratch):
    _, path = g1
    src, fq, seqs, recs, conv, dup, eligible, text = se_case(scratch, g1, g1_all, "se", os.path.join(refio.GOLDEN, "se_ct.fastq"), "T")
    o = lambda name: os.path.join(scratch, "dedup_cli_se_" + name)
    # -D -MC -M -sam: the table without the duplicates; FLAG 0x400 on exactly their lines, nothing else on any line
    run_walt(["-i", path, "-r", fq, "-o", o("sam"), "-a", "-u", "-sam", "-M", "-MC"])
    run_walt(["-i", path, "-r", fq, "-o", o("sam_D"), "-a", "-u", "-sam", "-M", "-MC", "-D"])
    assert open(o("sam_D") + ".methcounts").read() == text
    assert open(o("sam") + ".methcounts").read() != text and not os.path.exists(o("sam") + ".dupstats")
    flags = sam_flags(o("sam_D"))
    assert len(flags) == len(seqs) and [(f >> 10) & 1 for f in flags] == dup.tolist()
    assert sam_without_flag_bit(o("sam_D")) == open(o("sam")).readlines()
    assert open(o("sam_D") + ".mapstats").read() == open(o("sam") + ".mapstats").read()
    assert open(o("sam_D") + ".dupstats").read() == dupstats_text(eligible, int(dup.sum()))
    # .methstats leave the duplicates out: the totals of the kept records
    kept = recs.copy()
    kept["times"][dup != 0] = 0
    bases, offs = __import__("walt_amd").pack_reads(seqs)
    want_stats = g1_all.meth_call_batch(bases, offs, kept, conv, want_calls=False, want_counts=False)[2]
    from test_gpu_meth import methstats_text
    assert open(o("sam_D") + ".methstats").read() == methstats_text([(None, {k: want_stats[k][0] for k in ("reads", "meth", "unmeth")})])
    # the table is the original library's minus its own internal duplicates: the first copy of every key wins
    n0 = len(seqs) // 2
    run_walt(["-i", path, "-r", src, "-o", o("orig_D"), "-MC", "-D"])
    assert open(o("orig_D") + ".methcounts").read() == text
    assert open(o("orig_D") + ".dupstats").read() == dupstats_text(int((recs["times"][:n0] == 1).sum()), int(dup[:n0].sum()))
    if int(dup[:n0].sum()) == 0:
        run_walt(["-i", path, "-r", src, "-o", o("orig"), "-MC"])
        assert open(o("orig") + ".methcounts").read() == text
    # .mr lacks exactly the duplicates' lines
    run_walt(["-i", path, "-r", fq, "-o", o("mr"), "-a", "-u"])
    run_walt(["-i", path, "-r", fq, "-o", o("mr_D"), "-a", "-u", "-D"])
    plain = open(o("mr")).readlines()
    uniq = [j for j in range(len(seqs)) if int(recs["times"][j]) == 1]
    assert len(plain) == len(uniq)
    assert open(o("mr_D")).readlines() == [l for l, j in zip(plain, uniq) if not dup[j]]
    for sfx in ("_ambiguous", "_unmapped", ".mapstats"):
        assert open(o("mr_D") + sfx).read() == open(o("mr") + sfx).read(), sfx
    # the verdict does not depend on -N or -g: byte-identical outputs
    want = all_outputs(o("sam_D"))
    assert set(want) == {"", ".mapstats", ".methstats", ".methcounts", ".dupstats"}
    import walt_amd
    for name, extra in (("N64", ["-N", "64"]), ("g", ["-g", "0,1" if walt_amd.device_count() >= 2 else "0,0"])):
        run_walt(["-i", path, "-r", fq, "-o", o(name), "-a", "-u", "-sam", "-M", "-MC", "-D"] + extra)
        got = all_outputs(o(name))
        assert set(got) == set(want)
        for sfx in want:
            assert got[sfx] == want[sfx], (name, sfx)
    # two read files in one run: the set is cleared in between
    run_walt(["-i", path, "-r", fq + "," + fq, "-o", o("two"), "-MC", "--remove-duplicates"])
    assert open(o("two") + ".methcounts").read() == text + text
    assert open(o("two") + ".dupstats").read() == 2 * dupstats_text(eligible, int(dup.sum()))


def test_cli_random_pbat_single_end(g1, g1_all, scratch):
    from test_gpu_rpbat import mixed_library
    _, path = g1
    names, seqs, scores = mixed_library()
    src = os.path.join(scratch, "dedup_mixed.fastq")
    with open(src, "w") as f:
        for nm, s, q in zip(names, seqs, scores):
            f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
    _, fq, seqs, recs, conv, dup, eligible, text = se_case(scratch, g1, g1_all, "R", src, "R")
    out = os.path.join(scratch, "dedup_cli_R")
    run_walt(["-i", path, "-r", fq, "-o", out, "-R", "-a", "-u", "-sam", "-MC", "-dedup"])
    assert open(out + ".methcounts").read() == text
    assert [(f >> 10) & 1 for f in sam_flags(out)] == dup.tolist()
    assert open(out + ".dupstats").read() == dupstats_text(eligible, int(dup.sum()))


@pytest.mark.parametrize("mode", ["pe", "P", "RP"])
def test_cli_paired_end(g1, g1_all, scratch, mode):
    import walt_amd
    db, path = g1
    R = reference_bases(db)
    (_, f1), (_, f2) = doubled(scratch, "pe_" + mode, [os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")])
    s1, s2 = loaded(f1), loaded(f2)
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    if mode == "RP":
        res, conv, _ = g1_all.map_pe_rpbat_batch(b1, o1, b2, o2)
        dup = expect_pairs(DupRule(), res, conv)
        parts = [(s1, res["m1"], conv[:, 0]), (s2, res["m2"], conv[:, 1])]
    else:  # -P: a PBAT library has its A-rich mates in the -1 file; the run maps the -2 file C->T and the -1 file G->A
        res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
        dup = expect_pairs(DupRule(), res, "T")
        parts = [(s1, res["m1"], "T"), (s2, res["m2"], "A")]
    uniq = res["best_times"] == 1
    eligible = int(uniq.sum()) + int((res["m1"]["times"][~uniq] == 1).sum()) + int((res["m2"]["times"][~uniq] == 1).sum())
    n_dup = int(dup[uniq, 0].sum()) + int(dup[~uniq].sum())
    assert n_dup >= 100 and eligible - n_dup >= 100
    assert (dup[uniq, 0] == dup[uniq, 1]).all()
    acc = None
    for k, (seqs, recs, cv) in enumerate(parts):
        kept = np.ascontiguousarray(recs).copy()
        kept["times"][dup[:, k] != 0] = 0
        acc = expected_counts(R, db.start_index, seqs, kept, cv, into=acc)
    sites, off = expected_table(R[0], db.start_index, *acc)
    assert sites.size > 1000 and off == [0, 0]
    reads = ["-1", f2, "-2", f1, "-P"] if mode == "P" else ["-1", f1, "-2", f2] + (["-RP"] if mode == "RP" else [])
    out = os.path.join(scratch, "dedup_cli_pe_" + mode)
    run_walt(["-i", path] + reads + ["-o", out + "_D", "-a", "-u", "-sam", "-MC", "-D"])
    assert open(out + "_D.methcounts").read() == counts_text(db, sites)
    assert open(out + "_D.dupstats").read() == dupstats_text(eligible, n_dup)
    if mode != "pe":
        return
    run_walt(["-i", path] + reads + ["-o", out, "-a", "-u", "-sam", "-MC"])
    flags = sam_flags(out + "_D")
    assert len(flags) == 2 * len(s1) and [(f >> 10) & 1 for f in flags] == dup.reshape(-1).tolist()
    assert sam_without_flag_bit(out + "_D") == open(out).readlines()
    assert open(out + "_D.mapstats").read() == open(out + ".mapstats").read()
    # .mr: the fragment line of a duplicate pair and the line of a duplicate lone mate are missing, nothing else
    run_walt(["-i", path] + reads + ["-o", out + ".mr", "-a", "-u"])
    run_walt(["-i", path] + reads + ["-o", out + "_D.mr", "-a", "-u", "-D", "-N", "64"])
    owners = []
    for j in range(len(s1)):
        if uniq[j]:
            owners.append((j, 0))
        else:
            owners += [(j, k) for k in (0, 1) if int(res["m%d" % (k + 1)]["times"][j]) == 1]
    plain = open(out + ".mr").readlines()
    assert len(plain) == len(owners)
    assert open(out + "_D.mr").readlines() == [l for l, (j, k) in zip(plain, owners) if not dup[j, k]]
    assert open(out + "_D.mr.mapstats").read() == open(out + ".mr.mapstats").read()
    assert open(out + "_D.mr.dupstats").read() == dupstats_text(eligible, n_dup)


# ---------------------------------------------------------------------------
# 6. a soak slice
# ---------------------------------------------------------------------------
def test_dedup_soak_slice():
    import sys
    sys.path.insert(0, os.path.join(refio.ROOT, "tools"))
    import soak
    line = soak.run_soak_dedup(range(1, 4), pattern=3)
    assert line.startswith("soak ok"), line
