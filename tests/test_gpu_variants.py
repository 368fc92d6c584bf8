"""Opposite-strand evidence and the masking of C>T variant sites (walt_meth_evidence_batch, walt_meth_pileup_batch_ev,
walt_pileup_variants, walt_pileup_mask_variants, bin/walt -MV; the contract is in include/walt_amd.h, "opposite-strand
evidence").

The expected values come from the restatement below: every base of every counted record is walked to its forward
position, and the rule is applied to every position of the genome with Python integers.  No position is left out: the
two evidence planes are compared as dense arrays over the whole genome, the flagged records as whole tables, the masked
counters as dense arrays."""
import ctypes
import os
import random

import numpy as np
import pytest

import refio
from test_gpu_meth import load, planted, reference_bases
from test_gpu_pileup import chrom_of, site_class

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def base_letter(b):
    """the letter a byte counts as: the one whose bits 2..1 it shares (A 0x41, C 0x43, T 0x54, G 0x47)"""
    return "ACTG"[(int(b) >> 1) & 3]


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def expected_evidence(R, start_index, seqs, recs, conv, call_len=None, skip=None, into=None):
    """(match, other) int64 arrays over every forward position: the evidence of every record that counts."""
    glen = len(R[0])
    match, other = into if into is not None else (np.zeros(glen, dtype=np.int64), np.zeros(glen, dtype=np.int64))
    for i, s in enumerate(seqs):
        s = as_bytes(s)
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
            if chr(G[q]) != want:
                continue
            f = lo + hi - 1 - q if strand == b"-" else q
            (match if base_letter(s[k]) == want else other)[f] += 1
    return match, other


def judged(m, o, min_depth):
    return m + o >= min_depth


def flagged(m, o, min_depth, max_percent):
    return m + o >= min_depth and 100 * o > max_percent * (m + o)


def expected_variants(R0, start_index, meth, unmeth, match, other, min_depth, max_percent, lo=0, hi=None):
    import walt_amd
    hi = len(R0) if hi is None else hi
    rows = []
    for f in range(lo, hi):
        cls = site_class(R0, start_index, f)
        if cls is not None and flagged(int(match[f]), int(other[f]), min_depth, max_percent):
            rows.append((f, int(meth[f]), int(unmeth[f]), ord(cls[0]), cls[1], 0, int(match[f]), int(other[f])))
    return np.array(rows, dtype=walt_amd.variant_site_dtype)


def expected_mask(R0, meth, unmeth, match, other, min_depth, max_percent, lo=0, hi=None):
    """-> (meth, unmeth after the masking of [lo, hi), [judged, flagged, masked sites, meth removed, unmeth removed])"""
    hi = len(R0) if hi is None else hi
    m2, u2 = np.array(meth, dtype=np.int64), np.array(unmeth, dtype=np.int64)
    tot = [0] * 5
    for f in range(lo, hi):
        if chr(R0[f]) not in "CG":
            continue
        m, o = int(match[f]), int(other[f])
        tot[0] += judged(m, o, min_depth)
        if not flagged(m, o, min_depth, max_percent):
            continue
        tot[1] += 1
        if m2[f] or u2[f]:
            tot[2] += 1
            tot[3] += int(m2[f])
            tot[4] += int(u2[f])
            m2[f] = u2[f] = 0
    return m2, u2, tot


def assert_planes(ev, match, other, what=""):
    gm, go = ev.read()
    bad = np.nonzero((gm.astype(np.int64) != match) | (go.astype(np.int64) != other))[0]
    assert bad.size == 0, (what, [(int(f), int(gm[f]), int(match[f]), int(go[f]), int(other[f])) for f in bad[:5]])


# ---------------------------------------------------------------------------
# 1. hand-made records on the small planted genome
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(scratch):
    import walt_amd
    fa, p1, short, chr_e = planted(scratch)
    path = os.path.join(scratch, "variants_planted.dbindex")
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield {"db": db, "idx": idx, "R": reference_bases(db), "path": path}
    idx.close()


def hand_batch(R, start_index, seed):
    """records of every kind the contract names; -> seqs (bytes), records, conv bytes, call_len, skip"""
    import walt_amd
    rng = random.Random(seed)
    glen = len(R[0])
    rows = []

    def read_at(pos, n, strand, cv):
        """the strand's bases, with other bases at a third of the evidence positions and a few bytes that are no letters"""
        G = R[1 if strand == b"-" else 0]
        out = bytearray()
        for k in range(n):
            g = chr(G[pos + k]) if pos + k < glen else "A"
            if g == ("G" if cv == "T" else "C") and rng.random() < 0.33:
                g = rng.choice("ACGT")
            if rng.random() < 0.02:
                g = rng.choice("N.nacgt\x00\xff")
            out += g.encode("latin-1")
        return bytes(out)

    p1_len = int(start_index[1])
    for n in (1, 15, 16, 17, 100, 128, 129, 1024):
        for strand in (b"+", b"-"):
            for cv in "TA":
                for call_len in (None, 0, 1, 15, 16, 17, n, n + 3):
                    pos = rng.randrange(0, p1_len - n + 1)
                    rows.append((read_at(pos, n, strand, cv), pos, 1, strand, cv, n if call_len is None else call_len, 0))
    for times, skip in ((0, 0), (2, 0), (1, 1), (1, 255)):  # nothing is added for these
        for strand in (b"+", b"-"):
            rows.append((read_at(200, 100, strand, "T"), 200, times, strand, "T", 100, skip))
    # reads over a chromosome's end: chrS has 50 bases, and a read on the last base of the last chromosome
    s_lo, s_hi = int(start_index[1]), int(start_index[2])
    for strand in (b"+", b"-"):
        for cv in "TA":
            rows.append((read_at(s_lo + 10, 100, strand, cv), s_lo + 10, 1, strand, cv, 100, 0))
            rows.append((read_at(s_hi - 1, 17, strand, cv), s_hi - 1, 1, strand, cv, 17, 0))
            rows.append((read_at(glen - 1, 40, strand, cv), glen - 1, 1, strand, cv, 40, 0))
    rows.append((read_at(0, 30, b"+", "T"), glen, 1, b"+", "T", 30, 0))        # outside the genome
    rows.append((read_at(0, 30, b"+", "T"), 0xFFFFFFF0, 1, b"+", "T", 30, 0))
    rng.shuffle(rows)
    # fillers (times == 0) so that counted reads start at every alignment modulo 16
    out, at, seen = [], 0, set()
    for row in rows:
        want = next((a for a in range(16) if a not in seen), None)
        if want is not None and row[2] == 1 and not row[6] and row[1] < glen:
            fill = (want - at) % 16
            if fill:
                out.append((b"C" * fill, 0, 0, b"+", "T", fill, 0))
                at += fill
            seen.add(at % 16)
        out.append(row)
        at += len(row[0])
    assert len(seen) == 16
    recs = np.zeros(len(out), dtype=walt_amd.best_match_dtype)
    recs["genome_pos"] = [r[1] for r in out]
    recs["times"] = [r[2] for r in out]
    recs["strand"] = [r[3] for r in out]
    conv = np.array([ord(r[4]) for r in out], dtype=np.uint8)
    return ([r[0] for r in out], recs, conv, np.array([r[5] for r in out], dtype=np.uint32), np.array([r[6] for r in out], dtype=np.uint8))


def device_batch(seqs, recs, conv, call_len, skip):
    import torch
    dev = torch.device("cuda", 0)
    raw = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    t = {"bases": torch.from_numpy(raw.copy()).to(dev), "offs": torch.from_numpy(offs).to(dev),
         "recs": torch.from_numpy(recs.view(np.uint8).reshape(len(seqs), 16).copy()).to(dev),
         "conv": torch.from_numpy(conv.copy()).to(dev), "len": torch.from_numpy(call_len.view(np.int32).copy()).to(dev),
         "skip": torch.from_numpy(skip.copy()).to(dev)}
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("rows", [0, 1])
def test_hand_made_records_both_add_shapes(small, index_options, rows):
    import torch
    import walt_amd
    idx, db, R = small["idx"], small["db"], small["R"]
    seqs, recs, conv, call_len, skip = hand_batch(R, db.start_index, 21 + rows)
    match, other = expected_evidence(R, db.start_index, seqs, recs, conv, call_len, skip)
    assert int(match.sum()) > 3000 and int(other.sum()) > 1000
    on_c = np.isin(R[0], np.frombuffer(b"C", dtype=np.uint8))
    on_g = np.isin(R[0], np.frombuffer(b"G", dtype=np.uint8))
    assert ((match + other)[on_c].sum() > 1000 and (match + other)[on_g].sum() > 1000 and (match + other)[~(on_c | on_g)].sum() == 0)
    index_options(idx, pile_rows=rows)
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    ev = idx.pileup()
    try:
        ev.add_evidence_batch(bases, offs, recs, conv, call_len=call_len, skip=skip)
        assert_planes(ev, match, other, "host form, pile_rows=%d" % rows)
        # the host form leaves a batch that does not start at offset 0 where it is
        lead = 5
        ev.add_evidence_batch(np.concatenate([np.zeros(lead, dtype=np.uint8), bases]), offs + np.uint64(lead), recs, conv, call_len=call_len, skip=skip)
        assert_planes(ev, 2 * match, 2 * other, "host form at offsets[0] = 5")
        # device form: the same batch plus what a host form refuses -- a read of 1025 bases and an unknown conversion
        more = [bytes(R[0][:1025]), bytes(R[0][100:200])]
        recs2 = np.concatenate([recs, np.zeros(2, dtype=walt_amd.best_match_dtype)])
        recs2["genome_pos"][-2:], recs2["times"][-2:], recs2["strand"][-2:] = [0, 100], 1, b"+"
        conv2 = np.concatenate([conv, np.array([ord("T"), ord("X")], dtype=np.uint8)])
        len2 = np.concatenate([call_len, np.array([1025, 100], dtype=np.uint32)])
        skip2 = np.concatenate([skip, np.zeros(2, dtype=np.uint8)])
        assert expected_evidence(R, db.start_index, seqs + more, recs2, conv2, len2, skip2)[0].tolist() == match.tolist()
        t = device_batch(seqs + more, recs2, conv2, len2, skip2)
        ev.add_evidence_batch_device(t["bases"].data_ptr(), t["offs"].data_ptr(), len(seqs) + 2, t["recs"].data_ptr(), 16,
                                     t["conv"].data_ptr(), 1, "T", t["len"].data_ptr(), t["skip"].data_ptr(), 1)
        torch.cuda.synchronize()
        assert_planes(ev, 3 * match, 3 * other, "device form")
    finally:
        ev.close()


@pytest.mark.parametrize("rows", [0, 1])
def test_fifty_thousand_copies_of_one_read_and_its_reverse_complement(small, index_options, rows):
    """the adds are exact: 50,000 records on one position, then 50,000 reverse-complement records on the same counters"""
    import walt_amd
    idx, db, R = small["idx"], small["db"], small["R"]
    index_options(idx, pile_rows=rows)
    copies, pos, n = 50000, 333, 100
    read = bytearray(R[0][pos:pos + n].tobytes())
    g_at = [k for k in range(n) if chr(read[k]) == "G"]
    assert len(g_at) >= 10
    read[g_at[3]] = ord("A")  # one G shows A: `other` there, `match` at every other G
    read = bytes(read)
    _, lo, hi = chrom_of(db.start_index, pos)
    rc = refio.revcomp(read.decode()).encode()
    one = np.zeros(2, dtype=walt_amd.best_match_dtype)
    one["genome_pos"], one["times"], one["strand"] = [pos, lo + hi - (pos + n)], 1, [b"+", b"-"]
    m1, o1 = expected_evidence(R, db.start_index, [read], one[:1], "T")
    m2, o2 = expected_evidence(R, db.start_index, [rc], one[1:], "A")
    assert m1.tolist() == m2.tolist() and o1.tolist() == o2.tolist() and int(o1.sum()) == 1 and int(m1.sum()) == len(g_at) - 1
    ev = idx.pileup()
    try:
        for k, (s, cv) in enumerate(((read, "T"), (rc, "A"))):
            bases = np.frombuffer(s * copies, dtype=np.uint8)
            offs = np.arange(copies + 1, dtype=np.uint64) * np.uint64(n)
            ev.add_evidence_batch(bases, offs, np.repeat(one[k:k + 1], copies), cv)
            assert_planes(ev, (k + 1) * copies * m1, (k + 1) * copies * o1, "after %s" % cv)
    finally:
        ev.close()


# ---------------------------------------------------------------------------
# 2. golden reads: the device form on one stream and on two, the fused call against the stand-alone one
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "variants_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    _, seqs, _ = load("se_ct.fastq")
    seqs = seqs[:600]
    bases, offs = walt_amd.pack_reads(seqs)
    recs, _ = idx.map_se_batch(bases, offs)
    R = reference_bases(db)
    match, other = expected_evidence(R, db.start_index, seqs, recs, "T")
    assert int(match.sum()) > 5000 and int(other.sum()) > 0
    yield {"db": db, "path": path, "idx": idx, "R": R, "seqs": seqs, "bases": bases, "offs": offs, "recs": recs, "match": match,
           "other": other}
    idx.close()


def test_device_form_on_one_stream_and_on_two(g1):
    import torch
    idx, db, bases, offs, recs = g1["idx"], g1["db"], g1["bases"], g1["offs"], g1["recs"]
    n = len(g1["seqs"])
    dev = torch.device("cuda", 0)
    d_bases = torch.from_numpy(bases).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(n, 16)).to(dev)
    half = n // 2
    d_offs2 = torch.from_numpy((offs[half:] - offs[half]).view(np.int64)).to(dev)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ev, pile = idx.pileup(), idx.pileup()
    try:
        ev.add_evidence_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_recs.data_ptr(), stream=s1.cuda_stream)
        # the passes on the same stream come after the adds
        want = expected_variants(g1["R"][0], db.start_index, np.zeros(db.genome_len), np.zeros(db.genome_len), g1["match"], g1["other"], 1, 0)
        assert want.size > 0
        d_out = torch.zeros((want.size + 4, 24), dtype=torch.uint8, device=dev)
        d_n = torch.zeros(6, dtype=torch.int64, device=dev)
        pile.variants_device(ev, 0, db.genome_len, 1, 0, d_out.data_ptr(), want.size + 4, d_n.data_ptr(), stream=s1.cuda_stream)
        pile.mask_variants_device(ev, 0, db.genome_len, 1, 0, d_n.data_ptr() + 8, stream=s1.cuda_stream)
        s1.synchronize()
        assert int(d_n[0]) == want.size and d_out.cpu().numpy()[:want.size].tobytes() == want.tobytes()
        covered = int(((g1["match"] + g1["other"]) > 0).sum())
        assert d_n.cpu().numpy()[1:].tolist() == [covered, want.size, 0, 0, 0]
        # a cap that is too small: the count comes back, nothing is written
        d_out.fill_(0x23)
        pile.variants_device(ev, 0, db.genome_len, 1, 0, d_out.data_ptr(), want.size - 1, d_n.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        assert int(d_n[0]) == want.size and bool((d_out == 0x23).all())
        assert_planes(ev, g1["match"], g1["other"], "one stream")
        ev.clear()
        for _ in range(3):
            ev.add_evidence_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), half, d_recs.data_ptr(), stream=s1.cuda_stream)
            ev.add_evidence_batch_device(d_bases.data_ptr() + int(offs[half]), d_offs2.data_ptr(), n - half, d_recs.data_ptr() + 16 * half,
                                         stream=s2.cuda_stream)
        s1.synchronize()
        s2.synchronize()
        assert_planes(ev, 3 * g1["match"], 3 * g1["other"], "two streams")
    finally:
        ev.close()
        pile.close()


def test_fused_call_host_and_device_against_the_stand_alone_call(g1):
    import torch
    import walt_amd
    idx, db, bases, offs, recs = g1["idx"], g1["db"], g1["bases"], g1["offs"], g1["recs"]
    n = len(g1["seqs"])
    rng = random.Random(4)
    call_len = np.array([rng.choice([100, 100, 50, 0, 103]) for _ in range(n)], dtype=np.uint32)
    skip = np.array([rng.random() < 0.2 for _ in range(n)], dtype=np.uint8)
    alone, plain, pile, ev = idx.pileup(), idx.pileup(), idx.pileup(), idx.pileup()
    other_idx = walt_amd.Index.open(g1["path"], device=0, strands=walt_amd.STRANDS_CT | walt_amd.WITH_REFERENCE)
    foreign = other_idx.pileup()
    try:
        alone.add_evidence_batch(bases, offs, recs, "T", call_len=call_len, skip=skip)
        match, other = expected_evidence(g1["R"], db.start_index, g1["seqs"], recs, "T", call_len, skip)
        assert_planes(alone, match, other, "stand-alone")
        want = plain.add_batch(bases, offs, recs, "T", call_len=call_len, skip=skip)
        got = pile.add_batch(bases, offs, recs, "T", call_len=call_len, skip=skip, evidence=ev)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        assert pile.extract()[0].tobytes() == plain.extract()[0].tobytes()
        assert_planes(ev, match, other, "fused, host form")
        # -I5 / -I3 and -NO do not act on the evidence: ignored ends and an excluded interval change the calls alone
        excl = np.full(n, 10 | (60 << 16), dtype=np.uint32)
        pile.add_batch(bases, offs, recs, "T", call_len=call_len, skip=skip, excl=excl, trim5=7, trim3=9, evidence=ev)
        assert_planes(ev, 2 * match, 2 * other, "fused, with ignored ends and an excluded interval")
        # the evidence alone through the fused call: no calls, no counts, no statistics, no pile-up
        L = walt_amd.lib()
        args = (bases.ctypes.data, offs.ctypes.data, n, recs.ctypes.data, 16, None, 0, ord("T"), call_len.ctypes.data, None, None, None,
                skip.ctypes.data, 1, None, None, 0, 0, 0, None, None)
        assert L.walt_meth_pileup_batch_ev(idx.handle, None, *args, ev.handle) == 0
        assert_planes(ev, 3 * match, 3 * other, "fused, nothing else wanted")
        # device form
        dev = torch.device("cuda", 0)
        t = device_batch([as_bytes(s) for s in g1["seqs"]], recs, np.full(n, ord("T"), dtype=np.uint8), call_len, skip)
        d_calls = torch.zeros(bases.size + 32, dtype=torch.uint8, device=dev)
        s1 = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        pile.clear()
        pile.add_batch_device(t["bases"].data_ptr(), t["offs"].data_ptr(), n, t["recs"].data_ptr(), 16, None, 1, "T", t["len"].data_ptr(),
                              d_calls.data_ptr(), stream=s1.cuda_stream, d_skip=t["skip"].data_ptr(), evidence=ev)
        s1.synchronize()
        assert d_calls.cpu().numpy()[:bases.size].tobytes() == want[0].tobytes()
        assert pile.extract()[0].tobytes() == plain.extract()[0].tobytes()
        assert_planes(ev, 4 * match, 4 * other, "fused, device form")
        # refusals: ev == p, the evidence object of another index, a null evidence object
        E = walt_amd.WALT_EINVAL
        assert L.walt_meth_pileup_batch_ev(idx.handle, pile.handle, *args, pile.handle) == E and b"one object" in L.walt_last_error()
        assert L.walt_meth_pileup_batch_ev(idx.handle, pile.handle, *args, foreign.handle) == E and b"another index" in L.walt_last_error()
        assert L.walt_meth_pileup_batch_ev_device(idx.handle, pile.handle, *args, pile.handle, None) == E and b"one object" in L.walt_last_error()
        assert L.walt_meth_evidence_batch(idx.handle, foreign.handle, *args[:9], None, 1) == E and b"another index" in L.walt_last_error()
        assert L.walt_meth_evidence_batch(idx.handle, None, *args[:9], None, 1) == E and b"null evidence" in L.walt_last_error()
        n_out = ctypes.c_uint64(0)
        for fn, tail in ((L.walt_pileup_variants, (None, 0, ctypes.byref(n_out))), (L.walt_pileup_mask_variants, (None,))):
            assert fn(pile.handle, pile.handle, 0, 10, 5, 50, *tail) == E and b"one object" in L.walt_last_error()
            assert fn(pile.handle, foreign.handle, 0, 10, 5, 50, *tail) == E and b"another index" in L.walt_last_error()
            assert fn(pile.handle, ev.handle, 0, db.genome_len + 1, 5, 50, *tail) == E and b"range" in L.walt_last_error()
            assert fn(pile.handle, ev.handle, 0, 10, 0, 50, *tail) == E and b"min_depth" in L.walt_last_error()
            assert fn(pile.handle, ev.handle, 0, 10, 5, 100, *tail) == E and b"max_percent" in L.walt_last_error()
        assert_planes(ev, 4 * match, 4 * other, "after the refusals")
    finally:
        for p in (alone, plain, pile, ev, foreign):
            p.close()
        other_idx.close()


# ---------------------------------------------------------------------------
# 3. counters set by hand: the rule, ranges, caps, launch shapes, masking
# ---------------------------------------------------------------------------
MIN_DEPTH, MAX_PERCENT = 7, 30
FULL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hand(scratch):
    from test_gpu_levels import classes, small_genome
    from test_gpu_meth_contigs import build_index, remove_index
    g = small_genome(7)
    db, path, idx = build_index(g, scratch, "variants_hand")
    rng = random.Random(77)
    glen = g.genome_len
    R0 = g.R[0]
    pick_ev = [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 30]
    pick_calls = [0, 0, 1, 2, 5, 9, 100]
    match = np.array([rng.choice(pick_ev) for _ in range(glen)], dtype=np.uint32)
    other = np.array([rng.choice(pick_ev) for _ in range(glen)], dtype=np.uint32)
    meth = np.array([rng.choice(pick_calls) for _ in range(glen)], dtype=np.uint32)
    unmeth = np.array([rng.choice(pick_calls) for _ in range(glen)], dtype=np.uint32)
    sites = [f for f in range(100, 600) if chr(R0[f]) in "CG"]
    off_ref = [f for f in range(100, 600) if chr(R0[f]) in "AT"]
    # the five boundary cases of the rule at MIN_DEPTH 7, MAX_PERCENT 30, each on a site that carries calls, and an A/T
    # position whose evidence would be flagged if it were read
    edge = {"below the depth": (0, MIN_DEPTH - 1, False, False), "at the depth": (0, MIN_DEPTH, True, True),
            "100 other == p total": (7, 3, True, False), "one more other": (7, 4, True, True), "both counters full": (FULL, FULL, True, True)}
    at = {}
    for k, (name, (m, o, _, _)) in enumerate(edge.items()):
        f = sites[5 + 7 * k]
        at[name] = f
        match[f], other[f], meth[f], unmeth[f] = m, o, 3, 4
    at["A or T"] = off_ref[3]
    match[off_ref[3]], other[off_ref[3]], meth[off_ref[3]], unmeth[off_ref[3]] = 0, 50, 2, 2
    cls, pair = classes(R0, g.start_index)
    yield {"g": g, "idx": idx, "R0": R0, "match": match, "other": other, "meth": meth, "unmeth": unmeth, "edge": edge, "at": at,
           "cls": cls, "pair": pair}
    idx.close()
    remove_index(path)


def loaded(c):
    """a pile-up and an evidence object that hold the hand-set counters"""
    glen = c["g"].genome_len
    pile, ev = c["idx"].pileup(), c["idx"].pileup()
    pile.add(0, glen, c["meth"], c["unmeth"])
    ev.add(0, glen, c["match"], c["other"])
    return pile, ev


def test_rule_boundaries_ranges_and_caps(hand):
    import walt_amd
    c, g = hand, hand["g"]
    glen = g.genome_len
    pile, ev = loaded(c)
    try:
        full = pile.variants(ev, 0, glen, MIN_DEPTH, MAX_PERCENT)
        want = expected_variants(c["R0"], g.start_index, c["meth"], c["unmeth"], c["match"], c["other"], MIN_DEPTH, MAX_PERCENT)
        assert full.dtype == walt_amd.variant_site_dtype and full.tobytes() == want.tobytes() and full.size > 50
        assert {chr(int(s)) for s in full["strand"]} == {"+", "-"} and set(full["context"].tolist()) >= {0, 1, 2}
        got_at = set(full["pos"].tolist())
        for name, (m, o, is_judged, is_flagged) in c["edge"].items():
            f = c["at"][name]
            assert (f in got_at) == is_flagged == flagged(m, o, MIN_DEPTH, MAX_PERCENT) and judged(m, o, MIN_DEPTH) == is_judged, name
        assert c["at"]["A or T"] not in got_at
        row = full[full["pos"] == c["at"]["both counters full"]][0]
        assert (int(row["match"]), int(row["other"]), int(row["meth"]), int(row["unmeth"]), int(row["reserved"])) == (FULL, FULL, 3, 4, 0)
        # other rules: MethPipe's, the strictest and the loosest
        for d, p in ((5, 50), (1, 0), (1, 99), (FULL, 0), (31, 99)):
            w = expected_variants(c["R0"], g.start_index, c["meth"], c["unmeth"], c["match"], c["other"], d, p)
            assert pile.variants(ev, 0, glen, d, p).tobytes() == w.tobytes(), (d, p)
        # ranges that cut a chromosome, and the chromosomes of 1 and 2 bases
        rng = random.Random(3)
        starts = [int(x) for x in g.start_index]
        for cuts in ([0, 1, 2, glen - 1, glen], [0] + sorted(rng.sample(range(1, glen), 9)) + [glen],
                     sorted(set(starts + [s + 1 for s in starts[:-1]] + [max(s - 1, 0) for s in starts]))):
            parts = [pile.variants(ev, a, b, MIN_DEPTH, MAX_PERCENT) for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.concatenate(parts).tobytes() == full.tobytes(), cuts
        assert pile.variants(ev, 300, 300, MIN_DEPTH, MAX_PERCENT).size == 0
        # a cap that is too small: WALT_EINVAL, the count set, nothing written
        L = walt_amd.lib()
        n = ctypes.c_uint64(0)
        buf = np.full(24 * full.size, 0x23, dtype=np.uint8)
        rc = L.walt_pileup_variants(pile.handle, ev.handle, 0, glen, MIN_DEPTH, MAX_PERCENT, buf.ctypes.data, full.size - 1, ctypes.byref(n))
        assert rc == walt_amd.WALT_EINVAL and n.value == full.size and (buf == 0x23).all()
        msg = L.walt_last_error().decode()
        assert str(full.size) in msg and str(full.size - 1) in msg, msg
        rc = L.walt_pileup_variants(pile.handle, ev.handle, 0, glen, MIN_DEPTH, MAX_PERCENT, buf.ctypes.data, full.size, ctypes.byref(n))
        assert rc == 0 and buf.tobytes() == full.tobytes()
        # the extraction leaves both objects as they were
        assert pile.read()[0].tobytes() == c["meth"].tobytes() and ev.read()[1].tobytes() == c["other"].tobytes()
    finally:
        pile.close()
        ev.close()


@pytest.mark.parametrize("blocks", [0, 1, 7, 1000])
def test_masking_and_the_launch_shape(hand, index_options, blocks):
    from test_gpu_levels import as_dict, assert_same, expected_levels
    c, g = hand, hand["g"]
    glen = g.genome_len
    index_options(c["idx"], pile_extract_blocks=blocks)
    pile, ev = loaded(c)
    try:
        want_rows = expected_variants(c["R0"], g.start_index, c["meth"], c["unmeth"], c["match"], c["other"], MIN_DEPTH, MAX_PERCENT)
        assert pile.variants(ev, 0, glen, MIN_DEPTH, MAX_PERCENT).tobytes() == want_rows.tobytes()
        m2, u2, tot = expected_mask(c["R0"], c["meth"], c["unmeth"], c["match"], c["other"], MIN_DEPTH, MAX_PERCENT)
        assert tot[0] > tot[1] > tot[2] > 20 and tot[3] > 0 and tot[4] > 0
        # a range first: only its positions are masked
        a, b = 150, 2 * glen // 3
        ma, ua, ta = expected_mask(c["R0"], c["meth"], c["unmeth"], c["match"], c["other"], MIN_DEPTH, MAX_PERCENT, a, b)
        assert pile.mask_variants(ev, a, b, MIN_DEPTH, MAX_PERCENT).tolist() == ta
        gm, gu = pile.read()
        assert np.array_equal(gm, ma) and np.array_equal(gu, ua)
        # then everything: what this call removed, and the same judged and flagged as a call over untouched counters
        rest = pile.mask_variants(ev, 0, glen, MIN_DEPTH, MAX_PERCENT).tolist()
        assert rest == tot[:2] + [tot[k] - ta[k] for k in (2, 3, 4)]
        gm, gu = pile.read()
        assert np.array_equal(gm, m2) and np.array_equal(gu, u2)
        assert gm[c["at"]["A or T"]] == 2 and gm[c["at"]["100 other == p total"]] == 3 and gm[c["at"]["both counters full"]] == 0
        # masking twice
        assert pile.mask_variants(ev, 0, glen, MIN_DEPTH, MAX_PERCENT).tolist() == tot[:2] + [0, 0, 0]
        # the records afterwards: the same positions, no calls
        after = pile.variants(ev, 0, glen, MIN_DEPTH, MAX_PERCENT)
        assert after["pos"].tobytes() == want_rows["pos"].tobytes() and not after["meth"].any() and not after["unmeth"].any()
        # a masked cytosine is still a site of the genome, merely uncovered
        assert_same(as_dict(pile.levels()), expected_levels(c["cls"], c["pair"], m2, u2), "levels after masking, %d blocks" % blocks)
        assert ev.read()[0].tobytes() == c["match"].tobytes() and ev.read()[1].tobytes() == c["other"].tobytes()
    finally:
        pile.close()
        ev.close()


# ---------------------------------------------------------------------------
# 4. meaning, end to end: planted C>T changes, bisulfite reads of both strands, the unchanged index
# ---------------------------------------------------------------------------
def test_planted_variants_are_flagged_and_unmethylated_cytosines_are_not(g1):
    import walt_amd
    idx, db, R = g1["idx"], g1["db"], g1["R"]
    text = R[0].tobytes().decode()
    lo, hi = 2000, 6000  # a window of the first chromosome
    assert hi + 200 < int(db.start_index[1])
    rng = random.Random(12)
    sample = list(text)
    planted_at = []
    cpg_c = [f for f in range(lo + 150, hi - 150) if text[f:f + 2] == "CG"]
    for f in range(lo + 150, hi - 150, 45):  # a C>T on one strand or the other every 45 bases, CpGs first where there are any
        near = [c for c in cpg_c if f <= c < f + 20]
        cands = ([near[0], near[0] + 1] if near and rng.random() < 0.6 else []) or [q for q in range(f, f + 20) if text[q] in "CG"]
        q = rng.choice(cands)
        sample[q] = "T" if text[q] == "C" else "A"  # G>A is C>T on the '-' strand
        planted_at.append(q)
    sample = "".join(sample)
    at_cpg = [q for q in planted_at if text[q:q + 2] == "CG" or text[q - 1:q + 1] == "CG"]
    assert len(planted_at) > 70 and len(at_cpg) >= 10 and {text[q] for q in planted_at} == {"C", "G"}
    # fully unmethylated reads of both strands, one every 8 bases: depth 12 on each strand
    seqs = []
    for p in range(lo, hi - 100, 8):
        frag = sample[p:p + 100]
        seqs += [frag.replace("C", "T"), refio.revcomp(frag).replace("C", "T")]
    bases, offs = walt_amd.pack_reads(seqs)
    recs, _ = idx.map_se_batch(bases, offs)
    # (the genome has repeats: what the test needs is enough uniquely mapped reads of both strands for the counts below)
    assert (recs["times"] == 1).mean() > 0.8 and {b"+", b"-"} <= set(recs["strand"][recs["times"] == 1].tolist())
    pile, ev = idx.pileup(), idx.pileup()
    try:
        pile.add_batch(bases, offs, recs, "T", want_calls=False, want_counts=False, want_stats=False, evidence=ev)
        match, other = ev.read()
        meth, unmeth = pile.read()
        assert not meth.any()  # no read kept a C
        deep = [q for q in planted_at if int(match[q]) + int(other[q]) >= 5]
        assert len(deep) >= 50 and sum(q in at_cpg for q in deep) >= 5 and {text[q] for q in deep} == {"C", "G"}
        got = pile.variants(ev, 0, db.genome_len, 5, 50)
        flagged_at = set(got["pos"].tolist())
        assert set(deep) <= flagged_at, sorted(set(deep) - flagged_at)
        # no unmutated cytosine is flagged although every one of them is fully unmethylated
        assert flagged_at <= set(planted_at), sorted(flagged_at - set(planted_at))
        covered = [f for f in range(lo, hi) if unmeth[f] >= 5 and f not in flagged_at]
        assert len(covered) > 1000
        # without the evidence the planted positions look like unmethylated cytosines; masked, they carry no call
        assert all(unmeth[q] >= 5 for q in deep)
        tot = pile.mask_variants(ev, 0, db.genome_len, 5, 50).tolist()
        assert tot[1] == len(flagged_at) == tot[2] and tot[3] == 0 and tot[4] == int(unmeth[sorted(flagged_at)].sum())
        m2, u2 = pile.read()
        assert not u2[sorted(flagged_at)].any() and all(u2[f] == unmeth[f] for f in covered)
    finally:
        pile.close()
        ev.close()


# ---------------------------------------------------------------------------
# 5. command line
# ---------------------------------------------------------------------------
SAM_SKIP = 0x4 | 0x100 | 0x200 | 0x400  # unmapped, ambiguous, filtered (-F), duplicate (-D)
D2, P0 = 2, 0  # the rule of the command-line tests: -MVD 2 -MVP 0
MIN_FLAGGED_WITH_CALLS, MIN_UNFLAGGED_COVERED = 10, 1000


def sam_walk(sam_text, names, seqs, conv_of=None, limit_of=None):
    """What a run's SAM implies, over forward positions: (meth, unmeth, match, other, reads walked, reads left out for want of
    a call letter).  SEQ and XM:Z: of a record are in forward order: index k lies on forward position POS - 1 + k.  A record
    calls forward C's -- and is evidence at forward G's -- when it is ('+', 'T') or ('-', 'A'), else the other way round;
    which of the two it is comes from conv_of(flag) -> 'T' / 'A' where the run's mode says it, else from the reference base
    under the record's first call letter.  The calls come from XM:Z: where the run wrote it, else from the calling rule.
    limit_of(name, flag, n): the read positions below it count (-C); read position i is index n - 1 - i of a reversed record."""
    text = "".join(seqs)
    starts = [0]
    for q in seqs:
        starts.append(starts[-1] + len(q))
    glen = len(text)
    meth, unmeth, match, other = (np.zeros(glen, dtype=np.int64) for _ in range(4))
    walked = undecided = 0
    for line in sam_text.splitlines():
        if line.startswith("@"):
            continue
        p = line.split("\t")
        flag = int(p[1])
        if flag & SAM_SKIP:
            continue
        xm = [t[5:] for t in p[11:] if t.startswith("XM:Z:")]
        c = names.index(p[2])
        pos0, seq, hi = starts[c] + int(p[3]) - 1, p[9], starts[c + 1]
        n = len(seq)
        rev = bool(flag & 0x10)
        if conv_of is not None:
            on_c = rev == (conv_of(flag) == "A")
        else:
            letters = [k for k, ch in enumerate(xm[0]) if ch != "."]
            if not letters:
                undecided += 1
                continue
            on_c = text[pos0 + letters[0]] == "C"
        limit = n if limit_of is None else min(n, limit_of(p[0], flag, n))
        ks = range(n - limit, n) if rev else range(limit)
        walked += 1
        site, kept, conv_to, opp = ("C", "C", "T", "G") if on_c else ("G", "G", "A", "C")
        for k in ks:
            f = pos0 + k
            if not starts[c] <= f < hi:
                continue
            g, b = text[f], base_letter(ord(seq[k]))
            if g == opp:
                (match if b == opp else other)[f] += 1
            if xm:
                if xm[0][k] != ".":
                    (meth if xm[0][k].isupper() else unmeth)[f] += 1
            elif g == site and b in (kept, conv_to):
                (meth if b == kept else unmeth)[f] += 1
    return meth, unmeth, match, other, walked, undecided


def cli_texts(names, R0, start_index, meth, unmeth, match, other, min_depth, max_percent):
    """-> (.variants, one block of .variantstats, the masked .methcounts, the masked counters) of one read file"""
    def where(f):
        c = int(np.searchsorted(start_index, f, side="right")) - 1
        return names[c], f - int(start_index[c])

    ctx = ("CpG", "CHG", "CHH", "unknown")
    rows = expected_variants(R0, start_index, meth, unmeth, match, other, min_depth, max_percent)
    variants = "".join("%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\n" % (where(int(r["pos"])) + (chr(int(r["strand"])), ctx[int(r["context"])], int(r["meth"]),
                                                                 int(r["unmeth"]), int(r["match"]), int(r["other"]))) for r in rows)
    m2, u2, tot = expected_mask(R0, meth, unmeth, match, other, min_depth, max_percent)
    stats = "judged: %d\nflagged: %d\nmasked sites: %d\nmasked meth: %d\nmasked unmeth: %d\nrule\t%d\t%d\n" % (tuple(tot) + (min_depth, max_percent))
    counts = []
    for f in np.nonzero((m2 + u2) > 0)[0]:
        cls = site_class(R0, start_index, int(f))
        if cls is not None:
            counts.append("%s\t%d\t%s\t%s\t%d\t%d\n" % (where(int(f)) + (cls[0], ctx[cls[1]], int(m2[f]), int(u2[f]))))
    return variants, stats, "".join(counts), (m2, u2, tot, rows)


def enough_to_test(R0, meth, unmeth, match, other, min_depth=D2, max_percent=P0):
    """the condition the command-line tests carry: they cannot pass on an empty set"""
    on_ref = np.isin(R0, np.frombuffer(b"CG", dtype=np.uint8))
    flag = np.array([flagged(int(m), int(o), min_depth, max_percent) for m, o in zip(match, other)]) & on_ref
    covered = ((meth + unmeth) > 0) & on_ref
    return int((flag & covered).sum()), int((~flag & covered).sum())


@pytest.fixture(scope="module")
def cli(scratch):
    import walt_amd
    from test_gpu_cpgpairs import read_fasta
    path = os.path.join(scratch, "variants_cli_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    db = refio.DbIndex(path)
    names, seqs = read_fasta(os.path.join(refio.GOLDEN, "g1.fa"))
    R0 = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    assert names == db.names and R0.tobytes() == reference_bases(db)[0].tobytes()
    return {"db": db, "path": path, "names": names, "seqs": seqs, "R0": R0}


def check_run(c, out, conv_of=None, limit_of=None, blocks=1):
    """<out>.variants, .variantstats and the masked .methcounts of a run with -M -sam -MC against the walk over its own SAM"""
    db = c["db"]
    meth, unmeth, match, other, walked, undecided = sam_walk(open(out).read(), c["names"], c["seqs"], conv_of, limit_of)
    assert walked > 200 and undecided == 0
    variants, stats, counts, (m2, u2, tot, rows) = cli_texts(c["names"], c["R0"], db.start_index, meth, unmeth, match, other, D2, P0)
    assert open(out + ".variants").read() == variants * blocks
    assert open(out + ".variantstats").read() == stats * blocks
    assert open(out + ".methcounts").read() == counts * blocks
    with_calls, unflagged = enough_to_test(c["R0"], meth, unmeth, match, other)
    print("%s: %d flagged with calls, %d unflagged covered sites" % (os.path.basename(out), with_calls, unflagged))
    assert with_calls >= MIN_FLAGGED_WITH_CALLS and unflagged >= MIN_UNFLAGGED_COVERED, (with_calls, unflagged)
    assert tot[2] == with_calls
    return meth, unmeth, m2, u2


def own_files(out):
    d, b = os.path.dirname(out), os.path.basename(out)
    return sorted(f[len(b):] for f in os.listdir(d) if f.startswith(b) and f[len(b):][:1] not in ("", "-"))


MV = ["-MV", "-MVD", str(D2), "-MVP", str(P0)]


@pytest.mark.parametrize("mode", ["r", "A", "pe", "P", "R", "RP"])
def test_cli_every_mode_against_its_own_sam(cli, scratch, mode):
    from test_gpu_cpgpairs import mode_args, run_walt
    out = os.path.join(scratch, "variants_cli_" + mode)
    base = ["-i", cli["path"]] + mode_args(scratch, mode) + ["-a", "-u"]
    spelling = {"r": ["-MV"], "A": ["-variants"], "pe": ["--mask-variants"]}.get(mode, ["-MV"])
    rule = {"r": MV[1:], "A": ["-variant-min-depth", str(D2), "-variant-max-percent", str(P0)]}.get(mode, MV[1:])
    log = run_walt(base + ["-o", out, "-MC", "-M", "-sam", "-v"] + spelling + rule)
    conv_of = {"r": lambda flag: "T", "A": lambda flag: "A"}.get(mode)
    meth, unmeth, m2, u2 = check_run(cli, out, conv_of)
    if conv_of:  # the reference base under a record's first call letter says the same as the mode
        assert sam_walk(open(out).read(), cli["names"], cli["seqs"])[2].tolist() == sam_walk(open(out).read(), cli["names"], cli["seqs"], conv_of)[2].tolist()
    assert open(out + ".variantstats").read() in log  # -v
    # without -MV: no .variants, no .variantstats, unmasked counts, and every other output byte for byte
    run_walt(base + ["-o", out + "-plain", "-MC", "-M", "-sam"])
    assert sorted(own_files(out)) == sorted(own_files(out + "-plain") + [".variants", ".variantstats"])
    for sfx in [""] + own_files(out + "-plain"):
        same = open(out + sfx, "rb").read() == open(out + "-plain" + sfx, "rb").read()
        assert same == (sfx != ".methcounts"), sfx
    plain = cli_texts(cli["names"], cli["R0"], cli["db"].start_index, meth, unmeth, 0 * meth, 0 * meth, D2, P0)[2]
    assert open(out + "-plain.methcounts").read() == plain
    # -MV alone is a consumer: its own two files, the same as beside the others
    run_walt(base + ["-o", out + "-alone"] + MV)
    assert [f for f in own_files(out + "-alone") if f.startswith(".")] == [".mapstats", ".variants", ".variantstats"]
    for sfx in (".variants", ".variantstats"):
        assert open(out + "-alone" + sfx, "rb").read() == open(out + sfx, "rb").read(), sfx
    if mode in ("r", "pe"):
        # two shares of every batch on two pile-ups and two evidence objects (the same device twice), small batches: the
        # counters and the evidence are folded into the first before anything is judged
        run_walt(base + ["-o", out + "-g00", "-MC", "-g", "0,0", "-N", "1000"] + MV)
        for sfx in (".variants", ".variantstats", ".methcounts"):
            assert open(out + "-g00" + sfx, "rb").read() == open(out + sfx, "rb").read(), sfx
    if mode == "r":
        # two read files that share an output name: one table after another, the objects cleared in between
        fq = mode_args(scratch, mode)[1]
        run_walt(["-i", cli["path"], "-r", fq + "," + fq, "-o", out + "-two," + out + "-two", "-MC"] + MV)
        for sfx in (".variants", ".variantstats", ".methcounts"):
            assert open(out + "-two" + sfx).read() == 2 * open(out + sfx).read(), sfx


@pytest.mark.parametrize("case", ["D", "F", "C", "MC_ML_MR"])
def test_cli_options_act_on_the_evidence(cli, scratch, case):
    from test_gpu_cpgpairs import run_walt
    from test_gpu_dedup import doubled
    from test_gpu_levels import as_dict, classes, expected_levels, levels_text
    from test_gpu_meth import clip_point
    out = os.path.join(scratch, "variants_opt_" + case)
    fq = os.path.join(refio.GOLDEN, "se_ct.fastq")
    extra, limit_of = {"D": ["-D"], "F": ["-F", "2"]}.get(case, []), None
    if case == "D":
        (_, fq), = doubled(scratch, "variants_D", [fq])
    if case == "C":
        args = refio.golden_meta()["cases"]["se_clip_sam_au"]["args"]
        adaptor = args[args.index("-C") + 1]
        fq, extra = os.path.join(refio.GOLDEN, "se_clip.fastq"), ["-C", adaptor]
        reads = dict(zip(*load("se_clip.fastq")[:2]))
        limit_of = lambda name, flag, n: clip_point(adaptor, reads[name])
    if case == "MC_ML_MR":
        bed = os.path.join(scratch, "variants_regions.bed")
        with open(bed, "w") as f:
            f.write("%s\t0\t%d\n%s\t100\t5000\n" % (cli["names"][0], len(cli["seqs"][0]), cli["names"][1]))
        extra = ["-ML", "-MR", bed]
    base = ["-i", cli["path"], "-r", fq, "-a", "-u", "-M", "-sam", "-MC"]
    run_walt(base + ["-o", out] + MV + extra)
    meth, unmeth, m2, u2 = check_run(cli, out, lambda flag: "T", limit_of)
    if case in ("D", "F"):  # the option takes evidence away
        run_walt(base + ["-o", out + "-without"] + MV)
        assert int(open(out + ".variantstats").read().split()[1]) < int(open(out + "-without.variantstats").read().split()[1])
    if case == "C":  # the clip point bounds the evidence: the walk over whole reads gives another table
        whole = sam_walk(open(out).read(), cli["names"], cli["seqs"], lambda flag: "T")
        clipped = sam_walk(open(out).read(), cli["names"], cli["seqs"], lambda flag: "T", limit_of)
        assert int(whole[2].sum() + whole[3].sum()) > int(clipped[2].sum() + clipped[3].sum())
        assert whole[3].tolist() != clipped[3].tolist()  # (the bases behind a clip point are random: other bases there)
    if case == "MC_ML_MR":
        cls, pair = classes(cli["R0"], cli["db"].start_index)
        assert open(out + ".levels").read() == levels_text(expected_levels(cls, pair, m2, u2))
        run_walt(base + ["-o", out + "-plain"] + extra)
        assert open(out + "-plain.levels").read() == levels_text(expected_levels(cls, pair, meth, unmeth))
        assert open(out + ".regions").read() != open(out + "-plain.regions").read() and len(open(out + ".regions").read()) > 100


@pytest.mark.parametrize("pattern", [5, 7])
def test_cli_seed_patterns_5_and_7(cli, scratch, pattern):
    import walt_amd
    from test_gpu_cpgpairs import run_walt
    binary = os.path.join(refio.ROOT, "walt_amd", "bin", "walt_sp%d" % pattern)
    path = os.path.join(scratch, "variants_g1_sp%d.dbindex" % pattern)
    old = walt_amd.PATTERN
    walt_amd.set_pattern(pattern)
    try:
        walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    finally:
        walt_amd.set_pattern(old)
    out = os.path.join(scratch, "variants_cli_sp%d" % pattern)
    run_walt(["-i", path, "-r", os.path.join(refio.GOLDEN, "sp_se_ct.fastq"), "-o", out, "-MC", "-M", "-sam"] + MV, binary=binary)
    check_run(cli, out, lambda flag: "T")
