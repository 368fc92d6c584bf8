"""Paired-end random PBAT (-RP, walt_map_pe_rpbat_batch) without a GPU: the command line refuses the combinations the
mode does not define before it opens a file or a device, every library and the Python binding carry the new calls,
the workspace arithmetic is the header's, and the contract's rule (include/walt_amd.h) as the GPU tests apply it.

The rule helpers here (pair_min_mm, pe_rpbat_rule, oracle_pe_rpbat) are what tests/test_gpu_pe_rpbat.py and
tools/soak.py check the call against."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import refio

WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
PE_RPBAT_SYMBOLS = ("walt_pe_rpbat_workspace_bytes", "walt_pe_rpbat_workspace_bytes_best", "walt_map_pe_rpbat_batch",
                    "walt_map_pe_rpbat_batch_device")
MATE_FIELDS = ("genome_pos", "times", "strand", "mismatch")
PAIR_FIELDS = ("best_times", "frag_len", "best_i", "best_j", "pair_mm")


# ---------------------------------------------------------------- the rule (include/walt_amd.h)
def pair_min_mm(db, ranked, len1, len2, max_mm, frag_range):
    """The final min_mm of the pair search per pair: the smallest r1[i].mismatch + r2[j].mismatch over the combinations
    it accepts (opposite strands, one chromosome, 0 < fragment <= frag_range, mismatches <= max_mm); -1 where none."""
    r1, n1, r2, n2 = ranked
    n, k = r1.shape
    out = np.full(n, -1, dtype=np.int64)
    start = db.start_index.astype(np.int64)
    length = np.diff(start)

    def prep(r, cnt, ln):
        pos = r["genome_pos"].astype(np.int64)
        chrom = np.searchsorted(start, pos, side="right") - 1 if db.n_chrom > 1 else np.zeros_like(pos)
        chrom = np.clip(chrom, 0, len(length) - 1)
        minus = r["strand"] == b"-"
        s = pos - start[chrom]
        s = np.where(minus, length[chrom] - s - ln[:, None], s)
        valid = np.arange(k)[None, :] < cnt[:, None]
        return chrom, minus, s, s + ln[:, None], r["mismatch"].astype(np.int64), valid

    c1, m1, s1, e1, mm1, v1 = prep(r1, n1, len1)
    c2, m2, s2, e2, mm2, v2 = prep(r2, n2, len2)
    for lo in range(0, n, 2048):
        sl = slice(lo, min(n, lo + 2048))
        frag = np.where(m1[sl][:, :, None], e1[sl][:, :, None] - s2[sl][:, None, :], e2[sl][:, None, :] - s1[sl][:, :, None])
        mm = mm1[sl][:, :, None] + mm2[sl][:, None, :]
        ok = (v1[sl][:, :, None] & v2[sl][:, None, :] & (m1[sl][:, :, None] != m2[sl][:, None, :]) &
              (c1[sl][:, :, None] == c2[sl][:, None, :]) & (frag > 0) & (frag <= frag_range) & (mm <= max_mm))
        best = np.where(ok, mm, 1 << 40).reshape(mm.shape[0], -1).min(axis=1)
        out[sl] = np.where(best < (1 << 40), best, -1)
    return out


def to_user_order(q):
    """A mate-exchanged result put back into user order: m1 <-> m2, best_i <-> best_j."""
    u = q.copy()
    u["m1"], u["m2"] = q["m2"], q["m1"]
    u["best_i"], u["best_j"] = q["best_j"], q["best_i"]
    return u


def se_pick(c, g):
    """Single-end random-PBAT rules 1-4 on two mate record arrays -> (records, True where the G->A record won)."""
    ct, gt = c["times"].astype(np.int64), g["times"].astype(np.int64)
    r1 = (ct == 1) & (gt == 1) & (c["genome_pos"] == g["genome_pos"]) & (c["strand"] == g["strand"])
    r2 = ~r1 & ((gt == 0) | ((ct > 0) & (c["mismatch"] < g["mismatch"])))
    r3 = ~r1 & ~r2 & ((ct == 0) | (g["mismatch"] < c["mismatch"]))
    r4 = ~r1 & ~r2 & ~r3
    rec = {f: np.where(r3, g[f], c[f]) for f in MATE_FIELDS}
    rec["times"] = np.where(r4, ct + gt, rec["times"]).astype(np.uint32)
    return rec, r3


def pe_rpbat_rule(p, q, mp, mq):
    """The contract on orientation T's records p and the mate-exchanged orientation's q (as returned, NOT in user
    order), with the pair searches' min_mm mp / mq -> (records as a dict of arrays, conv uint8[n, 2], rule per pair)."""
    u = to_user_order(q)
    P, Q = p["best_times"].astype(np.int64), u["best_times"].astype(np.int64)
    mp, mq = np.asarray(mp, dtype=np.int64), np.asarray(mq, dtype=np.int64)
    same = ((P == 1) & (Q == 1) & (p["m1"]["genome_pos"] == u["m1"]["genome_pos"]) & (p["m1"]["strand"] == u["m1"]["strand"]) &
            (p["m2"]["genome_pos"] == u["m2"]["genome_pos"]) & (p["m2"]["strand"] == u["m2"]["strand"]))
    r1 = same
    r2 = ~r1 & (P > 0) & ((Q == 0) | (mp < mq))
    r3 = ~r1 & ~r2 & (Q > 0) & ((P == 0) | (mq < mp))
    r4 = ~r1 & ~r2 & ~r3 & (P > 0) & (Q > 0)
    r5 = ~r1 & ~r2 & ~r3 & ~r4
    assert not (r4 & (mp != mq)).any()
    a = r4 | r5
    rec = {}
    mate1, g1 = se_pick(p["m1"], u["m1"])
    mate2, g2 = se_pick(u["m2"], p["m2"])
    for f in MATE_FIELDS:
        rec["m1." + f] = np.where(r3, u["m1"][f], np.where(a, mate1[f], p["m1"][f]))
        rec["m2." + f] = np.where(r3, u["m2"][f], np.where(a, mate2[f], p["m2"][f]))
    for f in PAIR_FIELDS:
        rec[f] = np.where(r3, u[f], p[f]).astype(np.int64)
    rec["best_times"] = np.where(a, P + Q, rec["best_times"])
    rec["frag_len"] = np.where(a, 0, rec["frag_len"])
    rec["best_i"] = np.where(a, -1, rec["best_i"])
    rec["best_j"] = np.where(a, -1, rec["best_j"])
    rec["pair_mm"] = np.where(a, 0, rec["pair_mm"])
    conv = np.zeros((len(P), 2), dtype=np.uint8)
    conv[:, 0] = np.where(r3 | (a & g1), ord("A"), ord("T"))
    # mate 2: c = q.m2 (C->T, conversion 'T'), g = p.m2 (G->A, 'A'): se_pick's True means p.m2 won -> 'A'
    conv[:, 1] = np.where(r3, ord("T"), np.where(a, np.where(g2, ord("A"), ord("T")), ord("A")))
    rule = np.select([r1, r2, r3, r4, r5], [1, 2, 3, 4, 5])
    return rec, conv, rule


def oracle_pe_rpbat(db, s1, s2, m=6, b=5000, k=50, L=1000):
    """The rule applied to the oracle's two orientations -> (records, conv, rule, too_short per mate)."""
    p, rp_, wp = refio.oracle_pe(db, s1, s2, max_mm=m, b=b, top_k=k, frag_range=L)
    q, rq_, _ = refio.oracle_pe(db, s2, s1, max_mm=m, b=b, top_k=k, frag_range=L)
    len1 = np.array([len(s) for s in s1], dtype=np.int64)
    len2 = np.array([len(s) for s in s2], dtype=np.int64)
    # min_mm is defined where best_times >= 1 (the search can accept combinations and still count none: both mates at
    # position 0 with max_mm mismatches equal the fold's initial best, core.h pair_merge)
    mp = np.where(p["best_times"] >= 1, pair_min_mm(db, rp_, len1, len2, m, L), -1)
    mq = np.where(q["best_times"] >= 1, pair_min_mm(db, rq_, len2, len1, m, L), -1)
    assert (mp[p["best_times"] >= 1] >= 0).all() and (mq[q["best_times"] >= 1] >= 0).all()
    assert (mp[p["best_times"] == 1] == p["pair_mm"][p["best_times"] == 1]).all()
    rec, conv, rule = pe_rpbat_rule(p, q, mp, mq)
    return rec, conv, rule, (int(wp[0]["too_short"]), int(wp[1]["too_short"]))


def compare(got, conv, want, want_conv, what=""):
    """Field-by-field comparison of walt_pair_result records (and conv[n, 2]) with the rule's."""
    for key, w in want.items():
        if "." in key:
            mate, f = key.split(".")
            g = got[mate][f]
        else:
            g = got[key]
        g = g.astype(np.int64) if g.dtype.kind in "iu" else g
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s %s differs at %s: got %s want %s" % (what, key, bad[:5], g[bad[:5]], w[bad[:5]])
    conv = np.asarray(conv).reshape(-1, 2)
    bad = np.nonzero((conv != want_conv).any(axis=1))[0]
    assert bad.size == 0, "%s conv differs at %s: got %s want %s" % (what, bad[:5], conv[bad[:5]], want_conv[bad[:5]])


# ---------------------------------------------------------------- the command line
@pytest.mark.parametrize("extra, word", [
    (["-r", "reads.fq"], "-r"),
    (["-1", "r1.fq", "-2", "r2.fq", "-A"], "-A"),
    (["-1", "r1.fq", "-2", "r2.fq", "-P"], "-P"),
    (["-1", "r1.fq", "-2", "r2.fq", "-R"], "-R"),
    (["-1", "r1.fq", "-2", "r2.fq", "--random-pbat"], "-R"),
])
def test_cli_refuses_random_pbat_pe_combinations(tmp_path, extra, word):
    # neither the index nor the reads exist: the refusal comes from the option check, before any file or device
    for opt in ("-RP", "--random-pbat-pe"):
        p = subprocess.run([WALT_BIN, "-i", str(tmp_path / "none.dbindex"), "-o", str(tmp_path / "out.mr"), opt] + extra,
                           capture_output=True, text=True, cwd=str(tmp_path))
        assert p.returncode != 0
        assert "-RP" in p.stderr and word in p.stderr, p.stderr
        assert "index file missing" not in p.stderr
        assert not os.path.exists(tmp_path / "out.mr")


def test_cli_knows_the_option(tmp_path):
    # -RP with -1 / -2 passes the option check and stops at the missing index, like any other paired-end run
    p = subprocess.run([WALT_BIN, "-i", str(tmp_path / "none.dbindex"), "-o", str(tmp_path / "out.mr"), "-RP", "-1",
                        "r1.fq", "-2", "r2.fq"], capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode != 0 and "index file missing" in p.stderr, p.stderr
    p = subprocess.run([WALT_BIN], capture_output=True, text=True)
    assert " -RP " in p.stderr


def test_single_end_option_points_to_the_paired_one(tmp_path):
    p = subprocess.run([WALT_BIN, "-i", str(tmp_path / "none.dbindex"), "-o", str(tmp_path / "out.mr"), "-R", "-1",
                        "r1.fq", "-2", "r2.fq"], capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode != 0 and "-R" in p.stderr and "-1" in p.stderr and "-RP" in p.stderr, p.stderr


# ---------------------------------------------------------------- the library and the binding
def test_index_has_pe_random_pbat_methods():
    import walt_amd
    assert callable(getattr(walt_amd.Index, "map_pe_rpbat_batch", None))
    assert callable(getattr(walt_amd.Index, "map_pe_rpbat_batch_device", None))
    assert callable(getattr(walt_amd.Index, "pe_rpbat_workspace_bytes", None))
    assert callable(getattr(walt_amd, "pe_rpbat_workspace_bytes", None))


@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_pe_random_pbat_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    for nm in PE_RPBAT_SYMBOLS:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)


def header_formula(n, top_k, pe_bytes):
    """walt_pe_rpbat_workspace_bytes as include/walt_amd.h states it."""
    c = min(n, max(65536, min(1 << 23, (10 << 30) // (24 * top_k))))
    s = 2 if n > c else 1
    return pe_bytes + s * ((64 * c + 255) // 256 * 256)


@pytest.mark.parametrize("n, read_len, top_k", [(1, 100, 50), (1800, 150, 2), (100000, 100, 50), (9000000, 100, 50),
                                                (20000000, 150, 300), (5000000, 100, 2)])
def test_workspace_holds_the_second_record_array(n, read_len, top_k):
    """walt_pe_rpbat_workspace_bytes = walt_pe_workspace_bytes plus one pass of 64-byte records per pipeline slot."""
    import walt_amd
    L = walt_amd.lib(3)
    pe = L.walt_pe_workspace_bytes(n, read_len, top_k)
    both = L.walt_pe_rpbat_workspace_bytes(n, read_len, top_k)
    assert both >= pe + 64 * min(n, 65536)
    assert both == header_formula(n, top_k, pe)
    assert walt_amd.pe_rpbat_workspace_bytes(n, read_len, top_k) == both
    assert L.walt_pe_rpbat_workspace_bytes_best(None, n, read_len, top_k) == both


# ---------------------------------------------------------------- the rule on hand-made records
def _pairs(rows):
    """rows: (m1 (pos, times, strand, mm), m2 (...), best_times, frag_len, best_i, best_j, pair_mm) -> pair_dtype."""
    a = np.zeros(len(rows), dtype=refio.pair_dtype)
    for i, (m1, m2, bt, fl, bi, bj, pm) in enumerate(rows):
        for mate, v in (("m1", m1), ("m2", m2)):
            a[mate]["genome_pos"][i], a[mate]["times"][i], a[mate]["strand"][i], a[mate]["mismatch"][i] = v
        a["best_times"][i], a["frag_len"][i], a["best_i"][i], a["best_j"][i], a["pair_mm"][i] = bt, fl, bi, bj, pm
    return a


UNM = (0, 0, b"+", 6)


def test_rule_on_hand_made_records():
    # p: orientation T (mate 1 C->T, mate 2 G->A); q: mates exchanged (q.m1 is the user's mate 2, mapped C->T)
    p = _pairs([
        ((100, 1, b"+", 0), (300, 1, b"-", 0), 1, 250, 2, 1, 0),   # 1: the same pair both ways
        ((100, 1, b"+", 1), (300, 1, b"-", 0), 1, 250, 2, 1, 1),   # 2: T with fewer mismatches
        ((100, 1, b"+", 2), (300, 1, b"-", 2), 1, 250, 2, 1, 4),   # 3: A with fewer mismatches
        ((100, 2, b"+", 1), (300, 2, b"-", 1), 2, 0, -1, -1, 0),   # 4: ambiguous both ways, mp == mq == 2
        (UNM, (300, 1, b"-", 3), 0, 0, -1, -1, 0),                 # 5: no pair either way
        (UNM, UNM, 0, 0, -1, -1, 0),                               # 3: only A pairs
    ])
    q = _pairs([
        ((300, 1, b"-", 0), (100, 1, b"+", 0), 1, 250, 1, 2, 0),
        ((900, 1, b"-", 1), (700, 1, b"+", 1), 1, 200, 0, 0, 2),
        ((900, 1, b"-", 0), (700, 1, b"+", 1), 1, 200, 3, 4, 1),
        ((500, 1, b"-", 1), (600, 1, b"+", 1), 3, 0, -1, -1, 0),
        ((800, 1, b"+", 2), (400, 2, b"+", 1), 0, 0, -1, -1, 0),
        ((800, 1, b"-", 0), (700, 1, b"+", 0), 1, 200, 0, 5, 0),
    ])
    mp = np.array([0, 1, 4, 2, -1, -1])
    mq = np.array([0, 2, 1, 2, -1, 0])
    rec, conv, rule = pe_rpbat_rule(p, q, mp, mq)
    assert list(rule) == [1, 2, 3, 4, 5, 3]
    assert [bytes(c).decode() for c in conv[:3]] == ["TA", "TA", "AT"]
    # rule 3 in user order: mate 1 is q.m2, mate 2 is q.m1, best_i / best_j exchanged
    assert rec["m1.genome_pos"][2] == 700 and rec["m2.genome_pos"][2] == 900
    assert (rec["best_i"][2], rec["best_j"][2]) == (4, 3) and rec["pair_mm"][2] == 1 and rec["frag_len"][2] == 200
    # rule 4: P + Q, no pair; mate 1: p.m1 (2 hits, 1 mm) vs q.m2 (600, 1 hit, 1 mm): equal mismatches -> T, times 3;
    # mate 2: q.m1 (500, 1 mm) vs p.m2 (300, 2 hits, 1 mm): equal -> T (q.m1), times 3
    assert rec["best_times"][3] == 5 and rec["frag_len"][3] == 0 and rec["best_i"][3] == -1 and rec["pair_mm"][3] == 0
    assert rec["m1.times"][3] == 3 and rec["m1.genome_pos"][3] == 100
    assert rec["m2.times"][3] == 3 and rec["m2.genome_pos"][3] == 500
    assert bytes(conv[3]).decode() == "TT"
    # rule 5: mate 1 unmapped in p, q.m2 = (400, 2 hits, 1 mm) -> A; mate 2: q.m1 (800, 2 mm) vs p.m2 (300, 3 mm) -> T
    assert rec["best_times"][4] == 0
    assert rec["m1.genome_pos"][4] == 400 and rec["m1.times"][4] == 2 and rec["m2.genome_pos"][4] == 800
    assert bytes(conv[4]).decode() == "AT"
    assert bytes(conv[5]).decode() == "AT" and rec["m1.genome_pos"][5] == 700
