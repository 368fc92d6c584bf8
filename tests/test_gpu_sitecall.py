"""Called sites on the device (include/walt_amd.h, "called sites"): the joint histogram of (depth, meth) per context and the
extraction by a table "smallest significant meth per depth", against numpy folds and filters of Pileup.extract() over
hand-set counters -- every depth boundary, every launch shape, ranges, caps, the device forms -- and bin/walt -MS against a
Python restatement (binomial tail, textbook Benjamini-Hochberg) of the run's own <out>.methcounts.  The restatement at the
top needs no device: tests/test_sitecall_cpu.py checks the host code against it."""
import math
import os
import random

import numpy as np
import pytest

import refio

pytestmark = pytest.mark.gpu

CONTEXTS = ("CpG", "CHG", "CHH", "unknown")
DEPTH, BINS = 127, 8255   # WALT_SITECALL_DEPTH, WALT_SITECALL_BINS
LDS_DEPTH = 31            # sitecall_core.h kSiteLdsDepth: depths a block histograms in LDS; deeper bins are global atomics
FULL = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# the restatement (no device)
# ---------------------------------------------------------------------------
def site_bin(d, m):
    return (d - 1) * (d + 2) // 2 + m


def py_pval(d, m, r, _cache={}):
    """P(X >= m | d, r) as the issue words it: every term from k = d down to m, no early stop"""
    key = (d, m, r)
    if key not in _cache:
        if m == 0:
            p = 1.0
        elif r == 0:
            p = 0.0
        else:
            lr, l1, s = math.log(r), math.log1p(-r), 0.0
            for k in range(d, m - 1, -1):
                s += math.exp(math.lgamma(d + 1) - math.lgamma(k + 1) - math.lgamma(d - k + 1) + k * lr + (d - k) * l1)
            p = min(s, 1.0)
        _cache[key] = p
    return _cache[key]


def textbook_bh(ps, alpha):
    """the sorted-list Benjamini-Hochberg over one p-value per site: the cutoff (the largest p_(i) with p_(i) <= i * alpha
    / n), or None"""
    s = sorted(ps)
    cut = None
    for i, p in enumerate(s, 1):
        if p <= i * alpha / len(s):
            cut = p
    return cut


def bh_clearance(ps, alpha):
    """the smallest relative distance of a group's p-value from its line K_j * alpha / n (inf without sites)"""
    s = sorted(ps)
    n, best = len(s), float("inf")
    for i, p in enumerate(s, 1):
        if i == n or s[i] != p:  # the last site of its group: K_j = i
            line = i * alpha / n
            best = min(best, abs(p - line) / line)
    return best


def table_from_cutoffs(cutoffs, r, min_depth):
    """min_meth[4][128] of the four contexts' cutoffs (None: nothing passes)"""
    t = np.zeros((4, DEPTH + 1), dtype=np.uint32)
    for c in range(4):
        for d in range(DEPTH + 1):
            t[c, d] = d + 1
            if cutoffs[c] is None or d < max(min_depth, 1):
                continue
            for m in range(1, d + 1):
                if py_pval(d, m, r) <= cutoffs[c]:
                    t[c, d] = m
                    break
    return t


def fold_sites(sites):
    """(hist[4][BINS], deep[4]) of extracted records"""
    hist, deep = np.zeros((4, BINS), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    d = sites["meth"].astype(np.int64) + sites["unmeth"].astype(np.int64)
    c = sites["context"].astype(np.int64)
    shallow = d <= DEPTH
    ds, ms = d[shallow], sites["meth"][shallow].astype(np.int64)
    np.add.at(hist, (c[shallow], (ds - 1) * (ds + 2) // 2 + ms), 1)
    np.add.at(deep, c[~shallow], 1)
    return hist, deep


def filter_sites(sites, table):
    """the records walt_pileup_call_sites gives for extracted records and a table"""
    d = sites["meth"].astype(np.int64) + sites["unmeth"].astype(np.int64)
    is_deep = d > DEPTH
    need = np.asarray(table, dtype=np.int64)[sites["context"].astype(np.int64), np.minimum(d, DEPTH)]
    keep = is_deep | (sites["meth"].astype(np.int64) >= need)
    out = sites[keep].copy()
    out["reserved"] = is_deep[keep]
    return out


def g6(x):
    return "%.6g" % x


def restate_run(counts_text, control, rate, alpha, min_depth):
    """(<out>.methsites, <out>.sitestats' block, per-context (tested, called), clearance) of one read file from its own
    <out>.methcounts; control: a sequence's name (the rate from its counts, its sites left out) or None (rate given)"""
    rows = [line.split("\t") for line in counts_text.splitlines()]
    cm = cu = 0
    if control is not None:
        for nm, _, _, _, m, u in rows:
            if nm == control:
                cm, cu = cm + int(m), cu + int(u)
        rate = cm / (cm + cu)
    tested = [[] for _ in range(4)]
    for row in rows:
        nm, _, _, ctx, m, u = row
        m, u = int(m), int(u)
        if nm != control and m + u >= min_depth:
            tested[CONTEXTS.index(ctx)].append((py_pval(m + u, m, rate), row))
    cutoffs = [textbook_bh([p for p, _ in t], alpha) if t else None for t in tested]
    clearance = min(bh_clearance([p for p, _ in t], alpha) for t in tested)
    called = [0] * 4
    lines = []
    for row in rows:
        nm, _, _, ctx, m, u = row
        c, m, u = CONTEXTS.index(ctx), int(m), int(u)
        if nm == control or m + u < min_depth or cutoffs[c] is None:
            continue
        p = py_pval(m + u, m, rate)
        if p <= cutoffs[c]:
            called[c] += 1
            lines.append("\t".join(row) + "\t" + g6(p) + "\n")
    stats = "control: %s\n" % (control if control is not None else "given")
    stats += "control meth: %s\ncontrol unmeth: %s\n" % ((cm, cu) if control is not None else ("NA", "NA"))
    stats += "non-conversion rate: %s\nrule\t%s\t%d\n" % (g6(rate), g6(alpha), min_depth)
    for c in range(4):
        stats += "%s\t%d\t%d\t%s\n" % (CONTEXTS[c], len(tested[c]), called[c], "NA" if cutoffs[c] is None else g6(cutoffs[c]))
    return "".join(lines), stats, [(len(tested[c]), called[c]) for c in range(4)], clearance


def sixth_digit_unit(text):
    """one unit in the sixth significant digit of a number printed with %.6g (which drops trailing zeros: the digits it
    dropped count)"""
    x = abs(float(text))
    return 0.0 if x == 0.0 else 10.0 ** (math.floor(math.log10(x)) - 5)


def same_pval_text(a, b):
    """two %.6g texts are equal or differ by one unit in the sixth significant digit at the most (the unit of the
    larger, where a power of ten lies between them; 1e-9 of a unit for the rounding of the subtraction)"""
    if a == b:
        return True
    return abs(float(a) - float(b)) <= max(sixth_digit_unit(a), sixth_digit_unit(b)) * (1 + 1e-9)


def assert_sites_text(got, want, what=""):
    g, w = got.splitlines(), want.splitlines()
    assert len(g) == len(w), (what, len(g), len(w))
    for a, b in zip(g, w):
        pa, pb = a.split("\t"), b.split("\t")
        assert pa[:6] == pb[:6] and same_pval_text(pa[6], pb[6]), (what, a, b)


def assert_stats_text(got, want, what=""):
    g, w = got.splitlines(), want.splitlines()
    assert len(g) == len(w) == 9, (what, got)
    for i, (a, b) in enumerate(zip(g, w)):
        if i == 3:  # the rate
            assert a.split(": ")[0] == b.split(": ")[0] and same_pval_text(a.split(": ")[1], b.split(": ")[1]), (what, a, b)
        elif i >= 5:  # context tested called cutoff: the integers exact
            pa, pb = a.split("\t"), b.split("\t")
            assert pa[:3] == pb[:3] and (pa[3] == pb[3] or same_pval_text(pa[3], pb[3])), (what, a, b)
        else:
            assert a == b, (what, a, b)


# ---------------------------------------------------------------------------
# 1. hand-set counters on small genomes
# ---------------------------------------------------------------------------
PICK = [0, 0, 0, 0, 1, 1, 1, 2, 3, 5, 15, 16, 30, 31, 32, 33, 63, 64, 100, 126, 127, 128, 1000, FULL]


# (meth, unmeth) set by hand on C's and G's: depth 1, each side of 31 | 32 and of 127 | 128 with meth 0, meth == depth and
# between, and full counters
EDGES = [(1, 0), (0, 1), (31, 0), (0, 31), (15, 16), (32, 0), (0, 32), (16, 16), (127, 0), (0, 127), (63, 64), (128, 0), (0, 128),
         (64, 64), (FULL, FULL), (FULL, 0), (0, FULL)]


def hand_counters(glen, seed):
    """every position, A and T included: depths on each side of the LDS / global boundary (31 | 32) and of the deep one
    (127 | 128), meth 0 and meth == depth, and both counters full"""
    rng = random.Random(seed)
    meth = np.array([rng.choice(PICK) for _ in range(glen)], dtype=np.uint32)
    unmeth = np.array([rng.choice(PICK) for _ in range(glen)], dtype=np.uint32)
    return meth, unmeth


@pytest.fixture(scope="module", params=[1, 7, 40])
def small(request, scratch):
    from test_gpu_levels import small_genome
    from test_gpu_meth_contigs import build_index, remove_index
    n_chrom = request.param
    g = small_genome(n_chrom)
    db, path, idx = build_index(g, scratch, "sitecall_small_%d" % n_chrom)
    pile = idx.pileup()
    try:
        meth, unmeth = hand_counters(g.genome_len, 50 + n_chrom)
        at = np.nonzero(np.isin(g.R[0], np.frombuffer(b"CG", dtype=np.uint8)))[0][7::11]  # C's and G's, a few apart
        for f, (m, u) in zip(at, EDGES):
            meth[f], unmeth[f] = m, u
        pile.add(0, g.genome_len, meth, unmeth)
        sites, off = pile.extract()
        yield {"g": g, "idx": idx, "pile": pile, "meth": meth, "unmeth": unmeth, "sites": sites, "off": off}
    finally:
        pile.close()
        idx.close()
        remove_index(path)


def within(sites, lo, hi):
    return sites[(sites["pos"] >= lo) & (sites["pos"] < hi)]


def random_table(seed):
    rng = random.Random(seed)
    return np.array([[rng.randrange(0, d + 3) for d in range(DEPTH + 1)] for _ in range(4)], dtype=np.uint32)


def none_table():
    return np.tile(np.arange(1, DEPTH + 2, dtype=np.uint32), (4, 1))


@pytest.mark.parametrize("blocks", [0, 1, 2, 7])
def test_histogram_and_calls_against_the_extraction_in_every_launch_shape(small, index_options, blocks):
    c = small
    g, pile, sites = c["g"], c["pile"], c["sites"]
    want_hist, want_deep = fold_sites(sites)
    # what the counters were chosen for is there
    d = sites["meth"].astype(np.int64) + sites["unmeth"].astype(np.int64)
    for depth in (1, LDS_DEPTH, LDS_DEPTH + 1, DEPTH, DEPTH + 1, 2 ** 33 - 2):
        assert (d == depth).any(), depth
    assert ((sites["meth"] == 0) & (d <= DEPTH)).any() and ((sites["unmeth"] == 0) & (d <= DEPTH)).any()
    assert int(c["off"].sum()) > 0  # counts on A / T positions, which appear nowhere
    assert (sites["context"] == 3).any() or g.n_chrom == 1  # a C on a chromosome's last base
    assert int(want_deep.sum()) > 10 and int(want_hist[:, site_bin(LDS_DEPTH + 1, 0):].sum()) > 10
    table = random_table(3)
    default = (pile.depth_hist(), pile.call_sites(table))
    index_options(c["idx"], pile_extract_blocks=blocks)
    hist, deep = pile.depth_hist()
    assert np.array_equal(hist, want_hist) and np.array_equal(deep, want_deep)
    for k in range(4):
        assert int(hist[k].sum() + deep[k]) == int((sites["context"] == k).sum())
    called = pile.call_sites(table)
    assert called.tobytes() == filter_sites(sites, table).tobytes()
    assert hist.tobytes() == default[0][0].tobytes() and deep.tobytes() == default[0][1].tobytes()
    assert called.tobytes() == default[1].tobytes()


def test_ranges_and_partitions(small):
    c = small
    g, pile, sites = c["g"], c["pile"], c["sites"]
    glen = g.genome_len
    whole_hist, whole_deep = pile.depth_hist()
    empty = pile.depth_hist(5, 5)
    assert not empty[0].any() and not empty[1].any() and len(pile.call_sites(none_table(), 5, 5)) == 0
    first = int(sites["pos"][0])
    one = pile.depth_hist(first, first + 1)
    assert int(one[0].sum() + one[1].sum()) == 1 and len(pile.call_sites(np.zeros((4, 128), dtype=np.uint32), first, first + 1)) == 1
    cut = int(g.start_index[1]) // 2 if g.n_chrom > 1 else glen // 3  # a range that cuts a chromosome
    for lo, hi in ((cut, glen), (0, cut), (cut, cut + 300)):
        h, dp = pile.depth_hist(lo, hi)
        wh, wd = fold_sites(within(sites, lo, hi))
        assert np.array_equal(h, wh) and np.array_equal(dp, wd), (lo, hi)
    rng = random.Random(17)
    table = random_table(4)
    for trial in range(3):
        cuts = sorted({0, glen} | {rng.randrange(glen) for _ in range(9)})
        sum_h, sum_d, parts = np.zeros_like(whole_hist), np.zeros_like(whole_deep), []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            h, dp = pile.depth_hist(lo, hi)
            sum_h += h
            sum_d += dp
            parts.append(pile.call_sites(table, lo, hi))
        assert np.array_equal(sum_h, whole_hist) and np.array_equal(sum_d, whole_deep)
        assert np.concatenate(parts).tobytes() == filter_sites(sites, table).tobytes()


def test_call_sites_at_the_table_and_on_either_side(small):
    c = small
    pile, sites = c["pile"], c["sites"]
    d = sites["meth"].astype(np.int64) + sites["unmeth"].astype(np.int64)
    shallow = sites[d <= DEPTH]
    ds = d[d <= DEPTH]
    # a table through the middle of what is there: for every (context, depth) the median meth of its sites
    table = none_table()
    for k in range(4):
        for depth in np.unique(ds[shallow["context"] == k]):
            ms = np.sort(shallow["meth"][(shallow["context"] == k) & (ds == depth)])
            table[k, depth] = ms[len(ms) // 2]
    need = table[shallow["context"].astype(np.int64), ds].astype(np.int64)
    diff = shallow["meth"].astype(np.int64) - need
    assert (diff == 0).any() and (diff == -1).any() and (diff == 1).any()
    got = pile.call_sites(table)
    assert got.tobytes() == filter_sites(sites, table).tobytes()
    assert int((got["reserved"] == 0).sum()) == int((diff >= 0).sum())
    # all d + 1: exactly the deep sites, reserved 1
    got = pile.call_sites(none_table())
    assert len(got) == int((d > DEPTH).sum()) > 0 and (got["reserved"] == 1).all()
    assert np.array_equal(got["pos"], sites["pos"][d > DEPTH])
    # all 1: every site with a methylated call, plus the deep sites (two of which have none)
    got = pile.call_sites(np.ones((4, 128), dtype=np.uint32))
    want = sites[(sites["meth"] >= 1) | (d > DEPTH)]
    assert np.array_equal(got["pos"], want["pos"]) and ((got["meth"] == 0) & (got["reserved"] == 1)).any()
    assert got.tobytes() == filter_sites(sites, np.ones((4, 128), dtype=np.uint32)).tobytes()
    with pytest.raises(ValueError):
        pile.call_sites(np.ones((4, 127), dtype=np.uint32))


def test_cap_too_small_host_and_device(small):
    import ctypes

    import torch
    import walt_amd
    c = small
    pile, glen = c["pile"], c["g"].genome_len
    L = walt_amd.lib()
    table = np.ones((4, 128), dtype=np.uint32)
    total = len(pile.call_sites(table))
    assert total > 20
    buf = np.full(total, 0xAB, dtype=np.uint8).repeat(16).view(walt_amd.meth_site_dtype)
    n = ctypes.c_uint64(0)
    rc = L.walt_pileup_call_sites(pile.handle, 0, glen, table.ctypes.data, buf.ctypes.data, total - 1, ctypes.byref(n))
    assert rc == walt_amd.WALT_EINVAL and n.value == total
    msg = L.walt_last_error().decode()
    assert str(total) in msg and str(total - 1) in msg and "walt_pileup_call_sites:" in msg
    assert (buf.view(np.uint8) == 0xAB).all()
    rc = L.walt_pileup_call_sites(pile.handle, 0, glen, table.ctypes.data, buf.ctypes.data, total, ctypes.byref(n))
    assert rc == walt_amd.WALT_OK and n.value == total and buf.tobytes() == pile.call_sites(table).tobytes()
    dev = torch.device("cuda", 0)
    d_table = torch.from_numpy(table.view(np.int32)).to(dev)
    d_out = torch.full((total, 2), -1, dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    pile.call_sites_device(0, glen, d_table.data_ptr(), d_out.data_ptr(), total - 1, d_n.data_ptr())
    torch.cuda.synchronize()
    assert int(d_n.item()) == total and bool((d_out == -1).all())
    pile.call_sites_device(0, glen, d_table.data_ptr(), d_out.data_ptr(), total, d_n.data_ptr())
    torch.cuda.synchronize()
    assert int(d_n.item()) == total and d_out.cpu().numpy().tobytes() == buf.tobytes()
    # cap 0 counts only
    pile.call_sites_device(0, glen, d_table.data_ptr(), None, 0, d_n.data_ptr())
    torch.cuda.synchronize()
    assert int(d_n.item()) == total


def test_device_forms_on_a_side_stream_and_refusals(small):
    import ctypes

    import torch
    import walt_amd
    c = small
    pile, glen = c["pile"], c["g"].genome_len
    L = walt_amd.lib()
    E = walt_amd.WALT_EINVAL
    dev = torch.device("cuda", 0)
    fresh = c["idx"].pileup()
    try:
        # the counters arrive on the side stream too: the passes are ordered behind them by the stream alone
        table = random_table(8)
        want_hist, want_deep = pile.depth_hist()
        want = pile.call_sites(table)
        d_hist = torch.full((4 * BINS + 1,), -1, dtype=torch.int64, device=dev)  # (a word behind it: stays as it is)
        d_deep = torch.full((4,), -1, dtype=torch.int64, device=dev)
        d_table = torch.from_numpy(table.view(np.int32)).to(dev)
        d_out = torch.zeros((len(want) + 1, 2), dtype=torch.int64, device=dev)
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        pile.depth_hist_device(0, glen, d_hist.data_ptr(), d_deep.data_ptr(), stream=side.cuda_stream)
        pile.call_sites_device(0, glen, d_table.data_ptr(), d_out.data_ptr(), len(want) + 1, d_n.data_ptr(), stream=side.cuda_stream)
        side.synchronize()
        assert d_hist[:-1].cpu().numpy().tobytes() == want_hist.tobytes() and int(d_hist[-1].item()) == -1
        assert d_deep.cpu().numpy().tobytes() == want_deep.tobytes()
        assert int(d_n.item()) == len(want) and d_out[:len(want)].cpu().numpy().tobytes() == want.tobytes()
        assert not d_out[len(want)].any()
        assert walt_amd.sitecall_bin(1, 0) == 0 and walt_amd.sitecall_bin(DEPTH, DEPTH) == BINS - 1 == walt_amd.SITECALL_BINS - 1
        assert pile.device_bytes == 8 * glen + (1 << 20)
        # misaligned and null addresses, a null pile-up, ranges outside the genome
        h, dp, t, o, nn = d_hist.data_ptr(), d_deep.data_ptr(), d_table.data_ptr(), d_out.data_ptr(), d_n.data_ptr()
        for args in ((h + 4, dp), (h, dp + 4)):
            assert L.walt_pileup_depth_hist_device(pile.handle, 0, glen, *args, None) == E and b"aligned" in L.walt_last_error()
        for args in ((None, dp), (h, None)):
            assert L.walt_pileup_depth_hist_device(pile.handle, 0, glen, *args, None) == E
        assert L.walt_pileup_depth_hist_device(None, 0, glen, h, dp, None) == E and b"null pile-up" in L.walt_last_error()
        assert L.walt_pileup_depth_hist_device(pile.handle, 0, glen + 1, h, dp, None) == E and b"range" in L.walt_last_error()
        for args in ((t + 2, o, 5, nn), (t, o + 8, 5, nn), (t, o, 5, nn + 4)):
            assert L.walt_pileup_call_sites_device(pile.handle, 0, glen, *args, None) == E and b"aligned" in L.walt_last_error()
        for args in ((None, o, 5, nn), (t, None, 5, nn), (t, o, 5, None)):
            assert L.walt_pileup_call_sites_device(pile.handle, 0, glen, *args, None) == E
        assert L.walt_pileup_call_sites_device(None, 0, glen, t, o, 5, nn, None) == E and b"null pile-up" in L.walt_last_error()
        assert L.walt_pileup_call_sites_device(pile.handle, 7, 6, t, o, 5, nn, None) == E and b"range" in L.walt_last_error()
        hist = np.zeros((4, BINS), dtype=np.uint64)
        deep = np.zeros(4, dtype=np.uint64)
        n = ctypes.c_uint64(0)
        assert L.walt_pileup_depth_hist(pile.handle, 0, glen + 1, hist.ctypes.data, deep.ctypes.data) == E
        assert L.walt_pileup_depth_hist(pile.handle, 0, glen, None, deep.ctypes.data) == E
        assert L.walt_pileup_depth_hist(None, 0, 0, hist.ctypes.data, deep.ctypes.data) == E
        assert L.walt_pileup_call_sites(pile.handle, 0, glen, None, None, 0, ctypes.byref(n)) == E
        assert L.walt_pileup_call_sites(pile.handle, 0, glen, table.ctypes.data, None, 0, None) == E
        assert L.walt_pileup_call_sites(None, 0, 0, table.ctypes.data, None, 0, ctypes.byref(n)) == E
        # (None of the four calls takes an index beside the pile-up -- a pile-up carries its own, as for
        # walt_pileup_extract_device -- so there is no "pile-up of another index" to refuse; null is the case that exists.)
        # a pile-up of the same index without counters: nothing anywhere
        eh, ed = fresh.depth_hist()
        assert not eh.any() and not ed.any() and len(fresh.call_sites(np.zeros((4, 128), dtype=np.uint32))) == 0
    finally:
        fresh.close()


# ---------------------------------------------------------------------------
# 2. more sequences than the chromosome table in LDS holds; one hot bin
# ---------------------------------------------------------------------------
def test_more_sequences_than_the_lds_table_holds(scratch):
    from test_gpu_meth_contigs import K_LDS, build_index, contig_genome, remove_index
    g = contig_genome(2047)
    assert g.n_chrom > K_LDS
    db, path, idx = build_index(g, scratch, "sitecall_contigs")
    pile = idx.pileup()
    try:
        meth, unmeth = hand_counters(g.genome_len, 9)
        pile.add(0, g.genome_len, meth, unmeth)
        sites, _ = pile.extract()
        assert (sites["context"] == 3).sum() > 100  # C's and G's at the ends of sequences
        table = random_table(5)
        for blocks in (0, 3):
            idx.set_option("pile_extract_blocks", blocks)  # (the index is this test's own)
            hist, deep = pile.depth_hist()
            wh, wd = fold_sites(sites)
            assert np.array_equal(hist, wh) and np.array_equal(deep, wd)
            assert pile.call_sites(table).tobytes() == filter_sites(sites, table).tobytes()
        lo, hi = int(g.start_index[1030]) + 3, int(g.start_index[1900]) + 1
        hist, deep = pile.depth_hist(lo, hi)
        wh, wd = fold_sites(within(sites, lo, hi))
        assert np.array_equal(hist, wh) and np.array_equal(deep, wd)
    finally:
        pile.close()
        idx.close()
        remove_index(path)


def test_one_hot_bin(scratch):
    """2^17 sites and more, every one of depth 1 with one methylated call: all adds of a block fall on one LDS word"""
    from test_gpu_meth_contigs import Genome, build_index, remove_index
    rng = random.Random(23)
    g = Genome(["hot"], ["".join(rng.choice("ACGTCG") for _ in range(210000))])
    db, path, idx = build_index(g, scratch, "sitecall_hot")
    pile = idx.pileup()
    try:
        pile.add(0, g.genome_len, np.ones(g.genome_len, dtype=np.uint32), None)
        n_sites = int(np.isin(g.R[0], np.frombuffer(b"CG", dtype=np.uint8)).sum())
        assert n_sites >= 1 << 17
        for blocks in (0, 1):
            idx.set_option("pile_extract_blocks", blocks)  # (the index is this test's own)
            hist, deep = pile.depth_hist()
            assert int(hist[:, site_bin(1, 1)].sum()) == n_sites == int(hist.sum()) and not deep.any()
            assert (hist[:3, site_bin(1, 1)] > 1000).all()
        assert len(pile.call_sites(np.ones((4, 128), dtype=np.uint32))) == n_sites
        assert len(pile.call_sites(none_table())) == 0
    finally:
        pile.close()
        idx.close()
        remove_index(path)


# ---------------------------------------------------------------------------
# 3. command line
# ---------------------------------------------------------------------------
# The golden libraries are shallow (depth 1 at two sites in three, seldom above 5) and methylated at about 5.5 % in every
# context and on every sequence alike: whichever sequence serves as the control, the sample is at its non-conversion rate
# and next to nothing is significant.  What the restatement gives for the settings below, from the libraries' golden
# records (CpG tested / called, the smallest relative distance of a p-value from its Benjamini-Hochberg line):
#   rate given, 0.001 at an FDR of 0.05   r 4261 / 317, 0.022   pe 4924 / 325, 0.037   R 5495 / 455, 0.016
#   control sequence (rate about 0.055)   r chrC, FDR 0.5, depth >= 3:  71 / 2, 0.38
#                                         pe chrC, FDR 0.5, depth >= 3: 257 / 2, 0.33
#                                         R chrB, FDR 0.5, depth >= 5:  170 / 1, 0.40
# so 0 < called < tested holds for CpG in every run, and no p-value lies near its line (CLEARANCE, asserted in every run).
RATE, ALPHA = "0.001", "0.05"
CONTROL_RUN = {"r": ("chrC", "0.5", 3), "pe": ("chrC", "0.5", 3), "R": ("chrB", "0.5", 5)}  # -MSN, -MSA, -MSD
CLEARANCE = 1e-6
SITE_FILES = [".methsites", ".sitestats"]


@pytest.fixture(scope="module")
def cli(scratch):
    import walt_amd
    path = os.path.join(scratch, "sitecall_cli_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    return {"path": path}


def own_files(out):
    d, b = os.path.dirname(out), os.path.basename(out)
    return sorted(f[len(b):] for f in os.listdir(d) if f.startswith(b) and f[len(b):][:1] not in ("", "-"))


def check_against_counts(out, control, rate, alpha=float(ALPHA), min_depth=1, blocks=1):
    sites, stats, per_context, clearance = restate_run(open(out + ".methcounts").read(), control, rate, alpha, min_depth)
    print("%s: rate %s, CpG tested %d called %d, clearance %.3g" % (os.path.basename(out), stats.splitlines()[3], per_context[0][0],
                                                                      per_context[0][1], clearance))
    assert clearance > CLEARANCE, clearance
    assert 0 < per_context[0][1] < per_context[0][0], per_context
    assert_sites_text(open(out + ".methsites").read(), sites * blocks, out)
    got = open(out + ".sitestats").read().splitlines(True)
    assert len(got) == 9 * blocks
    for k in range(blocks):
        assert_stats_text("".join(got[9 * k:9 * k + 9]), stats, out)
    return sites, stats


@pytest.mark.parametrize("mode", ["r", "pe", "R"])
def test_cli_against_the_restatement_of_its_own_counts(cli, scratch, mode):
    from test_gpu_cpgpairs import mode_args, run_walt
    out = os.path.join(scratch, "sitecall_cli_" + mode)
    base = ["-i", cli["path"]] + mode_args(scratch, mode) + ["-a", "-u"]
    spelling = {"r": "-MS", "pe": "-sites", "R": "--call-sites"}[mode]
    # the control sequence
    control, alpha, depth = CONTROL_RUN[mode]
    by_control = ["-MSN", control, "-MSA", alpha, "-MSD", str(depth)]
    log = run_walt(base + ["-o", out, "-MC", spelling, "-v"] + by_control)
    sites, stats = check_against_counts(out, control, None, float(alpha), depth)
    assert open(out + ".sitestats").read() in log  # -v
    assert sites and not any(line.startswith(control + "\t") for line in sites.splitlines())
    assert any(line.startswith(control + "\t") for line in open(out + ".methcounts"))
    # the rate given: no sequence is left out
    run_walt(base + ["-o", out + "-rate", "-MC", "-MS", "-MSR", RATE, "-MSA", ALPHA])
    sites_r, _ = check_against_counts(out + "-rate", None, float(RATE))
    assert any(line.startswith(control + "\t") for line in sites_r.splitlines())
    # a minimum depth
    run_walt(base + ["-o", out + "-d2", "-MC", "-MS", "-MSR", RATE, "-MSA", ALPHA, "-MSD", "2"])
    d2 = restate_run(open(out + "-d2.methcounts").read(), None, float(RATE), float(ALPHA), 2)
    assert d2[3] > CLEARANCE
    assert_sites_text(open(out + "-d2.methsites").read(), d2[0])
    assert_stats_text(open(out + "-d2.sitestats").read(), d2[1])
    assert all(int(p[4]) + int(p[5]) >= 2 for p in (line.split("\t") for line in d2[0].splitlines()))
    # without -MS: no new file, and every other output byte for byte
    run_walt(base + ["-o", out + "-plain", "-MC"])
    assert sorted(own_files(out)) == sorted(own_files(out + "-plain") + SITE_FILES)
    for sfx in [""] + own_files(out + "-plain"):
        assert open(out + sfx, "rb").read() == open(out + "-plain" + sfx, "rb").read(), sfx
    # -MS alone is a consumer: its own two files and no .methcounts
    run_walt(base + ["-o", out + "-alone", "-MS"] + by_control)
    assert [f for f in own_files(out + "-alone") if f.startswith(".")] == [".mapstats"] + SITE_FILES
    for sfx in SITE_FILES:
        assert open(out + "-alone" + sfx, "rb").read() == open(out + sfx, "rb").read(), sfx


def test_cli_two_devices_two_read_files_and_masked_counters(cli, scratch):
    from test_gpu_cpgpairs import mode_args, run_walt
    out = os.path.join(scratch, "sitecall_cli_more")
    reads = mode_args(scratch, "r")
    base = ["-i", cli["path"]] + reads + ["-a", "-u"]
    ms = ["-MS", "-MSR", RATE, "-MSA", ALPHA]
    run_walt(base + ["-o", out, "-MC"] + ms)
    check_against_counts(out, None, float(RATE))
    # -g 0,0: two shares on two pile-ups (the same device twice), small batches, folded into the first
    run_walt(base + ["-o", out + "-g00", "-MC", "-g", "0,0", "-N", "1000"] + ms)
    for sfx in SITE_FILES + [".methcounts"]:
        assert open(out + "-g00" + sfx, "rb").read() == open(out + sfx, "rb").read(), sfx
    # two read files that share an output name: one block after another, the counters cleared in between
    fq = reads[1]
    run_walt(["-i", cli["path"], "-r", fq + "," + fq, "-o", out + "-two," + out + "-two", "-MC"] + ms)
    for sfx in SITE_FILES + [".methcounts"]:
        assert open(out + "-two" + sfx).read() == 2 * open(out + sfx).read(), sfx
    # -MV: the calls come from the masked counters -- the restatement of the masked .methcounts -- and a site that the
    # plain run calls and -MV masks is gone
    run_walt(base + ["-o", out + "-mv", "-MC", "-MV", "-MVD", "2", "-MVP", "0"] + ms)
    check_against_counts(out + "-mv", None, float(RATE))
    key = lambda line: tuple(line.split("\t")[:2])
    masked = {key(line) for line in open(out + ".methcounts")} - {key(line) for line in open(out + "-mv.methcounts")}
    called = {key(line) for line in open(out + ".methsites")}
    called_mv = {key(line) for line in open(out + "-mv.methsites")}
    assert len(masked & called) >= 1 and not (masked & called_mv)
    flagged = {key(line) for line in open(out + "-mv.variants")}
    assert masked <= flagged


def test_cli_deep_sites_go_through_the_host(cli, scratch):
    """the golden library with five of its reads 140 times each: sites deeper than 127, which the device hands over as
    records (reserved 1) and the host ranks and judges by their own p-values -- the kept C's are called, the converted not"""
    from test_gpu_cpgpairs import mode_args, run_walt
    fq = mode_args(scratch, "r")[1]
    lines = open(fq).read().splitlines(True)
    deep_fq = os.path.join(scratch, "sitecall_deep.fastq")
    with open(deep_fq, "w") as f:
        f.write("".join(lines))
        for k in range(5):
            for copy in range(140):
                f.write("@deep%d_%d\n" % (k, copy) + "".join(lines[4 * k + 1:4 * k + 4]))
    out = os.path.join(scratch, "sitecall_cli_deep")
    for tag, more in (("", []), ("-g00", ["-g", "0,0", "-N", "700"])):
        run_walt(["-i", cli["path"], "-r", deep_fq, "-o", out + tag, "-MC", "-MS", "-MSR", RATE, "-MSA", ALPHA] + more)
    check_against_counts(out, None, float(RATE))
    depth = lambda line: int(line.split("\t")[4]) + int(line.split("\t")[5])
    deep_counts = [line for line in open(out + ".methcounts") if depth(line) > DEPTH]
    deep_called = [line for line in open(out + ".methsites") if depth(line) > DEPTH]
    assert len(deep_counts) >= 10 and 0 < len(deep_called) < len(deep_counts)
    assert all(int(line.split("\t")[4]) >= 100 for line in deep_called)
    for sfx in SITE_FILES + [".methcounts"]:
        assert open(out + "-g00" + sfx, "rb").read() == open(out + sfx, "rb").read(), sfx


def test_cli_refusals(cli, scratch):
    import subprocess

    from test_gpu_cpgpairs import mode_args
    from test_gpu_meth import WALT_BIN
    out = os.path.join(scratch, "sitecall_cli_refused")
    base = [WALT_BIN, "-i", cli["path"]] + mode_args(scratch, "r") + ["-o", out]

    def refused(args, *says):
        pr = subprocess.run(base + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert pr.returncode != 0, (args, pr.stdout[-500:])
        for s in says:
            assert s in pr.stdout, (args, s, pr.stdout[-500:])

    refused(["-MS"], "-MSN", "-MSR")
    refused(["-MS", "-MSN", "chrC", "-MSR", RATE], "not from both")
    for flag, values in (("-MSR", ("1", "-0.1", "1.5", "x", "")), ("-MSA", ("0", "1", "-1", "x", "0.0")), ("-MSD", ("0", "128", "-1", "2.5"))):
        for v in values:
            refused(["-MS", "-MSR", RATE][:1 if flag == "-MSR" else 3] + [flag, v], flag)
    for args in (["-MSN", "chrC"], ["-MSR", RATE], ["-MSA", ALPHA], ["-MSD", "3"], ["-MC", "-MSD", "3"]):
        refused(args, "go with -MS")
    assert not os.path.exists(out) and not any(os.path.exists(out + sfx) for sfx in SITE_FILES)
    # a control the index does not have is named once the index is open, before a read is mapped
    refused(["-MS", "-MSN", "chrNone"], "chrNone", "-MSN")
    assert os.path.getsize(out) == 0 and os.path.getsize(out + ".methsites") == 0
