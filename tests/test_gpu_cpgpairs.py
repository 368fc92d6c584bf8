"""Adjacent-CpG state pairs per read on the GPU (include/walt_amd.h, "adjacent CpG pairs"): walt_cpgpairs_* through
walt_amd.CpgPairs, the composition with the calling (pairs= on Index.meth_call_batch / Pileup.add_batch and their device
forms) and bin/walt -MA, all against one pure-Python restatement of the contract (find_pairs / expected_table below),
which never uses the code under test: it finds the pairs by scanning the genome's text and walks the calls of a read in
order as the contract says."""
import bisect
import math
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import refio
from test_gpu_meth_contigs import Genome, build_index, remove_index

WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
LENGTHS = (1, 15, 16, 17, 31, 127, 128, 129, 1024)
COLUMNS = ("MM", "MU", "UM", "UU")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def find_pairs(text, start_index):
    """the forward positions c with text[c] == 'C', text[c + 1] == 'G' and c + 1 in c's chromosome, ascending"""
    starts = [int(v) for v in start_index]
    out = []
    for k in range(len(starts) - 1):
        for c in range(starts[k], starts[k + 1] - 1):
            if text[c] == "C" and text[c + 1] == "G":
                out.append(c)
    return out


def expected_table(text, start_index, calls, offsets, pos, times, strand, skip=None, base=None, into=None):
    """count[n_pairs][4].  calls: uint8 array whose element 0 is byte `base` (default offsets[0]) of what the offsets index;
    pos / times / strand: per record (strand '+' / '-' as str or bytes)."""
    starts = [int(v) for v in start_index]
    genome_len = starts[-1]
    pairs = find_pairs(text, starts)
    number = {c: j for j, c in enumerate(pairs)}
    calls = np.asarray(calls, dtype=np.uint8)
    offsets = [int(v) for v in offsets]
    base = offsets[0] if base is None else base
    table = np.zeros((len(pairs), 4), dtype=np.uint64) if into is None else into
    for r in range(len(offsets) - 1):
        lo_b, hi_b = offsets[r] - base, offsets[r + 1] - base
        p = int(pos[r])
        if int(times[r]) != 1 or (skip is not None and int(skip[r]) != 0) or not 1 <= hi_b - lo_b <= 1024 or p >= genome_len:
            continue
        k = bisect.bisect_right(starts, p) - 1
        lo, hi = starts[k], starts[k + 1]
        minus = strand[r] in ("-", b"-")
        prev = None
        for i, b in enumerate(calls[lo_b:hi_b].tolist()):
            if b not in (0x7A, 0x5A):  # z, Z
                continue
            q = p + i
            if q >= hi:
                continue
            f = lo + hi - 1 - q if minus else q
            j = number.get(f, number.get(f - 1))
            if j is None:
                continue
            cur = (j, 1 if b == 0x7A else 0)
            if prev is not None and abs(cur[0] - prev[0]) == 1:
                (jl, ul), (jh, uh) = sorted([prev, cur])
                table[jl, 2 * ul + uh] += np.uint64(1)
            prev = cur
    return table


def sites_of(table, pairs, pos_lo=0, pos_hi=None):
    """the extraction of a table: [(pos, next, MM, MU, UM, UU)] of the non-zero entries with pos in [pos_lo, pos_hi)"""
    out = []
    for j in np.nonzero(np.asarray(table).any(axis=1))[0].tolist():
        if pos_lo <= pairs[j] and (pos_hi is None or pairs[j] < pos_hi):
            out.append((pairs[j], pairs[j + 1]) + tuple(int(v) for v in table[j]))
    return out


def sites_list(sites):
    return [(int(s["pos"]), int(s["next"])) + tuple(int(v) for v in s["n"]) for s in sites]


def fisher_exact(a, b, c, d):
    """two-sided Fisher exact test of [[a, b], [c, d]] in exact arithmetic: the sum of the probabilities of the tables with
    the same margins whose probability is at most P(observed) * (1 + 1e-7), capped at 1"""
    # (the test does not change when rows or columns swap or the table is transposed: the smallest margin goes first,
    # which keeps the binomials small)
    a, b, c, d = min(((a, b, c, d), (b, a, d, c), (a, c, b, d), (c, a, d, b)), key=lambda t: t[0] + t[2])
    r1, c1, n = a + b, a + c, a + b + c + d
    if n == 0:
        return Fraction(1)
    den = math.comb(n, c1)
    prob = lambda x: Fraction(math.comb(r1, x) * math.comb(n - r1, c1 - x), den)
    bound = prob(a) * (1 + Fraction(1, 10 ** 7))
    probs = [prob(x) for x in range(max(0, r1 + c1 - n), min(r1, c1) + 1)]
    return min(sum((p for p in probs if p <= bound), Fraction(0)), Fraction(1))


def allelic_line(chrom, pos, nxt, n):
    return "%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % (chrom, pos, nxt, "%.6g" % float(fisher_exact(*n)), sum(n), n[0], n[1], n[2], n[3])


def parse_allelic(text):
    """-> [(chrom, pos, next, pval, total, MM, MU, UM, UU)]"""
    out = []
    for line in text.splitlines():
        p = line.split("\t")
        assert len(p) == 9, line
        out.append((p[0], int(p[1]), int(p[2]), float(p[3])) + tuple(int(v) for v in p[4:]))
    return out


def same_allelic(got, want):
    """integers exactly, pval within 1e-5 relative"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g[:3] == w[:3] and g[4:] == w[4:], (g, w)
        assert g[4] == sum(g[5:])
        assert abs(g[3] - w[3]) <= 1e-5 * w[3], (g, w)


def read_fasta(path):
    names, seqs = [], []
    for line in open(path):
        if line.startswith(">"):
            names.append(line[1:].split()[0])
            seqs.append([])
        else:
            seqs[-1].append(line.strip().upper())
    return names, ["".join(s) for s in seqs]


def table_from_sam(sam_text, names, seqs):
    """The table a run's own SAM implies: unique records (no 0x4, 0x100, 0x200, 0x400) with an XM:Z: string, which is in
    the order of SEQ -- XM[k] lies on forward position POS - 1 + k -- walked forwards: a couple does not depend on the
    direction its read is walked in."""
    text = "".join(seqs)
    starts = [0]
    for s in seqs:
        starts.append(starts[-1] + len(s))
    pairs = find_pairs(text, starts)
    table = np.zeros((len(pairs), 4), dtype=np.uint64)
    calls, offsets, pos = [], [0], []
    for line in sam_text.splitlines():
        if line.startswith("@"):
            continue
        p = line.split("\t")
        xm = [t[5:] for t in p[11:] if t.startswith("XM:Z:")]
        if int(p[1]) & (0x4 | 0x100 | 0x200 | 0x400) or not xm:
            continue
        calls.append(xm[0])
        offsets.append(offsets[-1] + len(xm[0]))
        pos.append(starts[names.index(p[2])] + int(p[3]) - 1)
    flat = np.frombuffer("".join(calls).encode(), dtype=np.uint8)
    expected_table(text, starts, flat, offsets, pos, [1] * len(pos), ["+"] * len(pos), into=table)
    return table, pairs, starts


def allelic_rows(table, pairs, names, starts):
    out = []
    for pos, nxt, *n in sites_of(table, pairs):
        k = bisect.bisect_right(starts, pos) - 1
        out.append((names[k], pos - starts[k], nxt - starts[k], float(fisher_exact(*n)), sum(n)) + tuple(n))
    return out


# ---------------------------------------------------------------------------
# the hand-made genome and its batches
# ---------------------------------------------------------------------------
RULERS = (14, 15, 16, 30, 126, 127, 128, 1022, 1023)  # two neighbouring pairs whose C's lie this far apart, none between


def pair_genome():
    """About 20,000 bases in 4 chromosomes, CpG density near 1/16 (uniform random bases).  Chromosome 0 starts with the
    rulers -- CG, G-free filler, CG -- and a CGCGCG stretch of 64 bases; chromosome 1 ends in C and chromosome 2 starts with
    G (no pair); the starts are no multiples of 128."""
    rng = random.Random(2024)
    rnd = lambda n, al="ACGT": "".join(rng.choice(al) for _ in range(n))
    parts, at, where = [], 0, {}

    def put(s):
        nonlocal at
        parts.append(s)
        at += len(s)

    put(rnd(37, "ACT"))
    for d in RULERS:
        where[d] = at
        put("CG" + rnd(d - 2, "ACT") + "CG" + rnd(9, "ACT"))
    where["stretch"] = at
    put("CG" * 32)
    put(rnd(50, "ACT") + rnd(5000 - (at + 50) % 5000 + 77))
    c0 = "".join(parts)
    c1 = rnd(4999) + "C"
    c2 = "G" + rnd(6100)
    c3 = rnd(3333) + "CG"  # a pair that ends the genome
    g = Genome(["p0", "p1", "p2", "p3"], [c0, c1, c2, c3])
    assert all(int(s) % 128 for s in g.start_index[1:])
    return g, where


class Hand:
    """reads made by hand: add(pos, strand, calls, times) -> the arrays of one batch"""

    def __init__(self):
        self.pos, self.strand, self.times, self.calls = [], [], [], []

    def add(self, pos, strand, calls, times=1):
        self.pos.append(pos)
        self.strand.append(strand)
        self.times.append(times)
        self.calls.append(calls if isinstance(calls, bytes) else calls.encode())
        return self

    def arrays(self, stride=16):
        import walt_amd
        n = len(self.pos)
        rec = np.zeros(n, dtype=walt_amd.best_match_dtype if stride == 16 else walt_amd.pair_result_dtype)
        view = rec if stride == 16 else rec["m2"]  # the second mate of a walt_pair_result array: stride 64, base + 16
        view["genome_pos"], view["times"], view["strand"] = self.pos, self.times, [s.encode() for s in self.strand]
        if stride != 16:
            rec["m1"]["times"] = 1  # (the other mate's would be wrong)
            rec["m1"]["strand"] = b"+"
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(c) for c in self.calls])
        return np.frombuffer(b"".join(self.calls), dtype=np.uint8), offsets, view

    def head(self, n):
        h = Hand()
        h.pos, h.strand, h.times, h.calls = self.pos[:n], self.strand[:n], self.times[:n], self.calls[:n]
        return h

    def want(self, g, skip=None, into=None):
        calls, offsets, _ = self.arrays()
        return expected_table(g.text, g.start_index, calls, offsets, self.pos, self.times, self.strand, skip, into=into)


def calls_at(length, marks):
    """a read of `length` '.' with the given letters at the given read positions"""
    s = bytearray(b"." * length)
    for i, ch in marks.items():
        s[i] = ord(ch)
    return bytes(s)


def minus_pos(g, chrom, f_hi, a):
    """the strand-genome position of a '-' record whose read position a lies on forward position f_hi"""
    lo, hi = int(g.start_index[chrom]), int(g.start_index[chrom + 1])
    return lo + hi - 1 - f_hi - a


def edge_cases(g, where):
    """the contract's corner cases -> (Hand, the number of couples its first n_exact reads add, n_exact); the reads behind
    them run through random sequence"""
    h, couples = Hand(), 0
    st = where["stretch"]
    # couples at read positions (14, 16), (15, 17), (126, 128), (127, 129): two neighbouring pairs of the stretch, on both strands
    for a in (14, 15, 126, 127):
        h.add(st + 20 - a, "+", calls_at(a + 9, {a: "Z", a + 2: "z"}))
        h.add(minus_pos(g, 0, st + 22, a), "-", calls_at(a + 9, {a: "Z", a + 2: "z"}))
        couples += 2
    # (0, L - 1) for every length: the ruler whose C's lie L - 1 apart; L = 1: one call, no couple.  Each behind a read
    # of 0 .. 15 calls, so that the reads sit at all 16 residues of the calls array's address.
    for k, L in enumerate(LENGTHS):
        for lead in range(16):
            h.add(5000, "+", calls_at(lead, {}))
            if L == 1:
                h.add(st, "+", b"z")
            else:
                h.add(where[L - 1], "+", calls_at(L, {0: "zZ"[(k + lead) % 2], L - 1: "Zz"[lead % 2]}))
                couples += 1
    # calls landing on the G of a pair: a '+' record calling G's, a '-' record calling both C's (forward G's of its own strand)
    h.add(st + 1, "+", calls_at(40, {0: "z", 2: "Z"}))
    h.add(st, "+", calls_at(40, {0: "z", 3: "Z"}))  # the C of one pair, the G of the next
    h.add(minus_pos(g, 0, st + 9, 0), "-", calls_at(30, {0: "Z", 2: "z", 4: "z"}))
    couples += 4
    # eight pairs per slice: the whole stretch called, 31 couples of 32 pairs; and z on both the C and the G of one pair:
    # the two calls of one pair are no couple, the pairs around them still are
    h.add(st, "+", ("Zz" * 16 + ".." * 16).replace("Z", "Z.").replace("z", "z.")[:64])
    couples += 31
    h.add(st, "+", calls_at(64, {0: "z", 1: "Z", 2: "z"}))
    couples += 1
    # two CpGs 1,022 apart in a 1,024-base read (the last call sits on read position 1022; 1023 is the G)
    h.add(where[1022], "+", calls_at(1024, {0: "Z", 1022: "Z", 1023: "h"}))
    couples += 1
    # a '.' on a reference CpG between two called ones adds nothing; z on a non-CpG position is ignored
    h.add(st, "+", calls_at(64, {0: "z", 4: "z"}))
    h.add(where[14], "+", calls_at(30, {0: "z", 5: "z", 7: "Z", 14: "z"}))
    couples += 1
    # times 0 and 2 add nothing
    h.add(st, "+", calls_at(64, {0: "z", 2: "z"}), times=0)
    h.add(st, "+", calls_at(64, {0: "z", 2: "z"}), times=2)
    n_exact = len(h.pos)
    # z at or beyond the chromosome end is ignored: a read that runs over the end of chromosome 0 into chromosome 1
    end0 = int(g.start_index[1])
    h.add(end0 - 10, "+", b"z" * 40)
    # the chromosome-boundary C|G: calls on the C that ends chromosome 1 and on the G that starts chromosome 2
    end1 = int(g.start_index[2])
    h.add(end1 - 1, "+", b"Z")
    h.add(end1, "+", b"Zz")
    # the pair that ends the genome, called together with its left neighbour if it has one within the read
    h.add(g.genome_len - 600, "+", b"z" * 600)
    return h, couples, n_exact


def random_reads(g, rng, n, dense):
    """records anywhere in the genome (also across chromosome ends), both strands, calls of every letter"""
    h = Hand()
    al = "zZ" * 4 + "xXhHuU." if dense else "zZ" + "." * 12 + "xhHU#A"
    for _ in range(n):
        L = rng.choice(LENGTHS + (40, 100, 150, 300))
        pos = rng.randrange(0, g.genome_len)
        h.add(pos, rng.choice("+-"), "".join(rng.choice(al) for _ in range(L)), rng.choice([0, 1, 1, 1, 1, 2]))
    return h


# ---------------------------------------------------------------------------
# 1. hand-made adds and the extraction
# ---------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def small(wa, scratch):
    g, where = pair_genome()
    db, path, idx = build_index(g, scratch, "cpgpairs_small")
    try:
        yield {"g": g, "where": where, "idx": idx, "pairs": find_pairs(g.text, g.start_index)}
    finally:
        idx.close()
        remove_index(path)


def test_n_pairs_and_the_chromosome_boundary(wa, small):
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    assert 19000 < g.genome_len < 24000 and 0.8 < len(pairs) * 16 / g.genome_len < 1.25
    end1 = int(g.start_index[2])
    assert g.text[end1 - 1:end1 + 1] == "CG" and end1 - 1 not in pairs and pairs[-1] == g.genome_len - 2
    ap = idx.cpg_pairs()
    pile = idx.pileup()
    assert ap.n_pairs == len(pairs) == int(pile.levels()["row"][4]["sites"])
    assert ap.device_bytes >= 16 * len(pairs) + g.genome_len // 8 and ap.extract().size == 0
    pile.close()
    ap.close()


def test_hand_made_calls_host_form(wa, small):
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    h, couples, n_exact = edge_cases(g, small["where"])
    exact = h.head(n_exact).want(g)
    assert int(exact.sum()) == couples and (exact.sum(axis=0) > 0).all()  # every column is reached
    want = h.want(g)
    assert int(want.sum()) > couples + 20
    ap = idx.cpg_pairs()
    calls, offsets, rec = h.arrays()
    assert {int(o) % 16 for o in offsets[:-1]} == set(range(16))
    ap.add(calls, offsets, rec)
    assert sites_list(ap.extract()) == sites_of(want, pairs)
    # the rulers: next - pos is the distance, up to 1023
    assert {s[1] - s[0] for s in sites_of(want, pairs)} >= {2, 14, 15, 16, 30, 126, 127, 128, 1022, 1023}
    # random reads, sparse and dense, on top; offsets that do not start at 0; skip bytes at stride 2; records at stride 64
    rng = random.Random(5)
    for dense in (False, True):
        hr = random_reads(g, rng, 700, dense)
        calls, offsets, rec = hr.arrays(64)
        assert rec.strides[0] == 64
        skip = np.full((len(hr.pos), 2), 9, dtype=np.uint8)
        skip[:, 1] = [rng.choice([0, 0, 0, 1, 200]) for _ in hr.pos]
        before = int(want.sum())
        want = hr.want(g, skip[:, 1], into=want)
        assert int(want.sum()) > before + 50
        ap.add(calls, offsets + np.uint64(12345), rec, skip=skip[:, 1])
        assert sites_list(ap.extract()) == sites_of(want, pairs), dense
    # skip bytes at stride 1
    hs = random_reads(g, rng, 300, True)
    calls, offsets, rec = hs.arrays()
    skip1 = np.array([rng.choice([0, 1]) for _ in hs.pos], dtype=np.uint8)
    want = hs.want(g, skip1, into=want)
    ap.add(calls, offsets, rec, skip=skip1)
    got = ap.extract()
    assert sites_list(got) == sites_of(want, pairs) and all(0 < int(s["next"]) - int(s["pos"]) < 1024 for s in got)
    # n = 0; the host form rejects a read of 1025 calls and adds nothing of that batch; refusals name their cause
    ap.add(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), Hand().arrays()[2])
    with pytest.raises(wa.WaltError) as ei:
        two = Hand().add(small["where"]["stretch"], "+", b"z." * 20).add(small["where"]["stretch"], "+", b"z." * 512 + b"z")
        ap.add(*two.arrays())
    assert ei.value.code == wa.WALT_EINVAL and "1024" in str(ei.value)
    L = wa.lib()
    one, off, rec = Hand().add(small["where"]["stretch"], "+", b"z.z.").arrays()
    for args, word in (((ap.handle, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 12, None, 1), "stride 12"),
                       ((ap.handle, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, one.ctypes.data, 0), "skip stride 0"),
                       ((ap.handle, one.ctypes.data, None, 1, rec.ctypes.data, 16, None, 1), "null"),
                       ((None, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, None, 1), "null pair table")):
        assert L.walt_cpgpairs_batch(*args) == wa.WALT_EINVAL and word in L.walt_last_error().decode(), word
    assert sites_list(ap.extract()) == sites_of(want, pairs)
    ap.clear()
    assert ap.extract().size == 0 and ap.n_pairs == len(pairs)
    ap.close()


def to_device(torch, dev, calls, offsets, rec, shift=0):
    """calls at a device address that is `shift` modulo 16, with 'z' around it (a slice that reads outside the reads shows)"""
    d_raw = torch.full((calls.size + 96,), ord("z"), dtype=torch.uint8, device=dev)
    a = (-d_raw.data_ptr()) % 16 + shift
    d_raw[a:a + calls.size] = torch.from_numpy(np.ascontiguousarray(calls)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(dev)
    stride = rec.strides[0] if rec.size > 1 else rec.dtype.itemsize
    flat = np.zeros(max(rec.size, 1) * stride + 64, dtype=np.uint8)
    for i in range(rec.size):
        flat[i * stride:i * stride + 16] = np.frombuffer(rec[i].tobytes(), dtype=np.uint8)
    d_rec = torch.from_numpy(flat).to(dev)
    return d_raw, d_raw.data_ptr() + a, d_off, d_rec, stride


def test_device_form_alignments_strides_and_a_read_of_1025(wa, small):
    import torch
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    st = small["where"]["stretch"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ap = idx.cpg_pairs()
    h = edge_cases(g, small["where"])[0]
    # a read of more than 1,024 calls between counted reads adds nothing, its neighbours everything
    h.add(st, "+", b"z." * 20).add(st, "+", b"z." * 512 + b"z").add(st + 2, "+", b"Z." * 20)
    rng = random.Random(6)
    hr = random_reads(g, rng, 400, True)
    for k in range(len(hr.pos)):
        h.add(hr.pos[k], hr.strand[k], hr.calls[k], hr.times[k])
    want = h.want(g)
    assert int(want.sum()) > 500
    for shift in (0, 1, 7, 15):
        for stride in (16, 64):
            calls, offsets, rec = h.arrays(stride)
            keep, d_calls, d_off, d_rec, s = to_device(torch, dev, calls, offsets, rec, shift)
            assert s == stride
            torch.cuda.synchronize()
            ap.clear()
            ap.add_device(d_calls, d_off.data_ptr(), len(h.pos), d_rec.data_ptr(), stride, stream=stream.cuda_stream)
            stream.synchronize()
            assert sites_list(ap.extract()) == sites_of(want, pairs), (shift, stride)
    # skip bytes at stride 2 on the device, the null stream
    skip = np.full((len(h.pos), 2), 1, dtype=np.uint8)
    skip[:, 0] = [rng.choice([0, 0, 3]) for _ in h.pos]
    d_skip = torch.from_numpy(skip).to(dev)
    torch.cuda.synchronize()
    ap.clear()
    ap.add_device(d_calls, d_off.data_ptr(), len(h.pos), d_rec.data_ptr(), 64, d_skip.data_ptr(), 2)
    assert sites_list(ap.extract()) == sites_of(h.want(g, skip[:, 0]), pairs)
    # n = 0 with null arrays is fine; refusals
    ap.add_device(None, None, 0, None)
    for args, kw, word in (((d_calls, d_off.data_ptr(), 1, d_rec.data_ptr()), dict(record_stride=8), "stride 8"),
                           ((d_calls, d_off.data_ptr(), 1, d_rec.data_ptr()), dict(skip_stride=0, d_skip=d_skip.data_ptr()), "skip stride 0"),
                           ((d_calls, d_off.data_ptr() + 4, 1, d_rec.data_ptr()), {}, "aligned"),
                           ((d_calls, d_off.data_ptr(), 1, d_rec.data_ptr() + 2), {}, "aligned"),
                           ((None, d_off.data_ptr(), 1, d_rec.data_ptr()), {}, "null"), ((d_calls, d_off.data_ptr(), 1, None), {}, "null")):
        with pytest.raises(wa.WaltError) as ei:
            ap.add_device(*args, **kw)
        assert ei.value.code == wa.WALT_EINVAL and word in str(ei.value), word
    ap.close()


def test_50000_copies_and_the_reverse_complement_record(wa, small):
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    p = small["where"][30]
    j = pairs.index(p)
    ap = idx.cpg_pairs()
    n = 50000
    read = calls_at(40, {3: "z", 33: "Z"})  # pair j unmethylated, pair j + 1 methylated: UM
    h = Hand()
    h.pos, h.strand, h.times, h.calls = [p - 3] * n, ["+"] * n, [1] * n, [read] * n
    ap.add(*h.arrays())
    assert sites_list(ap.extract()) == [(p, pairs[j + 1], 0, 0, n, 0)]
    # the reverse-complement record of the same molecule: the calls in reverse order, on the G's; the same entry and column
    lo, hi = int(g.start_index[0]), int(g.start_index[1])
    f_last = p - 3 + 39  # forward position of the '+' read's last base
    rc = Hand().add(lo + hi - 1 - f_last, "-", calls_at(40, {39 - 34: "Z", 39 - 4: "z"}))
    assert sites_of(rc.want(g), pairs) == [(p, pairs[j + 1], 0, 0, 1, 0)]
    ap.add(*rc.arrays())
    assert sites_list(ap.extract()) == [(p, pairs[j + 1], 0, 0, n + 1, 0)]
    ap.close()


@pytest.fixture(scope="module")
def filled(wa, small):
    g, idx = small["g"], small["idx"]
    ap = idx.cpg_pairs()
    h = random_reads(g, random.Random(7), 1500, True)
    ap.add(*h.arrays())
    want = sites_of(h.want(g), small["pairs"])
    assert len(want) > 300
    yield ap, want
    ap.close()


def test_extraction_ranges_and_capacity(wa, small, filled):
    import torch
    g, pairs = small["g"], small["pairs"]
    ap, want = filled
    assert sites_list(ap.extract()) == want
    pos, nxt = want[len(want) // 2][:2]
    # a range that cuts between pos and next keeps the entry on the side of pos
    assert sites_list(ap.extract(0, pos + 1)) == [s for s in want if s[0] <= pos]
    assert sites_list(ap.extract(pos + 1, g.genome_len)) == [s for s in want if s[0] > pos]
    assert sites_list(ap.extract(pos, nxt)) == [s for s in want if pos <= s[0] < nxt] and pos < nxt
    for lo, hi in ((0, 0), (pos, pos), (g.genome_len, g.genome_len), (pos + 1, pos + 2)):  # empty, or no pair inside
        assert ap.extract(lo, hi).size == 0
    rng = random.Random(8)
    for _ in range(40):
        lo = rng.randrange(0, g.genome_len)
        hi = rng.randrange(lo, g.genome_len + 1)
        assert sites_list(ap.extract(lo, hi)) == [s for s in want if lo <= s[0] < hi], (lo, hi)
    # range errors
    for lo, hi in ((5, 4), (0, g.genome_len + 1)):
        with pytest.raises(wa.WaltError) as ei:
            ap.extract(lo, hi)
        assert ei.value.code == wa.WALT_EINVAL and "range" in str(ei.value)
    # cap too small, host form: WALT_EINVAL, *n_out set, nothing written
    import ctypes
    L = wa.lib()
    buf = np.full(len(want), 0x55, dtype=np.uint8).repeat(24).view(wa.cpgpair_site_dtype)
    n = ctypes.c_uint64(0)
    assert L.walt_cpgpairs_extract(ap.handle, 0, g.genome_len, buf.ctypes.data, len(want) - 1, ctypes.byref(n)) == wa.WALT_EINVAL
    assert n.value == len(want) and "room for" in L.walt_last_error().decode() and (buf.view(np.uint8) == 0x55).all()
    assert L.walt_cpgpairs_extract(ap.handle, 0, g.genome_len, buf.ctypes.data, len(want), ctypes.byref(n)) == 0
    assert sites_list(buf) == want
    # device form on a side stream: exact cap, then cap too small: *d_n_out > cap and nothing written
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for cap in (len(want), len(want) - 1, 0):
        d_out = torch.full((len(want) * 24 + 8,), 0x55, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ap.extract_device(0, g.genome_len, d_out.data_ptr() if cap else None, cap, d_n.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert int(d_n.item()) == len(want)
        got = d_out.cpu().numpy()
        if cap == len(want):
            assert sites_list(got[:len(want) * 24].view(wa.cpgpair_site_dtype)) == want and (got[len(want) * 24:] == 0x55).all()
        else:
            assert (got == 0x55).all()


@pytest.mark.parametrize("blocks", [1, 2, 7, 300, 65536])
def test_extraction_does_not_depend_on_the_launch_shape(small, filled, index_options, blocks):
    ap, want = filled
    g = small["g"]
    plain = ap.extract().tobytes()
    part = ap.extract(1234, g.genome_len - 777).tobytes()
    index_options(small["idx"], pile_extract_blocks=blocks)
    assert ap.extract().tobytes() == plain and ap.extract(1234, g.genome_len - 777).tobytes() == part
    assert sites_list(ap.extract()) == want


def test_two_streams_feed_one_table(wa, small):
    import torch
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    dev = torch.device("cuda", 0)
    ap = idx.cpg_pairs()
    rng = random.Random(9)
    batches = [random_reads(g, rng, 400 + 37 * k, True) for k in range(2)]
    want = batches[1].want(g, into=batches[0].want(g))
    staged = [to_device(torch, dev, *b.arrays(), shift=5 * k) for k, b in enumerate(batches)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    reps = 5
    for _ in range(reps):
        for k in range(2):
            _, d_calls, d_off, d_rec, _ = staged[k]
            ap.add_device(d_calls, d_off.data_ptr(), len(batches[k].pos), d_rec.data_ptr(), stream=streams[k].cuda_stream)
    for s in streams:
        s.synchronize()
    assert sites_list(ap.extract()) == sites_of(want * np.uint64(reps), pairs)
    ap.close()


# ---------------------------------------------------------------------------
# 2. the composition with the calling
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "cpgpairs_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    db = refio.DbIndex(path)
    names, fasta = read_fasta(os.path.join(refio.GOLDEN, "g1.fa"))
    # The pairs are those of the reference the index holds: g1.fa with its N's filled as makedb fills them (R alone decides
    # what a pair is, and a fill can make or break one).  Everywhere else the text is the file's.
    from test_gpu_meth import reference_bases
    text = reference_bases(db)[0].tobytes().decode()
    starts = [int(v) for v in db.start_index]
    seqs = [text[starts[k]:starts[k + 1]] for k in range(len(starts) - 1)]
    assert names == list(db.names) and [len(s) for s in seqs] == [len(s) for s in fasta]
    assert all(a == b or b not in "ACGT" for sa, sb in zip(seqs, fasta) for a, b in zip(sa, sb))
    return db, path, names, seqs


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


def g1_want(g1, calls, offsets, rec, skip=None):
    db, _, names, seqs = g1
    text = "".join(seqs)
    assert len(text) == int(db.start_index[-1])
    table = expected_table(text, db.start_index, calls, offsets, rec["genome_pos"], rec["times"], [bytes(s) for s in rec["strand"]], skip)
    return sites_of(table, find_pairs(text, db.start_index))


def test_fused_call_host_form(wa, g1, g1_all, g1_pairs):
    (b1, o1, b2, o2), res, excl = g1_pairs
    n = res.size
    rng = np.random.default_rng(8)
    skip = (rng.integers(0, 4, size=n) == 0).astype(np.uint8)
    call_len = rng.integers(20, 101, size=n).astype(np.uint32)
    ap, ap2 = g1_all.cpg_pairs(), g1_all.cpg_pairs()
    # Pileup.add_batch(..., pairs=ap) equals CpgPairs.add on the calls it returns; both mates into one table
    pile, plain_pile = g1_all.pileup(), g1_all.pileup()
    for bases, offs, mate, cv in ((b1, o1, "m1", "T"), (b2, o2, "m2", "A")):
        got = pile.add_batch(bases, offs, res[mate], cv, pairs=ap)
        plain = plain_pile.add_batch(bases, offs, res[mate], cv)
        for x, y in zip(got, plain):  # with pairs=None: calls, counts, stats byte-identical
            assert x.tobytes() == y.tobytes()
        ap2.add(got[0], offs, res[mate])
    assert pile.extract()[0].tobytes() == plain_pile.extract()[0].tobytes()
    pile.close()
    plain_pile.close()
    both = ap.extract()
    assert both.tobytes() == ap2.extract().tobytes() and both.size > 300 and int(both["n"].sum()) > 1000
    # with call_len, excl, trim5 / trim3 and skip: the table is the restatement's on those calls
    for kw in (dict(call_len=call_len), dict(excl=excl), dict(trim5=7, trim3=5), dict(skip=skip),
               dict(call_len=call_len, excl=excl, trim5=3, trim3=9, skip=skip)):
        ap.clear()
        calls, _, _ = g1_all.meth_call_batch(b2, o2, res["m2"], "A", pairs=ap, **kw)
        want = g1_want(g1, calls, o2, res["m2"], kw.get("skip"))
        assert sites_list(ap.extract()) == want and len(want) > 100, sorted(kw)
        plain = g1_all.meth_call_batch(b2, o2, res["m2"], "A", **kw)
        assert plain[0].tobytes() == calls.tobytes()
    # the caller's calls NULL: the host form counts from its device copy
    ap.clear()
    none = g1_all.meth_call_batch(b1, o1, res["m1"], "T", want_calls=False, want_counts=False, want_stats=False, pairs=ap)
    assert none == (None, None, None)
    full = g1_all.meth_call_batch(b1, o1, res["m1"], "T")
    assert sites_list(ap.extract()) == g1_want(g1, full[0], o1, res["m1"])
    ap.close()
    ap2.close()


def test_fused_call_device_form_and_refusals(wa, g1, g1_all, g1_pairs, small):
    import torch
    (b1, o1, b2, o2), res, excl = g1_pairs
    n = res.size
    dev = torch.device("cuda", 0)
    d_bases = torch.from_numpy(b2).to(dev)
    d_offs = torch.from_numpy(o2.view(np.int64)).to(dev)
    d_pairs = torch.from_numpy(res.view(np.uint8).reshape(n, 64)).to(dev)
    d_excl = torch.from_numpy(excl.view(np.int32)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    ap = g1_all.cpg_pairs()
    total = int(o2[-1])
    outs = []
    for with_ap in (False, True):
        d_calls = torch.full((total + 48,), 0x23, dtype=torch.uint8, device=dev)
        d_counts = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
        pile = g1_all.pileup()
        torch.cuda.synchronize()
        pile.add_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_pairs.data_ptr() + 16, 64, None, 1, "A", None,
                              d_calls.data_ptr() + 3, d_counts.data_ptr(), d_stats.data_ptr(), stream=stream.cuda_stream,
                              d_excl=d_excl.data_ptr(), trim5=2, trim3=4, pairs=ap if with_ap else None)
        stream.synchronize()
        outs.append((d_calls.cpu().numpy(), d_counts.cpu().numpy(), d_stats.cpu().numpy(), pile.extract()[0].tobytes()))
        pile.close()
    for x, y in zip(outs[0], outs[1]):
        assert (x == y) if isinstance(x, bytes) else np.array_equal(x, y)
    calls = outs[1][0][3:3 + total]
    want = g1_want(g1, calls, o2, res["m2"])
    assert sites_list(ap.extract()) == want and len(want) > 100
    # d_calls NULL with a table: refused, and the message says why; a table of another index
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_call_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_pairs.data_ptr() + 16, 64, None, 1, "A", None,
                                      None, None, None, pairs=ap)
    assert ei.value.code == wa.WALT_EINVAL and "d_calls" in str(ei.value) and "counted from the calls" in str(ei.value)
    other = small["idx"].cpg_pairs()
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_call_batch(b2, o2, res["m2"], "A", pairs=other)
    assert ei.value.code == wa.WALT_EINVAL and "another index" in str(ei.value)
    other.close()
    assert sites_list(ap.extract()) == want
    ap.close()
    # an index without the reference has no table
    bare = wa.Index.open(g1[1], device=0, strands=wa.STRANDS_CT)
    with pytest.raises(wa.WaltError) as ei:
        bare.cpg_pairs()
    assert ei.value.code == wa.WALT_EINVAL and "reference" in str(ei.value)
    bare.close()


# ---------------------------------------------------------------------------
# 3. command line
# ---------------------------------------------------------------------------
def run_walt(args, binary=WALT_BIN, timeout=600):
    pr = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert pr.returncode == 0, pr.stdout[-2000:]
    return pr.stdout


def other_files(out):
    d, b = os.path.dirname(out), os.path.basename(out)
    return sorted(f[len(b):] for f in os.listdir(d) if f.startswith(b) and f[len(b):][:1] not in ("", "-") and f != b + ".allelic")


def check_run_against_its_sam(g1, out, min_rows=100):
    _, _, names, seqs = g1
    table, pairs, starts = table_from_sam(open(out).read(), names, seqs)
    want = allelic_rows(table, pairs, names, starts)
    got = parse_allelic(open(out + ".allelic").read())
    same_allelic(got, want)
    assert len(got) >= min_rows
    return got


MODES = {"r": ["-r", "se_ct.fastq"], "A": ["-r", "se_ga.fastq", "-A"], "pe": ["-1", "pe_1.fastq", "-2", "pe_2.fastq"],
         "P": ["-1", "pe_2.fastq", "-2", "pe_1.fastq", "-P"], "RP": ["-1", "pe_1.fastq", "-2", "pe_2.fastq", "-RP"]}


def mode_args(scratch, mode):
    if mode == "R":
        from test_gpu_rpbat import mixed_library
        fq = os.path.join(scratch, "cpgpairs_mixed.fastq")
        with open(fq, "w") as f:
            for nm, s, q in zip(*mixed_library()):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
        return ["-r", fq, "-R"]
    return [os.path.join(refio.GOLDEN, a) if a.endswith(".fastq") else a for a in MODES[mode]]


@pytest.mark.parametrize("mode", ["r", "A", "pe", "P", "R", "RP"])
def test_cli_every_mode_against_its_own_sam(wa, g1, scratch, mode):
    path = g1[1]
    out = os.path.join(scratch, "cpgpairs_cli_" + mode)
    base = ["-i", path] + mode_args(scratch, mode) + ["-a", "-u"]
    spelling = {"r": "-MA", "A": "-allelic", "pe": "--allelic-meth"}.get(mode, "-MA")
    log = run_walt(base + ["-o", out, spelling, "-M", "-sam", "-v"])
    got = check_run_against_its_sam(g1, out)
    assert "[walt_amd allelic: %d entries, %d couples" % (len(got), sum(r[4] for r in got)) in log
    # .allelic is absent without -MA, and every other output of the run with it is byte-identical
    run_walt(base + ["-o", out + "-plain", "-M", "-sam"])
    assert not os.path.exists(out + "-plain.allelic")
    assert other_files(out) == other_files(out + "-plain") and ".methstats" in other_files(out)
    for sfx in [""] + other_files(out):
        assert open(out + sfx, "rb").read() == open(out + "-plain" + sfx, "rb").read(), sfx
    # -MA alone is a consumer: the same table, no .methstats
    run_walt(base + ["-o", out + "-alone", "-MA"])
    assert open(out + "-alone.allelic", "rb").read() == open(out + ".allelic", "rb").read()
    assert not os.path.exists(out + "-alone.methstats")
    if mode == "r":
        # two shares of the batch on two tables (the same device twice), and small batches: the same file
        run_walt(base + ["-o", out + "-g00", "-MA", "-g", "0,0", "-N", "1000"])
        assert open(out + "-g00.allelic", "rb").read() == open(out + ".allelic", "rb").read()
        # two read files that share an output name: one table after another
        fq = mode_args(scratch, mode)[1]
        run_walt(["-i", path, "-r", fq + "," + fq, "-o", out + "-two," + out + "-two", "-MA"])
        assert open(out + "-two.allelic").read() == 2 * open(out + ".allelic").read()


@pytest.mark.parametrize("case", ["D", "NO", "C_I3", "F", "MC_MB_ML"])
def test_cli_options_act_through_the_calls(wa, g1, scratch, case):
    from test_gpu_dedup import doubled
    path = g1[1]
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    extra = {"D": ["-D"], "NO": ["-NO"], "F": ["-F", "2"], "MC_MB_ML": ["-MC", "-MB", "-ML"]}.get(case)
    if case == "D":
        (_, f1), (_, f2) = doubled(scratch, "cpgpairs_D", [f1, f2])
    if case == "C_I3":
        args = refio.golden_meta()["cases"]["pe_clip_sam_au"]["args"]
        extra = ["-C", args[args.index("-C") + 1], "-I3", "3"]
        f1, f2 = os.path.join(refio.GOLDEN, "pe_clip_1.fastq"), os.path.join(refio.GOLDEN, "pe_clip_2.fastq")
    out = os.path.join(scratch, "cpgpairs_opt_" + case)
    base = ["-i", path, "-1", f1, "-2", f2, "-a", "-u", "-M", "-sam"]
    run_walt(base + ["-o", out, "-MA"] + extra)
    got = check_run_against_its_sam(g1, out)
    if case in ("D", "NO", "F"):  # the option takes couples away
        run_walt(base + ["-o", out + "-without", "-MA"])
        without = check_run_against_its_sam(g1, out + "-without")
        assert sum(r[4] for r in got) < sum(r[4] for r in without)
    if case == "MC_MB_ML":
        run_walt(base + ["-o", out + "-plain"] + extra)
        for sfx in [""] + other_files(out):
            assert open(out + sfx, "rb").read() == open(out + "-plain" + sfx, "rb").read(), sfx
        assert {".methcounts", ".mbias", ".levels"} <= set(other_files(out))


@pytest.mark.parametrize("pattern", [5, 7])
def test_cli_seed_patterns_5_and_7(wa, g1, scratch, pattern):
    binary = os.path.join(refio.ROOT, "walt_amd", "bin", "walt_sp%d" % pattern)
    path = os.path.join(scratch, "cpgpairs_g1_sp%d.dbindex" % pattern)
    old = wa.PATTERN
    wa.set_pattern(pattern)
    try:
        wa.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    finally:
        wa.set_pattern(old)
    out = os.path.join(scratch, "cpgpairs_cli_sp%d" % pattern)
    run_walt(["-i", path, "-r", os.path.join(refio.GOLDEN, "sp_se_ct.fastq"), "-o", out, "-MA", "-M", "-sam"], binary=binary)
    check_run_against_its_sam(g1, out, min_rows=50)
