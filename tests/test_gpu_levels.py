"""Genome-wide methylation levels of a pile-up (walt_pileup_levels, walt_pileup_read / _add, bin/walt -ML; the contract
is in include/walt_amd.h, "methylation levels").

The expected values come from the restatement below, which walks every position of the genome in Python: the class of
a position is `site_class` of tests/test_gpu_pileup.py, a CpG pair is a C followed by a G of the same chromosome, and
the two statistics of a covered site are Python's own integer divisions.  Counters are set by hand through Pileup.add,
so the summary is checked on values no mapped library reaches (0xFFFFFFFF on both halves of a pair)."""
import os
import random

import numpy as np
import pytest

import refio
from test_gpu_meth import load, reference_bases, run_walt
from test_gpu_meth_contigs import Genome, build_index, remove_index
from test_gpu_pileup import chrom_of, expected_counts, site_class

pytestmark = pytest.mark.gpu

ROW_NAMES = ("CpG", "CHG", "CHH", "unknown", "CpG_symmetric")
FIELDS = ("sites", "covered", "meth", "unmeth", "max_depth", "level_sum")
HEADER = ("context\tsites\tcovered\tmeth\tunmeth\tmax_depth\tmean_depth\tcovered_fraction\tmean_meth\tweighted_meth"
          "\th0\th1\th2\th3\th4\th5\th6\th7\th8\th9\n")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def level_q30(m, u):
    return (m << 30) // (m + u)


def level_bin(m, u):
    return min(9, 10 * m // (m + u))


def classes(R0, start_index):
    """per forward position: the row 0..3 of a site (None where R[f] is A or T), and whether f starts a CpG pair"""
    cls, pair = [], []
    for f in range(len(R0)):
        c = site_class(R0, start_index, f)
        cls.append(None if c is None else c[1])
        _, _, hi = chrom_of(start_index, f)
        pair.append(chr(R0[f]) == "C" and f + 1 < hi and chr(R0[f + 1]) == "G")
    return cls, pair


def empty_levels():
    return {"row": [dict([(k, 0) for k in FIELDS] + [("hist", [0] * 10)]) for _ in range(5)], "offref": [0, 0]}


def take(row, m, u):
    row["sites"] += 1
    if m + u == 0:
        return
    row["covered"] += 1
    row["meth"] += m
    row["unmeth"] += u
    row["max_depth"] = max(row["max_depth"], m + u)
    row["level_sum"] += level_q30(m, u)
    row["hist"][level_bin(m, u)] += 1


def expected_levels(cls, pair, meth, unmeth, lo=0, hi=None):
    """the summary of [lo, hi): every position walked; a pair belongs to the range of its C and reads its G anywhere"""
    hi = len(cls) if hi is None else hi
    out = empty_levels()
    for f in range(lo, hi):
        m, u = int(meth[f]), int(unmeth[f])
        if cls[f] is None:
            out["offref"][0] += m
            out["offref"][1] += u
        else:
            take(out["row"][cls[f]], m, u)
        if pair[f]:
            take(out["row"][4], m + int(meth[f + 1]), u + int(unmeth[f + 1]))
    return out


def as_dict(rec):
    """a levels_dtype record -> the restatement's form (Python integers)"""
    return {"row": [dict([(k, int(rec["row"][r][k])) for k in FIELDS] + [("hist", [int(x) for x in rec["row"][r]["hist"]])])
                    for r in range(5)],
            "offref": [int(rec["offref"][0]), int(rec["offref"][1])]}


def fold(parts):
    """what a partition's summaries add up to: sums, and the maximum for max_depth"""
    out = empty_levels()
    for p in parts:
        for r in range(5):
            for k in FIELDS:
                out["row"][r][k] = max(out["row"][r][k], p["row"][r][k]) if k == "max_depth" else out["row"][r][k] + p["row"][r][k]
            out["row"][r]["hist"] = [a + b for a, b in zip(out["row"][r]["hist"], p["row"][r]["hist"])]
        out["offref"] = [a + b for a, b in zip(out["offref"], p["offref"])]
    return out


def levels_text(lv):
    """<out>.levels' block of one summary"""
    total = fold([{"row": [lv["row"][r]] + [empty_levels()["row"][0]] * 4, "offref": [0, 0]} for r in range(4)])["row"][0]

    def ratio(a, b):
        return "NA" if b == 0 else "%.6f" % (a / b)

    lines = [HEADER]
    for name, x in [("cytosines", total)] + list(zip(ROW_NAMES, lv["row"])):
        cols = [name] + [str(x[k]) for k in FIELDS[:5]]
        cols += [ratio(x["meth"] + x["unmeth"], x["sites"]), ratio(x["covered"], x["sites"]),
                 ratio(x["level_sum"], x["covered"] * 1073741824.0), ratio(x["meth"], x["meth"] + x["unmeth"])]
        lines.append("\t".join(cols + [str(h) for h in x["hist"]]) + "\n")
    return "".join(lines)


def extract_aggregate(sites, off):
    """rows 0..3 of a summary as far as the records of an extraction give them (no `sites`: uncovered ones are not listed)"""
    out = empty_levels()
    for s in sites:
        m, u = int(s["meth"]), int(s["unmeth"])
        take(out["row"][int(s["context"])], m, u)
    out["offref"] = [int(off[0]), int(off[1])]
    return out


def assert_same(got, want, what=""):
    for r in range(5):
        for k in FIELDS + ("hist",):
            assert got["row"][r][k] == want["row"][r][k], (what, ROW_NAMES[r], k, got["row"][r][k], want["row"][r][k])
    assert got["offref"] == want["offref"], (what, got["offref"], want["offref"])


# ---------------------------------------------------------------------------
# 1. hand-set counters on small genomes
# ---------------------------------------------------------------------------
def small_genome(n_chrom):
    """a few thousand bases, C / G rich; chromosomes of 1, 2, 255, 256 and 257 bases where there are several; a CG at
    positions 63/64 and 255/256 of the first chromosome (the last lane of a wavefront and of a 256-position step)"""
    rng = random.Random(900 + n_chrom)
    if n_chrom == 1:
        lengths = [3001]
    else:
        lengths = [700, 1, 2, 255, 256, 257] + [rng.randrange(20, 90) for _ in range(n_chrom - 7)] + [1]
    assert len(lengths) == n_chrom
    seqs = ["".join(rng.choice("ACGTCG") for _ in range(L)) for L in lengths]
    first = list(seqs[0])
    for at in (63, 255, 319, 511):
        first[at:at + 2] = "CG"
    seqs[0] = "".join(first)
    if n_chrom > 1:  # a C that ends a chromosome in front of a G that starts the next: no pair
        seqs[3] = seqs[3][:-1] + "C"
        seqs[4] = "G" + seqs[4][1:]
    return Genome(["c%d" % i for i in range(n_chrom)], seqs)


def hand_counters(glen, seed):
    """mostly small counts, many zeros, a few at the counters' limit -- on every position, A and T included"""
    rng = random.Random(seed)
    pick = [0, 0, 0, 1, 1, 2, 3, 5, 9, 10, 30, 100, 1000, 0xFFFFFFFF]
    return (np.array([rng.choice(pick) for _ in range(glen)], dtype=np.uint32),
            np.array([rng.choice(pick) for _ in range(glen)], dtype=np.uint32))


@pytest.fixture(scope="module", params=[1, 7, 40])
def small(request, scratch):
    n_chrom = request.param
    g = small_genome(n_chrom)
    db, path, idx = build_index(g, scratch, "levels_small_%d" % n_chrom)
    pile = idx.pileup()
    try:
        meth, unmeth = hand_counters(g.genome_len, n_chrom)
        pile.add(0, g.genome_len, meth, unmeth)
        cls, pair = classes(g.R[0], g.start_index)
        yield {"g": g, "idx": idx, "pile": pile, "meth": meth, "unmeth": unmeth, "cls": cls, "pair": pair,
               "whole": expected_levels(cls, pair, meth, unmeth)}
    finally:
        pile.close()
        idx.close()
        remove_index(path)


def pair_cuts(c):
    """a partition whose cuts fall at f and f + 1 of CpG pairs: those at lane 63 of a wavefront and at the end of a
    256-position step, and a sample of the others"""
    g, pair = c["g"], c["pair"]
    at = [f for f in range(g.genome_len) if pair[f]]
    edge = [f for f in at if f % 64 == 63]
    assert any(f % 256 == 255 for f in edge) and any(f % 256 == 63 for f in edge)
    some = random.Random(5).sample(at, min(24, len(at)))
    cuts = {0, g.genome_len}
    for f in edge + some:
        cuts.update((f, f + 1))
    return sorted(cuts)


@pytest.mark.parametrize("blocks", [0, 1, 7, 1000])
def test_hand_set_counters_whole_and_partition(small, index_options, blocks):
    c = small
    pile = c["pile"]
    index_options(c["idx"], pile_extract_blocks=blocks)
    whole = as_dict(pile.levels())
    assert_same(whole, c["whole"], "whole genome, %d blocks" % blocks)
    for r in (0, 1, 2, 4):  # every row has covered sites, and uncovered sites are counted
        assert whole["row"][r]["sites"] >= whole["row"][r]["covered"] > 0, r
    assert sum(whole["row"][r]["sites"] - whole["row"][r]["covered"] for r in range(4)) > 20
    assert whole["row"][3]["sites"] > 0 or c["g"].n_chrom == 1
    cuts = pair_cuts(c)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got = as_dict(pile.levels(lo, hi))
        assert_same(got, expected_levels(c["cls"], c["pair"], c["meth"], c["unmeth"], lo, hi), "[%d, %d), %d blocks" % (lo, hi, blocks))
        parts.append(got)
    assert_same(fold(parts), whole, "the partition's sum")
    assert as_dict(pile.levels(5, 5)) == empty_levels()


def test_cross_checks_with_the_extraction(small):
    c = small
    g, pile = c["g"], c["pile"]
    glen = g.genome_len
    for lo, hi in [(0, glen), (0, 1), (glen - 1, glen), (63, 257), (glen // 3, 2 * glen // 3)]:
        got = as_dict(pile.levels(lo, hi))
        want = extract_aggregate(*pile.extract(lo, hi))
        for r in range(4):
            for k in ("covered", "meth", "unmeth", "max_depth", "level_sum", "hist"):
                assert got["row"][r][k] == want["row"][r][k], (lo, hi, r, k)
        assert got["offref"] == want["offref"]
    # an N-free genome: every CpG pair is two CpG sites, every CpG site lies in one pair
    whole = as_dict(pile.levels())
    assert whole["row"][0]["sites"] == 2 * whole["row"][4]["sites"] > 0


def test_clear_leaves_the_sites_alone(small):
    c = small
    pile = c["idx"].pileup()
    try:
        pile.add(0, c["g"].genome_len, c["meth"], c["unmeth"])
        before = as_dict(pile.levels())
        assert_same(before, c["whole"])
        pile.clear()
        after = as_dict(pile.levels())
        want = empty_levels()
        for r in range(5):
            want["row"][r]["sites"] = before["row"][r]["sites"]
        assert after == want
    finally:
        pile.close()


def test_large_counters_on_both_halves_of_a_pair(small):
    c = small
    g = c["g"]
    pile = c["idx"].pileup()
    try:
        f = 255
        assert c["pair"][f]
        big = np.full(2, 0xFFFFFFFF, dtype=np.uint32)
        pile.add(f, f + 2, big, None)
        got = as_dict(pile.levels())["row"][4]
        assert got["covered"] == 1 and got["meth"] == 2 ** 33 - 2 and got["unmeth"] == 0 and got["max_depth"] == 2 ** 33 - 2
        assert got["level_sum"] == 1 << 30 and got["hist"] == [0] * 9 + [1]
        pile.add(f, f + 2, None, big)
        got = as_dict(pile.levels(f, f + 1))["row"][4]
        assert got["meth"] == got["unmeth"] == 2 ** 33 - 2 and got["max_depth"] == 2 ** 34 - 4
        assert got["level_sum"] == 1 << 29 and got["hist"] == [0] * 5 + [1] + [0] * 4
        # the counters wrap as they do under the calls: one more on each gives 0
        pile.add(f, f + 2, np.ones(2, dtype=np.uint32), np.ones(2, dtype=np.uint32))
        m, u = pile.read(f, f + 2)
        assert m.tolist() == [0, 0] and u.tolist() == [0, 0]
        pile.add(7, 7, None, None)  # an empty range, and nothing to add
        pile.add(0, g.genome_len, None, None)
        assert as_dict(pile.levels())["row"][4]["covered"] == 0
    finally:
        pile.close()


# ---------------------------------------------------------------------------
# 2. the golden genome: read / add, the device form, the golden libraries
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "levels_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    R = reference_bases(db)
    cls, pair = classes(R[0], db.start_index)
    _, seqs, _ = load("se_ct.fastq")
    bases, offs = walt_amd.pack_reads(seqs)
    recs, _ = idx.map_se_batch(bases, offs)
    fed = expected_counts(R, db.start_index, seqs, recs, "T")
    yield {"db": db, "path": path, "idx": idx, "R": R, "cls": cls, "pair": pair, "seqs": seqs, "bases": bases, "offs": offs,
           "recs": recs, "fed": fed}
    idx.close()


def test_read_and_add(g1):
    c = g1
    idx, glen = c["idx"], c["db"].genome_len
    first, second = idx.pileup(), idx.pileup()
    try:
        m0, u0 = hand_counters(glen, 77)
        first.add(0, glen, m0, u0)
        m, u = first.read()
        assert np.array_equal(m, m0) and np.array_equal(u, u0)
        _, _, stats = first.add_batch(c["bases"], c["offs"], c["recs"], "T")
        want_m = (m0.astype(np.int64) + c["fed"][0]) & 0xFFFFFFFF
        want_u = (u0.astype(np.int64) + c["fed"][1]) & 0xFFFFFFFF
        m, u = first.read()
        assert np.array_equal(m, want_m) and np.array_equal(u, want_u) and int(c["fed"][0].sum()) > 1000
        lo, hi = glen // 3, glen // 3 + 1001
        m, u = first.read(lo, hi)
        assert np.array_equal(m, want_m[lo:hi]) and np.array_equal(u, want_u[lo:hi])
        # a second pile-up's counters read and added into the first: the levels of the summed arrays
        m1, u1 = hand_counters(glen, 78)
        second.add(0, glen, m1, u1)
        cut = glen // 2 + 1
        first.add(0, cut, *second.read(0, cut))
        first.add(cut, glen, *second.read(cut, glen))
        sum_m, sum_u = (want_m + m1) & 0xFFFFFFFF, (want_u + u1) & 0xFFFFFFFF
        assert_same(as_dict(first.levels()), expected_levels(c["cls"], c["pair"], sum_m, sum_u), "two pile-ups folded")
    finally:
        first.close()
        second.close()


def test_device_form_on_a_side_stream(g1):
    import torch
    import walt_amd
    c = g1
    idx, glen, n = c["idx"], c["db"].genome_len, len(c["seqs"])
    host_pile, pile = idx.pileup(), idx.pileup()
    try:
        host_pile.add_batch(c["bases"], c["offs"], c["recs"], "T", want_calls=False, want_counts=False, want_stats=False)
        want = host_pile.levels()
        dev = torch.device("cuda", 0)
        d_bases = torch.from_numpy(c["bases"]).to(dev)
        d_offs = torch.from_numpy(c["offs"].view(np.int64)).to(dev)
        d_recs = torch.from_numpy(c["recs"].view(np.uint8).reshape(n, 16)).to(dev)
        d_out = torch.full((82,), -1, dtype=torch.int64, device=dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        pile.add_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_recs.data_ptr(), 16, None, 1, "T", stream=side.cuda_stream)
        pile.levels_device(0, glen, d_out.data_ptr(), stream=side.cuda_stream)
        side.synchronize()
        assert d_out.cpu().numpy().tobytes() == want.tobytes() and walt_amd.levels_dtype.itemsize == 656
        assert_same(as_dict(want), expected_levels(c["cls"], c["pair"], *c["fed"]), "se_ct")
        L = walt_amd.lib()
        assert L.walt_pileup_levels_device(pile.handle, 0, glen, d_out.data_ptr() + 4, None) == walt_amd.WALT_EINVAL
        assert b"aligned" in L.walt_last_error()
        assert L.walt_pileup_levels_device(pile.handle, 0, glen, None, None) == walt_amd.WALT_EINVAL
        out = np.zeros(1, dtype=walt_amd.levels_dtype)
        assert L.walt_pileup_levels(pile.handle, 5, 4, out.ctypes.data) == walt_amd.WALT_EINVAL
        assert L.walt_pileup_levels(pile.handle, 0, glen + 1, out.ctypes.data) == walt_amd.WALT_EINVAL and b"range" in L.walt_last_error()
        assert L.walt_pileup_levels(pile.handle, 0, glen, None) == walt_amd.WALT_EINVAL
        assert L.walt_pileup_read(pile.handle, 0, glen + 1, None, None) == walt_amd.WALT_EINVAL
        assert L.walt_pileup_add(pile.handle, 3, 2, None, None) == walt_amd.WALT_EINVAL
        assert pile.device_bytes == 8 * glen + (1 << 20)
    finally:
        pile.close()
        host_pile.close()


@pytest.mark.parametrize("library", ["single", "paired"])
def test_golden_libraries_sum_to_the_stats(g1, library):
    import walt_amd
    c = g1
    idx = c["idx"]
    pile = idx.pileup()
    try:
        if library == "single":
            _, _, stats = pile.add_batch(c["bases"], c["offs"], c["recs"], "T")
        else:
            _, s1, _ = load("pe_1.fastq")
            _, s2, _ = load("pe_2.fastq")
            b1, o1 = walt_amd.pack_reads(s1)
            b2, o2 = walt_amd.pack_reads(s2)
            res, _ = idx.map_pe_batch(b1, o1, b2, o2)
            _, _, stats = pile.add_batch(b1, o1, res["m1"], "T")
            _, _, stats = pile.add_batch(b2, o2, res["m2"], "A", stats=stats)  # the two mates summed
        got = as_dict(pile.levels())
        assert got["offref"] == [0, 0]
        for r in range(4):
            assert got["row"][r]["meth"] == int(stats["meth"][0][r]) and got["row"][r]["unmeth"] == int(stats["unmeth"][0][r]), (library, r)
        assert got["row"][0]["meth"] + got["row"][0]["unmeth"] > 1000
        # a pair's calls are its two sites' calls
        assert got["row"][4]["meth"] == got["row"][0]["meth"] and got["row"][4]["unmeth"] == got["row"][0]["unmeth"]
    finally:
        pile.close()


# ---------------------------------------------------------------------------
# 3. command line
# ---------------------------------------------------------------------------
def text_from_counts(c, counts_path):
    """<out>.levels' block as the restatement computes it from a run's <out>.methcounts and the reference"""
    db = c["db"]
    first = {nm: int(db.start_index[i]) for i, nm in enumerate(db.names)}
    meth, unmeth = np.zeros(db.genome_len, dtype=np.int64), np.zeros(db.genome_len, dtype=np.int64)
    for line in open(counts_path):
        nm, off, _, _, m, u = line.rstrip("\n").split("\t")
        meth[first[nm] + int(off)], unmeth[first[nm] + int(off)] = int(m), int(u)
    return levels_text(expected_levels(c["cls"], c["pair"], meth, unmeth))


def other_files(out):
    d, base = os.path.dirname(out), os.path.basename(out)
    return sorted(f[len(base):] for f in os.listdir(d) if f.startswith(base) and not f.endswith(".levels"))


@pytest.mark.parametrize("mode", ["r", "paired", "R"])
def test_cli_adds_one_file_and_changes_no_other(g1, scratch, mode):
    c = g1
    if mode == "r":
        reads, extra = ["-r", os.path.join(refio.GOLDEN, "se_ct.fastq")], []
    elif mode == "paired":
        reads, extra = ["-1", os.path.join(refio.GOLDEN, "pe_1.fastq"), "-2", os.path.join(refio.GOLDEN, "pe_2.fastq")], []
    else:
        from test_gpu_rpbat import mixed_library
        fq = os.path.join(scratch, "levels_mixed.fastq")
        with open(fq, "w") as f:
            for nm, s, q in zip(*mixed_library()):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
        reads, extra = ["-r", fq], ["-R"]
    texts = []
    for tag, more in (("plain", []), ("all", ["-MC", "-M", "-sam"])):
        base = os.path.join(scratch, "levels_cli_%s_%s.base" % (mode, tag))
        with_ml = os.path.join(scratch, "levels_cli_%s_%s.ml" % (mode, tag))
        common = ["-i", c["path"]] + reads + ["-a", "-u"] + extra + more
        run_walt(common + ["-o", base])
        run_walt(common + ["-o", with_ml, "-ML"])
        assert not os.path.exists(base + ".levels")
        files = other_files(base)
        assert files == other_files(with_ml) and "" in files and (".methcounts" in files) == bool(more)
        for sfx in files:
            assert open(base + sfx, "rb").read() == open(with_ml + sfx, "rb").read(), (mode, tag, sfx)
        text = open(with_ml + ".levels").read()
        assert text.startswith(HEADER) and text.count("\n") == 7
        if more:
            assert text == text_from_counts(c, with_ml + ".methcounts")
        texts.append(text)
    assert texts[0] == texts[1]  # -ML alone counts what -MC counts


def test_cli_devices_filters_and_read_files(g1, scratch):
    c = g1
    fq = os.path.join(refio.GOLDEN, "se_ct.fastq")
    out = os.path.join(scratch, "levels_cli_one.out")
    run_walt(["-i", c["path"], "-r", fq, "-o", out, "-ML", "-MC"])
    block = open(out + ".levels").read()
    assert block == text_from_counts(c, out + ".methcounts")
    # -g 0,0: two shares, two pile-ups, the second folded into the first
    two = os.path.join(scratch, "levels_cli_g00.out")
    log = run_walt(["-i", c["path"], "-r", fq, "-o", two, "-ML", "-g", "0,0", "-v"])
    assert open(two + ".levels").read() == block and not os.path.exists(two + ".methcounts")
    assert block in log  # -v prints the block
    # -D and -I5 5 change it exactly as they change <out>.methcounts
    # (the library written twice into one file, so that every read has a duplicate)
    twice = os.path.join(scratch, "levels_twice.fastq")
    with open(twice, "w") as f:
        f.write(open(fq).read() * 2)
    seen = {}
    for tag, reads, opt in (("twice", twice, []), ("D", twice, ["-D"]), ("I5", fq, ["-I5", "5"])):
        o2 = os.path.join(scratch, "levels_cli_%s.out" % tag)
        run_walt(["-i", c["path"], "-r", reads, "-o", o2, "-ML", "-MC"] + opt)
        seen[tag] = (open(o2 + ".methcounts").read(), open(o2 + ".levels").read())
        assert seen[tag][1] == text_from_counts(c, o2 + ".methcounts"), tag
    assert seen["D"][0] != seen["twice"][0] and seen["D"][1] != seen["twice"][1]
    assert seen["I5"][0] != open(out + ".methcounts").read() and seen["I5"][1] != block
    # two read files that share one output name: two blocks; the other spellings
    o3 = os.path.join(scratch, "levels_cli_two.out")
    run_walt(["-i", c["path"], "-r", fq + "," + fq, "-o", o3, "-levels"])
    assert open(o3 + ".levels").read() == block + block
    run_walt(["-i", c["path"], "-r", fq, "-o", o3, "--meth-levels"])
    assert open(o3 + ".levels").read() == block
