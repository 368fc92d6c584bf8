"""Methylation levels per region (walt_pileup_regions, walt_pileup_regions_device, bin/walt -MR; the contract is in
include/walt_amd.h, "methylation levels per region").

The contract is an equivalence: record i of a call equals the summary of [lo, hi) of region i in the fields it has.
So the expected values are those of tests/test_gpu_levels.py: `expected_levels`, the Python walk over every position,
per region; a sample is also compared with Pileup.levels(lo, hi) on the device.  Only the call of 70,000 regions is
checked against prefix sums of the same per-position values (the walk would take minutes), and those are compared
with the walk on a sample first.  Counters are set by hand through Pileup.add."""
import os
import random

import numpy as np
import pytest

import refio
from test_gpu_levels import (ROW_NAMES, classes, expected_levels, g1, hand_counters, level_q30, small_genome)  # noqa: F401 (g1: a fixture)
from test_gpu_meth import run_walt
from test_gpu_meth_contigs import Genome, build_index, remove_index

pytestmark = pytest.mark.gpu

U = 4096  # positions of a unit (walt_amd/csrc/regions_core.h kRegionUnit)
REGION_FIELDS = ("sites", "covered", "meth", "unmeth", "level_sum")
REGION_COLS = ("sites", "covered", "meth", "unmeth", "mean_meth", "weighted_meth")
REGIONS_HEADER = "\t".join(["chrom", "start", "end", "name"] + ["%s_%s" % (r, c) for r in ROW_NAMES for c in REGION_COLS]) + "\n"


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def want_record(cls, pair, meth, unmeth, lo, hi):
    """the record of [lo, hi): the fields a region's record has, out of the walk's summary"""
    lv = expected_levels(cls, pair, meth, unmeth, lo, hi)
    return [{k: lv["row"][r][k] for k in REGION_FIELDS} for r in range(5)]


def zero_record():
    return [{k: 0 for k in REGION_FIELDS} for _ in range(5)]


def rec_rows(rec):
    """a region_levels_dtype record -> the restatement's form (Python integers)"""
    return [{k: int(rec["row"][r][k]) for k in REGION_FIELDS} for r in range(5)]


def levels_rows(lv):
    """a levels_dtype record (Pileup.levels) -> the same form"""
    return [{k: int(lv["row"][r][k]) for k in REGION_FIELDS} for r in range(5)]


def fold_rows(parts):
    out = zero_record()
    for p in parts:
        for r in range(5):
            for k in REGION_FIELDS:
                out[r][k] += p[r][k]
    return out


def regions_text(bed, records):
    """<out>.regions' block: bed = [(chrom, start, end, name)], records in the restatement's form"""
    def ratio(a, b):
        return "NA" if b == 0 else "%.6f" % (a / b)

    lines = [REGIONS_HEADER]
    for (chrom, start, end, name), rows in zip(bed, records):
        cols = [chrom, str(start), str(end), name]
        for x in rows:
            cols += [str(x["sites"]), str(x["covered"]), str(x["meth"]), str(x["unmeth"]),
                     ratio(x["level_sum"], x["covered"] * 1073741824.0), ratio(x["meth"], x["meth"] + x["unmeth"])]
        lines.append("\t".join(cols) + "\n")
    return "".join(lines)


def prefix_sums(cls, pair, meth, unmeth):
    """per row and field, the sums over the positions in front of f (int64; the largest, a pair's calls over a few
    thousand positions, stays far below 2^63): a record is a difference of two entries"""
    n = len(cls)
    per = np.zeros((5, len(REGION_FIELDS), n + 1), dtype=np.int64)
    for f in range(n):
        hits = []
        if cls[f] is not None:
            hits.append((cls[f], int(meth[f]), int(unmeth[f])))
        if pair[f]:
            hits.append((4, int(meth[f]) + int(meth[f + 1]), int(unmeth[f]) + int(unmeth[f + 1])))
        for r, m, u in hits:
            per[r, 0, f + 1] = 1
            if m + u:
                per[r, 1, f + 1] = 1
                per[r, 2, f + 1], per[r, 3, f + 1], per[r, 4, f + 1] = m, u, level_q30(m, u)
    return np.cumsum(per, axis=2)


def records_by_prefix(sums, regions):
    lo, hi = np.asarray(regions)[:, 0], np.asarray(regions)[:, 1]
    return sums[:, :, hi] - sums[:, :, lo]  # [row, field, region]


def assert_records(got, regions, c, what=""):
    assert len(got) == len(regions)
    for i, (lo, hi) in enumerate(regions):
        assert rec_rows(got[i]) == want_record(c["cls"], c["pair"], c["meth"], c["unmeth"], lo, hi), (what, i, lo, hi)


# ---------------------------------------------------------------------------
# 1. hand-set counters: the small genomes of the genome-wide tests, and one of three units
# ---------------------------------------------------------------------------
def unit_genome():
    """about 3 U bases in 3 chromosomes; CG pairs whose C is the last position of a unit of the regions that start at 3
    and at 100 (3 + U - 1, 100 + U - 1, 100 + 2U - 1), so that a unit boundary falls between the C and the G"""
    rng = random.Random(4096)
    lengths = [U + 7, 61, 2 * U]
    seqs = ["".join(rng.choice("ACGTCG") for _ in range(L)) for L in lengths]
    text = list("".join(seqs))
    for at in (3 + U - 1, 100 + U - 1, 100 + 2 * U - 1):
        text[at:at + 2] = "CG"
    text = "".join(text)
    cuts = [0, lengths[0], lengths[0] + lengths[1], sum(lengths)]
    return Genome(["u%d" % i for i in range(3)], [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


@pytest.fixture(scope="module", params=[1, 7, 40, "units"])
def piled(request, scratch):
    g = unit_genome() if request.param == "units" else small_genome(request.param)
    db, path, idx = build_index(g, scratch, "regions_%s" % request.param)
    pile = idx.pileup()
    try:
        meth, unmeth = hand_counters(g.genome_len, 31 + g.n_chrom)
        pile.add(0, g.genome_len, meth, unmeth)
        cls, pair = classes(g.R[0], g.start_index)
        yield {"g": g, "idx": idx, "pile": pile, "meth": meth, "unmeth": unmeth, "cls": cls, "pair": pair, "units": request.param == "units"}
    finally:
        pile.close()
        idx.close()
        remove_index(path)


def region_list(c):
    """one call's regions, unsorted: every edge the contract names"""
    g, pair = c["g"], c["pair"]
    glen, start = g.genome_len, [int(x) for x in g.start_index]
    at = [f for f in range(glen) if pair[f]]
    f0, f1 = at[0], at[len(at) // 2]
    a0 = g.text.index("A")
    regs = [(0, 0), (glen, glen), (glen // 2, glen // 2)]                       # empty ones
    regs += [(f0, f0 + 1), (f0 + 1, f0 + 2), (a0, a0 + 1)]                      # one base: a C, its G, an A
    regs += [(max(0, f1 - 10), f1 + 1), (f1 + 1, min(glen, f1 + 30))]           # ends between C and G; begins on the G
    regs += [(f0, f0 + 2), (63, 65), (64, 66)]
    regs += [(off, off + n) for n in (63, 64, 65) for off in (0, 1, 63)]
    if g.n_chrom > 1:
        regs += [(start[1] - 5, start[1] + 1), (start[1], start[2]), (start[2], start[3])]
        regs += [(start[1] - 7, min(glen, start[3] + 9)), (start[g.n_chrom - 1] - 3, glen), (0, start[g.n_chrom - 1])]
        if g.n_chrom > 5:
            regs += [(start[4] - 1, start[4] + 1), (start[4] - 1, start[4]), (start[4], start[4] + 1)]  # ...C | G...: no pair
    regs += [(0, glen)]                                                          # the whole genome
    regs += [(10, 300)] * 3                                                      # the same region three times
    regs += [(100, 900), (200, 400), (300, 301), (350, 1200), (0, 700)]         # nested and partly overlapping
    if c["units"]:
        regs += [(3, 3 + U - 1), (3, 3 + U), (3, 3 + U + 1), (100, 100 + 2 * U + 1), (3 + U - 1, 3 + U), (3 + U, 3 + U + 1)]
        regs += [(0, U), (U, 2 * U), (2 * U, glen), (1, glen - 1), (U - 64, U + 64)]
        assert pair[3 + U - 1] and pair[100 + U - 1] and pair[100 + 2 * U - 1]
    random.Random(17).shuffle(regs)
    assert all(0 <= lo <= hi <= glen for lo, hi in regs)
    return regs


def partition(c):
    """the genome cut at chromosome starts, at f and f + 1 of some pairs and at a few other places"""
    g = c["g"]
    at = [f for f in range(g.genome_len) if c["pair"][f]]
    cuts = {0, g.genome_len, 64, 65, 1000} | {int(x) for x in g.start_index}
    for f in random.Random(3).sample(at, min(12, len(at))):
        cuts.update((f, f + 1))
    cuts = sorted(cuts)
    return list(zip(cuts[:-1], cuts[1:]))


def test_every_record_equals_the_walk_and_the_summary(piled):
    import walt_amd
    c = piled
    pile = c["pile"]
    regs = region_list(c)
    got = pile.regions(np.array(regs, dtype=np.int64))
    assert got.dtype == walt_amd.region_levels_dtype and got.shape == (len(regs),)
    assert_records(got, regs, c, "the list")
    for i in range(0, len(regs), 4):  # a sample against the genome-wide call on the same range
        assert rec_rows(got[i]) == levels_rows(pile.levels(*regs[i])), regs[i]
    whole = rec_rows(got[regs.index((0, c["g"].genome_len))])
    assert whole == levels_rows(pile.levels())
    for r in (0, 1, 2, 4):  # every row has covered sites, and uncovered sites are counted
        assert whole[r]["sites"] >= whole[r]["covered"] > 0, r
    assert sum(whole[r]["sites"] - whole[r]["covered"] for r in range(4)) > 20
    # the same regions as a region_dtype array
    typed = np.zeros(len(regs), dtype=walt_amd.region_dtype)
    typed["lo"], typed["hi"] = [r[0] for r in regs], [r[1] for r in regs]
    assert pile.regions(typed).tobytes() == got.tobytes()
    # a partition folds to the genome-wide summary
    parts = partition(c)
    got_parts = pile.regions(np.array(parts, dtype=np.uint32))
    assert_records(got_parts, parts, c, "the partition")
    assert fold_rows([rec_rows(x) for x in got_parts]) == whole


def test_launch_shapes_give_identical_bytes(piled, index_options):
    c = piled
    regs = np.array(region_list(c) + partition(c), dtype=np.uint32)
    seen = []
    for blocks in (0, 1, 7, 1000):
        index_options(c["idx"], pile_extract_blocks=blocks)
        seen.append(c["pile"].regions(regs).tobytes())
    assert seen[0] == seen[1] == seen[2] == seen[3] and any(seen[0])


def test_large_counters_on_both_halves_of_a_pair(piled):
    c = piled
    f = 3 + U - 1 if c["units"] else 255
    assert c["pair"][f]
    pile = c["idx"].pileup()
    try:
        big = np.full(2, 0xFFFFFFFF, dtype=np.uint32)
        pile.add(f, f + 2, big, None)
        got = pile.regions(np.array([(f, f + 1), (f, f + 2), (f + 1, f + 2), (f - 1, f)], dtype=np.uint32))
        for i in (0, 1):
            row = rec_rows(got[i])[4]
            assert row == {"sites": 1, "covered": 1, "meth": 2 ** 33 - 2, "unmeth": 0, "level_sum": 1 << 30}, (i, row)
        assert rec_rows(got[2])[4] == zero_record()[4] and rec_rows(got[3])[4]["covered"] == 0
        assert rec_rows(got[1])[0]["meth"] == 2 ** 33 - 2 and rec_rows(got[0])[0]["meth"] == 2 ** 32 - 1
        pile.add(f, f + 2, None, big)
        row = rec_rows(pile.regions(np.array([(f, f + 1)], dtype=np.uint32))[0])[4]
        assert row == {"sites": 1, "covered": 1, "meth": 2 ** 33 - 2, "unmeth": 2 ** 33 - 2, "level_sum": 1 << 29}
    finally:
        pile.close()


# ---------------------------------------------------------------------------
# 2. sizes and forms
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seven(scratch):
    g = small_genome(7)
    db, path, idx = build_index(g, scratch, "regions_forms")
    pile = idx.pileup()
    try:
        meth, unmeth = hand_counters(g.genome_len, 38)
        pile.add(0, g.genome_len, meth, unmeth)
        cls, pair = classes(g.R[0], g.start_index)
        yield {"g": g, "idx": idx, "pile": pile, "meth": meth, "unmeth": unmeth, "cls": cls, "pair": pair, "units": False,
               "sums": prefix_sums(cls, pair, meth, unmeth)}
    finally:
        pile.close()
        idx.close()
        remove_index(path)


def test_no_region_and_one_region(seven):
    import walt_amd
    c = seven
    pile, glen = c["pile"], c["g"].genome_len
    for empty in (np.zeros((0, 2), dtype=np.uint32), np.zeros(0, dtype=walt_amd.region_dtype), []):
        got = pile.regions(empty)
        assert got.shape == (0,) and got.dtype == walt_amd.region_levels_dtype
    L = walt_amd.lib()
    assert L.walt_pileup_regions(pile.handle, None, 0, None) == walt_amd.WALT_OK
    assert L.walt_pileup_regions_device(pile.handle, None, 0, None, None, None) == walt_amd.WALT_OK
    for reg in [(0, glen), (5, 5), (63, 64), (1, 700)]:
        assert_records(pile.regions(np.array([reg], dtype=np.uint32)), [reg], c, "one region")
    assert walt_amd.regions_workspace_bytes(0) >= 8 and walt_amd.regions_workspace_bytes(70000) >= 8 * 70001
    assert walt_amd.regions_workspace_bytes(1 << 22) <= 64 << 20  # O(n), whatever the regions span


def test_seventy_thousand_short_regions(seven, index_options):
    """more regions than 65,535 and no multiple of the scan's block: several blocks of sums, a ragged last one"""
    c = seven
    glen = c["g"].genome_len
    rng = np.random.RandomState(70)
    n = 70001
    lo = rng.randint(0, glen + 1, size=n)
    hi = np.minimum(lo + rng.randint(0, 200, size=n), glen)
    hi[::1000] = lo[::1000]      # empty ones throughout
    lo[-1], hi[-1] = 0, glen     # and a long one last
    regs = np.stack([lo, hi], axis=1).astype(np.uint32)
    want = records_by_prefix(c["sums"], regs.astype(np.int64))
    for i in list(range(0, n, 2500)) + [n - 1]:  # the prefix sums say what the walk says
        w = want_record(c["cls"], c["pair"], c["meth"], c["unmeth"], int(lo[i]), int(hi[i]))
        assert [[int(want[r, k, i]) for k in range(5)] for r in range(5)] == [[w[r][k] for k in REGION_FIELDS] for r in range(5)], i
    got = c["pile"].regions(regs)
    for k, name in enumerate(REGION_FIELDS):
        assert np.array_equal(got["row"][name].astype(np.int64).T, want[:, k, :]), name
    index_options(c["idx"], pile_extract_blocks=3)
    assert c["pile"].regions(regs).tobytes() == got.tobytes()


def test_device_form_on_a_side_stream_and_refusals(seven):
    import torch
    import walt_amd
    c = seven
    pile, glen = c["pile"], c["g"].genome_len
    regs = region_list(c)
    bad_at = {3: (glen - 1, glen + 1), 11: (9, 8), 20: (0, 0xFFFFFFFF)}  # not inside the genome: a zero record each
    arr = np.array(regs, dtype=np.uint32)
    for i, r in bad_at.items():
        arr[i] = r
    n = len(regs)
    dev = torch.device("cuda", 0)
    d_regs = torch.from_numpy(arr.view(np.int32).copy()).to(dev)
    d_out = torch.full((n * 20,), -1, dtype=torch.int64, device=dev)
    d_work = torch.empty(walt_amd.regions_workspace_bytes(n), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    pile.regions_device(d_regs.data_ptr(), n, d_out.data_ptr(), d_work.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    got = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=walt_amd.region_levels_dtype)
    for i, (lo, hi) in enumerate(regs):
        want = zero_record() if i in bad_at else want_record(c["cls"], c["pair"], c["meth"], c["unmeth"], lo, hi)
        assert rec_rows(got[i]) == want, (i, lo, hi)
    good = [i for i in range(n) if i not in bad_at]
    assert got[good].tobytes() == pile.regions(arr[good]).tobytes()
    # refusals of the device form: alignment, null pointers, too many regions
    L = walt_amd.lib()
    args = [d_regs.data_ptr(), n, d_out.data_ptr(), d_work.data_ptr()]
    for k in (0, 2, 3):
        odd = list(args)
        odd[k] += 4
        assert L.walt_pileup_regions_device(pile.handle, *odd, None) == walt_amd.WALT_EINVAL and b"aligned" in L.walt_last_error()
        odd[k] = None
        assert L.walt_pileup_regions_device(pile.handle, *odd, None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_regions_device(pile.handle, args[0], walt_amd.REGIONS_MAX + 1, args[2], args[3], None) == walt_amd.WALT_EINVAL
    assert b"at most" in L.walt_last_error()
    assert L.walt_pileup_regions_device(None, *args, None) == walt_amd.WALT_EINVAL
    assert pile.device_bytes == 8 * glen + (1 << 20)


def test_host_form_refusals_name_the_region_and_write_nothing(seven):
    import walt_amd
    c = seven
    pile, glen = c["pile"], c["g"].genome_len
    L = walt_amd.lib()
    for k, wrong in ((0, (5, 4)), (2, (0, glen + 1)), (3, (glen + 1, glen + 1))):
        regs = np.array([(0, 10), (3, 9), (5, 5), (0, glen)], dtype=np.uint32)
        regs[k] = wrong
        out = np.full(4 * 20, 0x55, dtype=np.uint64)
        assert L.walt_pileup_regions(pile.handle, regs.ctypes.data, 4, out.ctypes.data) == walt_amd.WALT_EINVAL
        assert b"region %d " % k in L.walt_last_error(), L.walt_last_error()
        assert (out == 0x55).all()
        with pytest.raises(walt_amd.WaltError):
            pile.regions(regs)
    one = np.array([(0, 1)], dtype=np.uint32)
    out = np.zeros(20, dtype=np.uint64)
    assert L.walt_pileup_regions(pile.handle, None, 1, out.ctypes.data) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_regions(pile.handle, one.ctypes.data, 1, None) == walt_amd.WALT_EINVAL
    assert L.walt_pileup_regions(None, one.ctypes.data, 1, out.ctypes.data) == walt_amd.WALT_EINVAL
    with pytest.raises(ValueError):
        pile.regions(np.zeros((3, 3), dtype=np.uint32))
    with pytest.raises(ValueError):
        pile.regions(np.array([(-1, 4)]))


# ---------------------------------------------------------------------------
# 3. command line
# ---------------------------------------------------------------------------
def bed_for(db, scratch, tag, unknown=False):
    """about 30 regions of the golden genome in every accepted form: one whole chromosome, an empty region, names and
    further columns, blanks and tabs, comment, track and browser lines; -> (path, [(chrom, start, end, name)])"""
    rng = random.Random(5)
    length = {nm: int(db.start_index[i + 1]) - int(db.start_index[i]) for i, nm in enumerate(db.names)}
    rows = [(db.names[1], 0, length[db.names[1]], "whole"), (db.names[0], 77, 77, "empty"), (db.names[-1], 0, 1, ".")]
    for k in range(27):
        nm = rng.choice(db.names)
        a = rng.randrange(0, length[nm])
        rows.append((nm, a, min(length[nm], a + rng.choice([1, 2, 50, 300, 1000, 5000])), rng.choice([".", "r%d" % k])))
    if unknown:
        rows.insert(4, ("chrNowhere", 5, 900, "lost"))
        rows.append(("chrNowhere", 0, 0, "."))
    path = os.path.join(scratch, "regions_%s.bed" % tag)
    with open(path, "w") as f:
        f.write("# regions of the golden genome\ntrack name=test\nbrowser position x:1-2\n\n")
        for k, (nm, a, b, name) in enumerate(rows):
            if name == ".":
                f.write("%s\t%d\t%d\n" % (nm, a, b))
            elif k % 3 == 0:
                f.write("%s %d  %d %s 0 -\n" % (nm, a, b, name))
            else:
                f.write("%s\t%d\t%d\t%s\t960\t+\n" % (nm, a, b, name))
    return path, rows


def counters_from(c, counts_path):
    """the counters a run's <out>.methcounts lists"""
    db = c["db"]
    first = {nm: int(db.start_index[i]) for i, nm in enumerate(db.names)}
    meth, unmeth = np.zeros(db.genome_len, dtype=np.int64), np.zeros(db.genome_len, dtype=np.int64)
    for line in open(counts_path):
        nm, off, _, _, m, u = line.rstrip("\n").split("\t")
        meth[first[nm] + int(off)], unmeth[first[nm] + int(off)] = int(m), int(u)
    return meth, unmeth


def text_from_counts(c, rows, counts_path):
    """<out>.regions' block as the restatement computes it from a run's <out>.methcounts and the reference"""
    db = c["db"]
    first = {nm: int(db.start_index[i]) for i, nm in enumerate(db.names)}
    meth, unmeth = counters_from(c, counts_path)
    recs = [want_record(c["cls"], c["pair"], meth, unmeth, first[nm] + a, first[nm] + b) if nm in first else zero_record()
            for nm, a, b, _ in rows]
    return regions_text(rows, recs)


def other_files(out):
    d, base = os.path.dirname(out), os.path.basename(out)
    return sorted(f[len(base):] for f in os.listdir(d) if f.startswith(base) and not f.endswith(".regions"))


@pytest.mark.parametrize("mode", ["r", "paired", "R"])
def test_cli_adds_one_file_and_changes_no_other(g1, scratch, mode):
    c = g1
    bed, rows = bed_for(c["db"], scratch, "cli_" + mode)
    if mode == "r":
        reads, extra = ["-r", os.path.join(refio.GOLDEN, "se_ct.fastq")], []
    elif mode == "paired":
        reads, extra = ["-1", os.path.join(refio.GOLDEN, "pe_1.fastq"), "-2", os.path.join(refio.GOLDEN, "pe_2.fastq")], []
    else:
        from test_gpu_rpbat import mixed_library
        fq = os.path.join(scratch, "regions_mixed.fastq")
        with open(fq, "w") as f:
            for nm, s, q in zip(*mixed_library()):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
        reads, extra = ["-r", fq], ["-R"]
    texts = []
    for tag, more in (("plain", []), ("counts", ["-MC"]), ("all", ["-MC", "-ML", "-M", "-sam"])):
        base = os.path.join(scratch, "regions_cli_%s_%s.base" % (mode, tag))
        with_mr = os.path.join(scratch, "regions_cli_%s_%s.mr" % (mode, tag))
        common = ["-i", c["path"]] + reads + ["-a", "-u"] + extra + more
        run_walt(common + ["-o", base])
        run_walt(common + ["-o", with_mr, "-MR", bed])
        assert not os.path.exists(base + ".regions")  # without -MR: no such file, and every other byte as with it
        files = other_files(base)
        assert files == other_files(with_mr) and "" in files and (".methcounts" in files) == bool(more)
        for sfx in files:
            assert open(base + sfx, "rb").read() == open(with_mr + sfx, "rb").read(), (mode, tag, sfx)
        text = open(with_mr + ".regions").read()
        assert text.startswith(REGIONS_HEADER) and text.count("\n") == 1 + len(rows)
        if more:
            assert text == text_from_counts(c, rows, with_mr + ".methcounts")
        texts.append(text)
    assert texts[0] == texts[1] == texts[2]  # -MR alone counts what -MC counts
    covered = [ln.split("\t") for ln in texts[0].split("\n")[1:-1]]
    assert covered[0][3] == "whole" and int(covered[0][4]) > 0 and covered[1][3] == "empty" and covered[1][4:10] == ["0", "0", "0", "0", "NA", "NA"]


def test_cli_devices_filters_read_files_and_unknown_chromosomes(g1, scratch):
    c = g1
    fq = os.path.join(refio.GOLDEN, "se_ct.fastq")
    bed, rows = bed_for(c["db"], scratch, "cli_more", unknown=True)
    out = os.path.join(scratch, "regions_cli_one.out")
    log = run_walt(["-i", c["path"], "-r", fq, "-o", out, "-MR", bed, "-MC", "-v"])
    block = open(out + ".regions").read()
    assert block == text_from_counts(c, rows, out + ".methcounts")
    assert "2 on chromosomes the index does not have" in log
    lost = block.split("\n")[5].split("\t")  # its line stays, zeros and NA
    assert lost[:4] == ["chrNowhere", "5", "900", "lost"] and set(lost[4:]) == {"0", "NA"}
    # -g 0,0: two shares, two pile-ups, the second folded into the first -- once, also beside -ML
    for tag, more in (("g00", []), ("g00_ml", ["-ML"])):
        two = os.path.join(scratch, "regions_cli_%s.out" % tag)
        run_walt(["-i", c["path"], "-r", fq, "-o", two, "-MR", bed, "-g", "0,0"] + more)
        assert open(two + ".regions").read() == block and not os.path.exists(two + ".methcounts")
        if more:
            one = os.path.join(scratch, "regions_cli_ml_one.out")
            run_walt(["-i", c["path"], "-r", fq, "-o", one, "-ML"])
            assert open(two + ".levels").read() == open(one + ".levels").read()
    # -D and -I5 5 change it exactly as they change <out>.methcounts
    twice = os.path.join(scratch, "regions_twice.fastq")
    with open(twice, "w") as f:
        f.write(open(fq).read() * 2)
    seen = {}
    for tag, reads, opt in (("twice", twice, []), ("D", twice, ["-D"]), ("I5", fq, ["-I5", "5"])):
        o2 = os.path.join(scratch, "regions_cli_%s.out" % tag)
        run_walt(["-i", c["path"], "-r", reads, "-o", o2, "-MR", bed, "-MC"] + opt)
        seen[tag] = (open(o2 + ".methcounts").read(), open(o2 + ".regions").read())
        assert seen[tag][1] == text_from_counts(c, rows, o2 + ".methcounts"), tag
    assert seen["D"][0] != seen["twice"][0] and seen["D"][1] != seen["twice"][1]
    assert seen["I5"][0] != open(out + ".methcounts").read() and seen["I5"][1] != block
    # two read files that share one output name: two blocks; the other spellings
    o3 = os.path.join(scratch, "regions_cli_two.out")
    run_walt(["-i", c["path"], "-r", fq + "," + fq, "-o", o3, "-regions", bed])
    assert open(o3 + ".regions").read() == block + block
    run_walt(["-i", c["path"], "-r", fq, "-o", o3, "--meth-regions", bed])
    assert open(o3 + ".regions").read() == block


def test_cli_refusals(g1, scratch):
    import subprocess
    c = g1
    fq = os.path.join(refio.GOLDEN, "se_ct.fastq")
    walt = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
    long_one = int(c["db"].start_index[1]) - int(c["db"].start_index[0])
    name = c["db"].names[0]
    cases = [("%s 1 2\n%s 5\n" % (name, name), ":2:", "three columns"),
             ("%s x 2\n" % name, ":1:", "not a number"),
             ("\n# c\n%s 1 2e3\n" % name, ":3:", "not a number"),
             ("%s 9 2\n" % name, ":1:", "behind end"),
             ("%s 0 5\n%s 0 %d\n" % (name, name, long_one + 1), ":2:", "beyond"),
             ("# nothing\n\ntrack x\n", ":0:", "no region")]
    for k, (text, where, what) in enumerate(cases):
        bed = os.path.join(scratch, "regions_bad_%d.bed" % k)
        with open(bed, "w") as f:
            f.write(text)
        out = os.path.join(scratch, "regions_bad_%d.out" % k)
        pr = subprocess.run([walt, "-i", c["path"], "-r", fq, "-o", out, "-MR", bed], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                            text=True, timeout=120)
        assert pr.returncode != 0 and bed + where in pr.stdout and what in pr.stdout, (k, pr.stdout)
        assert not os.path.exists(out + ".regions") or open(out + ".regions").read() == ""
    pr = subprocess.run([walt, "-i", c["path"], "-r", fq, "-o", os.path.join(scratch, "regions_bad_none.out"), "-MR",
                         os.path.join(scratch, "no_such.bed")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert pr.returncode != 0 and "no_such.bed" in pr.stdout and "cannot open" in pr.stdout
