"""Single-end random PBAT (walt_map_se_rpbat_batch, bin/walt -R): every read mapped under both conversions, one record
per read.  The contract (include/walt_amd.h) is checked read by read against the rule applied to the oracle's C->T and
G->A runs (tests/refio.py), through the C ABI, its device form, seed patterns 5 and 7, and the command line."""
import os
import random
import subprocess

import numpy as np
import pytest

import refio

pytestmark = pytest.mark.gpu

WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
MAKEDB_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "makedb")
FIELDS = ("genome_pos", "times", "strand", "mismatch")


def rpbat_rule(c, g):
    """The contract applied to two single-conversion record arrays -> (records, conv, rule number per read)."""
    import walt_amd
    ct, gt = c["times"].astype(np.int64), g["times"].astype(np.int64)
    r1 = (ct == 1) & (gt == 1) & (c["genome_pos"] == g["genome_pos"]) & (c["strand"] == g["strand"])
    r2 = ~r1 & ((gt == 0) | ((ct > 0) & (c["mismatch"] < g["mismatch"])))
    r3 = ~r1 & ~r2 & ((ct == 0) | (g["mismatch"] < c["mismatch"]))
    r4 = ~r1 & ~r2 & ~r3
    rec = np.zeros(len(c), dtype=walt_amd.best_match_dtype)
    for f in FIELDS:
        rec[f] = np.where(r3, g[f], c[f])
    rec["times"][r4] = (ct + gt)[r4]
    conv = np.where(r3, ord("A"), ord("T")).astype(np.uint8)
    rule = np.select([r1, r2, r3, r4], [1, 2, 3, 4])
    return rec, conv, rule


def oracle_rpbat(db, seqs, m=6, b=5000):
    c, wc = refio.oracle_se(db, seqs, ag=False, max_mm=m, b=b)
    g, _ = refio.oracle_se(db, seqs, ag=True, max_mm=m, b=b)
    rec, conv, rule = rpbat_rule(c, g)
    return rec, conv, rule, int(wc["too_short"])


def assert_records(got, conv, want, want_conv, what=""):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s field %s differs at %s: got %s want %s" % (what, f, bad[:5], got[f][bad[:5]],
                                                                              want[f][bad[:5]])
    bad = np.nonzero(conv != want_conv)[0]
    assert bad.size == 0, "%s conv differs at %s: got %s want %s" % (what, bad[:5], conv[bad[:5]], want_conv[bad[:5]])


def load(name):
    names, seqs, scores = [], [], []
    for nm, sq, sc in refio.load_fastq_batches(os.path.join(refio.GOLDEN, name), 10 ** 7):
        names += nm
        seqs += sq
        scores += sc
    return names, seqs, scores


def mixed_library(ct="se_ct.fastq", ga="se_ga.fastq", seed=2024):
    """T-rich and A-rich reads of the golden set in one library, shuffled with a fixed seed."""
    a, b = load(ct), load(ga)
    names, seqs, scores = a[0] + b[0], a[1] + b[1], a[2] + b[2]
    perm = np.random.default_rng(seed).permutation(len(seqs))
    return [names[i] for i in perm], [seqs[i] for i in perm], [scores[i] for i in perm]


@pytest.fixture(scope="module")
def rp(scratch):
    import walt_amd
    path = os.path.join(scratch, "rpbat_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
    yield db, idx, path
    idx.close()


@pytest.fixture(scope="module")
def mixed(rp):
    db = rp[0]
    names, seqs, scores = mixed_library()
    rec, conv, rule, short = oracle_rpbat(db, seqs)
    return names, seqs, scores, rec, conv, rule, short


@pytest.mark.parametrize("b", [2, 5000])
@pytest.mark.parametrize("m", [0, 2, 6])
def test_mixed_library_follows_the_rule(rp, m, b):
    import walt_amd
    db, idx, _ = rp
    _, seqs, _ = mixed_library()
    want, want_conv, rule, short = oracle_rpbat(db, seqs, m, b)
    got, conv, st = idx.map_se_rpbat_batch(*walt_amd.pack_reads(seqs), max_mismatches=m, b=b)
    assert_records(got, conv, want, want_conv, "m=%d b=%d" % (m, b))
    assert int(st["too_short"]) == short
    assert (rule == 2).sum() > 100 and (rule == 3).sum() > 100  # both conversions decide reads of this library
    # the work counters are the sums over both conversions: at least what one conversion reports
    _, s1 = idx.map_se_batch(*walt_amd.pack_reads(seqs), ag_wildcard=False, max_mismatches=m, b=b)
    assert int(st["probes"]) > int(s1["probes"]) > 0


def planted_genome(tmp, seed=11):
    """A FASTA with a read for every rule: A/T-only stretches (no informative C or G: the same alignment under both
    conversions, rule 1), C->T / G->A conversions of random stretches (rules 2 / 3), and A/T reads whose C->T hit and
    G->A hit lie at two loci with equal mismatches (rule 4)."""
    rng = random.Random(seed)

    def rnd(n, al="ACGT"):
        return "".join(rng.choice(al) for _ in range(n))

    body, reads = [rnd(3000)], []
    for k in range(4):
        r = rnd(100, "AT")
        body += [r, rnd(500)]
        reads += [r, refio.revcomp(r)]
    for k in range(4):
        r = rnd(100, "AT")
        l1, l2 = list(r), list(r)
        for i in rng.sample([i for i, ch in enumerate(r) if ch == "T"], 10):
            l1[i] = "C"  # a C->T hit only: 10 mismatches under G->A
        for i in rng.sample([i for i, ch in enumerate(r) if ch == "A"], 10):
            l2[i] = "G"  # a G->A hit only
        body += ["".join(l1), rnd(400), "".join(l2), rnd(400)]
        reads.append(r)
    for k in range(4):
        s = rnd(100)
        body += [s, rnd(300)]
        reads.append(s.replace("C", "T"))
        reads.append(refio.revcomp(s).replace("G", "A"))
    fa = os.path.join(tmp, "rpbat_planted.fa")
    with open(fa, "w") as f:
        f.write(">p1\n%s\n>p2\n%s\n" % ("".join(body), rnd(2000)))
    return fa, reads


def test_every_rule_decides_a_read(scratch):
    import walt_amd
    fa, seqs = planted_genome(scratch)
    path = os.path.join(scratch, "rpbat_planted.dbindex")
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
    try:
        want, want_conv, rule, _ = oracle_rpbat(db, seqs)
        for k in (1, 2, 3, 4):
            assert (rule == k).sum() >= 1, "no read decided by rule %d: %s" % (k, rule)
        got, conv, _ = idx.map_se_rpbat_batch(*walt_amd.pack_reads(seqs))
        assert_records(got, conv, want, want_conv, "planted")
        assert (got["times"][rule == 4] >= 2).all()
    finally:
        idx.close()


def test_long_and_short_reads(rp):
    import walt_amd
    db, idx, _ = rp
    for files in (("se150_ga.fastq",), ("sp_short.fastq",), ("se150_ga.fastq", "sp_short.fastq", "se_ct.fastq")):
        seqs = sum((load(f)[1] for f in files), [])
        want, want_conv, _, short = oracle_rpbat(db, seqs, m=10)
        got, conv, st = idx.map_se_rpbat_batch(*walt_amd.pack_reads(seqs), max_mismatches=10)
        assert_records(got, conv, want, want_conv, str(files))
        _, s1 = idx.map_se_batch(*walt_amd.pack_reads(seqs), ag_wildcard=False, max_mismatches=10)
        assert int(st["too_short"]) == short == int(s1["too_short"])
        if "sp_short.fastq" in files:
            assert short > 0


def test_non_acgt_base_is_refused(rp):
    import walt_amd
    _, idx, _ = rp
    seqs = load("se_ct.fastq")[1][:20]
    seqs[7] = seqs[7][:30] + "N" + seqs[7][31:]
    with pytest.raises(walt_amd.WaltError) as ei:
        idx.map_se_rpbat_batch(*walt_amd.pack_reads(seqs))
    assert ei.value.code == walt_amd.WALT_EBASE


def test_index_without_every_strand_is_refused(rp):
    import walt_amd
    _, _, path = rp
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT)
    try:
        with pytest.raises(walt_amd.WaltError) as ei:
            idx.map_se_rpbat_batch(*walt_amd.pack_reads(["ACGT" * 25]))
        assert ei.value.code == walt_amd.WALT_EINVAL
        assert "_GA10" in str(ei.value) and "_GA11" in str(ei.value) and "_CT00" not in str(ei.value)
    finally:
        idx.close()


def test_device_form_on_a_side_stream_equals_host_form(rp, mixed):
    import torch
    import walt_amd
    _, idx, _ = rp
    _, seqs, _, want, want_conv, _, short = mixed
    bases, offsets = walt_amd.pack_reads(seqs)
    n, L = len(seqs), max(len(s) for s in seqs)
    dev = torch.device("cuda:0")
    d_bases = torch.from_numpy(bases).to(dev)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_conv = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = walt_amd.se_rpbat_workspace_bytes(n, L)
    guard = 1 << 16
    d_ws = torch.full((ws + guard,), 0xA5, dtype=torch.uint8, device=dev)  # guard bytes behind the workspace
    side = torch.cuda.Stream()
    with pytest.raises(walt_amd.WaltError) as ei:  # one byte short
        idx.map_se_rpbat_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_conv.data_ptr(),
                                      d_stats.data_ptr(), d_ws.data_ptr(), ws - 1, stream=side.cuda_stream)
    assert ei.value.code == walt_amd.WALT_EINVAL
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        idx.map_se_rpbat_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_conv.data_ptr(),
                                      d_stats.data_ptr(), d_ws.data_ptr(), ws, stream=side.cuda_stream)
    walt_amd.Index.check_batch(d_ws.data_ptr(), side.cuda_stream)
    side.synchronize()
    got = d_out.cpu().numpy().view(walt_amd.best_match_dtype)
    conv = d_conv.cpu().numpy()
    host, host_conv, host_st = idx.map_se_rpbat_batch(bases, offsets)
    assert_records(got, conv, host, host_conv, "device form vs host form")
    assert_records(got, conv, want, want_conv, "device form vs oracle")
    st = d_stats.cpu().numpy()
    assert int(st[0]) == short == int(host_st["too_short"])
    assert (d_ws[ws:].cpu().numpy() == 0xA5).all(), "the call wrote behind its workspace"


def test_single_conversion_calls_after_random_pbat(rp, mixed):
    import walt_amd
    db, idx, _ = rp
    _, seqs, _, _, _, _, _ = mixed
    idx.map_se_rpbat_batch(*walt_amd.pack_reads(seqs))
    for ag in (False, True):
        want, work = refio.oracle_se(db, seqs, ag=ag)
        got, st = idx.map_se_batch(*walt_amd.pack_reads(seqs), ag_wildcard=ag)
        for f in FIELDS:
            assert np.array_equal(got[f], want[f]), "ag=%s field %s" % (ag, f)
        assert int(st["too_short"]) == int(work["too_short"])


@pytest.mark.parametrize("opts", [{"se_pipe": 0}, {"se_heavy_chunk": 64}, {"se_pipe": 0, "se_heavy_chunk": 64},
                                  {"se_lit_side": 0}, pytest.param({"grid": 1}, id="opts6"),
                                  pytest.param({"grid": 2}, id="opts7")])  # (the ids they have always had)
def test_schedules_give_the_same_records(rp, mixed, index_options, opts):
    import walt_amd
    _, idx, _ = rp
    _, seqs, _, want, want_conv, _, short = mixed
    index_options(idx, **opts)
    got, conv, st = idx.map_se_rpbat_batch(*walt_amd.pack_reads(seqs))
    assert_records(got, conv, want, want_conv, str(opts))
    assert int(st["too_short"]) == short


@pytest.fixture(params=(5, 7))  # per test: the module's other tests run on pattern 3
def pat(request, scratch):
    import walt_amd
    p = request.param
    refio.set_pattern(p)
    walt_amd.set_pattern(p)
    try:
        path = os.path.join(scratch, "rpbat_g1_sp%d.dbindex" % p)
        walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
        db = refio.DbIndex(path)
        idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
        yield p, db, idx
        idx.close()
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)


def test_seed_patterns_5_and_7(pat):
    import walt_amd
    p, db, idx = pat
    _, seqs, _ = mixed_library("sp_se_ct.fastq", "sp_se_ga.fastq")
    for m in (2, 6):
        want, want_conv, _, short = oracle_rpbat(db, seqs, m=m)
        got, conv, st = idx.map_se_rpbat_batch(*walt_amd.pack_reads(seqs), max_mismatches=m)
        assert_records(got, conv, want, want_conv, "pattern %d m=%d" % (p, m))
        assert int(st["too_short"]) == short


# ---------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def cli_rp(scratch):
    """The product's makedb binary on g1.fa, and the mixed library as a FASTQ file."""
    out = os.path.join(scratch, "rpbat_cli_g1.dbindex")
    env = dict(os.environ, WALT_MAKEDB_SEED="1")
    subprocess.run([MAKEDB_BIN, "-c", os.path.join(refio.GOLDEN, "g1.fa"), "-o", out, "-t", "4"], check=True, env=env,
                   stderr=subprocess.DEVNULL)
    names, seqs, scores = mixed_library()
    fq = os.path.join(scratch, "rpbat_mixed.fastq")
    with open(fq, "w") as f:
        for nm, sq, sc in zip(names, seqs, scores):
            f.write("@%s\n%s\n+\n%s\n" % (nm, sq, sc))
    db = refio.DbIndex(out)
    names, seqs, scores = load_fq(fq)
    rec, conv, rule, short = oracle_rpbat(db, seqs)
    return out, fq, db, (names, seqs, scores), (rec, conv, rule, short)


def load_fq(fq):
    names, seqs, scores = [], [], []
    for nm, sq, sc in refio.load_fastq_batches(fq, 10 ** 7):
        names += nm
        seqs += sq
        scores += sc
    return names, seqs, scores


def expected_files(db, reads, want, sam):
    names, seqs, scores = reads
    rec, conv, _, short = want
    main = refio.sam_header(db) if sam else ""
    amb = unm = ""
    for r, cv, nm, sq, sc in zip(rec, conv, names, seqs, scores):
        if sam:
            line = refio.se_sam_line(db, r, nm, sq, sc, True, True)
            if line and int(r["times"]) > 0:
                line = line[:-1] + "\tCV:A:%s\n" % chr(cv)
            main += line
        else:
            a, b, c = refio.se_mr_route(db, r, nm, sq, sc, cv == ord("A"), True, True)
            main += a
            amb += b
            unm += c
    t = rec["times"]
    stats = refio.se_mapstats(len(rec), int((t == 1).sum()), int((t >= 2).sum()), int((t == 0).sum()), short) + "\n"
    base = "out.sam" if sam else "out.mr"
    files = {base: main, base + ".mapstats": stats}
    if not sam:
        files.update({base + "_ambiguous": amb, base + "_unmapped": unm})
    return files


def run_cli(binary, index, fq, wd, args, out_name):
    os.makedirs(wd, exist_ok=True)
    out = os.path.join(wd, out_name)
    subprocess.run([binary, "-i", index, "-r", fq, "-o", out] + args, check=True, cwd=wd, stderr=subprocess.DEVNULL)
    return {fn: open(os.path.join(wd, fn)).read() for fn in sorted(os.listdir(wd))}


def assert_files(got, want):
    assert sorted(got) == sorted(want)
    for fn in want:
        if got[fn] != want[fn]:
            for i, (a, b) in enumerate(zip(got[fn].splitlines(), want[fn].splitlines())):
                assert a == b, "%s line %d:\n got: %s\nwant: %s" % (fn, i + 1, a, b)
            assert got[fn] == want[fn], fn


@pytest.mark.parametrize("sam", [False, True])
def test_cli_random_pbat_files(cli_rp, scratch, sam):
    index, fq, db, reads, want = cli_rp
    args = (["-sam"] if sam else []) + ["-a", "-u", "-R"]
    name = "out.sam" if sam else "out.mr"
    got = run_cli(WALT_BIN, index, fq, os.path.join(scratch, "rpbat_cli_%d" % sam), args, name)
    assert_files(got, expected_files(db, reads, want, sam))
    two = run_cli(WALT_BIN, index, fq, os.path.join(scratch, "rpbat_cli_g00_%d" % sam), args + ["-g", "0,0"], name)
    assert two == got


def test_cli_two_read_files(cli_rp, scratch):
    index, fq, db, reads, want = cli_rp
    wd = os.path.join(scratch, "rpbat_cli_two")
    os.makedirs(wd, exist_ok=True)
    first = os.path.join(wd, "first.fastq")
    with open(fq) as f:
        lines = f.readlines()
    with open(first, "w") as f:
        f.writelines(lines[:4 * 300])
    subprocess.run([WALT_BIN, "-i", index, "-r", "%s,%s" % (first, fq), "-o", "o_s1.mr,o_s2.mr", "-R", "-a", "-u"],
                   check=True, cwd=wd, stderr=subprocess.DEVNULL)
    full = expected_files(db, reads, want, False)
    assert open(os.path.join(wd, "o_s2.mr")).read() == full["out.mr"]
    assert open(os.path.join(wd, "o_s2.mr.mapstats")).read() == full["out.mr.mapstats"]
    names, seqs, scores = reads
    rec, conv, rule, _ = want
    part = oracle_rpbat(db, seqs[:300])
    want1 = expected_files(db, (names[:300], seqs[:300], scores[:300]), part, False)
    assert open(os.path.join(wd, "o_s1.mr")).read() == want1["out.mr"]
    assert open(os.path.join(wd, "o_s1.mr_unmapped")).read() == want1["out.mr_unmapped"]


def by_name(files, sam):
    """read name -> line over every output file of a run (SAM: the name is field 1; MR: field 4, unmapped: field 1)."""
    out = {}
    for fn, text in files.items():
        if fn.endswith(".mapstats"):
            continue
        for line in text.splitlines():
            if not line or line.startswith("@"):
                continue
            f = line.split("\t")
            key = f[0] if sam or fn.endswith("_unmapped") else f[3]
            out[key] = (fn.replace("out.mr", "").replace("out.sam", ""), line)
    return out


@pytest.mark.parametrize("sam", [False, True])
def test_cli_lines_equal_the_reference_binary(cli_rp, scratch, sam):
    """Reads decided by rules 1-3 carry one conversion's record unchanged: their line (without the CV tag) is the line
    the reference binary writes for them in its run with (conv 'A') or without (conv 'T') -A, in the same file."""
    if not os.path.exists(refio.REF_WALT):
        pytest.skip("no reference binary built")
    index, fq, db, reads, want = cli_rp
    names = reads[0]
    rec, conv, rule, _ = want
    name = "out.sam" if sam else "out.mr"
    flags = (["-sam"] if sam else []) + ["-a", "-u"]
    got = by_name(run_cli(WALT_BIN, index, fq, os.path.join(scratch, "rpbat_ref_ours_%d" % sam), flags + ["-R"], name), sam)
    ref = {}
    for ag in (False, True):
        ref[ag] = by_name(run_cli(refio.REF_WALT, index, fq, os.path.join(scratch, "rpbat_ref_%d_%d" % (sam, ag)),
                                  flags + (["-A"] if ag else []), name), sam)
    checked = 0
    for i, key in enumerate(names):
        if rule[i] == 4:
            continue
        mine, theirs = got.get(key), ref[conv[i] == ord("A")].get(key)
        if mine is None and theirs is None:
            continue
        assert mine is not None and theirs is not None, (key, mine, theirs)
        line = mine[1].replace("\tCV:A:T", "").replace("\tCV:A:A", "")
        assert (mine[0], line) == (theirs[0], theirs[1]), key
        checked += 1
    assert checked > 1000
