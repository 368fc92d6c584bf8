"""Paired-end random PBAT (walt_map_pe_rpbat_batch, bin/walt -RP): every pair mapped in both orientations, one record
per pair.  The contract (include/walt_amd.h) is checked pair by pair against the rule applied to the oracle's two
orientations, oracle_pe(s1, s2) and oracle_pe(s2, s1) (tests/test_pe_rpbat_cpu.py holds the rule), through the C
ABI, its device form, seed patterns 5 and 7, the paired-end schedules and the command line."""
import os
import random
import subprocess

import numpy as np
import pytest

import refio
import test_pe_rpbat_cpu as rule_of

pytestmark = pytest.mark.gpu

WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
MAKEDB_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "makedb")


def load(name):
    names, seqs, scores = [], [], []
    for nm, sq, sc in refio.load_fastq_batches(os.path.join(refio.GOLDEN, name), 10 ** 7):
        names += nm
        seqs += sq
        scores += sc
    return names, seqs, scores


def mixed_pairs(f1="pe_1.fastq", f2="pe_2.fastq", seed=2024):
    """The golden pairs with the mates of a fixed random half exchanged, shuffled: a library whose T-rich read sits in
    either file.  Returns ((names, seqs, scores) of file 1, the same of file 2, True where the mates were exchanged)."""
    a, b = load(f1), load(f2)
    n = len(a[1])
    rng = np.random.default_rng(seed)
    swap = rng.random(n) < 0.5
    perm = rng.permutation(n)
    one = tuple([(b if swap[i] else a)[k][i] for i in perm] for k in range(3))
    two = tuple([(a if swap[i] else b)[k][i] for i in perm] for k in range(3))
    return one, two, swap[perm]


def pack(seqs):
    import walt_amd
    return walt_amd.pack_reads(seqs)


@pytest.fixture(scope="module")
def rp(scratch):
    import walt_amd
    path = os.path.join(scratch, "pe_rpbat_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
    yield db, idx, path
    idx.close()


@pytest.fixture(scope="module")
def mixed(rp):
    db = rp[0]
    one, two, swap = mixed_pairs()
    want = rule_of.oracle_pe_rpbat(db, one[1], two[1])
    return one, two, swap, want


@pytest.mark.parametrize("k", [2, 50])
@pytest.mark.parametrize("b", [2, 5000])
@pytest.mark.parametrize("m", [0, 2, 6])
def test_mixed_library_follows_the_rule(rp, m, b, k):
    db, idx, _ = rp
    one, two, swap = mixed_pairs()
    rec, conv, rule, short = rule_of.oracle_pe_rpbat(db, one[1], two[1], m=m, b=b, k=k)
    got, gconv, st = idx.map_pe_rpbat_batch(*pack(one[1]), *pack(two[1]), max_mismatches=m, b=b, top_k=k)
    rule_of.compare(got, gconv, rec, conv, "m=%d b=%d k=%d" % (m, b, k))
    assert (int(st[0]["too_short"]), int(st[1]["too_short"])) == short
    if m >= 2:  # both orientations decide a large share of this library
        n = len(rule)
        assert (rule == 2).sum() > n // 5 and (rule == 3).sum() > n // 5, np.bincount(rule)
        # the swapped pairs are the ones orientation A pairs
        assert (swap[rule == 3]).mean() > 0.9 and (~swap[rule == 2]).mean() > 0.9
    # the work counters are the sums over both orientations
    _, sp = idx.map_pe_batch(*pack(one[1]), *pack(two[1]), max_mismatches=m, b=b, top_k=k)
    for j in (0, 1):
        assert int(st[j]["probes"]) > int(sp[j]["probes"]) > 0


def planted_genome(tmp, seed=7):
    """A FASTA and pairs for every rule: A/T-only fragments (no informative C or G: the same pair in both orientations,
    rule 1), bisulfite fragments read T-first (rule 2) or A-first (rule 3), an A/T fragment present twice (ambiguous in
    both orientations, rule 4), and mates that do not pair in either orientation (rule 5)."""
    rng = random.Random(seed)

    def rnd(n, al="ACGT"):
        return "".join(rng.choice(al) for _ in range(n))

    body, pairs = [rnd(2000)], []
    for _ in range(3):  # rule 1
        f = rnd(300, "AT")
        body += [f, rnd(700)]
        pairs.append((f[:100], refio.revcomp(f[-100:])))
    for t in range(6):  # rules 2 / 3
        f = rnd(300)
        body += [f, rnd(700)]
        m1 = f[:100].replace("C", "T")
        m2 = refio.revcomp(f[-100:].replace("C", "T"))
        pairs.append((m1, m2) if t % 2 == 0 else (m2, m1))
    f = rnd(300, "AT")  # rule 4: the same A/T fragment twice
    body += [f, rnd(700), f, rnd(700)]
    pairs.append((f[:100], refio.revcomp(f[-100:])))
    # An A/T pair at two loci whose copies of mate 1 differ from it by edits that count in one orientation only: a G
    # where mate 1 has an A is a mismatch only where it is mapped C->T (orientation T), a C where it has a T only where
    # it is mapped G->A (orientation A); an A <-> T flip counts in both.  Orientation T: 1 (unique) and 2 mismatches;
    # orientation A: 2 and 2, ambiguous with min_mm 2 but pair_mm 0.  Rule 2 decides the pair; a merge that took
    # pair_mm for the ambiguous orientation would pick rule 3.
    f = rnd(300, "AT")
    a_at = [i for i in range(5, 95) if f[i] == "A"]
    t_at = [i for i in range(5, 95) if f[i] == "T"]

    def edit(flips, a_only, t_only):
        x = list(f)
        for i in t_at[:a_only]:
            x[i] = "C"
        for i in a_at[:t_only]:
            x[i] = "G"
        for i in t_at[-flips:] if flips else []:
            x[i] = "A"
        return "".join(x)
    body += [edit(1, 1, 0), rnd(700), edit(0, 2, 2), rnd(700)]
    pairs.append((f[:100], refio.revcomp(f[-100:])))
    for t in range(4):  # rule 5: each mate maps, but 5000 bases apart; mates exchanged in every other pair
        f1, f2 = rnd(100), rnd(100)
        body += [f1, rnd(5000), f2, rnd(700)]
        m1, m2 = f1.replace("C", "T"), refio.revcomp(f2.replace("C", "T"))
        pairs.append((m1, m2) if t % 2 == 0 else (m2, m1))
    fa = os.path.join(tmp, "pe_rpbat_planted.fa")
    with open(fa, "w") as fh:
        fh.write(">p1\n%s\n>p2\n%s\n" % ("".join(body), rnd(3000)))
    return fa, [p[0] for p in pairs], [p[1] for p in pairs]


def test_every_rule_decides_a_pair(scratch):
    import walt_amd
    fa, s1, s2 = planted_genome(scratch)
    path = os.path.join(scratch, "pe_rpbat_planted.dbindex")
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
    try:
        rec, conv, rule, short = rule_of.oracle_pe_rpbat(db, s1, s2)
        for k in (1, 2, 3, 4, 5):
            assert (rule == k).sum() >= 1, "no pair decided by rule %d: %s" % (k, rule)
        got, gconv, st = idx.map_pe_rpbat_batch(*pack(s1), *pack(s2))
        rule_of.compare(got, gconv, rec, conv, "planted")
        assert (got["best_times"][rule == 4] >= 2).all() and (got["best_times"][rule == 5] == 0).all()
        # the two-locus A/T pair: unique in orientation T with 1 mismatch, ambiguous in orientation A with min_mm 2
        assert rule[10] == 2 and got["best_times"][10] == 1 and got["pair_mm"][10] == 1
        # rule 5: mates of either conversion
        assert {bytes(c).decode() for c in gconv[rule == 5]} == {"TA", "AT"}
    finally:
        idx.close()


@pytest.mark.parametrize("files, m", [(("pe150_1.fastq", "pe150_2.fastq"), 10), (("pe_1.fastq", "pe_2.fastq"), 6)])
def test_other_read_sets(rp, files, m):
    db, idx, _ = rp
    one, two, _ = mixed_pairs(*files, seed=5)
    rec, conv, _, short = rule_of.oracle_pe_rpbat(db, one[1], two[1], m=m, L=2000)
    got, gconv, st = idx.map_pe_rpbat_batch(*pack(one[1]), *pack(two[1]), max_mismatches=m, frag_range=2000)
    rule_of.compare(got, gconv, rec, conv, str(files))
    assert (int(st[0]["too_short"]), int(st[1]["too_short"])) == short


@pytest.mark.parametrize("opts", [{"pe_mode": 0}, {"pe_mode": 1}, {"pe_serial": 1}, {"pe_chunk": 128},
                                  {"pe_chunk": 128, "pe_serial": 1}, {"pe_rounds": 1}, {"pe_rounds": 2},
                                  {"pe_roomy": 0}, {"pe_roomy": 1}, {"pe_lit_fuse": 0}])
def test_schedules_give_the_same_records(rp, mixed, index_options, opts):
    _, idx, _ = rp
    one, two, _, (rec, conv, _, short) = mixed
    index_options(idx, **opts)
    got, gconv, st = idx.map_pe_rpbat_batch(*pack(one[1]), *pack(two[1]))
    rule_of.compare(got, gconv, rec, conv, str(opts))
    assert (int(st[0]["too_short"]), int(st[1]["too_short"])) == short


@pytest.fixture(params=(5, 7))  # per test: the module's other tests run on pattern 3
def pat(request, scratch):
    import walt_amd
    p = request.param
    refio.set_pattern(p)
    walt_amd.set_pattern(p)
    try:
        path = os.path.join(scratch, "pe_rpbat_g1_sp%d.dbindex" % p)
        walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
        db = refio.DbIndex(path)
        idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
        yield p, db, idx
        idx.close()
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)


def test_seed_patterns_5_and_7(pat):
    p, db, idx = pat
    one, two, _ = mixed_pairs("sp_pe_1.fastq", "sp_pe_2.fastq")
    for m in (2, 6):
        rec, conv, _, short = rule_of.oracle_pe_rpbat(db, one[1], two[1], m=m)
        got, gconv, st = idx.map_pe_rpbat_batch(*pack(one[1]), *pack(two[1]), max_mismatches=m)
        rule_of.compare(got, gconv, rec, conv, "pattern %d m=%d" % (p, m))
        assert (int(st[0]["too_short"]), int(st[1]["too_short"])) == short


# ---------------------------------------------------------------- the device form and the error paths
def test_device_form_on_a_side_stream_equals_host_form(rp, mixed, index_options):
    import torch
    import walt_amd
    _, idx, _ = rp
    one, two, _, (rec, conv, _, short) = mixed
    index_options(idx, pe_chunk=200)  # several passes: both pipeline slots and their record arrays
    b1, o1 = pack(one[1])
    b2, o2 = pack(two[1])
    n, L = len(one[1]), max(max(len(s) for s in one[1]), max(len(s) for s in two[1]))
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(x if x.dtype == np.uint8 else x.astype(np.int64)).to(dev) for x in (b1, o1, b2, o2)]
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_conv = torch.zeros(2 * n, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(8, dtype=torch.int64, device=dev)
    ws = idx.pe_rpbat_workspace_bytes(n, L, 50)
    assert ws >= walt_amd.pe_rpbat_workspace_bytes(n, L, 50)
    guard = 1 << 16
    d_ws = torch.full((ws + guard,), 0xA5, dtype=torch.uint8, device=dev)  # guard bytes behind the workspace
    side = torch.cuda.Stream()
    args = [x.data_ptr() for x in d] + [n, L, d_out.data_ptr(), d_conv.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr()]
    with pytest.raises(walt_amd.WaltError) as ei:  # one byte short
        idx.map_pe_rpbat_batch_device(*args, ws - 1, stream=side.cuda_stream)
    assert ei.value.code == walt_amd.WALT_EINVAL
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        idx.map_pe_rpbat_batch_device(*args, ws, stream=side.cuda_stream)
    walt_amd.Index.check_batch(d_ws.data_ptr(), side.cuda_stream)
    side.synchronize()
    got = d_out.cpu().numpy().view(walt_amd.pair_result_dtype)
    gconv = d_conv.cpu().numpy().reshape(n, 2)
    rule_of.compare(got, gconv, rec, conv, "device form vs oracle")
    host, hconv, hst = idx.map_pe_rpbat_batch(b1, o1, b2, o2)
    assert host.tobytes() == got.tobytes() and np.array_equal(hconv, gconv)
    st = d_stats.cpu().numpy()
    assert (int(st[0]), int(st[4])) == short == (int(hst[0]["too_short"]), int(hst[1]["too_short"]))
    assert (d_ws[ws:].cpu().numpy() == 0xA5).all(), "the call wrote behind its workspace"


def test_records_have_zero_padding(rp, mixed):
    _, idx, _ = rp
    one, two, _, _ = mixed
    got, _, _ = idx.map_pe_rpbat_batch(*pack(one[1]), *pack(two[1]))
    raw = np.frombuffer(got.tobytes(), dtype=np.uint32).reshape(len(got), 16)
    assert (raw[:, 13:16] == 0).all()


def test_non_acgt_base_is_refused(rp):
    import walt_amd
    _, idx, _ = rp
    one, two, _ = mixed_pairs()
    s2 = list(two[1][:20])
    s2[7] = s2[7][:30] + "N" + s2[7][31:]
    with pytest.raises(walt_amd.WaltError) as ei:
        idx.map_pe_rpbat_batch(*pack(one[1][:20]), *pack(s2))
    assert ei.value.code == walt_amd.WALT_EBASE


def test_index_without_every_strand_is_refused(rp):
    import walt_amd
    _, _, path = rp
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT)
    try:
        with pytest.raises(walt_amd.WaltError) as ei:
            idx.map_pe_rpbat_batch(*pack(["ACGT" * 25]), *pack(["TTGCA" * 20]))
        assert ei.value.code == walt_amd.WALT_EINVAL
    finally:
        idx.close()


def test_plain_calls_after_random_pbat(rp, mixed):
    db, idx, _ = rp
    one, two, _, _ = mixed
    before, sb = idx.map_pe_batch(*pack(one[1]), *pack(two[1]))
    idx.map_pe_rpbat_batch(*pack(one[1]), *pack(two[1]))
    after, sa = idx.map_pe_batch(*pack(one[1]), *pack(two[1]))
    assert before.tobytes() == after.tobytes() and sb.tobytes() == sa.tobytes()
    want, _, _ = refio.oracle_pe(db, one[1], two[1])
    for f in ("best_times", "frag_len", "pair_mm"):
        assert np.array_equal(after[f], want[f]), f


# ---------------------------------------------------------------- the command line
def write_fq(path, reads):
    with open(path, "w") as f:
        for nm, sq, sc in zip(*reads):
            f.write("@%s\n%s\n+\n%s\n" % (nm, sq, sc))


@pytest.fixture(scope="module")
def cli_rp(scratch, mixed):
    """The product's makedb binary on g1.fa, and the mixed library as two FASTQ files."""
    out = os.path.join(scratch, "pe_rpbat_cli_g1.dbindex")
    env = dict(os.environ, WALT_MAKEDB_SEED="1")
    subprocess.run([MAKEDB_BIN, "-c", os.path.join(refio.GOLDEN, "g1.fa"), "-o", out, "-t", "4"], check=True, env=env,
                   stderr=subprocess.DEVNULL)
    one, two, _, _ = mixed
    fq1, fq2 = os.path.join(scratch, "pe_rpbat_1.fastq"), os.path.join(scratch, "pe_rpbat_2.fastq")
    write_fq(fq1, one)
    write_fq(fq2, two)
    db = refio.DbIndex(out)
    r1 = tuple(list(x) for x in zip(*[(n, s, q) for b in refio.load_fastq_batches(fq1, 10 ** 7) for n, s, q in zip(*b)]))
    r2 = tuple(list(x) for x in zip(*[(n, s, q) for b in refio.load_fastq_batches(fq2, 10 ** 7) for n, s, q in zip(*b)]))
    return out, fq1, fq2, db, r1, r2, rule_of.oracle_pe_rpbat(db, r1[1], r2[1])


def run_cli(index, fq1, fq2, wd, args, out_name):
    os.makedirs(wd, exist_ok=True)
    out = os.path.join(wd, out_name)
    subprocess.run([WALT_BIN, "-i", index, "-1", fq1, "-2", fq2, "-o", out] + args, check=True, cwd=wd,
                   stderr=subprocess.DEVNULL)
    return {fn: open(os.path.join(wd, fn)).read() for fn in sorted(os.listdir(wd))}


def expected_files(db, r1, r2, want, sam):
    """The -RP files built from the rule's records with the refio writers."""
    rec, conv, rule, short = want
    L = 1000
    main = refio.sam_header(db) if sam else ""
    side = {"_1_ambiguous": "", "_1_unmapped": "", "_2_ambiguous": "", "_2_unmapped": ""}
    hist = [0] * (L + 1)
    st = [[0, 0, 0, 0], [0, 0, 0, 0]]
    pairs = [len(rule), 0, 0, 0]
    for i in range(len(rule)):
        m1 = {f: rec["m1." + f][i] for f in rule_of.MATE_FIELDS}
        m2 = {f: rec["m2." + f][i] for f in rule_of.MATE_FIELDS}
        bt = int(rec["best_times"][i])
        nm = r1[0][i]
        ln = 0
        if bt == 1:
            pairs[1] += 1
            if conv[i, 0] == ord("A"):  # rule 3: the fragment from the T-rich mate 2, as -P writes it
                ln, text = refio.pe_frag_mr_line(db, m2, m1, nm, r2[1][i], r2[2][i], r1[1][i], r1[2][i], L)
            else:
                ln, text = refio.pe_frag_mr_line(db, m1, m2, nm, r1[1][i], r1[2][i], r2[1][i], r2[2][i], L)
            hist[ln] += 1
            if not sam:
                main += text
        else:
            pairs[2 if bt >= 2 else 3] += 1
            for j, m in enumerate((m1, m2)):
                t = int(m["times"])
                st[j][0] += 1
                st[j][1 if t == 1 else 2 if t >= 2 else 3] += 1
            if not sam:
                for j, (m, r) in enumerate(((m1, r1), (m2, r2))):
                    a, b_, c = refio.se_mr_route(db, m, nm, r[1][i], r[2][i], conv[i, j] == ord("A"), True, True)
                    main += a
                    side["_%d_ambiguous" % (j + 1)] += b_
                    side["_%d_unmapped" % (j + 1)] += c
        if sam:
            text = refio.pe_sam_lines(db, m1, m2, bt == 1, ln, nm, r1[1][i], r1[2][i], r2[1][i], r2[2][i], True, True)
            lines = text.splitlines(True)
            tags = ["\tCV:A:%s\n" % chr(conv[i, j]) for j in (0, 1)]  # (-a -u: both mates have a line)
            main += "".join(l[:-1] + tags[k] for k, l in enumerate(lines))
    mates = [(s[0], s[1], s[2], s[3], short[j]) for j, s in enumerate(st)]
    stats = refio.pe_mapstats(pairs, mates[0], mates[1], hist) + "\n"
    base = "out.sam" if sam else "out.mr"
    files = {base: main, base + ".mapstats": stats}
    if not sam:
        files.update({base + k: v for k, v in side.items()})
    return files


def assert_files(got, want):
    assert sorted(got) == sorted(want)
    for fn in want:
        if got[fn] != want[fn]:
            for i, (a, b) in enumerate(zip(got[fn].splitlines(), want[fn].splitlines())):
                assert a == b, "%s line %d:\n got: %s\nwant: %s" % (fn, i + 1, a, b)
            assert got[fn] == want[fn], fn


def by_name(files, sam):
    """(read name, mate) -> (file, line) over every output file of a run."""
    out = {}
    for fn, text in files.items():
        if fn.endswith(".mapstats"):
            continue
        for line in text.splitlines():
            if not line or line.startswith("@"):
                continue
            f = line.split("\t")
            if sam:
                key = (f[0], 1 if int(f[1]) & 0x40 else 2)
            elif fn.endswith("_unmapped"):
                key = (f[0], fn)
            else:
                key = (f[3], fn, f[1])
            out.setdefault(key, []).append(line)
    return out


@pytest.mark.parametrize("sam", [False, True])
def test_cli_random_pbat_pe_files(cli_rp, scratch, sam):
    index, fq1, fq2, db, r1, r2, want = cli_rp
    args = (["-sam"] if sam else []) + ["-a", "-u", "-RP"]
    name = "out.sam" if sam else "out.mr"
    got = run_cli(index, fq1, fq2, os.path.join(scratch, "pe_rpbat_cli_%d" % sam), args, name)
    exp = expected_files(db, r1, r2, want, sam)
    assert_files(got, exp)
    two = run_cli(index, fq1, fq2, os.path.join(scratch, "pe_rpbat_cli_g00_%d" % sam), args + ["-g", "0,0"], name)
    assert two == got
    # pairs decided by rules 1-2 are written as the plain run writes them, rule-3 pairs as the -P run does
    rule = want[2]
    flags = (["-sam"] if sam else []) + ["-a", "-u"]
    plain = run_cli(index, fq1, fq2, os.path.join(scratch, "pe_rpbat_plain_%d" % sam), flags, name)
    pbat = run_cli(index, fq1, fq2, os.path.join(scratch, "pe_rpbat_pbat_%d" % sam), flags + ["-P"], name)
    strip = {fn: t.replace("\tCV:A:T", "").replace("\tCV:A:A", "") for fn, t in got.items()}
    mine, ref = by_name(strip, sam), {2: by_name(plain, sam), 3: by_name(pbat, sam)}
    names = set(r1[0][i] for i in range(len(rule)) if rule[i] in (1, 2, 3))
    which = {r1[0][i]: (3 if rule[i] == 3 else 2) for i in range(len(rule)) if rule[i] in (1, 2, 3)}
    checked = 0
    for key, lines in mine.items():
        nm = key[0].replace("FRAG:", "")
        if nm not in names:
            continue
        assert ref[which[nm]].get(key) == lines, (key, lines, ref[which[nm]].get(key))
        checked += 1
    assert checked > len(rule) // 2
