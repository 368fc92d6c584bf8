"""Minimum base quality (include/walt_amd.h, "minimum base quality"), the parts that need no device: the mask function and
what the quality instances of the calling and evidence kernels run per lane (walt_amd/csrc/meth_core.h, variants_core.h),
compiled with g++ (tests/qual_harness.cpp) and compared with the pure-Python restatement of tests/test_gpu_qual.py; the
same code under the host's sanitizers as a stand-alone program; the pieces of bin/walt -MQ in hostio.h; the exports of the
three libraries and the binding's surface; bin/walt's refusals; and a check that the golden libraries hold what the
command-line tests on the device count on."""
import ctypes
import inspect
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_meth import expected_read
from test_gpu_overlap import counts_of, drop_letters
from test_gpu_qual import LENGTHS, MQ, expected_evidence_q, masked_xm, qual_letters, qual_pool
from test_gpu_variants import expected_evidence
from test_trim_cpu import genome, limit_of, make_read, trim_letters  # noqa: F401  (genome: a fixture)

NAMES = ("walt_meth_pileup_batch_qual", "walt_meth_pileup_batch_qual_device", "walt_meth_nonconv_batch_qual",
         "walt_meth_nonconv_batch_qual_device")
WALT = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
CSRC = os.path.join(refio.ROOT, "walt_amd", "csrc")
FLOORS = (0, 1, 2, 33, 35, 53, 64, 74, 126, 127)


@pytest.fixture(scope="module")
def harness(scratch):
    so = os.path.join(scratch, "libqual_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                    os.path.join(refio.HERE, "qual_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.qual_harness_mask.argtypes = [vp, u32]
    L.qual_harness_mask.restype = u32
    L.qual_harness_read.argtypes = [vp, u32, vp, vp, vp, u64, u64, u64, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, vp, vp]
    L.qual_harness_read.restype = None
    L.qual_harness_evidence.argtypes = [vp, u32, vp, vp, u64, u64, u64, u32, u32, u32, u32, u32, ci, u32, vp, vp]
    L.qual_harness_evidence.restype = ctypes.c_longlong
    L.qual_harness_parse.argtypes = [ctypes.c_char_p, ci, vp]
    L.qual_harness_floor.argtypes = [u32, u32, vp]
    L.qual_harness_line.argtypes = [u32, u32, vp, u32]
    L.qual_harness_line.restype = u32
    L.qual_harness_load.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ci, ci, vp, vp, u64, vp, u32, vp, u32]
    L.qual_harness_load.restype = ctypes.c_longlong
    return L


# ---------------------------------------------------------------------------
# the mask function
# ---------------------------------------------------------------------------
def mask_of(raw, t):
    return sum(1 << (2 * k) for k in range(16) if raw[k] >= t)


def test_mask_function_every_byte_value_at_every_position(harness):
    """every byte value 0 .. 255 at each of the 16 positions, among neighbours of 0, of 255 and of the value itself, against
    the ten floors and a per-byte compare; random slices on top"""
    for t in FLOORS:
        for k in range(16):
            for v in range(256):
                for around in (0, 255, v, 127, 128):
                    raw = bytearray([around] * 16)
                    raw[k] = v
                    qd = np.frombuffer(bytes(raw), dtype=np.uint32).copy()
                    assert harness.qual_harness_mask(qd.ctypes.data, t) == mask_of(raw, t), (t, k, v, around)
    rng = random.Random(3)
    for trial in range(20000):
        t = rng.choice(FLOORS)
        raw = bytes(rng.choice(qual_pool(t)) if rng.random() < 0.7 else rng.randrange(256) for _ in range(16))
        qd = np.frombuffer(raw, dtype=np.uint32).copy()
        assert harness.qual_harness_mask(qd.ctypes.data, t) == mask_of(raw, t), (t, raw)
    # a floor of 0 keeps everything, bytes of 128 and more pass 127
    assert mask_of(bytes(16), 0) == 0x55555555 and mask_of(bytes([128] * 16), 127) == 0x55555555 and mask_of(bytes([126] * 16), 127) == 0


# ---------------------------------------------------------------------------
# what the calling kernel's quality instances run per lane
# ---------------------------------------------------------------------------
def harness_read(L, ref, seq, quals, conv, pos, lo, hi, limit, ex, trim, t, shift, off, tail):
    """the read between two neighbours full of callable bases of full quality (none where off / tail is 0); the quality
    array has exactly batch_bytes elements, the calls array sits at address 16 k + shift"""
    n = len(seq)
    batch_bytes = off + n + tail
    bases = np.full(batch_bytes + 32, ord("C" if conv == "T" else "G"), dtype=np.uint8)
    bases[off:off + n] = np.frombuffer(seq.encode(), dtype=np.uint8)
    bases[batch_bytes:] = 0
    q = np.full(batch_bytes, 255, dtype=np.uint8)
    if quals is not None:
        q[off:off + n] = np.frombuffer(bytes(quals), dtype=np.uint8)
    raw = np.full(batch_bytes + 64, 0x23, dtype=np.uint8)
    a16 = (-raw.ctypes.data) % 16 + shift
    counts = np.zeros(8, dtype=np.uint16)
    cmu = np.zeros(n, dtype=np.uint8)
    L.qual_harness_read(ref.ctypes.data, ref.size - 1, bases.ctypes.data, q.ctypes.data if quals is not None else None,
                        raw.ctypes.data + a16, off, n, batch_bytes, limit, pos, lo, hi, 1 if conv == "A" else 0, ex[0], ex[1], trim[0],
                        trim[1], t, counts.ctypes.data, cmu.ctypes.data)
    assert (raw[:a16 + off] == 0x23).all() and (raw[a16 + off + n:] == 0x23).all(), "wrote outside the read"
    return raw[a16 + off:a16 + off + n].tobytes().decode(), counts.tolist(), cmu.tolist()


def compositions(n):
    """(call_len, excluded interval, bounds) a floor is composed with"""
    return [(None, (0, 0), (0, 0)), (n // 2, (0, 0), (0, 0)), (None, (n // 3, n // 3 + max(n // 4, 1)), (0, 0)), (None, (0, 0), (3, 4)),
            (max(n - 2, 0), (1, 1 + n // 5), (2, 1))]


@pytest.mark.parametrize("length", LENGTHS)
def test_slices_with_qualities_equal_the_restatement(harness, genome, length):
    """each length at every head alignment, first, in the middle and last in its batch (both byte-by-byte paths and the
    16-byte loads), both conversions, both strands, composed with call_len, an excluded interval and both bounds, quality
    bytes from {0, t - 1, t, t + 1, 127, 128, 255}; the calls, the counts and the pile-up's flags"""
    start, texts, R, refs = genome
    rng = random.Random(1000 + length)
    lost = kept = emptied = trial = 0
    places = ((0, 40), (29, 40), (29, 0), (0, 0), (16, 16))
    for conv in "TA":
        for strand in (b"+", b"-"):
            o = 1 if strand == b"-" else 0
            lo, hi = int(start[5]), int(start[6])
            for off, tail in places:
                for call_len, ex, trim in compositions(length):
                    pos = rng.choice([rng.randrange(lo, hi - length), hi - length, hi - max(length // 2, 1)])
                    seq = make_read(rng, texts[o], pos, length, conv)
                    plain, _ = expected_read(R, start, seq, pos, 1, strand, conv, call_len)
                    limit = limit_of(length, call_len)
                    composed = trim_letters(drop_letters(plain, [j for j in range(ex[0], min(ex[1], length))]), limit, *trim)
                    for shift in range(16):
                        t = FLOORS[trial % len(FLOORS)]
                        trial += 1
                        quals = bytes(rng.choice(qual_pool(t)) for _ in range(length))
                        want = qual_letters(composed, quals, t)
                        got, counts, cmu = harness_read(harness, refs[o], seq, quals, conv, pos, lo, hi, limit, ex, trim, t, shift, off, tail)
                        what = "len %d conv %s strand %s off %d tail %d shift %d floor %d %s" % (length, conv, strand, off, tail, shift, t,
                                                                                                  (call_len, ex, trim))
                        assert got == want, "%s\n got  %s\n want %s\n qual %s" % (what, got, want, list(quals))
                        assert counts == counts_of(want), what
                        assert cmu == [0 if ch == "." else 1 if ch.isupper() else 2 for ch in want], what
                        lost += sum(a != b for a, b in zip(composed, want))
                        kept += sum(ch != "." for ch in want)
                        emptied += set(want) == {"."} and set(composed) != {"."}
                    # a floor of 0 over any qualities, and no qualities at all, are the plain instance byte for byte
                    none = harness_read(harness, refs[o], seq, None, conv, pos, lo, hi, limit, ex, trim, 0, 5, off, tail)
                    zero = harness_read(harness, refs[o], seq, quals, conv, pos, lo, hi, limit, ex, trim, 0, 5, off, tail)
                    assert none == zero and none[0] == composed
    assert lost >= 10 * length ** 0.5 and kept >= 10 * length ** 0.5 and (emptied >= 1 or length > 17), (lost, kept, emptied)


# ---------------------------------------------------------------------------
# what the evidence kernel's quality instance runs per lane
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_evidence_with_qualities_equals_the_restatement(harness, genome, seed):
    start, texts, R, refs = genome
    rng = random.Random(seed)
    glen = len(texts[0])
    got_m, got_o = np.zeros(glen, dtype=np.uint32), np.zeros(glen, dtype=np.uint32)
    want = None
    recs = np.zeros(1, dtype=[("genome_pos", "<u4"), ("times", "<u4"), ("strand", "S1")])
    heads, masked = set(), 0
    for trial in range(1500):
        conv, strand = rng.choice("TA"), rng.choice([b"+", b"-"])
        o = 1 if strand == b"-" else 0
        c = rng.choice([0, 1, 4, 5])
        lo, hi = int(start[c]), int(start[c + 1])
        n = rng.choice(LENGTHS)
        pos = min(max(rng.choice([lo, hi - 1, hi - n, rng.randrange(lo, hi)]), lo), hi - 1)
        seq = list(make_read(rng, texts[o], pos, n, conv))
        for k, ch in enumerate(seq):
            if ch == ("G" if conv == "T" else "C") and rng.random() < 0.3:
                seq[k] = rng.choice("ACGT")
        seq = "".join(seq)
        t = rng.choice(FLOORS)
        quals = bytes(rng.choice(qual_pool(t)) for _ in range(n))
        call_len = rng.choice([None, 0, 1, 15, 16, 17, n, n + 5])
        limit = limit_of(n, call_len)
        off, tail = rng.choice([(0, 0), (0, 33), (21, 0), (37, 50), (trial % 16, 64)])
        batch_bytes = off + n + tail
        bases = np.full(batch_bytes + 16, ord("G"), dtype=np.uint8)
        base_at = (-bases.ctypes.data) % 16  # (any head: the slices are cut at the bases' own 16-byte boundaries)
        bases = bases[base_at:base_at + batch_bytes] if base_at + batch_bytes <= bases.size else bases[:batch_bytes]
        bases[off:off + n] = np.frombuffer(seq.encode(), dtype=np.uint8)
        q = np.full(batch_bytes, 255, dtype=np.uint8)
        q[off:off + n] = np.frombuffer(quals, dtype=np.uint8)
        heads.add((bases.ctypes.data + off) % 16)
        adds = harness.qual_harness_evidence(refs[o].ctypes.data, refs[o].size - 1, bases.ctypes.data, q.ctypes.data, off, n, batch_bytes,
                                             limit, pos, lo, hi, 1 if conv == "A" else 0, o, t, got_m.ctypes.data, got_o.ctypes.data)
        assert adds >= 0
        recs["genome_pos"], recs["times"], recs["strand"] = pos, 1, strand
        before = 0 if want is None else int(want[0].sum() + want[1].sum())
        want = expected_evidence_q(R, start, [seq], recs, conv, [quals], t, None if call_len is None else [call_len], into=want)
        assert adds == int(want[0].sum() + want[1].sum()) - before
        assert np.array_equal(got_m, want[0]) and np.array_equal(got_o, want[1]), (trial, conv, strand, pos, n, off, t, call_len)
        plain = expected_evidence(R, start, [seq], recs, conv, None if call_len is None else [call_len])
        masked += int(plain[0].sum() + plain[1].sum()) - adds
    assert len(heads) == 16 and masked > 1000 and int(want[0].sum()) > 2000 and int(want[1].sum()) > 500
    # without a floor the restatement is the one of tests/test_gpu_variants.py
    a = expected_evidence_q(R, start, [seq], recs, conv, None, 0)
    b = expected_evidence(R, start, [seq], recs, conv)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_per_lane_logic_under_the_host_sanitizers(scratch):
    """tests/qual_sanitize_main.cpp, a stand-alone program over tests/qual_harness.cpp built with the host's address and
    undefined-behaviour sanitizers: the quality array and the bases each in a heap block of exactly offsets[n] bytes -- a
    load in front of or behind either ends the program, and so do calls or evidence that differ from a plain walk"""
    exe = os.path.join(scratch, "qual_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(refio.HERE, "qual_sanitize_main.cpp"), os.path.join(refio.HERE, "qual_harness.cpp"), "-o", exe],
                   check=True, timeout=300)
    pr = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert pr.returncode == 0 and pr.stdout.startswith("ok "), pr.stdout[-2000:]
    kept, masked, adds = (int(v) for v in pr.stdout.split()[1:4])
    assert kept > 50000 and masked > 20000 and adds > 50000


# ---------------------------------------------------------------------------
# the host side of bin/walt -MQ
# ---------------------------------------------------------------------------
def test_value_parsers_floor_and_settings_line(harness):
    out = ctypes.c_uint32(0)
    for text, ok in (("1", 1), ("20", 1), ("93", 1), ("0", 0), ("94", 0), ("x", 0), ("", 0), ("2 ", 0), ("-3", 0), ("+5", 0), ("020", 1),
                     ("1e1", 0), ("12345", 0)):
        assert harness.qual_harness_parse(text.encode(), 0, ctypes.byref(out)) == ok, text
        if ok:
            assert out.value == int(text)
    for text, ok in (("33", 1), ("64", 1), ("50", 0), ("0", 0), ("", 0), ("33x", 0), ("65", 0)):
        assert harness.qual_harness_parse(text.encode(), 1, ctypes.byref(out)) == ok, text
    for n, b, ok in ((20, 33, 1), (93, 33, 1), (94 - 31, 64, 1), (64, 64, 0), (93, 64, 0), (1, 64, 1)):
        assert harness.qual_harness_floor(n, b, ctypes.byref(out)) == ok and out.value == n + b
    buf = ctypes.create_string_buffer(64)
    for n, b in ((20, 33), (5, 64)):
        length = harness.qual_harness_line(n, b, buf, 64)
        assert buf.raw[:length] == b"minqual\t%d\t%d\n" % (n, b)


def load_batch(L, fq, adaptor, threads, want_quals=1, cap_reads=5000):
    cap = 1 << 20
    bases, quals = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
    offsets = np.zeros(cap_reads + 1, dtype=np.uint64)
    err = ctypes.create_string_buffer(1024)
    n = L.qual_harness_load(fq.encode(), adaptor.encode(), threads, want_quals, bases.ctypes.data, quals.ctypes.data, cap,
                            offsets.ctypes.data, cap_reads, err, 1024)
    return n, bases, quals, offsets, err.value.decode()


def test_quality_packer(harness, scratch):
    """the loader under -MQ: the quality bytes at the offsets of the bases, in file order, on one thread and on five; -C
    leaves them in place; a quality line of another length is refused by file and read; without -MQ no buffer at all"""
    fq = os.path.join(scratch, "qual_packer.fastq")
    rng = random.Random(9)
    reads = []
    for i in range(37):
        n = rng.choice([1, 15, 16, 17, 40, 100])
        reads.append(("r%d extra" % i, "".join(rng.choice("ACGTN") for _ in range(n)), "".join(chr(rng.randrange(33, 127)) for _ in range(n))))
    reads[5] = (reads[5][0], reads[5][1], "#" * len(reads[5][1]))
    reads[21] = (reads[21][0], "ACGTN" * 8, "I" * 40)
    with open(fq, "w") as f:
        for nm, s, q in reads:
            f.write("@%s\n%s\n+\n%s\n" % (nm, s, q.replace("@", "A")))
    reads = [(nm, s, q.replace("@", "A")) for nm, s, q in reads]
    for threads in (1, 5):
        n, bases, quals, offsets, err = load_batch(harness, fq, "", threads)
        assert n == len(reads), err
        for j, (_, s, q) in enumerate(reads):
            a, b = int(offsets[j]), int(offsets[j + 1])
            assert b - a == len(s) and quals[a:b].tobytes().decode() == q
            assert all(x == y for x, y in zip(bases[a:b].tobytes().decode(), s) if y != "N")
    n, _, _, _, _ = load_batch(harness, fq, "", 2, want_quals=0)
    assert n == 1000000 + len(reads)
    # -C: the adaptor part becomes random bases, the qualities stay
    ad = "AGATCGGAAGAGCACACGTC"
    clip = os.path.join(scratch, "qual_packer_clip.fastq")
    with open(clip, "w") as f:
        f.write("@c0\n%s\n+\n%s\n" % ("ACGTTGCATGCATTGCAACG" + ad, "".join(chr(40 + k) for k in range(40))))
    n, bases, quals, offsets, err = load_batch(harness, clip, ad, 1)
    assert n == 1 and quals[:40].tobytes().decode() == "".join(chr(40 + k) for k in range(40))
    assert bases[:20].tobytes().decode() == "ACGTTGCATGCATTGCAACG" and set(bases[20:40].tobytes().decode()) <= set("ACGT")
    # a quality line one character short, and one too long
    for delta in (-1, 1):
        bad = os.path.join(scratch, "qual_packer_bad%d.fastq" % delta)
        with open(bad, "w") as f:
            for j, (nm, s, q) in enumerate(reads):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, (q + "I")[:len(q) + delta] if j == 21 else q))
        n, _, _, _, err = load_batch(harness, bad, "", 3)
        assert n == -1 and bad in err and "read r21:" in err and "quality line" in err, err
        assert load_batch(harness, bad, "", 3, want_quals=0)[0] == 1000000 + len(reads)  # without -MQ the file loads as it always did


# ---------------------------------------------------------------------------
# exports, binding, command line
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert hdr.index("---- opposite-strand evidence") < hdr.index("---- minimum base quality") < hdr.index("---- options")


def test_binding_surface_without_a_device():
    import walt_amd
    methods = (walt_amd.Index.meth_call_batch, walt_amd.Index.meth_call_batch_device, walt_amd.Index.meth_nonconv_batch,
               walt_amd.Index.meth_nonconv_batch_device, walt_amd.Pileup.add_batch, walt_amd.Pileup.add_batch_device,
               walt_amd.Pileup.add_evidence_batch, walt_amd.Pileup.add_evidence_batch_device)
    for fn in methods:  # keyword-only, behind parameter lists that stay what they were
        assert "quals" not in inspect.signature(fn).parameters and "min_qual" in (fn.__doc__ or ""), fn.__name__
    q = walt_amd.pack_quals(["II#", b"\x00\x80\xff", ""])
    assert q.dtype == np.uint8 and q.tolist() == [73, 73, 35, 0, 128, 255]
    assert walt_amd.pack_quals([]).size == 0
    bases, offs = walt_amd.pack_reads(["ACG", "TTT", ""])
    assert walt_amd.pack_quals(["II#", "###", ""]).size == bases.size == int(offs[-1])
    # the form a call with qualities reaches, and the arguments in front of and behind the batch
    L = walt_amd.lib()
    form, head, tail = walt_amd._meth_form(L, False, None, qual=(123, 20))
    assert form is L.walt_meth_pileup_batch_qual and head == (None,) and tail == (None, 1, None, None, 0, 0, 0, None, None, None, 123, 20)
    form, head, tail = walt_amd._meth_form(L, True, 7, skip=(5, 2), ev=(9,), qual=(123, 0))
    assert form is L.walt_meth_pileup_batch_qual_device and head == (7,) and tail == (5, 2, None, None, 0, 0, 0, None, None, 9, 123, 0)
    assert walt_amd._meth_form(L, False, None, ev=(9,))[0] is L.walt_meth_pileup_batch_ev  # without qualities: the form it was


def run(args):
    return subprocess.run([WALT] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_cli_refuses_what_it_cannot_do(tmp_path):
    """the refusals of the option parser: they come before the index is opened, so no device is needed"""
    base = ["-i", str(tmp_path / "none.dbindex"), "-r", str(tmp_path / "none.fastq"), "-o", str(tmp_path / "out")]
    for args, words in ((["-MQ", "20"], ("-MQ", "nothing for it to do")), (["-M", "-MQ", "0"], ("from 1 to 93", '"0"')),
                        (["-M", "-min-qual", "94"], ("from 1 to 93",)), (["-M", "--min-base-quality", "x"], ("from 1 to 93", '"x"')),
                        (["-M", "-MQ"], ("missing value",)), (["-M", "-MQ", "20", "-MQO", "50"], ("33 or 64",)),
                        (["-M", "-MQ", "20", "-qual-offset", "33x"], ("33 or 64",)), (["-M", "--quality-offset", "64"], ("goes with -MQ",)),
                        (["-M", "-MQ", "64", "-MQO", "64"], ("127",))):
        pr = run(base + args)
        assert pr.returncode != 0, args
        for w in words:
            assert w in pr.stdout, (args, w, pr.stdout[-500:])
    # every consumer is one: the parser lets these through (they fail later, at the index that is not there)
    for consumer in (["-M"], ["-MC"], ["-MB"], ["-ML"], ["-MA"], ["-ME"], ["-MV"], ["-MR", str(tmp_path / "x.bed")]):
        pr = run(base + consumer + ["-MQ", "20", "-MQO", "33"])
        assert pr.returncode != 0 and "nothing for it to do" not in pr.stdout and "wants" not in pr.stdout, consumer
    assert "-MQ <n> -MQO <b>" in run([]).stdout


# ---------------------------------------------------------------------------
# the condition the command-line tests on the device carry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,conv", [("se_sam_au", "T"), ("se_ag_sam_au", "A"), ("pe_sam_au", None)])
def test_golden_libraries_lose_a_share_of_their_letters_at_the_floor_of_the_cli_tests(case, conv):
    """the golden SAM of a run walked by the calling rule: at -MQ 20 between 10 % and 90 % of the letters of the run without
    a floor are lost (the golden qualities are uniform over '#' .. 'I', Phred 2 .. 40, so about half should be); and
    -F 3 marks fewer reads with the floor than without, but some"""
    from test_gpu_cpgpairs import read_fasta
    from test_gpu_nonconv import fails, tally_of
    from test_gpu_variants import SAM_SKIP, base_letter
    names, seqs = read_fasta(os.path.join(refio.GOLDEN, "g1.fa"))
    text = "".join(seqs)
    starts = [0]
    for s in seqs:
        starts.append(starts[-1] + len(s))
    letters = lost = reads = marked = marked_plain = 0
    for line in refio.golden_file(case, "out.sam").splitlines():
        if line.startswith("@"):
            continue
        p = line.split("\t")
        flag = int(p[1])
        if flag & SAM_SKIP:
            continue
        c = names.index(p[2])
        pos0, seq, qual, rev = starts[c] + int(p[3]) - 1, p[9], p[10], bool(flag & 0x10)
        cv = conv if conv is not None else ("A" if flag & 0x80 else "T")
        on_c = rev == (cv == "A")  # (tests/test_gpu_variants.py, sam_walk)
        site, kept, conv_to, ahead = ("C", "C", "T", 1) if on_c else ("G", "G", "A", -1)
        xm = []
        for k in range(len(seq)):
            f = pos0 + k
            g, b = text[f] if starts[c] <= f < starts[c + 1] else "N", base_letter(ord(seq[k]))
            if g != site or b not in (kept, conv_to):
                xm.append(".")
                continue
            n1 = text[f + ahead] if starts[c] <= f + ahead < starts[c + 1] else None
            n2 = text[f + 2 * ahead] if starts[c] <= f + 2 * ahead < starts[c + 1] else None
            key = "G" if on_c else "C"
            ch = "u" if n1 is None else "z" if n1 == key else "u" if n2 is None else "x" if n2 == key else "h"
            xm.append(ch.upper() if b == kept else ch)
        xm = "".join(xm)
        with_floor = masked_xm(xm, qual, MQ)
        letters += sum(ch != "." for ch in xm)
        lost += sum(a != b for a, b in zip(xm, with_floor))
        reads += 1
        marked_plain += fails(*tally_of(xm.encode()), (3, 0, 0, 0))
        marked += fails(*tally_of(with_floor.encode()), (3, 0, 0, 0))
    share = lost / letters
    print("%s: %d reads, %d letters, %.1f %% lost at -MQ %d; -F 3 marks %d, %d without the floor" % (case, reads, letters, 100 * share, MQ,
                                                                                                  marked, marked_plain))
    assert reads > 200 and letters > 2000 and 0.10 <= share <= 0.90
    if case == "se_sam_au":
        assert 0 < marked < marked_plain
