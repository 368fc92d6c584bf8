"""PCR-duplicate marking (include/walt_amd.h, "duplicates"), the parts that need no device: the key packing, the
eligibility rules and a sequential table built from walt_amd/csrc/dedup_core.h with g++ (tests/dedup_harness.cpp), against
the plain restatement of the contract below (a Python dict); the header, the libraries' exports, bin/walt -D and the loud
failure without a device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import refio

NAMES = ("walt_dedup_create", "walt_dedup_destroy", "walt_dedup_clear", "walt_dedup_reserve", "walt_dedup_count",
         "walt_dedup_device_bytes", "walt_dedup_batch", "walt_dedup_pairs_batch", "walt_dedup_batch_device",
         "walt_dedup_pairs_batch_device", "walt_meth_pileup_batch_skip", "walt_meth_pileup_batch_skip_device")
EMPTY = (1 << 64) - 1
NO_POS = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# the restatement (imported by tests/test_gpu_dedup.py and tools/soak.py)
# ---------------------------------------------------------------------------
def key_of(kind, conv, strand, aux, pos):
    """the 64-bit key as the header packs it"""
    return ((1 if conv == ord("A") else 0) << 63) | ((1 if strand == ord("-") else 0) << 62) | ((kind & 3) << 60) | \
           ((aux & 0x0FFFFFFF) << 32) | (pos & 0xFFFFFFFF)


def single_key(rec, conv, kind):
    """rec: (genome_pos, times, strand byte); -> key or None (ineligible)"""
    pos, times, strand = int(rec[0]), int(rec[1]), int(rec[2])
    if times != 1 or pos == NO_POS or conv not in (ord("T"), ord("A")):
        return None
    return key_of(kind, conv, strand, 0, pos)


def pair_keys(m1, m2, best_times, frag_len, conv1, conv2):
    """-> [key or None for mate 1, for mate 2]; a unique pair has one key, twice"""
    if int(best_times) == 1:
        if int(m1[0]) == NO_POS or conv1 not in (ord("T"), ord("A")):
            return [None, None]
        k = key_of(3, conv1, int(m1[2]), int(frag_len) & 0x0FFFFFFF, int(m1[0]))
        return [k, k]
    return [single_key(m1, conv1, 1), single_key(m2, conv2, 2)]


class DupRule:
    """first fed wins: a record is a duplicate when its key was seen under a smaller ordinal since the last clear"""

    def __init__(self):
        self.first = {}
        self.fed = 0

    def feed(self, keys_per_record):
        """keys_per_record: per record a list of keys (None: ineligible) that share the record's ordinal -> dup lists"""
        out = []
        for keys in keys_per_record:
            for k in keys:
                if k is not None:
                    self.first.setdefault(k, self.fed)
            self.fed += 1
        base = self.fed - len(keys_per_record)
        for i, keys in enumerate(keys_per_record):
            out.append([1 if (k is not None and self.first[k] != base + i) else 0 for k in keys])
        return out

    def clear(self):
        self.first, self.fed = {}, 0


def rec_fields(recs):
    """best_match_dtype array -> list of (genome_pos, times, strand byte)"""
    return [(int(p), int(t), s[0] if len(s) else 0) for p, t, s in zip(recs["genome_pos"], recs["times"], recs["strand"])]


def expect_single(rule, recs, conv, kind=0):
    """recs: best_match_dtype array; conv: 'T' / 'A' or a uint8 array -> dup uint8[n]"""
    cv = [ord(conv)] * len(recs) if isinstance(conv, str) else [int(c) for c in conv]
    return np.array([d[0] for d in rule.feed([[single_key(r, c, kind)] for r, c in zip(rec_fields(recs), cv)])], dtype=np.uint8).reshape(-1)


def expect_pairs(rule, pairs, conv):
    """pairs: pair_result_dtype array; conv: mate 1's letter for all, or uint8[n, 2] -> dup uint8[n, 2]"""
    n = len(pairs)
    if isinstance(conv, str):
        other = {"T": "A", "A": "T"}.get(conv, conv)
        cv = [(ord(conv), ord(other))] * n
    else:
        cv = [(int(a), int(b)) for a, b in conv]
    m1, m2 = rec_fields(pairs["m1"]), rec_fields(pairs["m2"])
    keys = [pair_keys(m1[i], m2[i], pairs["best_times"][i], pairs["frag_len"][i], cv[i][0], cv[i][1]) for i in range(n)]
    return np.array(rule.feed(keys), dtype=np.uint8).reshape(n, 2)


# ---------------------------------------------------------------------------
# header, exports, binding surface, command line
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [3, 5, 7])
def test_libraries_export_the_dedup_calls(pattern):
    import walt_amd
    L = ctypes.CDLL(walt_amd.lib_path(pattern))
    hdr = open(os.path.join(refio.ROOT, "include", "walt_amd.h")).read()
    for nm in NAMES:
        assert hasattr(L, nm), "%s does not export %s" % (os.path.basename(walt_amd.lib_path(pattern)), nm)
        assert nm + "(" in hdr
    assert "typedef struct walt_dedup walt_dedup;" in hdr and "---- duplicates" in hdr
    assert "2^27" in hdr and "One call at a time per set" in hdr


def test_binding_surface_and_no_device_is_loud():
    import walt_amd
    for nm in ("add_batch", "add_pairs", "add_batch_device", "add_pairs_device", "reserve", "count", "clear", "close", "device_bytes"):
        assert hasattr(walt_amd.Dedup, nm), nm
    import inspect
    assert "skip" in inspect.signature(walt_amd.Pileup.add_batch).parameters
    assert "skip" in inspect.signature(walt_amd.Index.meth_call_batch).parameters
    L = walt_amd.lib()
    for nm in NAMES:
        assert getattr(L, nm).argtypes is not None, nm
    # null handles are refused, not crashed on
    assert L.walt_dedup_create(0, 0, None) == walt_amd.WALT_EINVAL
    assert L.walt_dedup_clear(None) == walt_amd.WALT_EINVAL
    assert L.walt_dedup_reserve(None, 1) == walt_amd.WALT_EINVAL
    assert L.walt_dedup_count(None, None, None) == walt_amd.WALT_EINVAL
    assert L.walt_dedup_device_bytes(None) == 0
    L.walt_dedup_destroy(None)
    assert L.walt_dedup_batch(None, None, 16, None, 0, ord("T"), 0, 0, None) == walt_amd.WALT_EINVAL
    assert L.walt_dedup_pairs_batch(None, None, None, ord("T"), 0, None) == walt_amd.WALT_EINVAL
    assert L.walt_dedup_batch_device(None, None, 16, None, 0, ord("T"), 0, 0, None, None) == walt_amd.WALT_EINVAL
    assert L.walt_dedup_pairs_batch_device(None, None, None, ord("T"), 0, None, None) == walt_amd.WALT_EINVAL
    assert b"walt_dedup_pairs_batch_device" in L.walt_last_error()
    assert L.walt_meth_pileup_batch_skip(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None, None,
                                         0) == walt_amd.WALT_EINVAL
    assert L.walt_meth_pileup_batch_skip_device(None, None, None, None, 0, None, 16, None, 0, ord("T"), None, None, None, None,
                                                None, 0, None) == walt_amd.WALT_EINVAL
    if walt_amd.device_count() > 0:
        return  # (with a device the rest is tests/test_gpu_dedup.py's)
    out = ctypes.c_void_p()
    assert L.walt_dedup_create(0, 64, ctypes.byref(out)) == walt_amd.WALT_EHIP and not out.value
    assert b"no CPU fallback" in L.walt_last_error()
    with pytest.raises(walt_amd.WaltError) as ei:
        walt_amd.Dedup()
    assert ei.value.code == walt_amd.WALT_EHIP


MODES = [["-r", "x.fastq"], ["-r", "x.fastq", "-A"], ["-r", "x.fastq", "-R"], ["-1", "x_1.fastq", "-2", "x_2.fastq"],
         ["-1", "x_1.fastq", "-2", "x_2.fastq", "-P"], ["-1", "x_1.fastq", "-2", "x_2.fastq", "-RP"]]


@pytest.mark.parametrize("sfx", ["", "_sp5", "_sp7"])
def test_cli_accepts_the_option_in_every_mode_and_refuses_huge_fragments(tmp_path, sfx):
    walt = os.path.join(refio.ROOT, "walt_amd", "bin", "walt" + sfx)

    def run(args):
        return subprocess.run([walt] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)

    pr = run([])
    assert pr.returncode == 0 and " -D " in pr.stdout
    out = str(tmp_path / "o.mr")
    for mode in MODES:
        for flag in ("-D", "-dedup", "--remove-duplicates"):
            for extra in ([], ["-M"], ["-MC", "-sam"], ["-g", "0,0"]):
                if flag != "-D" and extra:
                    continue
                # parsed and accepted: the run gets as far as looking for the index, and writes nothing before that
                pr = run([flag, "-i", str(tmp_path / "none.dbindex"), "-o", out] + mode + extra)
                assert pr.returncode != 0 and "index file missing" in pr.stdout, (mode, flag, extra, pr.stdout)
                assert not os.path.exists(out + ".dupstats")
        pr = run(["-D", "-L", "134217728", "-i", str(tmp_path / "none.dbindex"), "-o", out] + mode)
        assert pr.returncode != 0 and "-L" in pr.stdout and "134217728" in pr.stdout and "index file missing" not in pr.stdout, pr.stdout
        pr = run(["-D", "-L", "134217727", "-i", str(tmp_path / "none.dbindex"), "-o", out] + mode)
        assert pr.returncode != 0 and "index file missing" in pr.stdout, pr.stdout
    pr = run(["-L", "134217728", "-i", str(tmp_path / "none.dbindex"), "-o", out, "-r", "x.fastq"])  # without -D nothing changes
    assert "index file missing" in pr.stdout


# ---------------------------------------------------------------------------
# what the kernels run per lane, on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dedup_harness(scratch):
    so = os.path.join(scratch, "libdedup_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", os.path.join(refio.ROOT, "walt_amd", "csrc"),
                    os.path.join(refio.HERE, "dedup_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.dedup_harness_key.argtypes = [u32] * 5
    L.dedup_harness_key.restype = u64
    L.dedup_harness_empty.restype = u64
    L.dedup_harness_hash.argtypes = [u64]
    L.dedup_harness_hash.restype = u64
    L.dedup_harness_round_slots.argtypes = [u64]
    L.dedup_harness_round_slots.restype = u64
    L.dedup_harness_single.argtypes = [u32] * 5 + [ctypes.POINTER(u64)]
    L.dedup_harness_pair.argtypes = [u32] * 7 + [ctypes.c_int32, u32, u32, vp, vp]
    L.dedup_harness_pair.restype = None
    L.dedup_harness_new.argtypes = [u64]
    L.dedup_harness_new.restype = vp
    L.dedup_harness_free.argtypes = [vp]
    L.dedup_harness_free.restype = None
    for nm in ("slots", "occupied", "grown"):
        getattr(L, "dedup_harness_" + nm).argtypes = [vp]
        getattr(L, "dedup_harness_" + nm).restype = u64
    L.dedup_harness_call.argtypes = [vp, vp, vp, u32, vp]
    L.dedup_harness_call.restype = ci
    return L


def test_key_packing_at_the_extremes(dedup_harness):
    H = dedup_harness
    T, A, P, M = ord("T"), ord("A"), ord("+"), ord("-")
    assert H.dedup_harness_empty() == EMPTY
    assert H.dedup_harness_key(0, T, P, 0, 0) == 0
    assert H.dedup_harness_key(0, A, P, 0, 0) == 1 << 63
    assert H.dedup_harness_key(0, T, M, 0, 0) == 1 << 62
    assert H.dedup_harness_key(1, T, P, 0, 0) == 1 << 60
    assert H.dedup_harness_key(2, T, P, 0, 0) == 2 << 60
    assert H.dedup_harness_key(3, T, P, 0, 0) == 3 << 60
    assert H.dedup_harness_key(0, T, P, 1, 0) == 1 << 32
    assert H.dedup_harness_key(0, T, P, 0x0FFFFFFF, 0) == 0x0FFFFFFF << 32
    assert H.dedup_harness_key(0, T, P, 0, 0xFFFFFFFE) == 0xFFFFFFFE
    assert H.dedup_harness_key(3, A, M, 0x0FFFFFFF, 0xFFFFFFFE) == EMPTY - 1
    # every field against the restatement, at random and at the extremes; no field leaks into another
    rng = random.Random(5)
    for _ in range(2000):
        kind, conv, strand = rng.randrange(4), rng.choice([T, A]), rng.choice([P, M])
        aux = rng.choice([0, 1, 0x0FFFFFFF, 0x0FFFFFFE, rng.randrange(1 << 28)])
        pos = rng.choice([0, 1, 0xFFFFFFFE, 0x80000000, rng.randrange(1 << 32)])
        assert H.dedup_harness_key(kind, conv, strand, aux, pos) == key_of(kind, conv, strand, aux, pos)
    # the empty word is unreachable: it would need pos == 0xFFFFFFFF, and that record has no key
    k = ctypes.c_uint64(0)
    for kind in range(3):
        for conv in (T, A):
            for strand in (P, M):
                assert H.dedup_harness_single(NO_POS, 1, strand, conv, kind, ctypes.byref(k)) == 0
                assert H.dedup_harness_single(NO_POS - 1, 1, strand, conv, kind, ctypes.byref(k)) == 1 and k.value != EMPTY
                assert k.value == single_key((NO_POS - 1, 1, strand), conv, kind)
    keys, has = (ctypes.c_uint64 * 2)(), (ctypes.c_uint8 * 2)()
    H.dedup_harness_pair(NO_POS, 1, M, 5, 1, P, 1, -1, A, T, keys, has)
    assert list(has) == [0, 0]
    H.dedup_harness_pair(NO_POS - 1, 1, M, 5, 1, P, 1, -1, A, T, keys, has)  # all fields ones but the last bit
    assert list(has) == [1, 1] and keys[0] == keys[1] == EMPTY - 1
    # ineligible single records: times 0 and 2, a conversion that is no letter
    assert H.dedup_harness_single(7, 0, P, T, 0, ctypes.byref(k)) == 0
    assert H.dedup_harness_single(7, 2, P, T, 0, ctypes.byref(k)) == 0
    assert H.dedup_harness_single(7, 1, P, ord("N"), 0, ctypes.byref(k)) == 0
    assert H.dedup_harness_single(7, 1, P, 0, 0, ctypes.byref(k)) == 0


def test_pair_keys_and_the_aliasing_at_2_27(dedup_harness):
    H = dedup_harness
    T, A, P, M = ord("T"), ord("A"), ord("+"), ord("-")
    keys, has = (ctypes.c_uint64 * 2)(), (ctypes.c_uint8 * 2)()

    def pk(best_times, frag_len, m1=(100, 1, P), m2=(300, 1, M), c1=T, c2=A):
        H.dedup_harness_pair(m1[0], m1[1], m1[2], m2[0], m2[1], m2[2], best_times, frag_len, c1, c2, keys, has)
        got = [keys[i] if has[i] else None for i in range(2)]
        assert got == pair_keys(m1, m2, best_times, frag_len, c1, c2)
        return got

    a = pk(1, 250)
    assert a[0] == a[1] == key_of(3, T, P, 250, 100)
    assert pk(1, 251) != a and pk(1, 250, m1=(101, 1, P)) != a and pk(1, 250, m1=(100, 1, M)) != a and pk(1, 250, c1=A, c2=T) != a
    assert pk(1, 250, m2=(999, 1, P)) == a  # mate 2 enters through the fragment length alone
    # lengths in [-2^27, 2^27) are distinct; 2^27 aliases with -2^27, 2^28 + x with x
    lim = 1 << 27
    assert len({pk(1, v)[0] for v in (0, 1, -1, lim - 1, -lim, 250)}) == 6
    assert pk(1, lim) == pk(1, -lim)
    assert pk(1, (1 << 28) + 5) == pk(1, 5)
    # not a unique pair: lone mates, by mate number and own conversion
    assert pk(0, 0) == [key_of(1, T, P, 0, 100), key_of(2, A, M, 0, 300)]
    assert pk(2, 0, m1=(100, 2, P)) == [None, key_of(2, A, M, 0, 300)]
    assert pk(0, 0, m2=(300, 0, M)) == [key_of(1, T, P, 0, 100), None]
    assert pk(0, 0, m1=(100, 1, P), m2=(100, 1, P), c1=T, c2=T)[0] != pk(0, 0, m1=(100, 1, P), m2=(100, 1, P), c1=T, c2=T)[1]
    assert pk(0, 0)[0] != key_of(0, T, P, 0, 100)  # never a single-end key


def test_hash_and_rounding(dedup_harness):
    H = dedup_harness
    assert [H.dedup_harness_round_slots(v) for v in (0, 1, 63, 64, 65, 4096, 4097)] == [64, 64, 64, 64, 128, 4096, 8192]
    # neighbouring positions do not stay neighbours: 4096 consecutive keys fall into nearly as many slots of 2^16 as random ones would
    slots = {H.dedup_harness_hash(key_of(0, ord("T"), ord("+"), 0, 1000 + i)) & 0xFFFF for i in range(4096)}
    assert len(slots) > 3800


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_sequential_table_equals_the_dict(dedup_harness, seed):
    """random record streams with heavy key repetition, cut into calls at random points, from 64 slots upward"""
    H = dedup_harness
    rng = random.Random(seed)
    n_keys = [5, 40, 3000, 3000][seed - 1]
    pool = [key_of(rng.randrange(4), rng.choice([84, 65]), rng.choice([43, 45]), rng.randrange(1 << 28), rng.randrange(1 << 32))
            for _ in range(n_keys)]
    total = 12000
    stream = []
    for _ in range(total):
        r = rng.random()
        if r < 0.1:
            stream.append([None, None])
        elif r < 0.5:
            k = rng.choice(pool)
            stream.append([k, k] if rng.random() < 0.5 else [k, None])
        else:
            stream.append([rng.choice(pool) if rng.random() < 0.8 else None, rng.choice(pool) if rng.random() < 0.8 else None])
    rule = DupRule()
    want = rule.feed(stream)
    assert sum(map(sum, want)) > total // 3
    t = H.dedup_harness_new(64)
    try:
        assert H.dedup_harness_slots(t) == 64
        got, at = [], 0
        while at < total:
            n = min(total - at, rng.choice([1, 1, 2, 7, 64, 1000, 5000]))
            keys = np.array([[EMPTY if k is None else k for k in rec] for rec in stream[at:at + n]], dtype=np.uint64)
            has = np.array([[k is not None for k in rec] for rec in stream[at:at + n]], dtype=np.uint8)
            dup = np.full((n, 2), 7, dtype=np.uint8)
            assert H.dedup_harness_call(t, keys.ctypes.data, has.ctypes.data, n, dup.ctypes.data) == 0
            got += dup.tolist()
            at += n
        assert got == want
        assert H.dedup_harness_occupied(t) == len(rule.first)
        assert H.dedup_harness_occupied(t) <= H.dedup_harness_slots(t) // 2
        if n_keys == 3000:
            assert H.dedup_harness_grown(t) >= 2 and H.dedup_harness_slots(t) >= 8192
    finally:
        H.dedup_harness_free(t)
