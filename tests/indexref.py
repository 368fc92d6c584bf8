"""A plain numpy restatement of the reference's BuildIndex (makedb.cpp:46-85), written from its semantics and sharing
no code with the two builders under test (walt_amd/csrc/host_index.cpp, build_index.hip) or with the canonicalising
helpers of the older builder tests.

TEST INFRASTRUCTURE ONLY -- a helper module for tests/test_index_builders_cpu.py and tests/test_gpu_builder_edges.py.

Per strand file (CT00, CT01, GA10, GA11):
  * the strand genome: every chromosome reverse-complemented in place for the two reverse strands
    (ReverseComplementGenome, reference.cpp:131-146), then C->T or G->A (148-162);
  * the bucket histogram (CountBucketSize, 192-207): position j is hashed when its chromosome has at least
    MINIMALSEEDLEN bases and j < chromosome end - MINIMALSEEDLEN; the bucket is getHashValue (util.hpp:175-182),
    the first 12 care characters, 2 bits each (A 0, C 1, G 2, T 3), first character most significant;
  * the erased buckets: every bucket of 500,000 or more positions is emptied (211-218);
  * counter[4^12 + 1]: the exclusive prefix sum of what is left (220-228);
  * index[]: bucket by bucket, each bucket sorted by SortHashTableBucketCMP (258-288).  That comparator walks the care
    characters 12 .. F2CAREDPOSITION_SIZE-1; at the first one it returns "not less" when the second position has run
    out of its chromosome, else "less" when the first has, else compares the two letters.  That is the lexicographic
    order of one digit per care character, 0 for "beyond the chromosome end" and the letter itself otherwise, and
    two positions are equivalent exactly when all their digits are equal (once a position has run out, every later
    care character has too).  The order std::sort leaves inside such a run is unspecified; here it is ascending
    position, and `ties` marks the entries of every run of two or more.

Care positions per seed pattern come from the data dumps of the reference header (tests/golden/seedpattern{3,5,7}.json,
tests/golden/make_seedtab_golden.py).
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

KEY_WEIGHT = 12  # F2SEEDKEYWEIGHT
NUM_BUCKETS = 4 ** KEY_WEIGHT
ERASE_AT = 500000  # reference.cpp:212
MINIMALSEEDLEN = {3: 36, 5: 30, 7: 21}  # seedpattern.hpp:360, 231, 34
STRANDS = ("CT00", "CT01", "GA10", "GA11")

_care = {}


def care_positions(pattern):
    if pattern not in _care:
        with open(os.path.join(GOLDEN, "seedpattern%d.json" % pattern)) as f:
            _care[pattern] = [int(x) for x in json.load(f)["F2CAREDPOSITION"]]
    return _care[pattern]


class StrandRef:
    """genome (uint8 ASCII), hist (uint32[4^12], before the erase), erased (sorted bucket numbers), counter
    (uint32[4^12+1]), index (uint32, canonical order), ties (bool per index entry), run_id (a number per
    index entry that changes exactly where (bucket, digits) changes), zero_digit (bool per index entry:
    its key holds a 0 digit), index_size"""


class IndexRef:
    """names, lengths (uint32), start (int64[n+1]), genome_len, strand[4] (StrandRef), max_index_size"""


_COMPLEMENT = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMPLEMENT[_a] = _b
_BITS = np.full(256, 255, dtype=np.uint8)
for _i, _a in enumerate(b"ACGT"):
    _BITS[_a] = _i


def _as_bytes(seq):
    a = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    assert a.size == 0 or (_BITS[a] != 255).all(), "the restatement takes upper-case ACGT only"
    return a


def strand_genome(chroms, strand):
    """chroms: list of uint8 arrays -> the concatenated genome of strand file `strand` (0..3)"""
    parts = []
    for c in chroms:
        if strand & 1:
            c = _COMPLEMENT[c[::-1]]
        parts.append(c)
    g = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    g = g.copy()
    if strand < 2:
        g[g == ord("C")] = ord("T")
    else:
        g[g == ord("G")] = ord("A")
    return g


def hashed_positions(start, min_seed_len):
    """ascending positions the reference hashes: chromosomes of at least MINIMALSEEDLEN bases, j < end - MINIMALSEEDLEN"""
    runs = []
    for i in range(len(start) - 1):
        lo, hi = int(start[i]), int(start[i + 1])
        if hi - lo < min_seed_len:
            continue
        runs.append(np.arange(lo, hi - min_seed_len, dtype=np.int64))
    return np.concatenate(runs) if runs else np.zeros(0, dtype=np.int64)


def hash_values(genome, pos, care):
    h = np.zeros(pos.size, dtype=np.int64)
    for k in range(KEY_WEIGHT):
        h = h * 4 + _BITS[genome[pos + care[k]]]
    return h


def build_strand(chroms, start, strand, pattern=3, want_index=True):
    care = care_positions(pattern)
    r = StrandRef()
    r.genome = strand_genome(chroms, strand)
    pos = hashed_positions(start, MINIMALSEEDLEN[pattern])
    h = hash_values(r.genome, pos, care)
    hist = np.bincount(h, minlength=NUM_BUCKETS).astype(np.int64)
    r.hist = hist.astype(np.uint32)
    r.erased = np.nonzero(hist >= ERASE_AT)[0]
    kept_hist = hist.copy()
    kept_hist[r.erased] = 0
    counter = np.zeros(NUM_BUCKETS + 1, dtype=np.int64)
    counter[1:] = np.cumsum(kept_hist)
    r.counter = counter.astype(np.uint32)
    r.index_size = int(counter[-1])
    if not want_index:
        return r
    keep = kept_hist[h] > 0
    pos, h = pos[keep], h[keep]
    # one digit per care character 12..: 0 beyond the chromosome end, else the letter (A < C < G < T as in ASCII)
    end = start[np.searchsorted(start, pos, side="right")]
    room = end - pos
    gpad = np.concatenate([r.genome, np.zeros(care[-1] + 1, dtype=np.uint8)])
    ncols = len(care) - KEY_WEIGHT
    # 8 digits (one byte each) per 64-bit word, the earlier care character more significant; the words compare like the digits
    words = []
    for w0 in range(0, ncols, 8):
        w = np.zeros(pos.size, dtype=np.uint64)
        for q in range(w0, w0 + 8):
            w <<= np.uint64(8)
            if q < ncols:
                cp = care[KEY_WEIGHT + q]
                w |= np.where(cp < room, gpad[pos + cp], 0).astype(np.uint64)
        words.append(w)
    order = np.lexsort([pos] + words[::-1] + [h])  # the last key is the primary one
    r.index = pos[order].astype(np.uint32)
    same = np.ones(max(pos.size - 1, 0), dtype=bool)  # entry i and entry i+1 have equal (bucket, digits)
    for k in [h] + words:
        ks = k[order]
        same &= ks[1:] == ks[:-1]
    r.ties = np.zeros(pos.size, dtype=bool)
    r.ties[1:] |= same
    r.ties[:-1] |= same
    r.run_id = np.concatenate([[0], np.cumsum(~same)]).astype(np.int64) if pos.size else np.zeros(0, dtype=np.int64)
    r.zero_digit = (room <= care[-1])[order]
    return r


def build(seqs, pattern=3, strands=(0, 1, 2, 3), want_index=True):
    """seqs: list of (name, upper-case ACGT sequence)"""
    ref = IndexRef()
    ref.pattern = pattern
    ref.names = [n for n, _ in seqs]
    chroms = [_as_bytes(s) for _, s in seqs]
    ref.lengths = np.array([c.size for c in chroms], dtype=np.uint32)
    ref.start = np.zeros(len(chroms) + 1, dtype=np.int64)
    ref.start[1:] = np.cumsum(ref.lengths.astype(np.int64))
    ref.genome_len = int(ref.start[-1])
    ref.strand = [None] * 4
    for s in strands:
        ref.strand[s] = build_strand(chroms, ref.start, s, pattern, want_index)
    ref.max_index_size = max([ref.strand[s].index_size for s in strands] + [0])  # makedb.cpp:82-84
    return ref


def same_up_to_ties(got_index, ref):
    """ref: StrandRef.  True when got_index equals ref.index outside tie runs and is a permutation of it inside each
    run.  Runs of different keys may touch in ref.index, so entries are kept to their own run by ref.run_id, which
    comes from the restatement's keys and never from the builder under test."""
    got = np.asarray(got_index)
    if got.shape != ref.index.shape:
        return False
    m = ref.ties
    if not np.array_equal(got[~m], ref.index[~m]):
        return False
    order = np.lexsort([got[m], ref.run_id[m]])
    return np.array_equal(got[m][order], ref.index[m])  # ref.index is (run, ascending position) already


def ascending_in_tie_runs(got_index, ref):
    """the GPU builder's stronger promise: inside every tie run the positions ascend"""
    got = np.asarray(got_index).astype(np.int64)
    step = np.diff(got)
    inside = ref.run_id[1:] == ref.run_id[:-1]
    return bool((step[inside] > 0).all())


# ---------------------------------------------------------------------------
# Genomes the builder tests make (seeded; none is stored).  Each returns a list of (name, sequence); the tests
# assert what a recipe promises on the restatement before any builder is consulted.
# ---------------------------------------------------------------------------
def random_sequence(rs, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, n)].tobytes().decode()


def genome_erase(seed=20):
    """About 1.1 Mbp in three sequences: a poly-T run in the first, a poly-A run in the third, random elsewhere.  The
    run lengths are solved from the restatement's own CT00 histogram (the random flanks feed both buckets too) so that
    the all-T bucket holds exactly 500,000 positions -- erased -- and the all-A bucket exactly 499,999 -- kept.  A base
    more in the middle of a run adds exactly one position to its bucket, so one correction step is exact.
    Returns (seqs, {"T": (sequence number, offset, length), "A": ...})."""
    rs = np.random.RandomState(seed)
    flank = [random_sequence(rs, n) for n in (41003, 30011, 12345, 11007, 7001)]

    def make(rt, ra):
        return [("polyT", flank[0] + "T" * rt + flank[1]), ("plain", flank[2]), ("polyA", flank[3] + "A" * ra + flank[4])]

    rt = ra = ERASE_AT
    for _ in range(3):
        hist = build(make(rt, ra), 3, strands=(0,), want_index=False).strand[0].hist
        d_t, d_a = ERASE_AT - int(hist[NUM_BUCKETS - 1]), ERASE_AT - 1 - int(hist[0])
        if d_t == 0 and d_a == 0:
            return make(rt, ra), {"T": (0, len(flank[0]), rt), "A": (2, len(flank[3]), ra)}
        rt, ra = rt + d_t, ra + d_a
    raise AssertionError("genome_erase: the run lengths did not settle")


def genome_edges(seed=21):
    """Under 50 kbp: sequences of 1, 20, 35, 36, 37, 38, 51 and 100 bases between sequences of 300 to 2,000 bases; the
    second sequence starts at a position that is 15 mod 16, the total is no multiple of 16, the last sequence has 37
    bases.  The short sequences from 37 bases on repeat the start of the long sequence before them, so that their few
    entries share buckets with entries that have all their room."""
    rs = np.random.RandomState(seed)
    seqs = []
    for i, short in enumerate((1, 20, 35, 36, 37, 38, 51, 100, 37)):
        n = 655 if i == 0 else int(rs.randint(300, 2001))
        if i == 8:
            so_far = sum(len(s) for _, s in seqs)
            while (so_far + n + short) % 16 == 0:
                n += 1
        big = random_sequence(rs, n)
        seqs.append(("long%d" % i, big))
        seqs.append(("short%d_%d" % (i, short), big[:short] if short >= 37 else random_sequence(rs, short)))
    return seqs


def ladder_lengths(pattern):
    """cut lengths of genome_ends: from the shortest sequence with one hashed position up to 236 bases (for pattern 3
    that is 37..236, and 236 = the last care position + 58), so that position 0 of the cuts runs out of room at
    every care character from 12 to the last"""
    return list(range(MINIMALSEEDLEN[pattern] + 1, max(236, care_positions(pattern)[-1] + 58) + 1))


def genome_ends(seed=22, pattern=3):
    """One 240-base sequence cut to every length of ladder_lengths() (position 0 of all cuts lies in one bucket, at every
    distance from a chromosome end), 50 exact duplicates of cuts (tie runs), and 2,000 sequences of 40..80 bases
    (more than 1,023 sequences in the chromosome look-up)."""
    rs = np.random.RandomState(seed)
    base = random_sequence(rs, 240)
    lengths = ladder_lengths(pattern)
    seqs = [("cut%d" % n, base[:n]) for n in lengths]
    for i, k in enumerate(rs.randint(0, len(lengths) // 2, 50)):
        seqs.append(("dup%d_%d" % (i, lengths[k]), base[:lengths[k]]))
    for i in range(2000):
        n = 40 + (i * 7 % 41 if i % 4 == 0 else i % 3)
        seqs.append(("s%d" % i, random_sequence(rs, n)))
    return seqs


def genome_tiefree(seed=23):
    """About 200 kbp of random sequence in five sequences; the tests assert that it has no tie run."""
    rs = np.random.RandomState(seed)
    return [("r%d" % i, random_sequence(rs, n)) for i, n in enumerate((70001, 50, 64013, 3999, 62000))]


def write_fasta(path, seqs, width=100):
    with open(path, "w") as f:
        for name, s in seqs:
            f.write(">%s\n" % name)
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")


RECIPES = {"erase": lambda pattern: genome_erase()[0], "edges": lambda pattern: genome_edges(),
           "ends": lambda pattern: genome_ends(pattern=pattern), "tiefree": lambda pattern: genome_tiefree()}


def assert_recipe(name, ref):
    """What a genome's recipe promises, asserted on the restatement alone: a genome that drifts fails here, loudly,
    instead of testing nothing."""
    lengths = ref.lengths.tolist()
    if name == "erase":
        assert len(lengths) == 3 and 1000000 < ref.genome_len < 1200000
        ct00 = ref.strand[0]
        assert int(ct00.hist[NUM_BUCKETS - 1]) == ERASE_AT, "all-T bucket of CT00: %d" % ct00.hist[NUM_BUCKETS - 1]
        assert int(ct00.hist[0]) == ERASE_AT - 1, "all-A bucket of CT00: %d" % ct00.hist[0]
        for s in range(4):
            assert ref.strand[s].erased.size == 1, "strand %d erases %s" % (s, ref.strand[s].erased)
            assert ref.strand[s].index_size == int(ref.strand[s].hist.sum()) - int(ref.strand[s].hist.max())
        assert ref.strand[0].erased[0] == ref.strand[1].erased[0] == NUM_BUCKETS - 1  # the runs swap roles
        assert ref.strand[2].erased[0] == ref.strand[3].erased[0] == 0
    elif name == "edges":
        assert ref.genome_len < 50000 and ref.genome_len % 16 != 0 and lengths[-1] == 37
        assert set((1, 20, 35, 36, 37, 38, 51, 100)) <= set(lengths)
        assert (ref.start[:-1] % 16 == 15).any()
        for s in range(4):
            assert ref.strand[s].erased.size == 0
    elif name == "ends":
        care = care_positions(ref.pattern)
        assert len(lengths) > 2048 and lengths[:len(ladder_lengths(ref.pattern))] == ladder_lengths(ref.pattern)
        # some cut's position 0 runs out of room exactly at care character q, for every q that a hashed position can
        # run out at (pattern 3: from 12 on; a hashed position of patterns 5 and 7 always has room for character 12)
        for q in range(KEY_WEIGHT, len(care)):
            if care[q] <= MINIMALSEEDLEN[ref.pattern]:
                continue
            assert any(care[q - 1] < n <= care[q] for n in ladder_lengths(ref.pattern)), q
        for s in range(4):
            assert int(ref.strand[s].ties.sum()) >= 100 and int(ref.strand[s].zero_digit.sum()) >= 100
    elif name == "tiefree":
        assert 190000 < ref.genome_len < 210000
        for s in range(4):
            assert not ref.strand[s].ties.any() and ref.strand[s].erased.size == 0
    else:
        raise KeyError(name)
