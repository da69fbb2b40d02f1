"""Deterministic read-set generators for fixtures, tests and the bench.

`survey_reads(G, L, N, seed)` reproduces the generator the survey used for its `toy` / `mid`
fixtures (Python `random`, seeds recorded there), so the md5 prefixes
recorded in that appendix can be checked.  `corner`, `rep` and `dup` are the hand-made fixtures
described in the same appendix.  `fast_reads` is the numpy generator bench.py uses at BASELINE sizes
(uniform i.i.d. genome, uniform positions, strand flipped with p=0.5, unique
(pos,strand), names r<i>).
"""
import random

import numpy as np

_TR = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_TR)[::-1]


def survey_reads(G, L, N, seed):
    random.seed(seed)
    g = "".join(random.choice("ACGT") for _ in range(G))
    seen = set()
    out = []
    while len(out) < N:
        p = random.randrange(0, G - L + 1)
        s = random.random() < 0.5
        if (p, s) in seen:
            continue
        seen.add((p, s))
        r = g[p:p + L]
        if s:
            r = revcomp(r)
        out.append(("r%d" % len(out), r))
    return out


def fasta_text(named_reads):
    return "".join(">%s\n%s\n" % (n, s) for n, s in named_reads)


def corner_reads():
    """6 hand-written 30-mers: b overlaps a by 21, c == a, d is a 16-mer substring of a, e == revcomp(b), f."""
    random.seed(4242)
    g = "".join(random.choice("ACGT") for _ in range(80))
    a = g[0:30]
    b = g[9:39]
    c = a
    d = a[5:21]
    e = revcomp(b)
    f = revcomp(g[22:52])
    return [("a", a), ("b", b), ("c", c), ("d", d), ("e", e), ("f", f)]


def rep_reads():
    """SURVEY.md App. C `rep`: exercises SubMaximalBlockFilter::resolve's re-mapping path."""
    random.seed(5)

    def rnd(n):
        return "".join(random.choice("ACGT") for _ in range(n))

    P = "ACGTTGCAAG"
    s0 = rnd(40) + P * 4
    s1 = P * 3 + rnd(50)
    s2 = P + rnd(70)
    s3 = rnd(30) + s0[:50]
    s4 = P * 2 + rnd(60)
    return [("s0", s0), ("s1", s1), ("s2", s2), ("s3", s3), ("s4", s4)]


def dup_reads():
    """SURVEY.md App. C `dup`: heavy duplicates + substrings, variable length."""
    random.seed(77)
    g = "".join(random.choice("ACGT") for _ in range(60))
    out = []
    for i in range(300):
        L = random.choice([12, 16, 20])
        p = random.randrange(0, 60 - L + 1)
        out.append(("q%d" % i, g[p:p + L]))
    return out


def fast_reads(G, L, N, seed, by_position=False, subset=None):
    """numpy generator for BASELINE-sized sets -> (uint8 array [N, L] of ASCII, genome array).  by_position: the same reads
    in genome order instead of random order (a measurement aid: what locality between neighbouring reads would be worth).
    subset=(lo, hi): only reads lo..hi-1 of the same set (one rank's shard, without materialising the other ranks'); or an
    index array: those reads, in that order."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=G, dtype=np.uint8)
    npos = G - L + 1
    if 2 * npos < N:
        raise ValueError("not enough distinct (pos,strand) draws")
    # unique (pos, strand) keys in random order: oversample, de-duplicate, shuffle, cut
    keys = np.unique(rng.integers(0, 2 * npos, size=int(N * 1.25) + 64, dtype=np.int64))
    while len(keys) < N:
        keys = np.unique(np.concatenate([keys, rng.integers(0, 2 * npos, size=N, dtype=np.int64)]))
    rng.shuffle(keys)
    keys = keys[:N]
    if by_position:
        keys = np.sort(keys)
    if subset is not None:
        keys = keys[subset] if isinstance(subset, np.ndarray) else keys[subset[0]:subset[1]]
    pos = (keys >> 1).astype(np.int64)
    strand = (keys & 1).astype(bool)
    codes = np.lib.stride_tricks.sliding_window_view(genome, L)[pos]  # [N, L] copy
    codes[strand] = (3 - codes[strand])[:, ::-1]
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return lut[codes], genome


def rank_of_r_names(n):
    """rank of the name "r<i>" under std::string operator< for i in [0, n): decimal strings compare like their digits
    left-aligned, a proper prefix first (sorting 2e7 Python strings would take a minute)."""
    i = np.arange(n, dtype=np.int64)
    ndig = np.ones(n, dtype=np.int64)
    p = 10
    while p <= n:
        ndig += i >= p
        p *= 10
    D = int(ndig.max()) if n else 1
    key = i * (10 ** (D - ndig))
    order = np.lexsort((ndig, key))
    rank = np.empty(n, dtype=np.uint32)
    rank[order] = np.arange(n, dtype=np.uint32)
    return rank


def substitute(reads, rate, seed):
    """ASCII read array [N, L] -> copy with each base replaced by a different one with probability `rate`."""
    rng = np.random.default_rng(seed)
    code = np.zeros(256, dtype=np.uint8)
    code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    c = code[reads]
    hit = rng.random(reads.shape) < rate
    c = np.where(hit, (c + rng.integers(1, 4, size=reads.shape, dtype=np.uint8)) & 3, c)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[c]


# ---- reads with non-ACGT bytes -----------------------------------------------------------------------------------------
# Every byte other than A C G T ranks as '$' (alphabet.h:19-39): it ends a stretch of the index, and the finder, the
# extractor and their tables each carry checks that only such a byte reaches.  Bytes >= 0x80 are left out: torank() of a
# negative char is undefined in the reference.
NON_ACGT_BYTES = "NacgtnRYKM."
NON_ACGT_MS = (12, 15, 16, 17, 31, 45, 56, 57)
NON_ACGT_SEEDS = tuple(range(1, 17))
NON_ACGT_DENSE = (4, 8, 12)            # every read of the base set carries an N (the rest: about one in 30)
NON_ACGT_LONG = {15: 250, 16: 700}     # the staged-64 and the unstaged finder forms


def non_acgt_offsets(m):
    """offsets (from either read end) at which a non-ACGT byte is planted: the read ends, the 12-mer start table's window
    edge, the deep table's K = min(m, 56) and the min-overlap itself"""
    K = min(m, 56)
    return sorted({0, 11, 12, K - 1, K, m - 1, m, m + 1})


def non_acgt_pieces(m):
    """ACGT pieces between two non-ACGT bytes: K - 1, K, K + 1 (deep table rows), 13-15 (a row-table entry's 14 leading
    symbols) and 27-29 (the 28-symbol text windows)"""
    K = min(m, 56)
    return sorted({K - 1, K, K + 1, 13, 14, 15, 27, 28, 29})


def non_acgt_runs(seed):
    """lengths of the runs of N one case plants; over NON_ACGT_SEEDS they cover 2..30"""
    return sorted({2, 30} | {2 + ((seed - 1) * 2 + j) % 29 for j in range(2)} | {2 + (seed * 11) % 29})


def non_acgt_case(seed):
    """One seeded read set mixing ACGT-only reads with reads that carry non-ACGT bytes (tests/test_gpu_non_acgt.py):
    substitution errors, both strands, duplicates and substrings as in tests/test_gpu_random.py, plus reads with a
    non-ACGT byte at every offset of non_acgt_offsets() from either end (both depth parities), several in one 12-symbol
    window, runs of N, pieces of non_acgt_pieces() symbols, an all-N read, one-byte reads and reads shorter than 12 and
    than m.  Returns dict(reads=[(name, seq)], m, irreducible, rc, dense)."""
    rnd = random.Random(7000 + seed)
    m = NON_ACGT_MS[seed % len(NON_ACGT_MS)]
    K = min(m, 56)
    Lmax = NON_ACGT_LONG.get(seed, rnd.choice([60, 100, 150]))
    Lmin = Lmax // 2 if Lmax > 150 else rnd.choice([20, 40, Lmax])
    G = max(rnd.choice([1500, 4000, 12000]), 12 * Lmax)
    genome = "".join(rnd.choice("ACGT") for _ in range(G))
    if rnd.random() < 0.5:  # a repeat: the same segment twice
        seg = genome[100:100 + rnd.choice([60, 150])]
        p = rnd.randrange(G // 2, G - len(seg))
        genome = genome[:p] + seg + genome[p + len(seg):]
    err = rnd.choice([0.0, 0.005, 0.02])
    cov = rnd.choice([6, 10, 20]) if Lmax <= 150 else 8
    dense = seed in NON_ACGT_DENSE

    def draw(l):
        p = rnd.randrange(0, G - l + 1)
        s = genome[p:p + l]
        if rnd.random() < 0.5:
            s = revcomp(s)
        return "".join((rnd.choice([c for c in "ACGT" if c != b]) if rnd.random() < err else b) for b in s)

    def length(at_least):
        lo = max(Lmin, at_least)
        return rnd.randrange(lo, max(Lmax, lo) + 1)

    k0 = rnd.randrange(len(NON_ACGT_BYTES))
    cyc = [k0]

    def byte():  # every byte of NON_ACGT_BYTES in turn
        cyc[0] += 1
        return NON_ACGT_BYTES[cyc[0] % len(NON_ACGT_BYTES)]

    def put(s, i, c):
        return s[:i] + c + s[i + 1:]

    base = []
    for _ in range(max(200, min(3000, G * cov // Lmax))):
        s = draw(length(Lmin))
        if dense or rnd.random() < 1.0 / 30:
            s = put(s, rnd.randrange(len(s)), "N")
        base.append(s)
    planted = []
    # one byte at a given offset from the start or from the end; two random offsets of either parity besides
    offs = non_acgt_offsets(m) + [2 * rnd.randrange(1, 20), 2 * rnd.randrange(1, 20) + 1]
    for o in offs:
        for from_end in (False, True):
            for _ in range(2):
                s = draw(length(o + 2))
                planted.append(put(s, len(s) - 1 - o if from_end else o, byte()))
    # several bytes inside the first or last twelve symbols
    for ps in ((3, 7), (0, 11), (10, 11, 12), (1, 2, 4, 8)):
        for from_end in (False, True):
            s = draw(length(24))
            for o in ps:
                s = put(s, len(s) - 1 - o if from_end else o, byte())
            planted.append(s)
    # runs of N: inside a read, at its start, at its end
    for j, r in enumerate(non_acgt_runs(seed)):
        s = draw(length(r + 4))
        a = (0, len(s) - r, rnd.randrange(1, len(s) - r))[j % 3]
        planted.append(s[:a] + "N" * r + s[a + r:])
        s = draw(length(r + 4))
        a = rnd.randrange(1, len(s) - r)
        planted.append(s[:a] + byte() * r + s[a + r:])
    # ACGT pieces of a given length between two non-ACGT bytes
    for p in non_acgt_pieces(m):
        for _ in range(2):
            s = draw(length(p + 2))
            a = rnd.randrange(0, len(s) - p - 1)
            planted.append(put(put(s, a, byte()), a + p + 1, byte()))
    s = draw(length(2 * K + 3))  # two pieces of K in a row
    planted.append(put(put(put(s, 0, "N"), K + 1, "n"), 2 * K + 2, "N"))
    # degenerate reads
    planted += ["N" * rnd.randrange(20, 60), "N", "A", byte(), "g",
                put(draw(5), 2, byte()), put(draw(11), 5, "N"), draw(11),
                put(draw(m - 1), (m - 1) // 2, byte()), draw(m - 1)]
    reads = base + planted
    for _ in range(rnd.choice([3, 20])):  # exact duplicates and substrings
        s = rnd.choice(reads)
        if rnd.random() < 0.5 and len(s) > 30:
            a = rnd.randrange(0, len(s) - 25)
            s = s[a:a + rnd.randrange(25, len(s) - a + 1)]
        reads.append(s)
    rnd.shuffle(reads)
    return {"reads": [("r%d" % i, s) for i, s in enumerate(reads)], "m": m, "irreducible": seed % 3 != 0,
            "rc": seed % 5 != 0, "dense": dense}
