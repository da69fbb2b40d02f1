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


# ---- `siga correct` across k, its options and the k-mer lookup forms ------------------------------------------------------
# k: the k-mer table's range (8..56) and both sides of it, the 13-mer prefix table's k >= pk edge (12, 13, 14), the one- and
# two-word keys of the table (31, 32, 33), candidates beyond one 64-base chunk (65, 100).
CORRECT_KS = (7, 8, 12, 13, 14, 31, 32, 33, 55, 56, 57, 65, 100)
# (kmer threshold -x, rounds -i, count offset -O): the defaults, negative thresholds (a support no count reaches), 0 with
# qualities (support 0 / 1), one round, no round, offset 0
CORRECT_OPTIONS = ((3, 10, 1), (-1, 10, 1), (-2, 10, 1), (0, 10, 0), (5, 1, 4), (3, 0, 1), (2, 3, 0))
# seed -> (k, options, with qualities)
CORRECT_CASES = {
    1: (31, (3, 10, 1), False), 2: (32, (-1, 10, 1), False), 3: (33, (2, 3, 0), True), 4: (7, (3, 10, 1), False),
    5: (8, (5, 1, 4), True), 6: (12, (3, 0, 1), False), 7: (13, (3, 10, 1), True), 8: (14, (0, 10, 0), True),
    9: (55, (-2, 10, 1), True), 10: (56, (3, 10, 1), False), 11: (57, (2, 3, 0), False), 12: (65, (3, 10, 1), True),
    13: (100, (5, 1, 4), False), 14: (32, (3, 10, 1), True), 15: (12, (2, 3, 0), False), 16: (57, (-1, 10, 1), True),
}
CORRECT_SEEDS = tuple(sorted(CORRECT_CASES))
CORRECT_LMAX = 200


def correct_offsets(k):
    """offsets (from either read end) of a planted single substitution: the read ends, the eighth candidate and its
    neighbours, the 32-symbol word edge of the packed key, the window edge"""
    return sorted({0, 1, 7, 8, 9, 31, 32, 33, k - 2, k - 1, k})


def correct_sh0_lengths(k):
    """read lengths k + 32 j and k + 32 j +- 1 (j >= 1) up to CORRECT_LMAX: window 0's key starts at a 64-bit word edge"""
    out = []
    j = 1
    while k + 32 * j - 1 <= CORRECT_LMAX:
        out += [L for L in (k + 32 * j - 1, k + 32 * j, k + 32 * j + 1) if L <= CORRECT_LMAX]
        j += 1
    return out


def fastq_text(named_reads, quals):
    return "".join("@%s\n%s\n+\n%s\n" % (n, s, q) for (n, s), q in zip(named_reads, quals))


def correct_case(seed):
    """One seeded case of tests/test_gpu_correct_matrix.py: reads of one strand of a random genome with about 1 %
    substitutions at a coverage that leaves the error-free k-mers well above the threshold, about one read in 30 with an N,
    plus PLANTED reads: error-free pieces of the genome with a substitution (or two, or an N, or chosen qualities) put where
    k_correct and kmer_occ change form.  Returns dict(reads=[(name, seq)], quals=[str] or None, k, threshold, rounds,
    offset, planted=[dict(i=read index, cls=class name, errs=[offsets of the substitutions])])."""
    rnd = random.Random(9000 + seed)
    k, (threshold, rounds, offset), with_q = CORRECT_CASES[seed]
    Lmax = CORRECT_LMAX
    Lmin = 60 if k <= 33 else 110 if k <= 65 else 150
    G = 1500 if k <= 8 else 6000 if k < 55 else 3000
    genome = "".join(rnd.choice("ACGT") for _ in range(G))
    err = 0.01
    Lavg = (Lmin + Lmax) // 2
    n_base = int(max(25 * G / Lavg, 15 * G / ((Lavg - k + 1) * (1 - err) ** k)))
    assert n_base <= 2400

    def piece(l):
        p = rnd.randrange(0, G - l + 1)
        return genome[p:p + l]

    def other(b):
        return rnd.choice([c for c in "ACGT" if c != b])

    def sub(s, i):
        return s[:i] + other(s[i]) + s[i + 1:]

    def put(s, i, c):
        return s[:i] + c + s[i + 1:]

    def length(at_least=0):
        lo = max(Lmin, at_least)
        return rnd.randrange(lo, max(Lmax, lo) + 1)

    def base_quals(l):
        # mostly good bases; about one read in six carries a few below the cutoff of 20
        q = [rnd.choice((30, 35, 40)) for _ in range(l)]
        if rnd.random() < 1.0 / 6:
            for _ in range(rnd.randrange(1, 4)):
                q[rnd.randrange(l)] = rnd.choice((2, 12, 19))
        return q

    items = []  # (seq, phreds or None, class or None, errs)

    def add(s, cls=None, errs=(), q=None):
        items.append((s, (q if q is not None else [40] * len(s)) if with_q else None, cls, list(errs)))

    for _ in range(n_base):
        s = piece(length())
        s = "".join(other(b) if rnd.random() < err else b for b in s)
        if rnd.random() < 1.0 / 30:
            s = put(s, rnd.randrange(len(s)), "N")
        add(s, q=base_quals(len(s)))
    # a single substitution at a given offset from the start, and from the end
    for o in correct_offsets(k):
        for from_end in (False, True):
            for _ in range(4):
                s = piece(length(k + 34))
                p = len(s) - 1 - o if from_end else o
                add(sub(s, p), "sub_end" if from_end else "sub_start", [p])
    if k >= 10:  # inside the first k bases, beyond the first eight candidates
        for _ in range(14):
            p = rnd.randrange(8, k)
            add(sub(piece(length(k + 34)), p), "first_k_beyond_8", [p])
    if k > 64:  # ... and beyond the first 64-base chunk
        for _ in range(10):
            p = rnd.randrange(64, k)
            add(sub(piece(length(k + 34)), p), "first_k_beyond_64", [p])
    # two substitutions closer than k
    for d in sorted({1, 2, k // 2, k - 1}):
        for _ in range(3):
            s = piece(length(2 * k + 2))
            p = rnd.randrange(0, len(s) - d)
            add(sub(sub(s, p), p + d), "two_subs", [p, p + d])
    # reads of k, k + 1, k - 1 bases and of one
    for L, cls in ((k, "len_k"), (k + 1, "len_k1"), (k - 1, "len_km1")):
        for j in range(4):
            s = piece(L)
            p = rnd.randrange(L)
            add(sub(s, p) if j >= 2 else s, cls, [p] if j >= 2 else [])
    add("A", "len_1")
    add("N", "len_1")
    # window 0 at a word edge of the packed read
    for L in correct_sh0_lengths(k):
        add(piece(L), "sh0_length")
        for p in (0, k - 1, rnd.randrange(L)):
            add(sub(piece(L), p), "sh0_length", [p])
    # one N: in the last 13 bases of a window that holds the error, in its first ones, nowhere near it
    for _ in range(4):
        L = length(k + 34)
        p = rnd.randrange(k, L - k) if L > 2 * k + 1 else k
        s0 = p - rnd.randrange(0, min(k, p + 1))           # a window [s0, s0 + k) over p
        s0 = min(s0, L - k)
        for cls, cand in (("n_window_tail", [s0 + k - 1 - r for r in range(min(13, k))]), ("n_window_head", [s0 + r for r in range(min(4, k))])):
            cand = [c for c in cand if c != p and 0 <= c < L]
            add(put(sub(piece(L), p), rnd.choice(cand), "N"), cls, [p])
        L = length(k + 34)
        p = rnd.randrange(0, 5)
        add(put(sub(piece(L), p), L - 1 - rnd.randrange(0, 5), "N"), "n_far", [p])
        s = piece(L)
        add(put(s, rnd.randrange(L), "N"), "n_alone")
    add("N" * 80, "all_n")
    # what no correction mends: runs of N, and reads that are not of this genome
    for _ in range(8):
        s = piece(length(k + 34))
        a = rnd.randrange(0, len(s) - 3)
        r = rnd.choice((2, 3))
        add(s[:a] + "N" * r + s[a + r:], "n_run")
    for _ in range(20):
        add("".join(rnd.choice("ACGT") for _ in range(length())), "foreign")
    if with_q:
        # the substituted base and its neighbours at phred 19 / 20 / 21: the cutoff of 20 picks `low` or `high`
        for trio in ((19, 19, 19), (20, 20, 20), (21, 21, 21), (19, 20, 21), (21, 19, 21), (19, 21, 19)):
            for _ in range(4):
                s = piece(length(k + 34))
                p = rnd.randrange(1, len(s) - 1)
                q = [40] * len(s)
                q[p - 1:p + 2] = trio
                add(sub(s, p), "qual_%d_%d_%d" % trio, [p], q=q)
    # exact duplicates, of planted reads and of the base set
    for _ in range(20):
        s, q, cls, errs = rnd.choice(items)
        items.append((s, q, "duplicate", errs))
    rnd.shuffle(items)
    assert len(items) <= 3000
    return {"reads": [("r%d" % i, it[0]) for i, it in enumerate(items)],
            "quals": ["".join(chr(33 + v) for v in it[1]) for it in items] if with_q else None,
            "k": k, "threshold": threshold, "rounds": rounds, "offset": offset,
            "planted": [dict(i=i, cls=it[2], errs=it[3]) for i, it in enumerate(items) if it[2]]}
