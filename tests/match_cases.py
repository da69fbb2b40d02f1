"""Cases of `siga match` (src/match.cpp:38-63): a named read set to index, a set of named queries that mixes every class of
pattern the kernel treats differently, and (L, rc) = (--max-length or None, both strands or not).  expected() is the
reference's loop, line by line, over the oracle's Interval::occurrences.  No tests here."""
import functools
import random

from oracle import pyoracle as po
from tests.golden import make_reads as mr

READ_LEN = 100
GENOME = 24000
N_READS = 2400
LS = (None, 0, 1, 13, 40, READ_LEN)
SEEDS = tuple(range(1, 2 * len(LS) + 1))  # seed -> L = LS[(seed - 1) // 2], rc = seed odd
CLASSES = ("verbatim", "revcomp", "subst", "substring", "palindrome", "non_acgt_first", "non_acgt_last", "non_acgt_inner",
           "length", "long")
LONG = 20000

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(w):
    """make_dna_reverse_complement_copy with the alphabet's rule: a byte outside ACGT ranks as '$' on either strand"""
    return "".join(_COMP.get(c, "N") for c in reversed(w))


def params(seed):
    return LS[(seed - 1) // 2], seed % 2 == 1


def lengths_for(L):
    l0 = L if L else READ_LEN // 2
    want = [1, 2, 12, 13, 14, l0 - 1, l0, l0 + 1, 2 * l0 - 1, 2 * l0]
    return [x for x in want if x > 0]


@functools.lru_cache(maxsize=None)
def match_case(seed):
    """-> dict(reads=[(name, seq)], queries=[(name, seq, class)], L=, rc=, genome=)"""
    L, rc = params(seed)
    rnd = random.Random(7700 + seed)
    g = "".join(rnd.choice("ACGT") for _ in range(GENOME))
    reads = []
    for i in range(N_READS):
        p = rnd.randrange(0, GENOME - READ_LEN + 1)
        r = g[p:p + READ_LEN]
        reads.append(("r%d" % i, revcomp(r) if rnd.random() < 0.5 else r))
    half = "".join(rnd.choice("ACGT") for _ in range(READ_LEN // 2))
    pal = half + revcomp(half)
    reads.append(("pal", pal))
    reads.append(("withN", reads[5][1][:30] + "N" + reads[5][1][31:]))
    q = []

    def add(cls, s):
        q.append(("q%d_%s" % (len(q), cls), s, cls))

    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    for i in range(20):
        add("verbatim", reads[rnd.randrange(N_READS)][1])
    for i in range(20):
        add("revcomp", revcomp(reads[rnd.randrange(N_READS)][1]))
    nsub = 80
    for i in range(nsub):  # one substitution, positions over the whole length: chains die at every depth
        s = reads[rnd.randrange(N_READS)][1]
        p = min(READ_LEN - 1, i * READ_LEN // nsub + rnd.randrange(2))
        add("subst", s[:p] + other[s[p]] + s[p + 1:])
    for i in range(10):
        s = reads[rnd.randrange(N_READS)][1]
        a = rnd.randrange(0, READ_LEN - 20)
        b = rnd.randrange(a + 15, READ_LEN)
        add("substring", s[a:b] if (a, b) != (0, READ_LEN) else s[1:])
    add("palindrome", pal)
    add("palindrome", pal[READ_LEN // 2 - 10:READ_LEN // 2 + 10])
    for k, c in enumerate(mr.NON_ACGT_BYTES):
        s = reads[rnd.randrange(N_READS)][1]
        add("non_acgt_first", c + s[1:])
        add("non_acgt_last", s[:-1] + c)
        p = 1 + (k * 9 + rnd.randrange(7)) % (READ_LEN - 2)
        add("non_acgt_inner", s[:p] + c + s[p + 1:])
    for l in lengths_for(L):
        p = rnd.randrange(0, GENOME - l + 1)
        add("length", g[p:p + l])
    add("long", g[1500:1500 + LONG + seed])
    return dict(reads=reads, queries=q, L=L, rc=rc, genome=g)


def count(fwd, w, rc):
    return fwd.occurrences(w) + (fwd.occurrences(revcomp(w)) if rc else 0)


def expected(fwd, named_queries, L, rc):
    """match.cpp:54-62 -> (head[n], tail[n] with None for a read that is not split, stdout text)"""
    head, tail, text = [], [], []
    for q in named_queries:
        name, seq = q[0], q[1]
        if L is not None and len(seq) > L:
            start, end = seq[:L], seq[len(seq) - L:]
            head.append(count(fwd, start, rc))
            tail.append(count(fwd, end, rc))
            text.append("VT\t0\t%s\t%s\t%d\n" % (name, seq, head[-1]))
            text.append("VT\t1\t%s\t%s\t%d\n" % (name, seq, tail[-1]))
        else:
            head.append(count(fwd, seq, rc))
            tail.append(None)
            text.append("VT\t0\t%s\t%s\t%d\n" % (name, seq, head[-1]))
    return head, tail, "".join(text)


def stop_depth(fwd, w):
    """symbols Interval::occurrences (src/fmindex.h:67-86) consumes of w: it takes them from the end and stops updating once
    the interval is empty.  occurrences(suffix) never grows with the suffix: bisection."""
    if not w or fwd.occurrences(w) > 0:
        return len(w)
    lo, hi = 1, len(w)  # the suffix of length hi has no occurrence; find the shortest such
    while lo < hi:
        mid = (lo + hi) // 2
        if fwd.occurrences(w[len(w) - mid:]) == 0:
            hi = mid
        else:
            lo = mid + 1
    return lo


def patterns(seqs, L, rc):
    """the non-empty patterns the reference searches for these reads, strand by strand"""
    out = []
    for s in seqs:
        segs = [s[:L], s[len(s) - L:]] if L is not None and len(s) > L else [s]
        for w in segs:
            if w:
                out.append(w)
                if rc:
                    out.append(revcomp(w))
    return out


def half_substituted(seed, n=200, nsub=3):
    """n indexed reads, every second one with nsub substitutions at positions drawn over the whole read"""
    case = match_case(seed)
    rnd = random.Random(99 + seed)
    other = {"A": "G", "C": "T", "G": "A", "T": "C"}
    out = []
    for i in range(n):
        s = case["reads"][rnd.randrange(N_READS)][1]
        if i % 2:
            for p in rnd.sample(range(READ_LEN), nsub):
                s = s[:p] + other[s[p]] + s[p + 1:]
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def oracle_index(seed):
    return po.Index.build([s for _, s in match_case(seed)["reads"]])
