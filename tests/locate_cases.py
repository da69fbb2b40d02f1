"""Cases of `siga locate` (csrc/sigax_locate.hip): two ACGT-only read sets to index and, for `small`, a set of named queries
that mixes every class of pattern the kernels treat differently.  expected() is brute-force string search: for every read,
every start at which the query, or its reverse complement, matches.  The oracle takes no part in it; it builds the index
files and gives the totals the brute force is cross-checked against.  No tests here."""
import functools
import random

import numpy as np

from oracle import pyoracle as po
from tests.match_cases import revcomp

SMALL_READS = 600
SMALL_LEN = 60
SMALL_GENOME = 6000
N_DUP = 9
MANY_READS = 20000
MANY_LEN = 60
MANY_GENOME = 50000

HIT_REV, HIT_CUT = 1, 2
SKIPPED, OVER = 1, 2


@functools.lru_cache(maxsize=None)
def small():
    """-> dict(reads=[(name, seq)], queries=[(name, seq, class)]); the queries hold no two equal names"""
    rnd = random.Random(3100)
    g = "".join(rnd.choice("ACGT") for _ in range(SMALL_GENOME))
    reads = []
    for i in range(SMALL_READS):
        p = rnd.randrange(0, SMALL_GENOME - SMALL_LEN + 1)
        r = g[p:p + SMALL_LEN]
        reads.append(("r%d" % i, revcomp(r) if i % 2 else r))
    dup = reads[3][1]
    for i in range(N_DUP):  # a block of exact duplicates of read 3
        reads.append(("dup%d" % i, dup))
    half = "".join(rnd.choice("ACGT") for _ in range(SMALL_LEN // 2))
    pal = half + revcomp(half)
    reads.append(("pal", pal))
    reads.append(("periodic", "AC" * (SMALL_LEN // 2)))
    reads.append(("len1", "G"))
    reads.append(("len2", "TG"))
    reads.append(("len13", g[100:113]))
    long_read = "".join(rnd.choice("ACGT") for _ in range(300))
    reads.append(("len300", long_read))

    q = []

    def add(cls, s):
        q.append(("q%d_%s" % (len(q), cls), s, cls))

    for l in (1, 2, 12, 13, 14, 31):
        for _ in range(2):
            s = reads[rnd.randrange(SMALL_READS)][1]
            a = rnd.randrange(0, SMALL_LEN - l + 1)
            add("len%d" % l, s[a:a + l])
    for i in (0, 1, 10, 11, 598, 599):  # whole reads, as stored and reverse-complemented ones
        add("read", reads[i][1])
    add("read_rc", revcomp(reads[20][1]))
    add("read_long", long_read)
    add("inside_long", long_read[140:171])
    add("at_start", reads[40][1][:25])
    add("at_end", reads[41][1][SMALL_LEN - 25:])
    add("at_end_long", long_read[300 - 14:])
    add("duplicate", dup)
    add("duplicate_part", dup[5:45])
    add("palindrome", pal)
    add("palindrome_part", pal[SMALL_LEN // 2 - 8:SMALL_LEN // 2 + 8])
    add("periodic", "AC")
    add("periodic", "ACACACACACACAC")
    add("periodic", "CACACACACACACA")
    add("short_read", "G")
    add("short_read", "TG")
    add("short_read", g[100:113])
    add("absent", "".join(rnd.choice("ACGT") for _ in range(40)))
    s = reads[50][1]
    add("absent_subst", s[:30] + {"A": "C", "C": "G", "G": "T", "T": "A"}[s[30]] + s[31:])
    add("longer_than_reads", "".join(rnd.choice("ACGT") for _ in range(400)))
    add("empty", "")
    s = reads[60][1]
    add("n_first", "N" + s[1:])
    add("n_inner", s[:27] + "N" + s[28:])
    add("n_last", s[:-1] + "N")
    add("n_last_short", s[10:14] + "N")
    add("n_only", "N")
    return dict(reads=reads, queries=q, genome=g)


@functools.lru_cache(maxsize=None)
def many():
    """20 000 x 60 bp: the one-base queries have several hundred thousand hits each, thousands of workgroups of the walk and
    more slots than a device-wide grid of resident waves holds at once.  -> dict(reads=uint8 [N, L] of ASCII,
    queries=[(name, seq, class)])"""
    from tests.golden import make_reads as mr
    reads, _ = mr.fast_reads(MANY_GENOME, MANY_LEN, MANY_READS, 3200)
    return dict(reads=reads, queries=[("A", "A", "one_base"), ("C", "C", "one_base")])


def many_seqs():
    return [bytes(r).decode() for r in many()["reads"]]


def is_acgt(w):
    return len(w) > 0 and set(w) <= set("ACGT")


def find_all(text, w):
    out, p = [], text.find(w)
    while p >= 0:
        out.append(p)
        p = text.find(w, p + 1)  # overlapping occurrences too
    return out


def expected(seqs, queries, rc):
    """-> per query None (empty, or a byte outside ACGT: nothing is listed) or the sorted list of (read, offset, strand) with
    strand 0 where read[offset:offset+len] == query and 1 where it is the query's reverse complement"""
    out = []
    for w in queries:
        if not is_acgt(w):
            out.append(None)
            continue
        hits = []
        wr = revcomp(w)
        for i, s in enumerate(seqs):
            if len(s) < len(w):
                continue
            hits += [(i, p, 0) for p in find_all(s, w)]
            if rc:
                hits += [(i, p, 1) for p in find_all(s, wr)]
        out.append(sorted(hits))
    return out


def expected_one_base(reads, base, rc):
    """the same for a one-base query over an [N, L] array of ASCII, with numpy -> sorted array [hits, 3]"""
    b = ord(base)
    r, o = np.nonzero(reads == b)
    hits = np.stack([r, o, np.zeros_like(r)], axis=1)
    if rc:
        r, o = np.nonzero(reads == ord(revcomp(base)))
        hits = np.concatenate([hits, np.stack([r, o, np.ones_like(r)], axis=1)])
    return hits[np.lexsort((hits[:, 2], hits[:, 1], hits[:, 0]))]


def text(named_queries, totals, listed):
    """stdout of `siga locate`: listed[q] = None or the (read, offset, strand) triples in any order -> the QT lines and, per
    query, its HT lines as a sorted list"""
    out = []
    for (name, seq), total, hits in zip(named_queries, totals, listed):
        qt = "QT\t%s\t%d\t%d\t%d" % (name, len(seq), total, len(hits) if hits is not None else 0)
        out.append((qt, sorted("HT\t%s\t%d\t%d\t%s" % (name, r, o, "-" if s else "+") for r, o, s in (hits or []))))
    return out


def parse_text(stdout):
    """`siga locate`'s stdout -> [(QT line, sorted HT lines)] in output order; an HT line before any QT line is an error"""
    out = []
    for line in stdout.split("\n"):
        if not line:
            continue
        if line.startswith("QT\t"):
            out.append((line, []))
        else:
            assert line.startswith("HT\t") and out, line
            assert line.split("\t")[1] == out[-1][0].split("\t")[1], "HT line of another query: " + line
            out[-1][1].append(line)
    return [(qt, sorted(ht)) for qt, ht in out]


@functools.lru_cache(maxsize=None)
def oracle_index(name):
    seqs = [s for _, s in small()["reads"]] if name == "small" else many_seqs()
    return po.Index.build(seqs)
