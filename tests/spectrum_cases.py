"""Cases of `siga preqc`: FMIndex::getString (src/fmindex.cpp:292-313) and KmerDistribution::sample's loop
(src/kmerdistr.cpp:12-33), computed from nothing but what the oracle answers: getchar, occ, pred, sai, occurrences.
walk() is the LF walk of getString; spectrum() is the reference's loop over match_cases.count(fwd, w, True).  No tests here."""
import functools
import os
import random

import numpy as np

from oracle import pyoracle as po
from tests import match_cases as mc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

KS = (1, 12, 13, 14, 31, 33, 59, 60, 61)
BINS = (1, 4, 1024)
NO_STRETCH = (1 << 64) - 1

_TABLES = {}


def lf_table(ix):
    """-> (codes u8[n]: rank of the BWT symbol of every row, by getchar; lf i64[n]: C[c] + Occ(c, row - 1), by pred and by
    counting those symbols; dollars i64[n + 1]: Occ('$', row - 1)).  Built once per index: a walk is then array reads."""
    key = id(ix)
    if key not in _TABLES:
        n = len(ix)
        codes = np.array(["$ACGT".index(ix.getchar(p)) for p in range(n)], dtype=np.uint8)
        pred = ix.pred().astype(np.int64)
        lf = np.zeros(n, dtype=np.int64)
        for r in range(1, 5):
            at = np.flatnonzero(codes == r)
            lf[at] = pred[r] + np.arange(len(at), dtype=np.int64)
        dollars = np.zeros(n + 1, dtype=np.int64)
        dollars[1:] = np.cumsum(codes == 0)
        _TABLES[key] = (ix, codes, lf, dollars)
    return _TABLES[key][1:]


def walk(ix, row, max_len=None):
    """getString(row) -> (text, the end row's Occ('$') - 1: the stretch index).  With max_len: the walk stops after max_len
    symbols when more would follow -> (its last max_len symbols, None)."""
    codes, lf, dollars = lf_table(ix)
    out = []
    p = row
    while codes[p] != 0:
        if max_len is not None and len(out) == max_len:
            return "".join(reversed(out)), None
        out.append("$ACGT"[codes[p]])
        p = int(lf[p])
    return "".join(reversed(out)), int(dollars[p])


_TABLES_FWD = {}


@functools.lru_cache(maxsize=None)
def _occurrences(key, w):
    return _TABLES_FWD[key].occurrences(w)


def window_counts(fwd, strings, k):
    """per string with len >= k the counts of its windows j = k .. len - 1 (NOT the one that ends at the last base), both
    strands: match_cases.count(fwd, w, True) with the oracle's answers remembered per pattern"""
    key = id(fwd)
    _TABLES_FWD[key] = fwd
    out = []
    for s in strings:
        if len(s) < k:
            continue
        out.append([_occurrences(key, s[j - k:j]) + _occurrences(key, mc.revcomp(s[j - k:j])) for j in range(k, len(s))])
    return out


def spectrum(fwd, strings, k, n_bins):
    """-> (hist[n_bins], strings with len >= k, L = their bases, windows)"""
    hist = [0] * n_bins
    counts = window_counts(fwd, strings, k)
    for cs in counts:
        for c in cs:
            hist[min(c, n_bins - 1)] += 1
    return hist, len(counts), sum(len(s) for s in strings if len(s) >= k), sum(len(cs) for cs in counts)


def spectrum_strings(reads, k, seed, extra=()):
    """[(class, string)]: every class of string the kernel treats differently, around this k"""
    rnd = random.Random(4100 + 17 * seed + k)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    acgt = [s for s in reads if set(s) <= set("ACGT") and len(s) >= 20]
    out = []
    for _ in range(10):
        out.append(("indexed", rnd.choice(acgt)))
    for _ in range(6):
        out.append(("revcomp", mc.revcomp(rnd.choice(acgt))))
    for _ in range(10):
        s = rnd.choice(acgt)
        p = rnd.randrange(len(s))
        out.append(("subst", s[:p] + other[s[p]] + s[p + 1:]))
    for s in extra:
        out.append(("palindrome", s))
    long = rnd.choice(acgt) + rnd.choice(acgt) + rnd.choice(acgt)  # the joints are in no read
    for l in (k - 1, k, k + 1, k + 2):
        if l > 0:
            out.append(("length", long[:l]))
    for c in mr.NON_ACGT_BYTES[:3]:
        s = rnd.choice(acgt) + rnd.choice(acgt)[:15]
        out.append(("non_acgt_first", c + s[1:]))
        out.append(("non_acgt_last", s[:-1] + c))
        out.append(("non_acgt_last_window", s[:-2] + c + s[-1]))
        p = 1 + rnd.randrange(len(s) - 2)
        out.append(("non_acgt_inner", s[:p] + c + s[p + 1:]))
    out.append(("empty", ""))
    return out


def match_files(seed):
    """index files of match_cases.match_case(seed), oracle-built (the files tests/test_gpu_match.py uses) -> prefix"""
    case = mc.match_case(seed)
    d = os.path.join(CACHE, "match%d" % seed)
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai")):
        seqs = [s for _, s in case["reads"]]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
    return prefix
