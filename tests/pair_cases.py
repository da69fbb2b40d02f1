"""Cases and brute force for `siga unitig --pairs` (csrc/sigax_pairs.hip); no tests here (tests/test_pair_cases.py,
tests/test_gpu_unitig_pairs.py).

expected_pairs()         the rules of include/sigax.h (the `--pairs` block), serially, with Python integers.
reference_insert_size()  the reference's InsertSizeEstimateVisitor (src/bigraph_visitors.cpp:517-663) written out: the graph as
                         Bigraph::load builds it, the reduced edges of edges(), the colours, the two walks per start vertex with
                         the distance counter and its strand-flip arithmetic.  Vertices are visited in id order (the reference's
                         order is its hash map's).
The two share nothing but the record classifier.  They are compared as multisets of samples on graphs where the reference's
chains are the unitigs: no rings, no containments, no duplicate reads, no record given twice (edges() folds parallel edges of
one label into one, the unitig rules count both), and reads of one length (see `unequal_flip`).

A case: dict(name, reads, edges, m, mate [read id or NO_MATE])."""
import functools
import math
import random

from tests import chimeric_cases as cc
from tests import trim_cases as tc
from tests import unitig_cases as uc

B, E = 0, 1
NO_MATE = 0xFFFFFFFF
M64 = (1 << 64) - 1
DEFAULT_OPTS = {"hist_bins": 1024, "hist_shift": 0, "max_span": 0, "outward": False}


def unitig_of(lay_offs, nu, p):
    """the bisection of the rules: the largest u < nu with lay_offs[u] <= p where lay_offs ascends"""
    lo, hi = 0, nu
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lay_offs[mid] <= p:
            lo = mid
        else:
            hi = mid
    return lo


def estimate(status):
    """sigax_pairs_estimate, in the operations the C code uses -> (insert_size, delta, span_mean, span_sd)"""
    def moments(at):
        n = status[at]
        if n == 0:
            return 0.0, 0.0
        mean = float(status[at + 1]) / float(n)
        sq = (float(status[at + 3]) * 18446744073709551616.0 + float(status[at + 2])) / float(n)
        var = sq - mean * mean
        return mean, math.sqrt(var) if var > 0.0 else 0.0

    m, s = moments(10)
    sm, sd = moments(14)
    return int(m), int(s), sm, sd


def expected_pairs(res, lengths, mate, opts=None, n_unitigs=None):
    """res: seq_offs, lay_offs, uflags, layout [(read, flags, offset)] of a unitig call (lists or arrays); n_unitigs: the count
    the device form is given, when it is not len(uflags) -> dict(status [24], hist, links [(a, b, count, min_span, sum_span)],
    samples [d of every SAME pair that is not FAR], insert_size, delta, span_mean, span_sd)"""
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    n = len(lengths)
    lengths = [int(x) for x in lengths]
    mate = [int(x) for x in mate]
    seq_offs = [int(x) for x in res["seq_offs"]]
    lay_offs = [int(x) for x in res["lay_offs"]]
    uflags = [int(x) for x in res["uflags"]]
    layout = [tuple(int(x) for x in p) for p in (res["layout"].tolist() if hasattr(res["layout"], "tolist") else res["layout"])]
    nu = min(len(uflags) if n_unitigs is None else n_unitigs, n)
    placed = min(lay_offs[nu], n) if nu else 0
    where = {}
    for p in range(placed):
        read = layout[p][0]
        if read < n:
            assert read not in where, "a read placed twice: the rules give no single answer"
            where[read] = (unitig_of(lay_offs, nu, p), p)
    st = [0] * 24
    hist = [0] * o["hist_bins"]
    links, samples = {}, []
    for i in range(n):
        j = mate[i]
        if j == NO_MATE:
            continue
        st[0] += 1
        if not (j < n and j != i and mate[j] == i):
            st[1] += 1
            continue
        if i > j:
            continue
        st[2] += 1
        if i not in where or j not in where:
            st[3] += 1
            continue
        (ui, pi), (uj, pj) = where[i], where[j]
        li, lj = layout[pi][2], layout[pj][2]
        ri, rj = (li + lengths[i]) & M64, (lj + lengths[j]) & M64
        vi, vj = bool(layout[pi][1] & uc.PLACED_REV), bool(layout[pj][1] & uc.PLACED_REV)
        if ui == uj:
            if uflags[ui] & uc.CIRCULAR:
                st[8] += 1
                continue
            st[4] += 1
            va, vb = (vi, vj) if li <= lj else (vj, vi)
            inward, outward = (not va) and vb, va and not vb
            st[5 if inward else 6 if outward else 7] += 1
            d = abs(lj - li)
            span = (max(ri, rj) - min(li, lj)) & M64
            if span >= 1 << 32:
                st[9] += 1
                continue
            samples.append(d)
            st[10] += 1
            st[11] += d
            sq = st[12] + (st[13] << 64) + d * d
            st[12], st[13] = sq & M64, sq >> 64
            if outward if o["outward"] else inward:
                st[14] += 1
                st[15] += span
                sq = st[16] + (st[17] << 64) + span * span
                st[16], st[17] = sq & M64, sq >> 64
                hist[min(span >> o["hist_shift"], o["hist_bins"] - 1)] += 1
            continue
        st[18] += 1
        ends, g = [], []
        for u, left, right, rev in ((ui, li, ri, vi), (uj, lj, rj, vj)):
            faces_e = rev == o["outward"]
            ends.append(2 * u + (E if faces_e else B))
            g.append((seq_offs[u + 1] - seq_offs[u] - left) & M64 if faces_e else right)
        s = (g[0] + g[1]) & M64
        if (uflags[ui] | uflags[uj]) & uc.CIRCULAR:
            st[19] += 1
        elif o["max_span"] and s > o["max_span"]:
            st[20] += 1
        else:
            key = (min(ends), max(ends))
            assert key[0] != key[1]
            c, mn, sm = links.get(key, (0, M64, 0))
            links[key] = (c + 1, min(mn, s), sm + s)
            st[21] += 1
    st[22] = len(links)
    out = {"status": st, "hist": hist, "samples": samples,
           "links": [(a, b, c, min(mn, (1 << 32) - 1), sm & M64) for (a, b), (c, mn, sm) in sorted(links.items())]}
    out["insert_size"], out["delta"], out["span_mean"], out["span_sd"] = estimate(st)
    return out


# ---- the reference's walk ----
class _Arc:
    __slots__ = ("start", "dir", "twin", "len", "label")

    def end(self):
        return self.twin.start


def reference_insert_size(reads, edges, m, mate):
    """-> the samples the visitor collects, in the order it collects them (vertices in id order)"""
    lens = [len(r) for r in reads]
    arcs = {i: [] for i in range(len(reads))}

    def label(v, d, w, e, ln):  # what w adds to v beyond the overlap, as seen from v (Vertex::merge reads it)
        o = reads[w] if d != e else uc.revcomp(reads[w])
        return o[ln:] if d == E else o[:len(o) - ln]

    def pair(sa, sb, ln):
        a, b = _Arc(), _Arc()
        a.start, a.dir, a.twin, a.len = sa >> 1, sa & 1, b, ln
        b.start, b.dir, b.twin, b.len = sb >> 1, sb & 1, a, ln
        a.label, b.label = label(a.start, a.dir, b.start, b.dir, ln), label(b.start, b.dir, a.start, a.dir, ln)
        arcs[a.start].append(a)
        arcs[b.start].append(b)

    for rec in edges:  # Bigraph::load: the minOverlap filter, EdgeCreator::create, containments in both directions
        c = uc.classify(rec, lens, m)
        if c in ("bad", "low"):
            continue
        sq, st, contain, _ = c
        pair(sq, st, rec[2])
        if contain:
            pair(sq ^ 1, st ^ 1, rec[2])

    def reduced(v, d):  # InsertSizeEstimateVisitor::edges
        es = sorted((a for a in arcs[v] if a.dir == d), key=lambda a: (-a.len, a.label))
        es = [a for a in es if a.len != lens[v]]  # its coordinate on v is all of v and touches an end: v is contained
        out = []
        for a in es:
            if not out or a.len != out[-1].len or a.label != out[-1].label:
                out.append(a)
        return out

    red = set()
    samples = []
    for v in range(len(reads)):
        if v in red:
            continue
        dist = {v: 0}
        red.add(v)
        for start_dir in (E, B):  # ED_SENSE, then ED_ANTISENSE
            d, distance, flag, p = start_dir, 0, (1 if start_dir == E else -1), v
            while True:
                straight = reduced(p, d)
                if len(straight) != 1 or straight[0].end() == p or straight[0].end() in red:
                    break
                single = straight[0]
                twin, end = single.twin, single.end()
                if len(reduced(end, twin.dir)) != 1:
                    break
                p = end
                if d == E:  # forward: the overhang of the read it leaves (single's coordinate)
                    distance += flag * (lens[single.start] - single.len)
                else:  # backward: the overhang of the read it enters (the twin's coordinate)
                    distance += flag * (lens[twin.start] - twin.len)
                if single.dir == twin.dir:  # EC_REVERSE
                    d = 1 - d
                dist[p] = distance
                red.add(p)
        for i, di in dist.items():
            j = mate[i]
            if j != NO_MATE and i < j and j in dist:
                samples.append(abs(dist[j] - di))
    return samples


def comparable(case):
    """the conditions under which the reference's chains are the unitigs and its distance is the left coordinate"""
    reads, lens = case["reads"], [len(r) for r in case["reads"]]
    if len(set(lens)) > 1:
        return False
    if len({min(bytes(r), uc.revcomp(r)) for r in reads}) != len(reads):  # a read given twice, on either strand
        return False
    seen = set()
    for rec in case["edges"]:
        c = uc.classify(rec, lens, case["m"])
        if c in ("bad", "low"):
            continue
        if c[2]:
            return False
        key = (min(c[0], c[1]), max(c[0], c[1]))
        if key in seen:
            return False
        seen.add(key)
    return not any(f & uc.CIRCULAR for f in uc.expected(reads, case["edges"], case["m"])["uflags"])


def pair_up(rng, n, share=0.8):
    """random reciprocal mates over n reads; about `share` of the reads get one"""
    ids = list(range(n))
    rng.shuffle(ids)
    mate = [NO_MATE] * n
    for k in range(0, n - 1, 2):
        if rng.random() < share:
            mate[ids[k]], mate[ids[k + 1]] = ids[k + 1], ids[k]
    return mate


# ---- hand-built graphs ----
def _with(b, name, pairs, extra=None):
    c = b.case(name)
    mate = [NO_MATE] * len(c["reads"])
    for x, y in pairs:
        mate[x], mate[y] = y, x
    for i, v in (extra or {}).items():
        mate[i] = v
    c["mate"] = mate
    return c


@functools.lru_cache(maxsize=None)
def hand_built():
    cases = []
    b = uc._Build(700)  # one chain, all forward: every pair tandem
    ids = b.chain(8, lens=[60] * 8, rc=[False] * 8)
    cases.append(_with(b, "chain_forward", [(ids[0], ids[5]), (ids[1], ids[7]), (ids[2], ids[3])]))
    b = uc._Build(701)  # strands mixed: inward, outward and tandem pairs, and walks that flip
    rc = [False, True, True, False, True, False, False, True, True, False]
    ids = b.chain(10, lens=[60] * 10, rc=rc)
    cases.append(_with(b, "chain_mixed", [(ids[0], ids[1]), (ids[2], ids[3]), (ids[4], ids[9]), (ids[5], ids[8]), (ids[6], ids[7])]))
    b = uc._Build(702)  # the smaller-id terminal at the right: the unitig runs against the chain
    ids = b.chain(6, lens=[60] * 6, rc=[True, False, True, True, False, False], order=[5, 1, 2, 3, 4, 0])
    cases.append(_with(b, "chain_reversed", [(ids[0], ids[4]), (ids[1], ids[5]), (ids[2], ids[3])]))
    b = uc._Build(703)  # two chains: pairs inside each and across
    x = b.chain(5, lens=[60] * 5, rc=[False, True, False, True, False])
    y = b.chain(5, lens=[60] * 5, rc=[True, True, False, False, True])
    cases.append(_with(b, "two_chains", [(x[0], x[3]), (y[1], y[4]), (x[1], y[0]), (x[2], y[2]), (x[4], y[3])]))
    b = uc._Build(704)  # a Y branch: three chains meet, pairs across the junction are ACROSS
    x = b.chain(4, lens=[60] * 4, rc=[False] * 4)
    z = b.read(b.reads[x[3]][-25:] + b.genome(35))
    b.edges.append((x[3], z, 25, 0))
    w = b.read(b.reads[x[3]][-30:] + b.genome(30))
    b.edges.append((x[3], w, 30, 0))
    cases.append(_with(b, "branch", [(x[0], x[2]), (x[1], z), (x[3], w)]))
    b = uc._Build(705)  # singles, a pair of singles, malformed entries
    for _ in range(6):
        b.read(b.genome(60))
    cases.append(_with(b, "singles", [(0, 1), (2, 5)], extra={3: 3, 4: 99}))
    b = uc._Build(706)  # a ring with a pair in it and a link into it
    r = b.chain(3, circular=True, rc=[False, True, False])
    x = b.chain(3, lens=[60] * 3, rc=[False] * 3)
    cases.append(_with(b, "ring", [(r[0], r[2]), (r[1], x[0]), (x[1], x[2])]))
    b = uc._Build(707)  # a containment blocks the chain
    x = b.chain(5, lens=[60] * 5, rc=[False] * 5)
    s = b.read(b.reads[x[2]][5:40])
    b.edges.append((x[2], s, 35, 0))
    cases.append(_with(b, "containment", [(x[0], x[1]), (x[3], x[4]), (x[2], s)]))
    b = uc._Build(708, m=10)  # unequal lengths and a strand flip: the reference's distance mixes left and right ends
    x = b.chain(4, lens=[40, 70, 50, 90], rc=[False, True, False, True], qfirst=[True] * 3)
    cases.append(_with(b, "unequal_flip", [(x[0], x[3]), (x[1], x[2])]))
    return cases


def case_named(name):
    return next(c for c in hand_built() if c["name"] == name)


# ---- seeded random graphs ----
@functools.lru_cache(maxsize=None)
def random_case(seed):
    """chimeric_cases.random_case(seed) -- prune_cases.random_case (at most 12 reads of 40 to 90 bases, random real overlaps, its
    round options) with bridge reads planted and chimeric options -- with random reciprocal mates and a few malformed entries"""
    c = dict(cc.random_case(seed))
    rng = random.Random(7000 + seed)
    n = len(c["reads"])
    mate = pair_up(rng, n)
    for i in range(n):
        if mate[i] == NO_MATE and rng.random() < 0.3:
            mate[i] = rng.choice((i, n + rng.randrange(5), rng.randrange(n)))
    c["mate"] = mate
    return c


UNIFORM_LEN = 60


@functools.lru_cache(maxsize=None)
def random_uniform_case(seed):
    """as prune_cases.random_case grows its graphs, with every read of UNIFORM_LEN bases; one graph in five gets a record
    twice and one in ten a containment, which comparable() turns away: some three in four stay"""
    g = tc._Grow(200000 + seed)
    rng = g.rng
    g.start(UNIFORM_LEN)
    for _ in range(rng.randint(1, 11)):
        x = len(g.w) - 1 if rng.random() < 0.7 else rng.randrange(len(g.w))  # mostly off the newest read: chains, some forks
        g.grow(x, 1, side=rng.choice((B, E)), lens=[UNIFORM_LEN], ovs=[rng.randint(g.m, UNIFORM_LEN - 1)])
    if rng.random() < 0.2:
        g.edges.append(rng.choice(g.edges))
    if rng.random() < 0.1:
        x = rng.randrange(len(g.w))
        g.w.append(g.w[x])
        g.rc.append(g.rc[x])
        g.edges.append((x, len(g.w) - 1, UNIFORM_LEN, 0))
    c = g.case("uniform%d" % seed, 0, 0)
    c["mate"] = pair_up(random.Random(8000 + seed), len(c["reads"]), share=1.0)
    return c
