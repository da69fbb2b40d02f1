"""Cases and two brute forces for non-maximal overlap cutting in the rounds of `siga unitig` (sigax_unitigs_prune_*, the rules
in include/sigax.h); no tests here (tests/test_prune_cases.py, tests/test_gpu_unitig_prune.py).

expected_prune()   the rules, serially from the reads: every step runs unitig_cases.expected over the alive reads and the live
                   records, takes the longest participant per read end, scores every unitig and judges every record.
reference_prune()  the reference's loop on merged vertices (src/assembler.cpp:166-221 without the loop, chimeric and linked-read
                   visitors): vertices with sequence, read count and edge lists; MaximumOverlapVisitor::visit
                   (src/bigraph_visitors.cpp:439-507) as it is written, its sort replaced by the tie rule of sigax.h; the sweep,
                   the simplify passes, TrimVisitor, the sweep, the simplify passes.
The two share nothing but revcomp() and the record classifier.  Every score either of them evaluates must lie at least
SCORE_MARGIN from the case's T (the device's log need not round as libm's does): both assert it.

A case: trim_cases' dict plus delta, careful, N, G, T.  Every kept record is a real overlap of the reads' bytes, except the
read-level self records, which are never merged."""
import functools
import math
import random

from tests import trim_cases as tc
from tests import unitig_cases as uc

B, E = uc.B, uc.E
SCORE_MARGIN = 1e-6
SCORES = None  # a list here collects (score, threshold) of every evaluation of _unique (tests/giant_cases.py asserts a wider margin)


# ---- the rules, serially ----
def _unique(N, K, bases, G, T):
    if bases >= G:  # the reference's unsigned G - bases wraps: not unique
        return False
    second = math.log(float(G - 2 * bases)) if G > 2 * bases else math.log(0.001)
    score = float(N - K) * (math.log(float(G - bases)) - second) - float(K) * math.log(2.0)
    if SCORES is not None:
        SCORES.append((score, T))
    assert abs(score - T) >= SCORE_MARGIN, "a score of %r against T = %r" % (score, T)
    return score >= T


def expected_prune(reads, edges, m, max_rounds, L, C=None, delta=0, careful=False, N=None, G=None, T=13.0, tables_only=False):
    """-> trim_cases.expected_trim's dict plus cut [n_edges], with status [16]; tables_only: as unitig_cases.expected's"""
    n = len(reads)
    N = n if N is None else N
    lens = [uc.nbases(r) for r in reads]
    kept, bad, low = tc._kept(edges, lens, m)
    removed, cut = [0] * n, [0] * len(edges)
    islands = dead_ends = rounds = cut_rounds = uniq_first = 0

    def graph():
        alive = [r for r in range(n) if not removed[r]]
        new = {r: k for k, r in enumerate(alive)}
        live = [(i, c) for i, c in kept if not cut[i] and not removed[edges[i][0]] and not removed[edges[i][1]]]
        sub = [(new[edges[i][0]], new[edges[i][1]], edges[i][2], edges[i][3]) for i, _ in live]
        sub_reads = [reads[r] for r in alive]
        res = uc.expected(sub_reads, sub, m, tables_only)
        deg = [0] * (2 * len(alive))
        for _, (sq, st, contain, _s) in live:
            sq, st = 2 * new[sq >> 1] + (sq & 1), 2 * new[st >> 1] + (st & 1)
            for s in ((sq & ~1, sq | 1, st & ~1, st | 1) if contain else (sq, st)):
                deg[s] += 1
        return alive, new, live, res, deg

    for rnd in range(1, max_rounds + 1):
        changed = False
        if delta > 0:  # the cut step
            alive, new, live, res, _ = graph()
            unit = {}
            uniq = []
            for u in range(len(res["uflags"])):
                lay = res["layout"][res["lay_offs"][u]:res["lay_offs"][u + 1]]
                for p in lay:
                    unit[alive[p[0]]] = u
                uniq.append(_unique(N, len(lay), res["seq_offs"][u + 1] - res["seq_offs"][u], G, T))
            if rnd == 1:
                uniq_first = sum(uniq)
            part = [(i, sq, st, edges[i][2]) for i, (sq, st, contain, _s) in live if not contain]
            mx = {}
            for _, s, t, ln in part:
                mx[s] = max(mx.get(s, 0), ln)
                mx[t] = max(mx.get(t, 0), ln)
            U = lambda s: unit[s >> 1]  # noqa: E731
            at = {}  # state -> [(the record's other state, its length)]
            for _, s, t, ln in part:
                at.setdefault(s, []).append((t, ln))
                at.setdefault(t, []).append((s, ln))
            now = []
            for i, s, t, ln in part:
                for a, b in ((s, t), (t, s)):  # a candidate from a?
                    if not (uniq[U(a)] and mx[a] - ln >= delta):
                        continue
                    if careful:
                        if U(a) != U(b):
                            held = any(mx[b] - lj < delta and U(o) == U(a) for o, lj in at[b])
                        else:
                            held = any(lj == mx[a] and U(o) == U(a) for o, lj in at[a])
                        if held:
                            continue
                    now.append(i)
                    break
            for i in now:  # (after every decision of the step)
                cut[i] = rnd
            if now:
                changed = True
                cut_rounds += 1
        alive, new, live, res, deg = graph()  # the trim step: trim_cases.expected_trim's round
        gone = []
        for u in range(len(res["uflags"])):
            lay = res["layout"][res["lay_offs"][u]:res["lay_offs"][u + 1]]
            first, last = lay[0], lay[-1]
            d_left = deg[2 * first[0] + (E if first[1] & uc.PLACED_REV else B)]
            d_right = deg[2 * last[0] + (B if last[1] & uc.PLACED_REV else E)]
            bases, k = res["seq_offs"][u + 1] - res["seq_offs"][u], len(lay)
            if not (d_left == 0 or d_right == 0) or bases > L:
                continue
            if C is not None and not (k - 1) * max(L, 1) <= (max(C, 1) - 1) * bases:
                continue
            if d_left == 0 and d_right == 0:
                islands += 1
            else:
                dead_ends += 1
            gone += [alive[p[0]] for p in lay]
        for r in gone:
            removed[r] = rnd
        if gone:
            changed = True
        if not changed:
            break
        rounds += 1
    alive, new, live, res, deg = graph()
    res["layout"] = [(alive[r], fl, off) for r, fl, off in res["layout"]]
    where, merged = {}, set()
    for u in range(len(res["uflags"])):
        lay = res["layout"][res["lay_offs"][u]:res["lay_offs"][u + 1]]
        for r, fl, _ in lay:
            where[r] = (u, fl & uc.PLACED_REV)
        for (a, fa, _), (b, fb, _) in zip(lay, lay[1:]):
            merged.add(frozenset((2 * a + (B if fa & uc.PLACED_REV else E), 2 * b + (E if fb & uc.PLACED_REV else B))))
    uedges = []
    for i, (sq, st, contain, self_edge) in live:
        q, t, ln, _ = edges[i]
        simple = not contain and not self_edge and deg[2 * new[q] + (sq & 1)] == 1 and deg[2 * new[t] + (st & 1)] == 1
        if simple and frozenset((sq, st)) in merged:
            continue
        (uq, vq), (ut, vt) = where[q], where[t]
        b0 = 1 if ((sq & 1) ^ vq) == B else 0
        b1 = 1 if ((st & 1) ^ vt) == E else 0
        uedges.append((uq, ut, ln, b0 | (b1 << 1) | ((b0 ^ b1) << 2)))
    dropped = sum(1 for i, _ in kept if not cut[i] and (removed[edges[i][0]] or removed[edges[i][1]]))
    st6 = res["status"]
    res["status"] = [st6[0], st6[1], bad, low, st6[4], st6[5], rounds, islands, dead_ends, sum(1 for x in removed if x), dropped, len(uedges),
                     sum(1 for x in cut if x), cut_rounds, uniq_first, 0]
    res["removed"] = removed
    res["cut"] = cut
    res["uedges"] = uedges
    return res


# ---- the reference's loop ----
class _Arc:
    __slots__ = ("start", "dir", "twin", "len", "block", "rec", "black")


def reference_prune(reads, edges, m, max_rounds, L, C=None, delta=0, careful=False, N=None, G=None, T=13.0):
    """-> ([(sequence, circular, closing overlap)], {read: round removed}, {record: round cut}, rounds that changed something)"""
    lens = [len(r) for r in reads]
    n_all = len(reads) if N is None else N
    verts = {i: {"seq": bytes(r), "arcs": [], "cov": 1, "reads": [i]} for i, r in enumerate(reads)}

    def pair(sa, sb, ln, block, rec):
        a, b = _Arc(), _Arc()
        a.start, a.dir, a.twin, a.len, a.block, a.rec, a.black = sa >> 1, sa & 1, b, ln, block, rec, False
        b.start, b.dir, b.twin, b.len, b.block, b.rec, b.black = sb >> 1, sb & 1, a, ln, block, rec, False
        verts[a.start]["arcs"].append(a)
        verts[b.start]["arcs"].append(b)

    for i, rec in enumerate(edges):  # Bigraph::load
        c = uc.classify(rec, lens, m)
        if c in ("bad", "low"):
            continue
        sq, st, contain, _ = c
        pair(sq, st, rec[2], contain, i)
        if contain:
            pair(sq ^ 1, st ^ 1, rec[2], True, i)

    def simplify(d):  # Bigraph::simplify(dir) with Vertex::merge and Bigraph::merge
        again = True
        while again:
            again = False
            for vid in list(verts):
                v = verts.get(vid)
                if v is None:
                    continue
                mine = [a for a in v["arcs"] if a.dir == d]
                if len(mine) != 1 or mine[0].twin.start == vid or mine[0].block:
                    continue
                arc, twin = mine[0], mine[0].twin
                wid = twin.start
                w = verts[wid]
                if sum(1 for a in w["arcs"] if a.dir == twin.dir) != 1:
                    continue
                if d == E:
                    o = w["seq"] if twin.dir == B else uc.revcomp(w["seq"])
                    v["seq"] = v["seq"] + o[arc.len:]
                else:
                    o = w["seq"] if twin.dir == E else uc.revcomp(w["seq"])
                    v["seq"] = o[:len(o) - arc.len] + v["seq"]
                v["cov"] += w["cov"]
                v["reads"] += w["reads"]
                for x in [a for a in w["arcs"] if a.dir != twin.dir]:
                    w["arcs"].remove(x)
                    x.start, x.dir = vid, d
                    v["arcs"].append(x)
                v["arcs"].remove(arc)
                w["arcs"].remove(twin)
                del verts[wid]
                again = True

    def avg(c, length):  # Point::avg
        return float(max(c, 1) - 1) / max(length, 1)

    def max_overlap_visit(vid, v):  # MaximumOverlapVisitor::visit -> the arcs it colours
        k, dlt = v["cov"], len(v["seq"])
        if dlt >= G:
            return []
        score = (n_all - k) * (math.log(G - dlt) - math.log(G - 2 * dlt if G > 2 * dlt else 0.001)) - k * math.log(2.0)
        assert abs(score - T) >= SCORE_MARGIN
        if score < T:
            return []
        out = []
        for d in (E, B):
            fwd = [a for a in v["arcs"] if a.dir == d and not a.block]
            if not fwd:
                continue
            top = max(a.len for a in fwd)
            for a in fwd:
                if top - a.len < delta:
                    continue
                if careful:
                    if a.twin.start != vid:  # not a self edge
                        rev = [x for x in verts[a.twin.start]["arcs"] if x.dir == a.twin.dir and not x.block]
                        top2 = max(x.len for x in rev)
                        if any(x.twin.start == vid and top2 - x.len < delta for x in rev):
                            continue
                    elif any(x.twin.start == vid for x in fwd if x.len == top):
                        continue
                out.append(a)
        return out

    def sweep_arcs(arcs):
        for a in arcs:
            for x in (a, a.twin):
                if x in verts[x.start]["arcs"]:
                    verts[x.start]["arcs"].remove(x)

    simplify(E)
    simplify(B)
    gone, cuts, rounds = {}, {}, 0
    for rnd in range(1, max_rounds + 1):
        modified = False
        if delta > 0:
            black = []
            for vid, v in verts.items():  # it only colours
                black += max_overlap_visit(vid, v)
            if black:
                modified = True
                for a in black:
                    cuts[a.rec] = rnd
                sweep_arcs(black)
                simplify(E)
                simplify(B)
        black = []
        for vid, v in verts.items():  # TrimVisitor::visit
            deg = [sum(1 for a in v["arcs"] if a.dir == d) for d in (B, E)]
            short = len(v["seq"]) <= L and (C is None or avg(v["cov"], len(v["seq"])) <= avg(C, L))
            if short and (deg[B] == 0 or deg[E] == 0):
                black.append(vid)
        if black:
            modified = True
            for vid in black:  # sweepVertices
                for a in verts[vid]["arcs"]:
                    if a.twin.start != vid:
                        verts[a.twin.start]["arcs"].remove(a.twin)
                for r in verts[vid]["reads"]:
                    gone[r] = rnd
                del verts[vid]
            simplify(E)
            simplify(B)
        if not modified:
            break
        rounds += 1
    out = []
    for vid, v in verts.items():
        loop = [a for a in v["arcs"] if not a.block and a.twin.start == vid and a.dir == E and a.twin.dir == B and v["cov"] > 1 and
                len(v["arcs"]) == 2]
        out.append((v["seq"], True, loop[0].len) if loop else (v["seq"], False, 0))
    return out, gone, cuts, rounds


# ---- hand-built graphs ----
def _case(g, name, x, L, delta, careful=False, N=1000, G=10000, T=10.0, C=None, **claims):
    c = g.case(name, x, L, C, **claims)
    c.update(delta=delta, careful=careful, N=N, G=G, T=T)
    return c


def rec_between(case, a, b, length=None):
    """the index of the record between reads a and b (of that length)"""
    hits = [i for i, (q, t, ln, _) in enumerate(case["edges"]) if {q, t} == {a, b} and (length is None or ln == length)]
    assert len(hits) == 1, (case["name"], a, b, hits)
    return hits[0]


def _fork(seed, ov_long=40, ov_short=25, third=None):
    """a three-read unitig a whose E end meets w (three reads, over ov_long) and l (two reads of 50, 78 bases, over ov_short); l's
    far end forks again into z and z2, so that l is no dead end before its record to a is cut"""
    g = tc._Grow(seed)
    a = g.chain(3, lens=[60] * 3, ovs=[22, 22])
    w = g.grow(a[2], 3, lens=[60] * 3, ovs=[ov_long, 22, 22])
    lo = g.grow(a[2], 2, lens=[50, 50], ovs=[ov_short, 22])
    z = g.grow(lo[1], 3, lens=[60] * 3, ovs=[22, 22, 22])
    z2 = g.grow(lo[1], 3, lens=[60] * 3, ovs=[24, 22, 22])
    t = g.grow(a[2], 1, lens=[60], ovs=[third]) if third else []
    return g, a, w, lo, z, z2, t


@functools.lru_cache(maxsize=None)
def hand_built():
    """claims: trim_cases' keys, and cut (records cut), cut_rounds, unique (status[14]), cut_recs {(read, read): round}, kept_recs
    [(read, read)]"""
    cases = []
    for careful in (False, True):
        tag = "_careful" if careful else ""
        # 1: the shorter record of a fork at a unique unitig is cut, the loser is a dead end and goes in the same round, the winner
        # merges (careful: the loser's own end knows no better record, so the record is held back)
        g, a, w, lo, z, z2, _ = _fork(1)
        if careful:
            cases.append(_case(g, "fork" + tag, 10, 100, 10, True, T=10.0, cut=0, rounds=0, unitigs=5, unique=4, kept_recs=[(a[2], lo[0])]))
        else:
            cases.append(_case(g, "fork", 10, 100, 10, T=10.0, cut=1, cut_rounds=1, rounds=1, unitigs=3, gone=2, dead_ends=1, unique=4,
                               cut_recs={(a[2], lo[0]): 1}, removed_ids=lo, kept_ids=a + w + z + z2, by_round={1: lo}))
        # 2: the same fork, nothing unique
        g, a, w, lo, z, z2, _ = _fork(1)
        cases.append(_case(g, "fork_not_unique" + tag, 10, 100, 10, careful, T=50.0, cut=0, rounds=0, unitigs=5, unique=0))
        # 3: a difference below delta
        g, a, w, lo, z, z2, _ = _fork(2, 40, 31)
        cases.append(_case(g, "below_delta" + tag, 10, 100, 10, careful, T=10.0, cut=0, rounds=0, unitigs=5))
        # 4: ties at the maximum with delta 1: both stay, the shorter third goes
        g, a, w, lo, z, z2, t = _fork(3, 40, 40, third=39)
        if not careful:
            cases.append(_case(g, "ties", 10, 30, 1, T=10.0, cut=1, cut_recs={(a[2], t[0]): 1}, kept_recs=[(a[2], w[0]), (a[2], lo[0])]))
    # 5: unique on one side only: q's record to the unique u is short at both its ends; only u's side may cut it.  v2's fork
    # lies between single reads: nothing there is unique
    for careful in (False, True):
        g = tc._Grow(5)
        u = g.chain(3, lens=[60] * 3, ovs=[22, 22])
        p = g.grow(u[2], 1, lens=[70], ovs=[40])
        q = g.grow(u[2], 1, lens=[70], ovs=[25])
        v = g.grow(q[0], 1, side=B, lens=[70], ovs=[45])
        v2 = g.start(70)
        r1 = g.grow(v2, 1, lens=[70], ovs=[40])
        r2 = g.grow(v2, 1, lens=[70], ovs=[25])
        # (careful, 6b: non-maximal at both its ends: cut all the same)
        cases.append(_case(g, "one_side" + ("_careful" if careful else ""), 10, 30, 10, careful, T=10.0, cut=1, unique=1,
                           cut_recs={(u[2], q[0]): 1}, kept_recs=[(v2, r1[0]), (v2, r2[0]), (v[0], q[0]), (u[2], p[0])]))
    # 6c: careful, held back only through a parallel record: q's B end meets u's E end over 25 and u's B end over 45
    for careful in (False, True):
        g = tc._Grow(6)
        q = g.start(80, rc=False)
        u0 = g.start(60, rc=False)
        g.w[u0] = uc.revcomp(g.w[q][:45]) + g.genome(15)
        u1 = g.grow(u0, 1, lens=[60], ovs=[22])[0]
        u2 = g.start(60, rc=False)
        g.w[u2] = g.w[u1][-22:] + g.genome(13) + g.w[q][:25]
        g.rc[u1] = False
        g.edges = [(u0, u1, 22, 0), (u1, u2, 22, 0), (u2, q, 25, 0), (q, u0, 45, 5)]
        p = g.grow(u2, 1, lens=[70], ovs=[40])
        if careful:
            cases.append(_case(g, "parallel_careful", 10, 30, 10, True, T=10.0, cut=0, unique=1, kept_recs=[(u2, q)]))
        else:
            cases.append(_case(g, "parallel", 10, 30, 10, T=10.0, cut=1, unique=1, cut_recs={(u2, q): 1}, kept_recs=[(q, u0), (u2, p[0])]))
    # 7: self records of the merged vertex.  A ring with a longer tip at one of its ends: the ring's own record is short there and is
    # cut in both modes.  A ring whose end also carries a longer read-level self record: careful holds the ring's record back
    for careful in (False, True):
        tag = "_careful" if careful else ""
        g = tc._Grow(7)
        ring = g.ring(4)
        tip = g.grow(ring[1], 3, lens=[60] * 3, ovs=[40, 22, 22])
        cases.append(_case(g, "self_tip" + tag, 10, 30, 10, careful, T=10.0, cut=1, cut_recs={(ring[1], ring[2]): 1}, unitigs=1, cycles=0))
        g = tc._Grow(8)
        ring = g.ring(4)
        g.edges.append((ring[1], ring[1], 35, 5 if g.rc[ring[1]] else 6))  # (both touches at the end that faces ring[2])
        if careful:
            cases.append(_case(g, "self_self" + tag, 10, 30, 10, True, T=10.0, cut=0, unitigs=1, kept_recs=[(ring[1], ring[2])]))
        else:
            cases.append(_case(g, "self_self", 10, 30, 10, T=10.0, cut=1, cut_recs={(ring[1], ring[2]): 1}, unitigs=1))
    # 8: what takes no part: a ring, a live containment at a fork (length 45: as a maximum it would cut both arms), a malformed
    # record of length 1000 and a low one.  T = 4: every read is unique
    g = tc._Grow(9)
    u = g.chain(3, lens=[60] * 3, ovs=[22, 22])
    p = g.grow(u[2], 1, lens=[70], ovs=[30])
    q = g.grow(u[2], 1, lens=[70], ovs=[25])
    s = g.start(45, rc=g.rc[u[2]])
    g.w[s] = g.w[u[2]][15:60]
    g.edges += [(u[2], s, 45, 0), (u[2], p[0], 1000, 0), (u[2], q[0], 19, 0)]
    ring = g.ring(3)
    cases.append(_case(g, "bystanders", 10, 30, 10, T=4.0, cut=0, rounds=0, cycles=1, kept_ids=u + p + q + [s] + ring))
    cases.append(dict(cases[-1], name="bystanders_careful", careful=True))
    # 9, 10: a cascade: c0 .. c3 is one unitig, and unique, only once round 1 has trimmed the tip at c1; round 2 cuts at its fork
    for name, x in (("cascade", 10), ("cascade_1round", 1)):
        g = tc._Grow(10)
        c = g.chain(4, lens=[80] * 4, ovs=[22, 22, 22])
        tip = g.grow(c[1], 1, lens=[40], ovs=[24])
        w = g.grow(c[3], 3, lens=[60] * 3, ovs=[40, 22, 22])
        lo = g.grow(c[3], 2, lens=[50, 50], ovs=[25, 22])
        g.grow(lo[1], 3, lens=[60] * 3, ovs=[22, 22, 22])
        g.grow(lo[1], 3, lens=[60] * 3, ovs=[24, 22, 22])
        if x == 10:
            cases.append(_case(g, name, x, 100, 10, T=18.0, cut=1, cut_rounds=1, rounds=2, gone=3, unique=0, cut_recs={(c[3], lo[0]): 2},
                               by_round={1: tip, 2: lo}, kept_ids=c + w))
        else:  # max_rounds reached before the loop is idle
            cases.append(_case(g, name, x, 100, 10, T=18.0, cut=0, rounds=1, gone=1, by_round={1: tip}, kept_ids=c + w + lo))
    # 11: bases < G <= 2 bases: log(0.001) stands in; the merged a + w of round 2 has more than G bases and is not unique
    g, a, w, lo, z, z2, _ = _fork(11)
    cases.append(_case(g, "small_genome", 10, 100, 10, N=14, G=200, T=13.0, cut=1, cut_recs={(a[2], lo[0]): 1}, unique=4))
    # 12: one read end with 300 records, and 3 000 reads in chains of 10
    g = tc._Grow(12)
    hub = g.start(150)
    for k in range(300):
        g.grow(hub, 1, lens=[110 + k % 21], ovs=[20 + (k * 7) % 90])
    for k in range(300):
        g.chain(10, lens=[60] * 10)
    cases.append(_case(g, "hub300", 3, 100, 10, N=100000, G=1000000, T=13.0, unique=301, cut_rounds=1))
    cases.append(dict(cases[-1], name="hub300_careful", careful=True, claims={"unique": 301}))
    return cases


def case_named(name):
    return next(c for c in hand_built() if c["name"] == name)


def run(fn, case, max_rounds=None, **over):
    kw = {k: case[k] for k in ("delta", "careful", "N", "G", "T")}
    kw.update(over)
    return fn(case["reads"], case["edges"], case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"], **kw)


@functools.lru_cache(maxsize=None)
def expected_of(name, max_rounds=None):
    return run(expected_prune, case_named(name), max_rounds)


# ---- seeded random graphs: at most 12 reads, random real overlaps ----
@functools.lru_cache(maxsize=None)
def random_case(seed):
    g = tc._Grow(100000 + seed)
    rng = g.rng
    g.start(rng.randint(40, 90))
    for _ in range(rng.randint(1, 11)):
        x = rng.randrange(len(g.w))
        ln = rng.randint(40, 90)
        g.grow(x, 1, side=rng.choice((B, E)), lens=[ln], ovs=[rng.randint(g.m, min(ln, len(g.w[x])) - 1)])
    for rec in list(g.edges):
        if rng.random() < 0.15:  # a parallel record
            g.edges.append(rec)
    return _case(g, "random%d" % seed, rng.randint(1, 4), rng.choice((50, 80, 150)), rng.randint(1, 30), rng.random() < 0.5,
                 T=rng.choice((3.0, 7.0, 10.0)))


# ---- one larger seeded graph: about 20 000 reads and 60 000 records ----
@functools.lru_cache(maxsize=None)
def large_case(n_reads=20000, seed=5):
    """reads of 100 drawn from a random genome at 9-fold coverage, one read in five with a substitution; records for every
    suffix-prefix overlap of at least 45 between neighbours in start order on the forward strand (all stored forward)"""
    rng = random.Random(seed)
    glen = n_reads * 100 // 9
    genome = bytes(rng.choice(b"ACGT") for _ in range(glen))
    starts = sorted(rng.randrange(glen - 100) for _ in range(n_reads))
    reads = []
    for p in starts:
        w = bytearray(genome[p:p + 100])
        if rng.random() < 0.2:
            at = rng.randrange(100)
            w[at] = rng.choice([b for b in b"ACGT" if b != w[at]])
        reads.append(bytes(w))
    order = list(range(n_reads))
    rng.shuffle(order)  # read ids in any order
    ids = {k: order[k] for k in range(n_reads)}
    edges = []
    for k in range(n_reads):
        for j in range(k + 1, min(k + 8, n_reads)):
            ov = 100 - (starts[j] - starts[k])
            if ov < 45 or ov >= 100:
                continue
            if reads[k][100 - ov:] == reads[j][:ov]:
                edges.append((ids[k], ids[j], ov, 0) if rng.random() < 0.5 else (ids[j], ids[k], ov, 3))
    by_id = [None] * n_reads
    for k in range(n_reads):
        by_id[ids[k]] = reads[k]
    rng.shuffle(edges)
    return {"name": "large", "reads": by_id, "edges": edges, "m": 45, "x": 4, "L": 150, "C": None, "delta": 10, "careful": False,
            "N": n_reads, "G": glen, "T": 13.0, "claims": {}}
