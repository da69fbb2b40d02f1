"""Cases and two brute forces for tip trimming and the lifted records of `siga unitig` (sigax_unitigs_trim_*, the rules in
include/sigax.h); no tests here (tests/test_trim_cases.py, tests/test_gpu_unitig_trim.py).

expected_trim()   the rules, serially: every round runs unitig_cases.expected over the alive reads renumbered in id order,
                  recomputes the degrees with the classifier and judges each unitig by its two end degrees, bases and reads.
reference_trim()  the reference's own loop at vertex level (src/assembler.cpp:138-159): vertices with merged sequence, read
                  count and edge lists; TrimVisitor's test per vertex (src/bigraph_visitors.cpp:1119-1161), the sweep, then the
                  SENSE and ANTISENSE simplify passes, until a round changes nothing or N rounds are done.
The two share nothing but revcomp() and the record classifier; they are compared as canonical sequence sets and as read ->
round maps.

A case: unitig_cases' dict plus x (max_rounds), L (min_branch_length), C (min_branch_coverage or None) and `claims`, what the
case was built to show.  Here EVERY kept record is a real overlap of the reads' bytes: a record at a branch becomes simple once
the other branch is gone."""
import functools
import random

from tests import unitig_cases as uc

B, E = uc.B, uc.E


def _kept(edges, lens, m):
    """[(index, class)] of the kept records, and the counts of the others"""
    kept, bad, low = [], 0, 0
    for i, rec in enumerate(edges):
        c = uc.classify(rec, lens, m)
        if c == "bad":
            bad += 1
        elif c == "low":
            low += 1
        else:
            kept.append((i, c))
    return kept, bad, low


# ---- the rules, serially ----
def expected_trim(reads, edges, m, max_rounds, L, C=None, tables_only=False):
    """-> unitig_cases.expected's dict over the final graph (layout with the original read ids, alive reads only) plus
    removed [n], uedges [(query, target, length, af)] and status [12]; tables_only: as unitig_cases.expected's"""
    n = len(reads)
    lens = [uc.nbases(r) for r in reads]
    kept, bad, low = _kept(edges, lens, m)
    removed = [0] * n
    islands = dead_ends = rounds = 0

    def graph():
        alive = [r for r in range(n) if not removed[r]]
        new = {r: k for k, r in enumerate(alive)}
        sub = [(new[edges[i][0]], new[edges[i][1]], edges[i][2], edges[i][3]) for i, _ in kept
               if not removed[edges[i][0]] and not removed[edges[i][1]]]
        sub_reads = [reads[r] for r in alive]
        res = uc.expected(sub_reads, sub, m, tables_only)
        deg = [0] * (2 * len(alive))
        sub_lens = [uc.nbases(r) for r in sub_reads]
        for rec in sub:
            sq, st, contain, _ = uc.classify(rec, sub_lens, m)
            for s in ((sq & ~1, sq | 1, st & ~1, st | 1) if contain else (sq, st)):
                deg[s] += 1
        return alive, res, deg

    for rnd in range(1, max_rounds + 1):
        alive, res, deg = graph()
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
        if not gone:
            break
        rounds += 1
        for r in gone:  # (after every decision of the round)
            removed[r] = rnd
    alive, res, deg = graph()
    res["layout"] = [(alive[r], fl, off) for r, fl, off in res["layout"]]
    where = {}  # read -> (unitig, placed reversed)
    merged = set()  # the two read ends a merge joined
    for u in range(len(res["uflags"])):
        lay = res["layout"][res["lay_offs"][u]:res["lay_offs"][u + 1]]
        for r, fl, _ in lay:
            where[r] = (u, fl & uc.PLACED_REV)
        for (a, fa, _), (b, fb, _) in zip(lay, lay[1:]):
            merged.add(frozenset((2 * a + (B if fa & uc.PLACED_REV else E), 2 * b + (E if fb & uc.PLACED_REV else B))))
    new = {r: k for k, r in enumerate(alive)}
    uedges, dropped = [], 0
    for i, (sq, st, contain, self_edge) in kept:
        q, t, ln, _ = edges[i]
        if removed[q] or removed[t]:
            dropped += 1
            continue
        simple = not contain and not self_edge and deg[2 * new[q] + (sq & 1)] == 1 and deg[2 * new[t] + (st & 1)] == 1
        if simple and frozenset((sq, st)) in merged:
            continue
        (uq, vq), (ut, vt) = where[q], where[t]
        b0 = 1 if ((sq & 1) ^ vq) == B else 0
        b1 = 1 if ((st & 1) ^ vt) == E else 0
        uedges.append((uq, ut, ln, b0 | (b1 << 1) | ((b0 ^ b1) << 2)))
    st6 = res["status"]
    res["status"] = [st6[0], st6[1], bad, low, st6[4], st6[5], rounds, islands, dead_ends, sum(1 for x in removed if x), dropped, len(uedges)]
    res["removed"] = removed
    res["uedges"] = uedges
    return res


# ---- the reference's loop ----
class _Arc:
    __slots__ = ("start", "dir", "twin", "len", "block")


def reference_trim(reads, edges, m, max_rounds, L, C=None):
    """-> ([(sequence, circular, overlap of the edge left on a circular vertex)], {read: round it was removed in}, rounds that
    removed something)"""
    lens = [len(r) for r in reads]
    verts = {i: {"seq": bytes(r), "arcs": [], "cov": 1, "reads": [i]} for i, r in enumerate(reads)}

    def pair(sa, sb, ln, block):
        a, b = _Arc(), _Arc()
        a.start, a.dir, a.twin, a.len, a.block = sa >> 1, sa & 1, b, ln, block
        b.start, b.dir, b.twin, b.len, b.block = sb >> 1, sb & 1, a, ln, block
        verts[a.start]["arcs"].append(a)
        verts[b.start]["arcs"].append(b)

    for rec in edges:  # Bigraph::load
        c = uc.classify(rec, lens, m)
        if c in ("bad", "low"):
            continue
        sq, st, contain, _ = c
        pair(sq, st, rec[2], contain)
        if contain:
            pair(sq ^ 1, st ^ 1, rec[2], True)

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

    simplify(E)
    simplify(B)
    gone, rounds = {}, 0
    for rnd in range(1, max_rounds + 1):
        black = []
        for vid, v in verts.items():  # TrimVisitor::visit: it only colours
            deg = [sum(1 for a in v["arcs"] if a.dir == d) for d in (B, E)]
            short = len(v["seq"]) <= L and (C is None or avg(v["cov"], len(v["seq"])) <= avg(C, L))
            if short and (deg[B] == 0 or deg[E] == 0):
                black.append(vid)
        if not black:
            break
        rounds += 1
        for vid in black:  # sweepVertices: the vertex with its edges and their twins
            for a in verts[vid]["arcs"]:
                if a.twin.start != vid:
                    verts[a.twin.start]["arcs"].remove(a.twin)
            for r in verts[vid]["reads"]:
                gone[r] = rnd
            del verts[vid]
        simplify(E)
        simplify(B)
    out = []
    for vid, v in verts.items():
        # a ring: the one edge at E is the one edge at B (simplify leaves it: it would merge the vertex with itself)
        loop = [a for a in v["arcs"] if not a.block and a.twin.start == vid and a.dir == E and a.twin.dir == B and v["cov"] > 1 and
                len(v["arcs"]) == 2]
        out.append((v["seq"], True, loop[0].len) if loop else (v["seq"], False, 0))
    return out, gone, rounds


def canonical_reference(ref):
    return sorted(uc.canonical(s, c, k) for s, c, k in ref)


# ---- hand-built graphs: every record a real overlap ----
class _Grow:
    """Reads as strings in one shared orientation (w), stored on either strand (rc); new reads grow off the right or the left
    end of an existing one, so that branches are real: both arms begin with the junction read's last bases."""

    def __init__(self, seed, m=20):
        self.rng = random.Random(seed)
        self.m, self.w, self.rc, self.edges = m, [], [], []

    def genome(self, n):
        return bytes(self.rng.choice(b"ACGT") for _ in range(n))

    def _len(self):
        return self.rng.randint(self.m + 10, self.m + 40)

    def _record(self, x, y, ov):  # x lies left of y
        rx, ry = self.rc[x], self.rc[y]
        if self.rng.random() < 0.5:
            q, t, af = x, y, (1 if rx else 0) | (2 if ry else 0)
        else:
            q, t, af = y, x, (0 if ry else 1) | (0 if rx else 2)
        self.edges.append((q, t, ov, af | (((af ^ (af >> 1)) & 1) << 2)))

    def start(self, length=None, rc=None):
        self.w.append(self.genome(length or self._len()))
        self.rc.append(self.rng.random() < 0.5 if rc is None else rc)
        return len(self.w) - 1

    def grow(self, x, k, side=E, lens=None, ovs=None, desc=False):
        """k new reads off read x's right (side E) or left (B) end, each overlapping the one before by m .. m + 5 (or ovs[i]);
        ids ascend away from x, or descend (desc) -> the new ids, nearest first"""
        ids = list(range(len(self.w), len(self.w) + k))
        if desc:
            ids.reverse()
        self.w += [None] * k
        self.rc += [None] * k
        prev = x
        for i, new in enumerate(ids):
            ln = lens[i] if lens else self._len()
            ov = ovs[i] if ovs else self.rng.randint(self.m, self.m + 5)
            assert ov < ln and ov < len(self.w[prev])
            self.w[new] = self.w[prev][-ov:] + self.genome(ln - ov) if side == E else self.genome(ln - ov) + self.w[prev][:ov]
            self.rc[new] = self.rng.random() < 0.5
            if side == E:
                self._record(prev, new, ov)
            else:
                self._record(new, prev, ov)
            prev = new
        return ids

    def chain(self, k, lens=None, ovs=None, desc=False):
        s = self.start(lens[0] if lens else None)
        return [s] + self.grow(s, k - 1, lens=lens[1:] if lens else None, ovs=ovs, desc=desc)

    def ring(self, k):
        lens = [self.rng.randint(self.m + 35, self.m + 40) for _ in range(k)]
        ovs = [self.rng.randint(self.m, self.m + 2) for _ in range(k)]
        pos = [0]
        for i in range(k):
            pos.append(pos[-1] + lens[i] - ovs[i])
        g = self.genome(pos[k])
        assert all(ln <= len(g) for ln in lens)
        gg = g + g
        ids = []
        for i in range(k):
            self.w.append(gg[pos[i]:pos[i] + lens[i]])
            self.rc.append(self.rng.random() < 0.5)
            ids.append(len(self.w) - 1)
        for i in range(k):
            self._record(ids[i], ids[(i + 1) % k], ovs[i])
        return ids

    def case(self, name, x, L, C=None, **claims):
        e = list(self.edges)
        self.rng.shuffle(e)  # records in any order
        reads = [uc.revcomp(w) if rc else w for w, rc in zip(self.w, self.rc)]
        return {"name": name, "reads": reads, "edges": e, "m": self.m, "x": x, "L": L, "C": C, "claims": claims}


HUGE = 1 << 30


@functools.lru_cache(maxsize=None)
def hand_built():
    """claims: rounds (status[6]), unitigs (status[0]), cycles (status[5]), islands, dead_ends, gone (reads removed), removed_ids
    (each of them removed), kept_ids (none of them removed), afs (the af values of the lifted records)"""
    cases = []
    g = _Grow(1)  # a Y with one single-read arm: without it the two other pieces are one unitig
    a = g.chain(3, lens=[50] * 3)
    tip = g.grow(a[2], 1, lens=[40])
    g.grow(a[2], 3, lens=[50] * 3)
    cases.append(g.case("y", 10, 60, rounds=1, unitigs=1, dead_ends=1, gone=1, removed_ids=tip))
    for k in (63, 64, 65, 200):  # a multi-read tip: the mark reaches every read of it, over a wave and over the jumping rounds
        g = _Grow(10 + k)
        ring = g.ring(5)
        tip = g.grow(ring[2], k, side=E if k % 2 else B, desc=k in (64, 65))
        cases.append(g.case("tip%d" % k, 10, HUGE, rounds=1, unitigs=1, cycles=1, dead_ends=1, gone=k, removed_ids=tip, kept_ids=ring))
    g = _Grow(2)  # tips on tips on a tip on a backbone: three removing rounds
    bb = g.chain(6, lens=[60] * 6)
    t1 = g.grow(bb[2], 1)
    t2 = g.grow(t1[0], 1) + g.grow(t1[0], 1)
    t3 = [g.grow(t, 1)[0] for t in t2 for _ in range(2)]
    cases.append(g.case("cascade", 10, 60, rounds=3, unitigs=1, dead_ends=7, gone=7, removed_ids=t1 + t2 + t3, kept_ids=bb,
                        by_round={1: t3, 2: t2, 3: t1}))
    g = _Grow(3)  # both arms of a fork short
    a = g.chain(4, lens=[60] * 4)
    arms = g.grow(a[3], 1) + g.grow(a[3], 1)
    cases.append(g.case("fork_short", 10, 60, rounds=1, unitigs=1, dead_ends=2, removed_ids=arms, kept_ids=a))
    g = _Grow(4)  # islands: a short read, a short chain of exactly L bases, one of L + 1 (kept), a long chain (kept)
    one = g.start(40)
    at_l = g.chain(2, lens=[50, 50], ovs=[20])
    above = g.chain(2, lens=[50, 51], ovs=[20])
    long_chain = g.chain(5, lens=[60] * 5)
    cases.append(g.case("islands", 10, 80, rounds=1, unitigs=2, islands=2, dead_ends=0, gone=3, removed_ids=[one] + at_l,
                        kept_ids=above + long_chain))
    g = _Grow(5)  # a ring shorter than L: never a dead end
    ring = g.ring(3)
    cases.append(g.case("ring_short", 10, 500, rounds=0, unitigs=1, cycles=1, gone=0, kept_ids=ring))
    g = _Grow(6)  # a ring with a tip: the tip goes in round 1, the ring closes
    ring = g.ring(4)
    tip = g.grow(ring[1], 1, lens=[40])
    cases.append(g.case("ring_tip", 10, 60, rounds=1, unitigs=1, cycles=1, dead_ends=1, removed_ids=tip, kept_ids=ring))
    g = _Grow(7)  # a live containment: all four ends of its two reads carry it, neither read ever goes
    c = g.chain(4, lens=[60] * 4)
    s = g.start(25, rc=g.rc[c[1]])
    g.w[s] = g.w[c[1]][5:30]
    g.edges.append((c[1], s, 25, 0))
    cases.append(g.case("containment", 10, HUGE, rounds=1, unitigs=2, gone=3, removed_ids=[c[0], c[2], c[3]], kept_ids=[c[1], s], afs={0}))
    g = _Grow(8)  # self edges: both touches at E and a free short B end (goes); E to B (stays)
    r1, r2 = g.start(40), g.start(40)
    g.edges += [(r1, r1, 21, 6), (r2, r2, 21, 0)]
    long_chain = g.chain(5, lens=[60] * 5)
    cases.append(g.case("self", 10, 60, rounds=1, unitigs=2, dead_ends=1, islands=0, removed_ids=[r1], kept_ids=[r2] + long_chain))
    g = _Grow(9)  # tips held only by a record below m or a malformed one: islands
    c = g.chain(4, lens=[60] * 4)
    w1, w2 = g.start(40), g.start(40)
    g.edges += [(c[1], w1, 19, 0), (c[2], w2, 25, 4), (w2, len(g.w), 25, 0)]
    cases.append(g.case("weak_tip", 10, 60, rounds=1, unitigs=1, islands=2, dead_ends=0, removed_ids=[w1, w2], kept_ids=c))
    g = _Grow(11)  # the first and the last read id removed
    t0 = g.start(40)
    j = g.grow(t0, 1, lens=[60])[0]
    g.grow(j, 3, side=B, lens=[60] * 3)
    bb = g.grow(j, 4, lens=[60] * 4)
    tl = g.grow(bb[1], 1, lens=[40])[0]
    assert t0 == 0 and tl == len(g.w) - 1
    cases.append(g.case("id0_last", 10, 60, rounds=1, unitigs=1, dead_ends=2, gone=2, removed_ids=[t0, tl]))
    g = _Grow(12)  # everything goes
    a = g.chain(3)
    g.grow(a[2], 2)
    g.grow(a[2], 2)
    g.start(30)
    cases.append(g.case("all_removed", 10, HUGE, rounds=1, unitigs=0, gone=len(g.w)))
    for name, cov in (("coverage", 2), ("coverage_off", None)):  # two tips of at most L bases: C spares the one of four reads
        g = _Grow(13)
        bb = g.chain(8, lens=[60] * 8)
        thin = g.grow(bb[2], 1, lens=[50])
        thick = g.grow(bb[5], 4, lens=[40] * 4, ovs=[35] * 4)
        if cov is None:
            cases.append(g.case(name, 10, 60, None, rounds=1, unitigs=1, gone=5, removed_ids=thin + thick))
        else:
            cases.append(g.case(name, 10, 60, cov, rounds=1, gone=1, removed_ids=thin, kept_ids=thick))
    g = _Grow(14)  # the graph: junctions between multi-read unitigs on either strand, ids ascending and descending
    for k in range(12):
        a = g.chain(3, lens=[60] * 3, desc=k % 2 == 1)
        g.grow(a[-1], 3, lens=[60] * 3, desc=k % 3 == 0)
        g.grow(a[-1], 3, lens=[60] * 3, desc=k % 4 < 2)
        g.grow(a[0], 3, side=B, lens=[60] * 3, desc=k % 3 == 1)
        g.grow(a[0], 3, side=B, lens=[60] * 3, desc=k % 4 >= 2)
        g.grow(a[1], 1, lens=[40])  # (and a tip, so that rounds run)
    cases.append(g.case("graph", 10, 60, rounds=1, gone=12, afs={0, 3, 5, 6}, reversed_multi=True))
    return cases


def case_named(name):
    return next(c for c in hand_built() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected_of(name, max_rounds=None):
    c = case_named(name)
    return expected_trim(c["reads"], c["edges"], c["m"], c["x"] if max_rounds is None else max_rounds, c["L"], c["C"])


# ---- end to end: the 600 error-free reads and 80 reads with one substitution near an end ----
# (a seed under which a second round removes something: an error read behind another one's tip)
E2E_ERR_SEED, E2E_ERR_READS, E2E_ERR_WITHIN, E2E_L, E2E_ROUNDS = 3, 80, 30, 60, 10


@functools.lru_cache(maxsize=None)
def end_to_end():
    """unitig_cases.end_to_end() plus 80 reads of the same genome, both strands, each with one substitution within 30 bases of an end"""
    base = uc.end_to_end()
    rng = random.Random(E2E_ERR_SEED)
    g = base["genome"]
    reads = list(base["reads"])
    for i in range(E2E_ERR_READS):
        p = rng.randrange(uc.E2E_GENOME - uc.E2E_LEN + 1)
        w = bytearray(g[p:p + uc.E2E_LEN])
        at = rng.randrange(E2E_ERR_WITHIN)
        if rng.random() < 0.5:
            at = uc.E2E_LEN - 1 - at
        w[at] = rng.choice([b for b in b"ACGT" if b != w[at]])
        w = bytes(w)
        reads.append(("e%d" % i, uc.revcomp(w) if rng.random() < 0.5 else w))
    return {"genome": g, "reads": reads, "m": base["m"], "L": E2E_L, "x": E2E_ROUNDS}


def render_graph(res):
    """the (reads, result) pair siga_amd.overlap.format_asqg takes, for the unitig graph of a result"""
    verts = []
    for u in range(len(res["uflags"])):
        k = int(res["lay_offs"][u + 1]) - int(res["lay_offs"][u])
        verts.append(("unitig-%d" % u, "CR:i:%d" % k if k > 1 else None, bytes(res["useqs"][int(res["seq_offs"][u]):int(res["seq_offs"][u + 1])])))
    return verts


def render_removed(names, removed):
    return "".join("%s\t%d\n" % (names[r], int(x)) for r, x in enumerate(removed) if int(x))
