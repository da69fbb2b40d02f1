"""Cases and two brute forces for chimeric unitig removal in the rounds of `siga unitig` (sigax_unitigs_chimeric_*, the rules in
include/sigax.h); no tests here (tests/test_chimeric_cases.py, tests/test_gpu_unitig_chimeric.py).

expected_chimeric()   the rules, serially from the reads: every step runs unitig_cases.expected over the alive reads and the live
                      records; the chimeric step finds the two outward read ends of every unitig, their one record, the read ends
                      at its other side, and judges by degrees, bases, reads and score.
reference_chimeric()  the reference's loop on merged vertices (src/assembler.cpp:166-221 without the loop and linked-read
                      visitors): vertices with sequence, read count and edge lists; MaximumOverlapVisitor, TrimVisitor and
                      ChimericVisitor::visit (src/bigraph_visitors.cpp:88-193) as it is written except for the end rule of sigax.h
                      (the neighbour's degree and edge list are those of the end the edge's twin leaves from), each with its sweep
                      and the simplify passes.  The reference asserts a graph without containments; here a vertex whose one edge
                      at an end is a containment is passed over, and containments are no "others".
The two share nothing but revcomp() and the record classifier.  Every score either of them evaluates must lie at least
SCORE_MARGIN from the threshold it is compared to: both assert it.

A case: prune_cases' dict plus Lc, Ac, delta_c, Tc.  Every kept record is a real overlap of the reads' bytes."""
import functools
import math
import random

from tests import prune_cases as pc
from tests import trim_cases as tc
from tests import unitig_cases as uc

B, E = uc.B, uc.E
SCORE_MARGIN = pc.SCORE_MARGIN
SCORES = None  # as prune_cases.SCORES, for this module's _unique (the bubble, indel and reduce restatements call it too)
CHIMERIC = 0x80000000  # SIGAX_REMOVED_CHIMERIC
SAT = (1 << 32) - 1


# ---- the rules, serially ----
def _unique(N, K, bases, G, T):
    if bases >= G:
        return False
    second = math.log(float(G - 2 * bases)) if G > 2 * bases else math.log(0.001)
    score = float(N - K) * (math.log(float(G - bases)) - second) - float(K) * math.log(2.0)
    if SCORES is not None:
        SCORES.append((score, T))
    assert abs(score - T) >= SCORE_MARGIN, "a score of %r against %r" % (score, T)
    return score >= T


def expected_chimeric(reads, edges, m, max_rounds, L, C=None, delta=0, careful=False, N=None, G=None, T=13.0, Lc=0, Ac=None, delta_c=0,
                      Tc=0.0, tables_only=False):
    """-> prune_cases.expected_prune's dict with status [20]; removed carries CHIMERIC on the reads a chimeric step took;
    tables_only: as unitig_cases.expected's"""
    n = len(reads)
    N = n if N is None else N
    lens = [uc.nbases(r) for r in reads]
    kept, bad, low = tc._kept(edges, lens, m)
    removed, cut = [0] * n, [0] * len(edges)
    islands = dead_ends = rounds = cut_rounds = uniq_first = chim_units = chim_reads = chim_rounds = 0

    def graph():
        alive = [r for r in range(n) if not removed[r]]
        new = {r: k for k, r in enumerate(alive)}
        live = [(i, c) for i, c in kept if not cut[i] and not removed[edges[i][0]] and not removed[edges[i][1]]]
        sub = [(new[edges[i][0]], new[edges[i][1]], edges[i][2], edges[i][3]) for i, _ in live]
        res = uc.expected([reads[r] for r in alive], sub, m, tables_only)
        deg = {}
        for _, (sq, st, contain, _s) in live:
            for s in ((sq & ~1, sq | 1, st & ~1, st | 1) if contain else (sq, st)):
                deg[s] = deg.get(s, 0) + 1
        units = []  # (reads in layout order, bases, left outward state, right outward state), states over the original ids
        for u in range(len(res["uflags"])):
            lay = res["layout"][res["lay_offs"][u]:res["lay_offs"][u + 1]]
            first, last = lay[0], lay[-1]
            units.append(([alive[p[0]] for p in lay], res["seq_offs"][u + 1] - res["seq_offs"][u],
                          2 * alive[first[0]] + (E if first[1] & uc.PLACED_REV else B), 2 * alive[last[0]] + (B if last[1] & uc.PLACED_REV else E)))
        return alive, new, live, res, deg, units

    def participants(live):
        part = [(i, sq, st, edges[i][2]) for i, (sq, st, contain, _s) in live if not contain]
        at = {}  # state -> [(the record's other state, its length)]
        for _, s, t, ln in part:
            at.setdefault(s, []).append((t, ln))
            at.setdefault(t, []).append((s, ln))
        return part, at

    for rnd in range(1, max_rounds + 1):
        changed = False
        if delta > 0:  # the cut step (as prune_cases.expected_prune)
            alive, new, live, res, deg, units = graph()
            unit = {r: u for u, (rs, _, _, _) in enumerate(units) for r in rs}
            uniq = [_unique(N, len(rs), bases, G, T) for rs, bases, _, _ in units]
            if rnd == 1:
                uniq_first = sum(uniq)
            part, at = participants(live)
            mx = {}
            for _, s, t, ln in part:
                mx[s] = max(mx.get(s, 0), ln)
                mx[t] = max(mx.get(t, 0), ln)
            U = lambda s: unit[s >> 1]  # noqa: E731
            now = []
            for i, s, t, ln in part:
                for a, b in ((s, t), (t, s)):
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
            for i in now:
                cut[i] = rnd
            if now:
                changed = True
                cut_rounds += 1
        alive, new, live, res, deg, units = graph()  # the trim step
        gone = []
        for rs, bases, s_left, s_right in units:
            d_left, d_right, k = deg.get(s_left, 0), deg.get(s_right, 0), len(rs)
            if not (d_left == 0 or d_right == 0) or bases > L:
                continue
            if C is not None and not (k - 1) * max(L, 1) <= (max(C, 1) - 1) * bases:
                continue
            if d_left == 0 and d_right == 0:
                islands += 1
            else:
                dead_ends += 1
            gone += rs
        for r in gone:
            removed[r] = rnd
        if gone:
            changed = True
        if Lc > 0:  # the chimeric step, over what the trim step left
            alive, new, live, res, deg, units = graph()
            unit = {r: u for u, (rs, _, _, _) in enumerate(units) for r in rs}
            part, at = participants(live)
            gone = []
            for u, (rs, bases, s_left, s_right) in enumerate(units):
                k = len(rs)
                if deg.get(s_left, 0) != 1 or deg.get(s_right, 0) != 1:
                    continue
                if len(at.get(s_left, [])) != 1 or len(at.get(s_right, [])) != 1:  # the one record is a containment
                    continue
                if bases > Lc or (Ac is not None and not (k - 1) * max(Lc, 1) <= (max(Ac, 1) - 1) * bases):
                    continue
                p, q = at[s_left][0][0], at[s_right][0][0]
                if deg[p] < 2 or deg[q] < 2:
                    continue

                def good(x):
                    rs_x, bases_x, _, _ = units[unit[x >> 1]]
                    if not _unique(N, len(rs_x), bases_x, G, Tc):
                        return False
                    others = [units[unit[o >> 1]] for o, _ in at[x] if unit[o >> 1] != u]
                    return all(min(o[1], SAT) > bases + delta_c for o in others) or all(len(o[0]) > k + 3 for o in others)

                if good(p) or good(q):
                    gone.append(rs)
            for rs in gone:  # (after every decision of the step)
                for r in rs:
                    removed[r] = rnd | CHIMERIC
            if gone:
                changed = True
                chim_units += len(gone)
                chim_reads += sum(len(rs) for rs in gone)
                chim_rounds += 1
        if not changed:
            break
        rounds += 1
    alive, new, live, res, deg, units = graph()
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
        simple = not contain and not self_edge and deg[sq] == 1 and deg[st] == 1
        if simple and frozenset((sq, st)) in merged:
            continue
        (uq, vq), (ut, vt) = where[q], where[t]
        b0 = 1 if ((sq & 1) ^ vq) == B else 0
        b1 = 1 if ((st & 1) ^ vt) == E else 0
        uedges.append((uq, ut, ln, b0 | (b1 << 1) | ((b0 ^ b1) << 2)))
    dropped = sum(1 for i, _ in kept if not cut[i] and (removed[edges[i][0]] or removed[edges[i][1]]))
    st6 = res["status"]
    res["status"] = [st6[0], st6[1], bad, low, st6[4], st6[5], rounds, islands, dead_ends, sum(1 for x in removed if x), dropped, len(uedges),
                     sum(1 for x in cut if x), cut_rounds, uniq_first, 0, chim_units, chim_reads, chim_rounds, 0]
    res["removed"] = removed
    res["cut"] = cut
    res["uedges"] = uedges
    return res


# ---- the reference's loop ----
class _Arc:
    __slots__ = ("start", "dir", "twin", "len", "block", "rec")


def reference_chimeric(reads, edges, m, max_rounds, L, C=None, delta=0, careful=False, N=None, G=None, T=13.0, Lc=0, Ac=None, delta_c=0,
                       Tc=0.0):
    """-> ([(sequence, circular, closing overlap)], {read: round removed, with CHIMERIC where the chimeric visitor took it},
    {record: round cut}, rounds that changed something)"""
    lens = [len(r) for r in reads]
    n_all = len(reads) if N is None else N
    verts = {i: {"seq": bytes(r), "arcs": [], "cov": 1, "reads": [i]} for i, r in enumerate(reads)}

    def pair(sa, sb, ln, block, rec):
        a, b = _Arc(), _Arc()
        a.start, a.dir, a.twin, a.len, a.block, a.rec = sa >> 1, sa & 1, b, ln, block, rec
        b.start, b.dir, b.twin, b.len, b.block, b.rec = sb >> 1, sb & 1, a, ln, block, rec
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

    def score_at_least(v, threshold):
        k, dlt = v["cov"], len(v["seq"])
        if dlt >= G:
            return False
        score = (n_all - k) * (math.log(G - dlt) - math.log(G - 2 * dlt if G > 2 * dlt else 0.001)) - k * math.log(2.0)
        assert abs(score - threshold) >= SCORE_MARGIN
        return score >= threshold

    def max_overlap_visit(vid, v):  # MaximumOverlapVisitor::visit -> the arcs it colours
        if not score_at_least(v, T):
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
                    if a.twin.start != vid:
                        rev = [x for x in verts[a.twin.start]["arcs"] if x.dir == a.twin.dir and not x.block]
                        top2 = max(x.len for x in rev)
                        if any(x.twin.start == vid and top2 - x.len < delta for x in rev):
                            continue
                    elif any(x.twin.start == vid for x in fwd if x.len == top):
                        continue
                out.append(a)
        return out

    def chimeric_visit(vid, v):  # ChimericVisitor::visit
        sense = [a for a in v["arcs"] if a.dir == E]
        anti = [a for a in v["arcs"] if a.dir == B]
        seq = v["seq"]
        if not (len(sense) == 1 and len(anti) == 1 and len(seq) <= Lc and (Ac is None or avg(v["cov"], len(seq)) <= avg(Ac, Lc))):
            return False
        prev_edge, next_edge = anti[0], sense[0]
        if prev_edge.block or next_edge.block:
            return False

        def edges_at(edge):  # the neighbour's edges at the end the twin leaves from
            return [a for a in verts[edge.twin.start]["arcs"] if a.dir == edge.twin.dir]

        if len(edges_at(prev_edge)) < 2 or len(edges_at(next_edge)) < 2:
            return False

        def smallest_new(edge):
            link = verts[edge.twin.start]
            if not score_at_least(link, Tc):
                return False
            others = [verts[a.twin.start] for a in edges_at(edge) if not a.block and a.twin.start != vid]
            smallest_length = all(min(len(o["seq"]), SAT) > len(seq) + delta_c for o in others)
            smallest_coverage = all(o["cov"] > v["cov"] + 3 for o in others)
            return smallest_length or smallest_coverage

        return smallest_new(prev_edge) or smallest_new(next_edge)

    def sweep_arcs(arcs):
        for a in arcs:
            for x in (a, a.twin):
                if x in verts[x.start]["arcs"]:
                    verts[x.start]["arcs"].remove(x)

    def sweep_vertices(black, mark):
        for vid in black:
            for a in verts[vid]["arcs"]:
                if a.twin.start != vid:
                    verts[a.twin.start]["arcs"].remove(a.twin)
            for r in verts[vid]["reads"]:
                gone[r] = mark
            del verts[vid]
        simplify(E)
        simplify(B)

    simplify(E)
    simplify(B)
    gone, cuts, rounds = {}, {}, 0
    for rnd in range(1, max_rounds + 1):
        modified = False
        if delta > 0:
            black = []
            for vid, v in verts.items():
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
            sweep_vertices(black, rnd)
        if Lc > 0:
            black = [vid for vid, v in verts.items() if chimeric_visit(vid, v)]  # it only colours
            if black:
                modified = True
                sweep_vertices(black, rnd | CHIMERIC)
        if not modified:
            break
        rounds += 1
    out = []
    for vid, v in verts.items():
        loop = [a for a in v["arcs"] if not a.block and a.twin.start == vid and a.dir == E and a.twin.dir == B and v["cov"] > 1 and
                len(v["arcs"]) == 2]
        out.append((v["seq"], True, loop[0].len) if loop else (v["seq"], False, 0))
    return out, gone, cuts, rounds


# ---- planting reads on a finished case: every record a real overlap of the stored bytes ----
def _outward(read, e, o):
    """the o bases a new read's prefix shares with end e of `read` (E: its suffix; B: the reverse complement of its prefix)"""
    return read[-o:] if e == E else uc.revcomp(read[:o])


def _record(rng, x, ex, y, ey, o):
    """the record that joins end ex of read x with end ey of read y, either way round"""
    if rng.random() < 0.5:
        x, ex, y, ey = y, ey, x, ex
    b0, b1 = int(ex == B), int(ey == E)
    return (x, y, o, b0 | (b1 << 1) | ((b0 ^ b1) << 2))


def plant(case, rng, left, right=None, o1=25, o2=25, mid=10, flip=False):
    """a new read whose B end overlaps state `left` = 2 * read + end by o1 and, with `right`, whose E end overlaps that state by
    o2, `mid` random bases between; flip: stored on the other strand (its ends swap) -> its id"""
    reads, edges = case["reads"], case["edges"]
    w = _outward(reads[left >> 1], left & 1, o1) + bytes(rng.choice(b"ACGT") for _ in range(mid))
    if right is not None:
        w += uc.revcomp(_outward(reads[right >> 1], right & 1, o2))
    new = len(reads)
    reads.append(uc.revcomp(w) if flip else w)
    edges.append(_record(rng, left >> 1, left & 1, new, E if flip else B, o1))
    if right is not None:
        edges.append(_record(rng, new, B if flip else E, right >> 1, right & 1, o2))
    return new


def _end(g, read, w_end):
    """the state of a _Grow read's end, named in the shared orientation"""
    return 2 * read + (w_end ^ int(g.rc[read]))


def _case(g, name, x=10, L=30, delta=0, careful=False, N=1000, G=10000, T=10.0, C=None, Lc=60, Ac=None, delta_c=0, Tc=3.0, **claims):
    c = g.case(name, x, L, C, **claims)
    c.update(delta=delta, careful=careful, N=N, G=G, T=T, Lc=Lc, Ac=Ac, delta_c=delta_c, Tc=Tc)
    return c


def _two_chains(seed, na=4, nc=4, at_a=1, at_c=2):
    """chains a and c of 60-base reads over 22; -> (g, a, c, p, q): p = the E end of a[at_a], q = the B end of c[at_c], the two
    read ends a bridge joins"""
    g = tc._Grow(seed)
    a = g.chain(na, lens=[60] * na, ovs=[22] * (na - 1))
    c = g.chain(nc, lens=[60] * nc, ovs=[22] * (nc - 1))
    return g, a, c, _end(g, a[at_a], E), _end(g, c[at_c], B)


@functools.lru_cache(maxsize=None)
def hand_built():
    """claims: prune_cases' keys, and chim (status[16]), chim_reads (17), chim_rounds (18), flagged {read: round}"""
    cases = []

    def add(g, name, build, **kw):
        c = _case(g, name, **kw)
        ids = build(c, random.Random(len(cases)))
        claims = c["claims"]
        for key in ("removed_ids", "kept_ids"):
            if key in claims:
                claims[key] = [ids[k] if isinstance(k, str) else k for k in claims[key]]
        if "flagged" in claims:
            claims["flagged"] = {(ids[k] if isinstance(k, str) else k): r for k, r in claims["flagged"].items()}
        cases.append(c)
        return c

    # 1, 2: a bridge read between two chains, on either strand: removed, and the four half chains merge into two unitigs
    for flip in (False, True):
        g, a, c, p, q = _two_chains(1)
        add(g, "bridge_flipped" if flip else "bridge", lambda cs, r: {"x": plant(cs, r, p, q, flip=flip)},
            chim=1, chim_reads=1, chim_rounds=1, rounds=1, unitigs=2, flagged={"x": 1}, kept_ids=a + c)
    # 3: a bridge of two merged reads (50 + 50 - 22 = 78 bases), within and beyond Lc
    for name, Lc, n in (("bridge2_within", 78, 1), ("bridge2_beyond", 77, 0)):
        g, a, c, p, q = _two_chains(3)

        def two(cs, r):
            x1 = plant(cs, r, p, o1=25, mid=25)
            return {"x1": x1, "x2": plant(cs, r, 2 * x1 + E, q, o1=22, o2=25, mid=3)}

        add(g, name, two, Lc=Lc, chim=n, chim_reads=2 * n, unitigs=2 if n else 5, **({"flagged": {"x1": 1, "x2": 1}} if n else {"kept_ids": ["x1", "x2"]}))
    # 4: the neighbours' touched ends have degree 1: the bridge is merged by simplify and nothing is removed
    g, a, c, p, q = _two_chains(4, at_a=3, at_c=0)
    add(g, "bridge_simple", lambda cs, r: {"x": plant(cs, r, p, q)}, chim=0, rounds=0, unitigs=1, kept_ids=["x"])
    # 5: good through length only (the default bridge: no other has 5 reads), through coverage only (delta_c = 1000 fails every
    # length test; a's far half has 5 reads), through neither
    g, a, c, p, q = _two_chains(5, na=7)
    add(g, "good_by_reads", lambda cs, r: {"x": plant(cs, r, p, q)}, delta_c=1000, chim=1, flagged={"x": 1})
    g, a, c, p, q = _two_chains(5)
    add(g, "good_by_neither", lambda cs, r: {"x": plant(cs, r, p, q)}, delta_c=1000, chim=0, rounds=0, unitigs=5, kept_ids=["x"])
    # 6: the others at exactly bases(U) + delta_c (60 + 38 = 98 bases against a bridge of 60) and one above
    for name, dc, n in (("others_at_bases", 38, 0), ("others_above_bases", 37, 1)):
        g, a, c, p, q = _two_chains(6)
        add(g, name, lambda cs, r: {"x": plant(cs, r, p, q)}, delta_c=dc, chim=n, unitigs=2 if n else 5)
    # 7: the others at exactly K + 3 reads and one above (no length test passes)
    for name, na, n in (("others_at_reads", 6, 0), ("others_above_reads", 7, 1)):
        g, a, c, p, q = _two_chains(7, na=na)
        add(g, name, lambda cs, r: {"x": plant(cs, r, p, q)}, delta_c=1000, chim=n)
    # 8: no neighbour unique; 9: both neighbours with bases >= G
    g, a, c, p, q = _two_chains(8)
    add(g, "not_unique", lambda cs, r: {"x": plant(cs, r, p, q)}, Tc=50.0, chim=0, rounds=0, unitigs=5)
    g, a, c, p, q = _two_chains(9)
    add(g, "beyond_genome", lambda cs, r: {"x": plant(cs, r, p, q)}, N=20, G=98, T=50.0, chim=0, rounds=0, unitigs=5)
    # 10: p == q: both ends of the bridge at one read end, which also carries the chain's own record
    g, a, c, p, q = _two_chains(10)
    add(g, "same_end", lambda cs, r: {"x": plant(cs, r, p, p)}, chim=1, flagged={"x": 1}, unitigs=2)
    # 11: P == Q with p != q: from the E end of a's first half to its B end, which a further chain z enters too
    g, a, c, p, q = _two_chains(11)
    z = g.grow(a[0], 2, side=B, lens=[60, 60], ovs=[22, 22])
    s0 = _end(g, a[0], B)
    add(g, "same_unitig", lambda cs, r: {"x": plant(cs, r, p, s0)}, chim=1, flagged={"x": 1}, kept_ids=a + z)
    # 12: parallel records from p into both ends of U and nothing else at p: no others, the tests hold vacuously
    g = tc._Grow(12)
    a = g.chain(2, lens=[60, 60], ovs=[22])
    p = _end(g, a[1], E)
    add(g, "parallel_no_others", lambda cs, r: {"x": plant(cs, r, p, p)}, chim=1, flagged={"x": 1}, kept_ids=a)
    # 13: a unitig whose one record at each end is a containment (a read that is the suffix of another), beside a real bridge
    g, a, c, p, q = _two_chains(13)
    big = g.start(70, rc=False)
    small = g.start(45, rc=False)
    g.w[small] = g.w[big][25:]
    g.edges.append((big, small, 45, 0))
    add(g, "containment_at_end", lambda cs, r: {"x": plant(cs, r, p, q)}, Lc=80, chim=1, flagged={"x": 1}, kept_ids=[big, small])
    # 14: a containment among the records at p: it is no other (as one, its 45 bases would fail the length test); q's side is not
    # good: c's first half is one read of 45
    g = tc._Grow(14)
    a = g.chain(4, lens=[60] * 4, ovs=[22] * 3)
    c = g.chain(3, lens=[45, 60, 60], ovs=[22, 22])
    small = g.start(45, rc=g.rc[a[1]])
    g.w[small] = g.w[a[1]][15:]
    g.edges.append((a[1], small, 45, 3 if g.rc[a[1]] else 0))  # (stored on the other strand it is a[1]'s prefix)
    p, q = _end(g, a[1], E), _end(g, c[1], B)
    add(g, "containment_at_p", lambda cs, r: {"x": plant(cs, r, p, q)}, chim=1, flagged={"x": 1}, kept_ids=a + c + [small])
    # 15: a ring: dL = dR = 1, short, and its ends carry each other
    g = tc._Grow(15)
    ring = g.ring(4)
    add(g, "ring", lambda cs, r: {}, Lc=1000, chim=0, rounds=0, unitigs=1, cycles=1, kept_ids=ring)
    # 16: two chimeric unitigs (50 and 55 bases) at one neighbour end p, whose third record leads to one read of 60.  x2 fails at p on
    # x1 and goes through its own q side; then that side is closed too (d's first half is one read of 45) and x2 waits, while x1, whose
    # q side is closed as well (c's first read cut to 45), goes through p alone: by the second minimum, the first being its own
    for name, n in (("two_bridges", 2), ("two_bridges_by_p", 1)):
        g, a, c, p, q = _two_chains(16, na=3, nc=3, at_a=1, at_c=1)
        if n == 1:
            g.w[c[0]] = g.w[c[0]][15:]  # (its last 22 bases, the overlap with c[1], stay)
        d = g.chain(3, lens=[60 if n == 2 else 45, 60, 60], ovs=[22, 22])
        q2 = _end(g, d[1], B)

        def two(cs, r):
            return {"x1": plant(cs, r, p, q, mid=0), "x2": plant(cs, r, p, q2, mid=5)}

        # (with x1 gone x2 is the shortest at p: it follows in round 2, the verdicts of round 1 being those of its start)
        add(g, name, two, chim=2, chim_reads=2, chim_rounds=3 - n, flagged={"x1": 1, "x2": 3 - n})
    # 17: the trim step of the same round makes the bridge: a tip of 40 bases at its E end goes first; 18: two tips on that tip: the
    # bridge is free in round 2 only (and with one round it stays)
    for name, x, deep in (("after_trim", 10, False), ("second_round", 10, True), ("second_round_1round", 1, True)):
        g, a, c, p, q = _two_chains(17)

        def tipped(cs, r):
            xx = plant(cs, r, p, q)
            t = plant(cs, r, 2 * xx + E, o1=22, mid=18)
            ids = {"x": xx, "t": t}
            if deep:
                ids["t1"] = plant(cs, r, 2 * t + E, o1=22, mid=18)
                ids["t2"] = plant(cs, r, 2 * t + E, o1=24, mid=16)
            return ids

        if not deep:
            add(g, name, tipped, x=x, L=45, chim=1, rounds=1, dead_ends=1, flagged={"x": 1}, removed_ids=["t"], kept_ids=a + c)
        elif x == 10:
            add(g, name, tipped, x=x, L=45, chim=1, chim_rounds=1, rounds=2, dead_ends=3, flagged={"x": 2}, by_round={}, kept_ids=a + c)
        else:
            add(g, name, tipped, x=x, L=45, chim=0, rounds=1, dead_ends=2, kept_ids=["x", "t"])
    # 19: Ac given: two reads on 78 bases under Lc = 100: (K - 1) * 100 <= (Ac - 1) * 78 from Ac = 3 on
    for name, Ac, n in (("coverage_low_enough", 3, 1), ("coverage_too_high", 2, 0)):
        g, a, c, p, q = _two_chains(19)

        def two(cs, r):
            x1 = plant(cs, r, p, o1=25, mid=25)
            return {"x1": x1, "x2": plant(cs, r, 2 * x1 + E, q, o1=22, o2=25, mid=3)}

        add(g, name, two, Lc=100, Ac=Ac, chim=n, chim_reads=2 * n)
    # 20: Lc = 0: no chimeric step
    g, a, c, p, q = _two_chains(20)
    add(g, "no_step", lambda cs, r: {"x": plant(cs, r, p, q)}, Lc=0, chim=0, rounds=0, unitigs=5, kept_ids=["x"])
    return cases


def case_named(name):
    return next(c for c in hand_built() if c["name"] == name)


KEYS = ("delta", "careful", "N", "G", "T", "Lc", "Ac", "delta_c", "Tc")


def run(fn, case, max_rounds=None, **over):
    kw = {k: case[k] for k in KEYS}
    kw.update(over)
    return fn(case["reads"], case["edges"], case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"], **kw)


@functools.lru_cache(maxsize=None)
def expected_of(name, max_rounds=None):
    return run(expected_chimeric, case_named(name), max_rounds)


# ---- seeded random graphs: prune_cases.random_case with up to three bridge reads planted ----
@functools.lru_cache(maxsize=None)
def random_case(seed):
    base = pc.random_case(seed)
    rng = random.Random(200000 + seed)
    case = dict(base, name="chimeric_random%d" % seed, reads=list(base["reads"]), edges=list(base["edges"]))
    n0 = len(case["reads"])
    for _ in range(rng.randint(1, 3)):
        left, right = rng.randrange(2 * n0), rng.randrange(2 * n0)
        plant(case, rng, left, right, o1=rng.randint(20, 35), o2=rng.randint(20, 35), mid=rng.randint(0, 30), flip=rng.random() < 0.5)
    case.update(Lc=rng.choice((60, 90, 150)), Ac=rng.choice((None, None, 2, 3)), delta_c=rng.choice((0, 0, 10, 40)), Tc=rng.choice((1.5, 3.0, 7.0)))
    if rng.random() < 0.3:
        case["delta"] = 0
    return case


# ---- one larger seeded graph: prune_cases.large_case with bridges planted ----
@functools.lru_cache(maxsize=None)
def large_case(n_reads=20000, seed=5, bridges=200):
    base = pc.large_case(n_reads, seed)
    rng = random.Random(300000 + seed)
    case = dict(base, name="chimeric_large", reads=list(base["reads"]), edges=list(base["edges"]))
    n0 = len(case["reads"])
    for k in range(bridges):
        if k % 4 == 3:  # several at one read end: contended minima
            left = 2 * (k % 7) + E
        else:
            left = rng.randrange(2 * n0)
        plant(case, rng, left, rng.randrange(2 * n0), o1=rng.randint(45, 60), o2=rng.randint(45, 60), mid=rng.randint(0, 20), flip=rng.random() < 0.5)
    # no cut step, and no read of 100 is short enough to trim: only the chimeric steps change the graph, three rounds of them, and
    # the rounds after those are idle
    case.update(Lc=150, Ac=None, delta_c=0, Tc=3.0, x=8, L=99, delta=0, N=len(case["reads"]))
    return case


# ---- end to end: reads tiling a random genome, and reads made of the halves of two distant places ----
E2E_SEED, E2E_GENOME, E2E_READS, E2E_LEN, E2E_M, E2E_PLANTED = 23, 10000, 3000, 100, 40, 8
E2E_X, E2E_L, E2E_DELTA, E2E_T, E2E_LC, E2E_TC = 10, 150, 0, 13.0, 100, 3.0


@functools.lru_cache(maxsize=None)
def end_to_end():
    """-> (names, reads, planted ids): 3 000 error-free reads of 100 from a 10 000-base random genome (30-fold), either strand, then
    8 reads whose halves come from two places at least 2 000 bases apart"""
    rng = random.Random(E2E_SEED)
    g = bytes(rng.choice(b"ACGT") for _ in range(E2E_GENOME))
    reads = []
    for _ in range(E2E_READS):
        at = rng.randrange(E2E_GENOME - E2E_LEN + 1)
        w = g[at:at + E2E_LEN]
        reads.append(uc.revcomp(w) if rng.random() < 0.5 else w)
    planted = []
    half = E2E_LEN // 2
    for _ in range(E2E_PLANTED):
        a = rng.randrange(E2E_GENOME - half)
        b = rng.randrange(E2E_GENOME - half)
        while abs(a - b) < 2000:
            b = rng.randrange(E2E_GENOME - half)
        w = g[a:a + half] + g[b:b + half]
        planted.append(len(reads))
        reads.append(uc.revcomp(w) if rng.random() < 0.5 else w)
    return ["r%d" % i for i in range(len(reads))], reads, planted
