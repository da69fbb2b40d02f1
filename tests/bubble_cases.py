"""Cases and two brute forces for bubble popping in the rounds of `siga unitig` (sigax_unitigs_bubble_*, the rules in
include/sigax.h); no tests here (tests/test_bubble_cases.py, tests/test_gpu_unitig_bubble.py).

expected_bubble()     the rules, serially from the reads: the round loop of chimeric_cases.expected_chimeric with the bubble step
                      between its trim and its chimeric step.  The bubble step finds every unitig's two outward read ends, their one
                      record, the read ends at its other side, and compares the windows [o_lo, o_lo + span) of the arms' bases in the
                      frame of the smaller neighbour state.
independent_bubble()  the same loop with another bubble step: no frames and no windows.  It lays neighbour + arm + neighbour out as
                      one string through the records' overlaps, for every arm, groups the strings of one (lo, hi) by their length and
                      counts the places where a string differs from its group's winner.
The reference has no such step (SmoothingVisitor::visit returns false, src/bigraph_visitors.cpp:1021-1036): there is nothing to
compare against but the rules themselves.

A case: chimeric_cases' dict plus Lb (max_bubble_span) and D (max divergence per mille, None = no bases test).  Every kept record is
a real overlap of the reads' bytes."""
import functools
import random

from tests import chimeric_cases as cc
from tests import prune_cases as pc
from tests import trim_cases as tc
from tests import unitig_cases as uc

B, E = uc.B, uc.E
CHIMERIC = cc.CHIMERIC
BUBBLE = 0x40000000  # SIGAX_REMOVED_BUBBLE
SAT = cc.SAT


# ---- the two bubble steps ----
def _arms(units, ring, unit, deg, at):
    """-> [(unitig, p, q, o_p, o_q)] of the arms: p, o_p the neighbour state and the record length at the left end"""
    out = []
    for u, (rs, bases, s_left, s_right) in enumerate(units):
        if ring[u] or deg.get(s_left, 0) != 1 or deg.get(s_right, 0) != 1:
            continue
        if len(at.get(s_left, [])) != 1 or len(at.get(s_right, [])) != 1:  # the one record is a containment
            continue
        (p, o_p), (q, o_q) = at[s_left][0], at[s_right][0]
        if unit[p >> 1] == u or unit[q >> 1] == u or p == q:
            continue
        out.append((u, p, q, o_p, o_q))
    return out


def _popped(mism, span, D):
    return D is None or mism * 1000 <= D * span


def _step_frames(units, ring, seqs, unit, deg, at, Lb, D):
    """the rules of sigax.h as they are written -> ([unitigs popped], losers kept, log)"""
    groups = {}
    for u, p, q, o_p, o_q in _arms(units, ring, unit, deg, at):
        lo, hi = min(p, q), max(p, q)
        o_lo, o_hi = (o_p, o_q) if p < q else (o_q, o_p)
        span = units[u][1] - o_lo - o_hi
        if 1 <= span <= Lb:
            groups.setdefault((lo, hi, span), []).append((u, o_lo, p == lo))
    gone, kept, log = [], 0, []
    for (lo, hi, span), arms in sorted(groups.items()):
        if len(arms) < 2:
            continue
        frame = lambda a: seqs[a[0]] if a[2] else uc.revcomp(seqs[a[0]])  # noqa: E731
        win = max(arms, key=lambda a: (len(units[a[0]][0]), -units[a[0]][0][0]))
        aw = frame(win)
        for a in arms:
            if a is win:
                continue
            al = frame(a)
            mism = sum(1 for t in range(span) if al[a[1] + t] != aw[win[1] + t])
            if _popped(mism, span, D):
                gone.append(a[0])
            else:
                kept += 1
            log.append({"lo": lo, "hi": hi, "span": span, "winner": units[win[0]][0][0], "loser": units[a[0]][0][0], "mism": mism,
                        "reversed": not a[2], "winner_reversed": not win[2], "reads": len(units[a[0]][0])})
    return gone, kept, log


def _step_strings(units, ring, seqs, unit, deg, at, Lb, D):
    """neighbour + arm + neighbour as one string -> ([unitigs popped], losers kept, [])"""

    def ending_in(s):  # the unitig of state s, read so that s is its right end
        rs, _, s_left, s_right = units[unit[s >> 1]]
        assert s in (s_left, s_right) and s_left != s_right
        return seqs[unit[s >> 1]] if s == s_right else uc.revcomp(seqs[unit[s >> 1]])

    by_ends = {}
    for u, p, q, o_p, o_q in _arms(units, ring, unit, deg, at):
        arm = seqs[u]
        if p > q:  # walk every arm from the smaller neighbour state to the larger
            arm, p, q, o_p, o_q = uc.revcomp(arm), q, p, o_q, o_p
        left, right = ending_in(p), uc.revcomp(ending_in(q))
        assert left[-o_p:] == arm[:o_p] and arm[-o_q:] == right[:o_q], "a record that is no overlap"
        inner = len(arm) - o_p - o_q
        if not 1 <= inner <= Lb:
            continue
        whole = left + arm[o_p:] + right[o_q:]
        by_ends.setdefault((p, q, len(whole)), []).append((len(units[u][0]), -units[u][0][0], u, whole, inner))
    gone, kept = [], 0
    for arms in by_ends.values():
        if len(arms) < 2:
            continue
        win = max(arms)
        for a in arms:
            if a is win:
                continue
            ham = sum(1 for x, y in zip(a[3], win[3]) if x != y)
            if _popped(ham, a[4], D):
                gone.append(a[2])
            else:
                kept += 1
    return gone, kept, []


# ---- the round loop: chimeric_cases.expected_chimeric's, with the bubble step ----
def _rounds(step, reads, edges, m, max_rounds, L, C=None, delta=0, careful=False, N=None, G=None, T=13.0, Lc=0, Ac=None, delta_c=0, Tc=0.0,
            Lb=0, D=50, tables_only=False):
    n = len(reads)
    N = n if N is None else N
    lens = [uc.nbases(r) for r in reads]
    kept, bad, low = tc._kept(edges, lens, m)
    removed, cut = [0] * n, [0] * len(edges)
    islands = dead_ends = rounds = cut_rounds = uniq_first = chim_units = chim_reads = chim_rounds = 0
    popped = bub_reads = bub_rounds = kept_div = 0
    log = []

    def graph():
        alive = [r for r in range(n) if not removed[r]]
        new = {r: k for k, r in enumerate(alive)}
        live = [(i, c) for i, c in kept if not cut[i] and not removed[edges[i][0]] and not removed[edges[i][1]]]
        sub = [(new[edges[i][0]], new[edges[i][1]], edges[i][2], edges[i][3]) for i, _ in live]
        sub_reads = [reads[r] for r in alive]
        res = uc.expected(sub_reads, sub, m, tables_only)
        if tables_only:  # the bytes of an arm are built when a step compares it
            res["lazy_seqs"] = uc.LazySeqs(sub_reads, res)
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
        if delta > 0:  # the cut step
            alive, new, live, res, deg, units = graph()
            unit = {r: u for u, (rs, _, _, _) in enumerate(units) for r in rs}
            uniq = [cc._unique(N, len(rs), bases, G, T) for rs, bases, _, _ in units]
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
        if Lb > 0:  # the bubble step, over what the trim step left
            alive, new, live, res, deg, units = graph()
            unit = {r: u for u, (rs, _, _, _) in enumerate(units) for r in rs}
            part, at = participants(live)
            seqs = res.pop("lazy_seqs") if tables_only else [res["useqs"][res["seq_offs"][u]:res["seq_offs"][u + 1]] for u in range(len(units))]
            ring = [bool(f & uc.CIRCULAR) for f in res["uflags"]]
            pop, kept_now, lg = step(units, ring, seqs, unit, deg, at, Lb, D)
            kept_div += kept_now
            log += [dict(e, round=rnd) for e in lg]
            for u in pop:  # (after every decision of the step)
                for r in units[u][0]:
                    removed[r] = rnd | BUBBLE
            if pop:
                changed = True
                popped += len(pop)
                bub_reads += sum(len(units[u][0]) for u in pop)
                bub_rounds += 1
        if Lc > 0:  # the chimeric step, over what the bubble step left
            alive, new, live, res, deg, units = graph()
            unit = {r: u for u, (rs, _, _, _) in enumerate(units) for r in rs}
            part, at = participants(live)
            gone = []
            for u, (rs, bases, s_left, s_right) in enumerate(units):
                k = len(rs)
                if deg.get(s_left, 0) != 1 or deg.get(s_right, 0) != 1:
                    continue
                if len(at.get(s_left, [])) != 1 or len(at.get(s_right, [])) != 1:
                    continue
                if bases > Lc or (Ac is not None and not (k - 1) * max(Lc, 1) <= (max(Ac, 1) - 1) * bases):
                    continue
                p, q = at[s_left][0][0], at[s_right][0][0]
                if deg[p] < 2 or deg[q] < 2:
                    continue

                def good(x):
                    rs_x, bases_x, _, _ = units[unit[x >> 1]]
                    if not cc._unique(N, len(rs_x), bases_x, G, Tc):
                        return False
                    others = [units[unit[o >> 1]] for o, _ in at[x] if unit[o >> 1] != u]
                    return all(min(o[1], SAT) > bases + delta_c for o in others) or all(len(o[0]) > k + 3 for o in others)

                if good(p) or good(q):
                    gone.append(rs)
            for rs in gone:
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
    res.pop("lazy_seqs", None)
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
                     sum(1 for x in cut if x), cut_rounds, uniq_first, 0, chim_units, chim_reads, chim_rounds, 0, popped, bub_reads, bub_rounds,
                     kept_div]
    res["removed"] = removed
    res["cut"] = cut
    res["uedges"] = uedges
    res["bubble_log"] = log
    return res


def expected_bubble(reads, edges, m, max_rounds, L, C=None, **kw):
    """-> chimeric_cases.expected_chimeric's dict with status [24]; removed carries BUBBLE on the reads a bubble step took; bubble_log:
    one entry per loser judged.  tables_only = True: as unitig_cases.expected's; a compared arm's reads must be bytes"""
    return _rounds(_step_frames, reads, edges, m, max_rounds, L, C, **kw)


def independent_bubble(reads, edges, m, max_rounds, L, C=None, **kw):
    return _rounds(_step_strings, reads, edges, m, max_rounds, L, C, **kw)


# ---- planting arms on a finished case: every record a real overlap of the stored bytes ----
def plant_arm(case, rng, left, right, mid, o1=25, o2=25, flip=False):
    """a new read whose B end overlaps state `left` by o1 and whose E end overlaps state `right` by o2, the bytes `mid` between;
    flip: stored on the other strand -> its id"""
    return plant_chain(case, rng, left, right, mid, o1, o2, pieces=1, flips=[flip])[0]


def plant_chain(case, rng, left, right, mid, o1=25, o2=25, pieces=3, flips=None, ov=22):
    """the same string cut into `pieces` reads that overlap by `ov`, each stored on the strand flips[i] says -> their ids"""
    reads, edges = case["reads"], case["edges"]
    w = cc._outward(reads[left >> 1], left & 1, o1) + bytes(mid) + uc.revcomp(cc._outward(reads[right >> 1], right & 1, o2))
    flips = flips or [False] * pieces
    step = (len(w) - ov) // pieces
    assert pieces == 1 or step >= 1
    cuts = [(k * step, len(w) if k == pieces - 1 else (k + 1) * step + ov) for k in range(pieces)]
    ids = []
    for (a, b), flip in zip(cuts, flips):
        ids.append(len(reads))
        reads.append(uc.revcomp(w[a:b]) if flip else w[a:b])
    edges.append(cc._record(rng, left >> 1, left & 1, ids[0], E if flips[0] else B, o1))
    for k in range(pieces - 1):
        edges.append(cc._record(rng, ids[k], B if flips[k] else E, ids[k + 1], E if flips[k + 1] else B, cuts[k][1] - cuts[k + 1][0]))
    edges.append(cc._record(rng, ids[-1], B if flips[-1] else E, right >> 1, right & 1, o2))
    return ids


def bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(rng, s, places):
    s = bytearray(s)
    for at in places:
        s[at] = rng.choice([b for b in b"ACGT" if b != s[at]])
    return bytes(s)


def _case(g, name, x=10, L=30, Lb=40, D=50, Lc=0, **claims):
    c = cc._case(g, name, x=x, L=L, Lc=Lc, **claims)
    c.update(Lb=Lb, D=D)
    return c


def _ends(seed, na=3, nc=3, at_a=None, at_c=0):
    """chains a and c; p = the E end of a[at_a] (default: its last read), q = the B end of c[at_c]"""
    at_a = na - 1 if at_a is None else at_a
    g, a, c, p, q = cc._two_chains(seed, na=na, nc=nc, at_a=at_a, at_c=at_c)
    return g, a, c, p, q


@functools.lru_cache(maxsize=None)
def hand_built():
    """claims: popped (status[20]), bub_reads (21), bub_rounds (22), kept_div (23), rounds (6), unitigs (0), flagged {read: round}:
    removed with BUBBLE in that round, kept_ids: not removed; log: a predicate over expected_bubble's bubble_log"""
    cases = []

    def add(g, name, build, **kw):
        c = _case(g, name, **kw)
        ids = build(c, random.Random(1000 + len(cases)))
        claims = c["claims"]
        look = lambda k: ids[k] if isinstance(k, str) else k  # noqa: E731
        if "kept_ids" in claims:
            claims["kept_ids"] = [look(k) for k in claims["kept_ids"]]
        if "flagged" in claims:
            claims["flagged"] = {look(k): r for k, r in claims["flagged"].items()}
        cases.append(c)
        return c

    # 1: two arms of one read each, one substitution in 30: the one with the larger id goes and the rest is one unitig
    def two(span=30, diff=(7,), flips=(False, False), **kw):
        def build(cs, r):
            mid = bases(r, span)
            return {"w": plant_arm(cs, r, cs["p"], cs["q"], mid, flip=flips[0], **kw),
                    "x": plant_arm(cs, r, cs["p"], cs["q"], mutate(r, mid, diff), flip=flips[1], **kw)}
        return build

    def ends_case(seed, name, build, **kw):
        g, a, c, p, q = _ends(seed)

        def wrapped(cs, r):
            cs["p"], cs["q"] = p, q
            ids = build(cs, r)
            ids.update(a=a, c=c)
            return ids

        return add(g, name, wrapped, **kw)

    ends_case(1, "two_arms", two(), popped=1, bub_reads=1, bub_rounds=1, rounds=1, unitigs=1, flagged={"x": 1}, kept_ids=["w"])
    # 2: stored on the other strand, either and both: the lookup complements
    ends_case(2, "loser_flipped", two(flips=(False, True)), popped=1, flagged={"x": 1}, kept_ids=["w"], unitigs=1)
    ends_case(3, "winner_flipped", two(flips=(True, False)), popped=1, flagged={"x": 1}, kept_ids=["w"], unitigs=1)
    # 3: span = 1, Lb and Lb + 1
    ends_case(4, "span_1", two(span=1, diff=()), D=0, popped=1, flagged={"x": 1})
    ends_case(5, "span_at_lb", two(span=40, diff=(3,)), popped=1, flagged={"x": 1})
    ends_case(6, "span_above_lb", two(span=41, diff=(3,)), popped=0, rounds=0, unitigs=4, kept_ids=["w", "x"])
    # 4: one mismatch at t = 0 only, at t = span - 1 only: seen (D = 0 keeps the loser), and nothing outside the window counts
    ends_case(7, "mismatch_first", two(diff=(0,)), D=0, popped=0, kept_div=1, rounds=0, kept_ids=["w", "x"])
    ends_case(8, "mismatch_last", two(diff=(29,)), D=0, popped=0, kept_div=1, rounds=0, kept_ids=["w", "x"])
    ends_case(9, "mismatch_first_flipped", two(diff=(0,), flips=(True, True)), D=0, popped=0, kept_div=1, kept_ids=["w", "x"])
    ends_case(10, "mismatch_last_flipped", two(diff=(29,), flips=(False, True)), D=0, popped=0, kept_div=1, kept_ids=["w", "x"])
    # 5: mism * 1000 == D * span exactly (2 of 40 at D = 50) and one mismatch more
    ends_case(11, "at_divergence", two(span=40, diff=(5, 31)), popped=1, kept_div=0, flagged={"x": 1})
    ends_case(12, "above_divergence", two(span=40, diff=(5, 17, 31)), popped=0, kept_div=1, rounds=0, kept_ids=["w", "x"])
    # 6: D = 0 with identical arms; the no-bases option with arms that share nothing
    ends_case(13, "identical_d0", two(diff=()), D=0, popped=1, flagged={"x": 1})
    ends_case(14, "no_bases", two(diff=tuple(range(30))), D=None, popped=1, flagged={"x": 1})
    ends_case(15, "all_differ", two(diff=tuple(range(30))), D=999, popped=0, kept_div=1, kept_ids=["w", "x"])

    # 7: an N inside the window: in one arm (a mismatch), in both (none), in a reversed arm (N is its own complement)
    def with_n(which, flips=(False, False)):
        def build(cs, r):
            mid = bytearray(bases(r, 30))
            other = bytearray(mid)
            if "w" in which:
                mid[11] = ord("N")
            if "x" in which:
                other[11] = ord("N")
            return {"w": plant_arm(cs, r, cs["p"], cs["q"], bytes(mid), flip=flips[0]),
                    "x": plant_arm(cs, r, cs["p"], cs["q"], bytes(other), flip=flips[1])}
        return build

    ends_case(16, "n_in_one", with_n("x"), D=0, popped=0, kept_div=1, kept_ids=["w", "x"])
    ends_case(17, "n_in_both", with_n("wx"), D=0, popped=1, flagged={"x": 1})
    ends_case(18, "n_in_reversed", with_n("wx", flips=(False, True)), D=0, popped=1, flagged={"x": 1})

    # 8: three arms in a group: two losers against one winner, one of them beyond the divergence
    def three(cs, r):
        mid = bases(r, 30)
        return {"w": plant_arm(cs, r, cs["p"], cs["q"], mid), "x": plant_arm(cs, r, cs["p"], cs["q"], mutate(r, mid, (4,))),
                "y": plant_arm(cs, r, cs["p"], cs["q"], mutate(r, mid, (1, 2, 3, 20)), flip=True)}

    # (round 1 changed something, so round 2 runs and judges y once more: kept on divergence is summed over the rounds that ran)
    ends_case(19, "three_arms", three, popped=1, kept_div=2, flagged={"x": 1}, kept_ids=["w", "y"], rounds=1)

    # 9: 65 and 130 arms at one (lo, hi): more than a wave in one group; every fifth beyond the divergence
    def many(k):
        def build(cs, r):
            mid = bases(r, 30)
            ids = {"w": plant_arm(cs, r, cs["p"], cs["q"], mid)}
            for i in range(1, k):
                ids["x%d" % i] = plant_arm(cs, r, cs["p"], cs["q"], mutate(r, mid, (3, 9, 14) if i % 5 == 0 else (i % 30,)), flip=i % 3 == 0)
            return ids
        return build

    for k in (65, 130):
        lost = (k - 1) // 5
        ends_case(20 + k, "arms%d" % k, many(k), popped=k - 1 - lost, kept_div=2 * lost, bub_rounds=1, kept_ids=["w", "x5"], flagged={"x1": 1, "x64": 1})

    # 10: arms of three reads, stored on either strand: the lookup crosses placements and strands; K decides against the id
    def chains(flips_w, flips_x, diff=(2, 33, 58), pieces=3):
        def build(cs, r):
            mid = bases(r, 60)
            x = plant_arm(cs, r, cs["p"], cs["q"], mutate(r, mid, diff), o1=22, o2=22)  # (one read of 104, the smaller id, and K = 1)
            w = plant_chain(cs, r, cs["p"], cs["q"], mid, o1=25, o2=27, pieces=pieces, flips=flips_w)
            y = plant_chain(cs, r, cs["p"], cs["q"], mutate(r, mid, (0, 59)), o1=30, o2=21, pieces=pieces, flips=flips_x)
            return {"x": x, "w0": w[0], "w1": w[1], "w2": w[2], "y0": y[0], "y1": y[1], "y2": y[2]}
        return build

    ends_case(30, "chains", chains([False, False, False], [False, False, False]), Lb=60, popped=2, bub_reads=4,
              flagged={"x": 1, "y0": 1, "y1": 1, "y2": 1}, kept_ids=["w0", "w1", "w2"], unitigs=1)
    ends_case(31, "chains_flipped", chains([True, False, True], [False, True, True]), Lb=60, popped=2, bub_reads=4,
              flagged={"x": 1, "y1": 1}, kept_ids=["w0", "w1", "w2"])
    ends_case(32, "chains_all_flipped", chains([True, True, True], [True, True, True]), Lb=60, popped=2, bub_reads=4, kept_ids=["w1"])
    # 11: a K tie decided by the first read id (two_arms), and a winner with larger K but larger ids (chains: x has the smallest id)

    # 12: one arm entered through its right end: p > q, so the arm whose left end is at p is read as its reverse complement
    def swapped(cs, r):
        mid = bases(r, 30)
        cs["p"], cs["q"] = max(cs["p"], cs["q"]), min(cs["p"], cs["q"])
        return {"w": plant_arm(cs, r, cs["p"], cs["q"], mid), "x": plant_arm(cs, r, cs["q"], cs["p"], uc.revcomp(mutate(r, mid, (0,))))}

    ends_case(33, "entered_right", swapped, D=40, popped=1, flagged={"x": 1}, kept_ids=["w"], log=lambda lg: lg[0]["reversed"] != lg[0]["winner_reversed"])
    ends_case(34, "entered_right_d0", swapped, D=0, popped=0, kept_div=1, kept_ids=["w", "x"], log=lambda lg: lg[0]["mism"] == 1)

    # 13: two groups at one (lo, hi) with different spans: each pops its own loser
    def two_spans(cs, r):
        m1, m2 = bases(r, 30), bases(r, 20)
        return {"w": plant_arm(cs, r, cs["p"], cs["q"], m1), "x": plant_arm(cs, r, cs["p"], cs["q"], mutate(r, m1, (9,))),
                "w2": plant_arm(cs, r, cs["p"], cs["q"], m2), "x2": plant_arm(cs, r, cs["p"], cs["q"], m2, flip=True),
                "lone": plant_arm(cs, r, cs["p"], cs["q"], bases(r, 25))}

    ends_case(35, "two_spans", two_spans, popped=2, flagged={"x": 1, "x2": 1}, kept_ids=["w", "w2", "lone"], rounds=1)

    # 14: the same span through different overlaps: one group; and equal bases with different spans: two groups of one
    def same_span(cs, r):
        mid = bases(r, 30)
        return {"w": plant_arm(cs, r, cs["p"], cs["q"], mid, o1=25, o2=25), "x": plant_arm(cs, r, cs["p"], cs["q"], mid, o1=31, o2=22)}

    ends_case(36, "overlaps_differ", same_span, D=0, popped=1, flagged={"x": 1})

    def same_bases(cs, r):
        return {"w": plant_arm(cs, r, cs["p"], cs["q"], bases(r, 30), o1=25, o2=25), "x": plant_arm(cs, r, cs["p"], cs["q"], bases(r, 28), o1=27, o2=25)}

    ends_case(37, "spans_differ", same_bases, D=None, popped=0, rounds=0, kept_ids=["w", "x"])

    # 15: U(p) == U(q): a bubble from the E end of a chain back to its B end
    g = tc._Grow(40)
    a = g.chain(4, lens=[60] * 4, ovs=[22] * 3)
    pe, pb = cc._end(g, a[3], E), cc._end(g, a[0], B)

    def loop_back(cs, r):
        mid = bases(r, 30)
        return {"w": plant_arm(cs, r, pe, pb, mid), "x": plant_arm(cs, r, pe, pb, mutate(r, mid, (12,)), flip=True)}

    add(g, "same_unitig", loop_back, popped=1, flagged={"x": 1}, kept_ids=a + ["w"], unitigs=1)
    # 16: p == q: both ends of each arm at one read end: no arms
    g, a, c, p, q = _ends(41)

    def hairpin(cs, r):
        mid = bases(r, 30)
        return {"w": plant_arm(cs, r, p, p, mid), "x": plant_arm(cs, r, p, p, mid)}

    add(g, "same_end", hairpin, D=None, popped=0, rounds=0, kept_ids=["w", "x"])
    # 17: a ring between nothing: dL = dR = 1 and its ends carry each other
    g = tc._Grow(42)
    ring = g.ring(4)
    add(g, "ring", lambda cs, r: {}, Lb=1000, D=None, popped=0, rounds=0, unitigs=1, kept_ids=ring)
    # 18: arms whose record at p is a containment: the neighbour read is as long as the overlap
    g = tc._Grow(43)
    small = g.start(25, rc=False)
    c = g.chain(3, lens=[60] * 3, ovs=[22] * 2)
    ps, qc = 2 * small + E, cc._end(g, c[0], B)

    def contained(cs, r):
        mid = bases(r, 30)
        return {"w": plant_arm(cs, r, ps, qc, mid), "x": plant_arm(cs, r, ps, qc, mid)}

    add(g, "containment_at_end", contained, D=None, popped=0, rounds=0, kept_ids=["w", "x"])
    # 19: an arm with dL == 2: a further read (too long to be trimmed) leaves its left end
    def branched(cs, r):
        mid = bases(r, 30)
        w = plant_arm(cs, r, cs["p"], cs["q"], mid)
        x = plant_arm(cs, r, cs["p"], cs["q"], mid)
        return {"w": w, "x": x, "t": cc.plant(cs, r, 2 * x + B, o1=22, mid=30)}

    ends_case(44, "branched_arm", branched, D=None, popped=0, rounds=0, kept_ids=["w", "x", "t"])

    # 20: two bubbles in series that share the unitig between them
    g = tc._Grow(45)
    a = g.chain(2, lens=[60, 60], ovs=[22])
    b = g.chain(2, lens=[60, 60], ovs=[22])
    c = g.chain(2, lens=[60, 60], ovs=[22])

    def series(cs, r):
        m1, m2 = bases(r, 30), bases(r, 35)
        return {"w1": plant_arm(cs, r, cc._end(g, a[1], E), cc._end(g, b[0], B), m1),
                "x1": plant_arm(cs, r, cc._end(g, a[1], E), cc._end(g, b[0], B), mutate(r, m1, (8,)), flip=True),
                "w2": plant_arm(cs, r, cc._end(g, b[1], E), cc._end(g, c[0], B), m2, flip=True),
                "x2": plant_arm(cs, r, cc._end(g, b[1], E), cc._end(g, c[0], B), mutate(r, m2, (30,)))}

    add(g, "series", series, popped=2, bub_rounds=1, rounds=1, unitigs=1, flagged={"x1": 1, "x2": 1}, kept_ids=a + b + c + ["w1", "w2"])

    # 21: a bubble that exists only after the trim steps of rounds 1 and 2 have taken a tip with two tips on it off one arm
    def late(cs, r):
        mid = bases(r, 30)
        w = plant_arm(cs, r, cs["p"], cs["q"], mid)
        x = plant_arm(cs, r, cs["p"], cs["q"], mutate(r, mid, (5,)))
        t = cc.plant(cs, r, 2 * x + E, o1=22, mid=18)
        return {"w": w, "x": x, "t": t, "t1": cc.plant(cs, r, 2 * t + E, o1=22, mid=18), "t2": cc.plant(cs, r, 2 * t + E, o1=24, mid=16)}

    ends_case(46, "second_round", late, L=45, popped=1, bub_rounds=1, rounds=2, flagged={"x": 2}, kept_ids=["w"], unitigs=1)

    # 22: the winner (two reads) is what the chimeric step would take: shorter than the other arm, between two branched ends of a
    # unique neighbour.  Without -b it goes as chimeric; with -b the loser goes first and the winner survives the round
    def thin_winner(cs, r):
        mid = bases(r, 30)
        x = plant_arm(cs, r, cs["p"], cs["q"], mutate(r, mid, (6,)), o1=40, o2=40)
        w = plant_chain(cs, r, cs["p"], cs["q"], mid, o1=22, o2=22, pieces=2, ov=30)
        return {"x": x, "w0": w[0], "w1": w[1]}

    ends_case(47, "chimeric_winner", thin_winner, Lc=100, popped=1, flagged={"x": 1}, kept_ids=["w0", "w1"], unitigs=1, chim=0)

    # 23: 2049 bubbles in one graph: more than a scan tile of unitigs, every third loser beyond the divergence
    g = tc._Grow(48)

    def field(cs, r):
        for k in range(2049):
            a, c = len(cs["reads"]), len(cs["reads"]) + 1
            cs["reads"] += [bases(r, 50), bases(r, 50)]
            mid = bases(r, 24)
            plant_arm(cs, r, 2 * a + E, 2 * c + B, mid, flip=k % 2 == 1)
            plant_arm(cs, r, 2 * a + E, 2 * c + B, mutate(r, mid, (1, 2) if k % 3 == 0 else (k % 24,)), flip=k % 4 >= 2)
        cs["N"] = len(cs["reads"])
        return {}

    add(g, "field2049", field, popped=2049 - 683, kept_div=2 * 683, bub_rounds=1, rounds=1, unitigs=2049 + 3 * 683)
    return cases


def case_named(name):
    return next(c for c in hand_built() if c["name"] == name)


KEYS = cc.KEYS + ("Lb", "D")


def run(fn, case, max_rounds=None, **over):
    kw = {k: case[k] for k in KEYS}
    kw.update(over)
    return fn(case["reads"], case["edges"], case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"], **kw)


@functools.lru_cache(maxsize=None)
def expected_of(name, max_rounds=None):
    return run(expected_bubble, case_named(name), max_rounds)


def with_bubble_keys(case, Lb=0, D=50):
    """a case of chimeric_cases, prune_cases or trim_cases as one of these"""
    c = dict(case)
    for k, v in (("delta", 0), ("careful", False), ("N", None), ("G", None), ("T", 13.0), ("Lc", 0), ("Ac", None), ("delta_c", 0), ("Tc", 0.0)):
        c.setdefault(k, v)
    c.update(Lb=Lb, D=D)
    return c


# ---- seeded random graphs: prune_cases.random_case with one or two bubbles planted ----
@functools.lru_cache(maxsize=None)
def random_case(seed):
    base = pc.random_case(seed)
    rng = random.Random(400000 + seed)
    case = dict(base, name="bubble_random%d" % seed, reads=list(base["reads"]), edges=list(base["edges"]))
    n0 = len(case["reads"])
    for _ in range(rng.randint(1, 2)):
        left, right = rng.randrange(2 * n0), rng.randrange(2 * n0)
        span = rng.randint(1, 40)
        mid = bases(rng, span)
        for k in range(rng.randint(2, 4)):
            diff = () if k == 0 else rng.sample(range(span), min(span, rng.choice((0, 1, 1, 1, 2, 6, 9))))
            m2 = mutate(rng, mid, diff) if rng.random() < 0.9 else bases(rng, rng.randint(1, 40))
            if rng.random() < 0.25 and len(m2) >= 30:
                plant_chain(case, rng, left, right, m2, o1=rng.randint(20, 35), o2=rng.randint(20, 35), pieces=2,
                            flips=[rng.random() < 0.5, rng.random() < 0.5], ov=rng.randint(20, 26))
            else:
                plant_arm(case, rng, left, right, m2, o1=rng.randint(20, 35), o2=rng.randint(20, 35), flip=rng.random() < 0.5)
    case.update(Lc=rng.choice((0, 0, 90)), Ac=None, delta_c=0, Tc=3.0, Lb=rng.choice((20, 40, 40, 60)), D=rng.choice((0, 50, 100, 100, 300, 300, None)),
                L=rng.choice((30, 30, 30, 50)))
    if rng.random() < 0.75:
        case["delta"] = 0
    return case


# ---- one larger seeded graph: prune_cases.large_case with 200 bubbles planted, about half of them within the divergence ----
@functools.lru_cache(maxsize=None)
def large_case(n_reads=20000, seed=5, bubbles=200):
    base = pc.large_case(n_reads, seed)
    rng = random.Random(500000 + seed)
    case = dict(base, name="bubble_large", reads=list(base["reads"]), edges=list(base["edges"]))
    n0 = len(case["reads"])
    for k in range(bubbles):
        left, right = rng.randrange(2 * n0), rng.randrange(2 * n0)
        span = rng.randint(20, 40)
        mid = bases(rng, span)
        other = mutate(rng, mid, rng.sample(range(span), 1 if k % 2 == 0 else 4))
        plant_arm(case, rng, left, right, mid, o1=rng.randint(45, 60), o2=rng.randint(45, 60), flip=rng.random() < 0.5)
        if k % 5 == 0:
            plant_chain(case, rng, left, right, other, o1=rng.randint(45, 60), o2=rng.randint(45, 60), pieces=2,
                        flips=[rng.random() < 0.5, rng.random() < 0.5], ov=50)
        else:
            plant_arm(case, rng, left, right, other, o1=rng.randint(45, 60), o2=rng.randint(45, 60), flip=rng.random() < 0.5)
    # no cut step, no chimeric step, and no read of 100 is short enough to trim: only the bubble steps change the graph
    case.update(Lc=0, Ac=None, delta_c=0, Tc=3.0, x=8, L=99, delta=0, N=len(case["reads"]), Lb=40, D=50)
    return case


# ---- end to end: reads that tile two haplotypes of a small genome ----
E2E_SEED, E2E_GENOME, E2E_READS, E2E_LEN, E2E_M, E2E_SNP_EVERY = 31, 6000, 2400, 100, 40, 1000
E2E_X, E2E_L, E2E_LB, E2E_D = 10, 150, 100, 1000  # (at 40-fold coverage a window is a few bases: one substitution is most of it)


@functools.lru_cache(maxsize=None)
def end_to_end():
    """-> (names, reads): 2 400 error-free reads of 100, every place and strand at most once, half each from a 6 000-base random genome and from a copy of
    it with a substitution every 1 000 bases"""
    rng = random.Random(E2E_SEED)
    g = bases(rng, E2E_GENOME)
    h = mutate(rng, g, range(E2E_SNP_EVERY // 2, E2E_GENOME, E2E_SNP_EVERY))
    draws = rng.sample(range(2 * (E2E_GENOME - E2E_LEN + 1)), E2E_READS)  # (no two reads from one place and strand: no containments)
    reads = []
    for key in draws:
        at = key >> 1
        w = (g if rng.random() < 0.5 else h)[at:at + E2E_LEN]
        reads.append(uc.revcomp(w) if key & 1 else w)
    return ["r%d" % i for i in range(len(reads))], reads
