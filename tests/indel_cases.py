"""Cases and two brute forces for indel bubble popping in the rounds of `siga unitig` (sigax_unitigs_indel_*, the rules in
include/sigax.h); no tests here (tests/test_indel_cases.py, tests/test_gpu_unitig_indel.py).

expected_indel()     the rules, serially from the reads: the round loop of bubble_cases._rounds with the indel step between its bubble
                     and its chimeric step.  The indel step finds the arms as the bubble step does, groups them by (lo, hi), and takes
                     the edit distance of the windows [o_lo, o_lo + span) in the frame of the smaller neighbour state by the plain
                     full-matrix recurrence.
independent_indel()  the same loop with the other bubble step (bubble_cases._step_strings) and another indel step: no frames and no
                     windows.  It lays neighbour + arm + neighbour out as one string, groups the strings by (p, q), and takes the edit
                     distance of the whole strings by the bit-vector algorithm (Myers 1999, as Hyyro 2001 states it).  A common
                     prefix and a common suffix do not change a Levenshtein distance, so the two must agree.
The reference has no such step (SmoothingVisitor::visit returns false): there is nothing to compare against but the rules themselves.

A case: bubble_cases' dict plus Ed (max_edits E) and De (max edits per mille of the shorter arm's bases)."""
import functools
import random

import numpy as np

from tests import bubble_cases as bc
from tests import chimeric_cases as cc
from tests import prune_cases as pc
from tests import trim_cases as tc
from tests import unitig_cases as uc

B, E = uc.B, uc.E
CHIMERIC, BUBBLE = cc.CHIMERIC, bc.BUBBLE
INDEL = 0x20000000  # SIGAX_REMOVED_INDEL
SAT = cc.SAT
MAX_EDITS, MAX_SPAN = 31, 4096


# ---- two edit distances ----
def lev(x, y):
    """unit-cost Levenshtein distance, the full matrix row by row (a row at a time in numpy: the minimum over the cell above, the cell
    above left and, as a running minimum along the row, the cell to the left)"""
    ya = np.frombuffer(bytes(y), dtype=np.uint8)
    ar = np.arange(len(y) + 1, dtype=np.int64)
    prev = ar.copy()
    for i, cx in enumerate(bytes(x), 1):
        row = np.empty(len(y) + 1, dtype=np.int64)
        row[0] = i
        row[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (ya != cx))
        prev = np.minimum.accumulate(row - ar) + ar
    return int(prev[len(y)])


def lev_bits(x, y):
    """the same distance by bit vectors over the columns of x: one big-integer step per byte of y"""
    m = len(x)
    if m == 0:
        return len(y)
    peq = {}
    for i, c in enumerate(x):
        peq[c] = peq.get(c, 0) | (1 << i)
    mask, top = (1 << m) - 1, 1 << (m - 1)
    pv, mv, score = mask, 0, m
    for c in y:
        eq = peq.get(c, 0)
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | (~(xh | pv) & mask)
        mh = pv & xh
        if ph & top:
            score += 1
        elif mh & top:
            score -= 1
        ph = ((ph << 1) | 1) & mask
        mh = (mh << 1) & mask
        pv = mh | (~(xv | ph) & mask)
        mv = ph & xv
    return score


def _verdict(ed, Ed, De, bases_l, bases_w):
    return ed <= Ed and ed * 1000 <= De * min(bases_l, bases_w)


# ---- the two indel steps ----
def _indel_frames(units, ring, seqs, unit, deg, at, Lb, Ed, De):
    """the rules of sigax.h as they are written -> ([unitigs popped], compared losers kept, losers not compared, log)"""
    groups = {}
    for u, p, q, o_p, o_q in bc._arms(units, ring, unit, deg, at):
        lo, hi = min(p, q), max(p, q)
        o_lo, o_hi = (o_p, o_q) if p < q else (o_q, o_p)
        span = units[u][1] - o_lo - o_hi
        if 1 <= span <= Lb:
            groups.setdefault((lo, hi), []).append((u, o_lo, p == lo, span))
    gone, kept, skipped, log = [], 0, 0, []
    for (lo, hi), arms in sorted(groups.items()):
        if len(arms) < 2:
            continue
        frame = lambda a: seqs[a[0]] if a[2] else uc.revcomp(seqs[a[0]])  # noqa: E731
        window = lambda a: frame(a)[a[1]:a[1] + a[3]]  # noqa: E731
        win = max(arms, key=lambda a: (len(units[a[0]][0]), -units[a[0]][0][0]))
        xw = window(win)
        for a in arms:
            if a is win:
                continue
            entry = {"lo": lo, "hi": hi, "span": a[3], "winner_span": win[3], "winner": units[win[0]][0][0], "loser": units[a[0]][0][0],
                     "reversed": not a[2], "winner_reversed": not win[2], "reads": len(units[a[0]][0]), "ed": None}
            if a[3] == win[3]:
                entry["cls"] = "SAME_SPAN"
                skipped += 1
            elif abs(a[3] - win[3]) > Ed:
                entry["cls"] = "FAR"
                skipped += 1
            else:
                ed = lev(window(a), xw)
                entry["ed"] = ed
                if _verdict(ed, Ed, De, units[a[0]][1], units[win[0]][1]):
                    entry["cls"] = "POPPED"
                    gone.append(a[0])
                else:
                    entry["cls"] = "KEPT_EDITS" if ed > Ed else "KEPT_PERMILLE"
                    kept += 1
            log.append(entry)
    return gone, kept, skipped, log


def _indel_strings(units, ring, seqs, unit, deg, at, Lb, Ed, De):
    """neighbour + arm + neighbour as one string -> ([unitigs popped], compared losers kept, losers not compared, [])"""

    def ending_in(s):  # the unitig of state s, read so that s is its right end
        rs, _, s_left, s_right = units[unit[s >> 1]]
        assert s in (s_left, s_right) and s_left != s_right
        return seqs[unit[s >> 1]] if s == s_right else uc.revcomp(seqs[unit[s >> 1]])

    by_ends = {}
    for u, p, q, o_p, o_q in bc._arms(units, ring, unit, deg, at):
        arm = seqs[u]
        if p > q:  # walk every arm from the smaller neighbour state to the larger
            arm, p, q, o_p, o_q = uc.revcomp(arm), q, p, o_q, o_p
        left, right = ending_in(p), uc.revcomp(ending_in(q))
        assert left[-o_p:] == arm[:o_p] and arm[-o_q:] == right[:o_q], "a record that is no overlap"
        inner = len(arm) - o_p - o_q
        if not 1 <= inner <= Lb:
            continue
        whole = left + arm[o_p:] + right[o_q:]
        by_ends.setdefault((p, q), []).append((len(units[u][0]), -units[u][0][0], u, whole, inner, len(arm)))
    gone, kept, skipped = [], 0, 0
    for arms in by_ends.values():
        if len(arms) < 2:
            continue
        win = max(arms)
        for a in arms:
            if a is win:
                continue
            if a[4] == win[4] or abs(a[4] - win[4]) > Ed:
                skipped += 1
                continue
            if _verdict(lev_bits(a[3], win[3]), Ed, De, a[5], win[5]):
                gone.append(a[2])
            else:
                kept += 1
    return gone, kept, skipped, []


def left_out(reads, edges, m, max_rounds, L, C=None, **kw):
    """-> how many arms of the round-1 state the indel step leaves out because span < 1 (the number a later change would need)"""
    return _rounds(bc._step_frames, _indel_frames, reads, edges, m, min(max_rounds, 1), L, C, **kw)["span_below_1"]


# ---- the round loop: bubble_cases._rounds', with the indel step behind the bubble step ----
def _rounds(bubble_step, indel_step, reads, edges, m, max_rounds, L, C=None, delta=0, careful=False, N=None, G=None, T=13.0, Lc=0, Ac=None,
            delta_c=0, Tc=0.0, Lb=0, D=50, Ed=0, De=50, tables_only=False):
    assert Ed == 0 or (0 < Lb <= MAX_SPAN and Ed <= MAX_EDITS)
    n = len(reads)
    N = n if N is None else N
    lens = [uc.nbases(r) for r in reads]
    kept, bad, low = tc._kept(edges, lens, m)
    removed, cut = [0] * n, [0] * len(edges)
    islands = dead_ends = rounds = cut_rounds = uniq_first = chim_units = chim_reads = chim_rounds = 0
    popped = bub_reads = bub_rounds = kept_div = 0
    ind_popped = ind_reads = ind_rounds = ind_kept = ind_skipped = span_below_1 = 0
    log, ilog = [], []

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

    def arms_state():
        alive, new, live, res, deg, units = graph()
        unit = {r: u for u, (rs, _, _, _) in enumerate(units) for r in rs}
        part, at = participants(live)
        seqs = res["lazy_seqs"] if tables_only else [res["useqs"][res["seq_offs"][u]:res["seq_offs"][u + 1]] for u in range(len(units))]
        ring = [bool(f & uc.CIRCULAR) for f in res["uflags"]]
        return units, ring, seqs, unit, deg, at

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
            units, ring, seqs, unit, deg, at = arms_state()
            pop, kept_now, lg = bubble_step(units, ring, seqs, unit, deg, at, Lb, D)
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
        if Ed > 0:  # the indel step, over what the bubble step left
            units, ring, seqs, unit, deg, at = arms_state()
            if rnd == 1:
                for u, p, q, o_p, o_q in bc._arms(units, ring, unit, deg, at):
                    span_below_1 += units[u][1] - o_p - o_q < 1
            pop, kept_now, skipped_now, lg = indel_step(units, ring, seqs, unit, deg, at, Lb, Ed, De)
            ind_kept += kept_now
            ind_skipped += skipped_now
            ilog += [dict(e, round=rnd) for e in lg]
            for u in pop:
                for r in units[u][0]:
                    removed[r] = rnd | INDEL
            if pop:
                changed = True
                ind_popped += len(pop)
                ind_reads += sum(len(units[u][0]) for u in pop)
                ind_rounds += 1
        if Lc > 0:  # the chimeric step, over what the step before left
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
                     kept_div, ind_popped, ind_reads, ind_rounds, ind_kept, ind_skipped, 0, 0, 0]
    res["removed"] = removed
    res["cut"] = cut
    res["uedges"] = uedges
    res["bubble_log"] = log
    res["indel_log"] = ilog
    res["span_below_1"] = span_below_1
    return res


def expected_indel(reads, edges, m, max_rounds, L, C=None, **kw):
    """-> bubble_cases.expected_bubble's dict with status [32]; removed carries INDEL on the reads an indel step took; indel_log: one
    entry per loser of an indel step, with its class (POPPED, KEPT_EDITS, KEPT_PERMILLE, SAME_SPAN, FAR) and, where compared, its ed.
    tables_only = True: as unitig_cases.expected's; a compared arm's reads must be bytes"""
    return _rounds(bc._step_frames, _indel_frames, reads, edges, m, max_rounds, L, C, **kw)


def independent_indel(reads, edges, m, max_rounds, L, C=None, **kw):
    return _rounds(bc._step_strings, _indel_strings, reads, edges, m, max_rounds, L, C, **kw)


# ---- edits on the bytes between the ends ----
bases, mutate, plant_arm, plant_chain = bc.bases, bc.mutate, bc.plant_arm, bc.plant_chain


def insert(rng, s, at, what=None):
    """one base put in before position `at` (at == len(s): behind the last)"""
    return s[:at] + (bytes([rng.choice(b"ACGT")]) if what is None else what) + s[at:]


def delete(s, at):
    return s[:at] + s[at + 1:]


def _case(g, name, x=10, L=30, Lb=40, D=50, Lc=0, Ed=2, De=1000, **claims):
    c = bc._case(g, name, x=x, L=L, Lb=Lb, D=D, Lc=Lc, **claims)
    c.update(Ed=Ed, De=De)
    return c


@functools.lru_cache(maxsize=None)
def hand_built():
    """claims: popped (status[24]), ind_reads (25), ind_rounds (26), kept (27), skipped (28), bub (20), chim (16), rounds (6), unitigs (0),
    flagged {read: round}: removed with INDEL in that round, kept_ids: not removed, eds: the sorted edit distances of round 1's
    compared pairs, classes: the sorted classes of round 1's losers"""
    cases = []

    def add(g, name, build, **kw):
        c = _case(g, name, **kw)
        ids = build(c, random.Random(7000 + len(cases)))
        claims = c["claims"]
        look = lambda k: ids[k] if isinstance(k, str) else k  # noqa: E731
        if "kept_ids" in claims:
            claims["kept_ids"] = [look(k) for k in claims["kept_ids"]]
        if "flagged" in claims:
            claims["flagged"] = {look(k): r for k, r in claims["flagged"].items()}
        cases.append(c)
        return c

    def ends_case(seed, name, build, **kw):
        g, a, c, p, q = bc._ends(seed)

        def wrapped(cs, r):
            cs["p"], cs["q"] = p, q
            ids = build(cs, r)
            ids.update(a=a, c=c)
            return ids

        return add(g, name, wrapped, **kw)

    def two(span=30, edit=lambda r, mid: delete(mid, 7), flips=(False, False), want=None, **kw):
        """the winner w over `span` random bases, the loser x over what `edit` makes of them"""
        def build(cs, r):
            mid = bases(r, span)
            other = edit(r, mid)
            assert want is None or lev(mid, other) == want, (lev(mid, other), want)
            return {"w": plant_arm(cs, r, cs["p"], cs["q"], mid, flip=flips[0], **kw),
                    "x": plant_arm(cs, r, cs["p"], cs["q"], other, flip=flips[1], **kw)}
        return build

    one = dict(popped=1, ind_reads=1, ind_rounds=1, rounds=1, unitigs=1, flagged={"x": 1}, kept_ids=["w"])
    stays = dict(popped=0, rounds=0, unitigs=4, kept_ids=["w", "x"])
    # 1: where the edit lies: one base out or in, at the first, a middle and the last place of the window; either strand
    for k, (name, at) in enumerate((("first", 0), ("middle", 14), ("last", 29))):
        ends_case(1 + k, "deleted_" + name, two(edit=lambda r, mid, at=at: delete(mid, at), want=1), eds=[1], **one)
        ends_case(4 + k, "inserted_" + name, two(edit=lambda r, mid, at=at: insert(r, mid, at + (at == 29)), want=1, flips=(False, True)), eds=[1], **one)
    ends_case(7, "deleted_flipped", two(edit=lambda r, mid: delete(mid, 0), flips=(True, True), want=1), eds=[1], **one)

    # 2: many optimal paths: a base more in a homopolymer, a unit more in a period-3 repeat
    def homopolymer(cs, r):
        mid = bases(r, 10) + b"A" * 9 + bases(r, 10)
        return {"w": plant_arm(cs, r, cs["p"], cs["q"], mid), "x": plant_arm(cs, r, cs["p"], cs["q"], mid[:14] + b"A" + mid[14:], flip=True)}

    def period3(cs, r):
        mid = bases(r, 8) + b"CAG" * 5 + bases(r, 8)
        return {"w": plant_arm(cs, r, cs["p"], cs["q"], mid), "x": plant_arm(cs, r, cs["p"], cs["q"], mid[:8] + b"CAG" + mid[8:])}

    ends_case(8, "homopolymer", homopolymer, Ed=1, eds=[1], **one)
    ends_case(9, "period3", period3, Ed=3, eds=[3], **one)
    ends_case(10, "period3_e2", period3, Ed=2, classes=["FAR"], skipped=1, **stays)
    # 3: an indel and substitutions: ed = E goes, ed = E + 1 stays, both with |a - b| = 1 < E
    sub2 = lambda r, mid: mutate(r, delete(mid, 20), (3,))  # noqa: E731
    sub3 = lambda r, mid: mutate(r, delete(mid, 20), (3, 11))  # noqa: E731
    ends_case(11, "ed_at_e", two(edit=sub2, want=2), Ed=2, eds=[2], **one)
    ends_case(12, "ed_above_e", two(edit=sub3, want=3), Ed=2, eds=[3], classes=["KEPT_EDITS"], kept=1, **stays)
    # 4: the limits of E: 1, 2 and 31; |a - b| = 1, E and E + 1
    ends_case(13, "e1_diff1", two(edit=lambda r, mid: delete(mid, 9), want=1), Ed=1, eds=[1], **one)
    ends_case(14, "e1_diff2", two(edit=lambda r, mid: delete(delete(mid, 9), 20)), Ed=1, classes=["FAR"], skipped=1, **stays)
    ends_case(15, "e2_diff2", two(edit=lambda r, mid: delete(delete(mid, 9), 20), want=2), Ed=2, eds=[2], **one)
    ends_case(16, "e2_diff3", two(edit=lambda r, mid: mid[:5] + mid[8:]), Ed=2, classes=["FAR"], skipped=1, **stays)
    ends_case(17, "e31_diff31", two(span=100, edit=lambda r, mid: mid[:40] + mid[71:], want=31), Lb=100, Ed=31, eds=[31], **one)
    ends_case(18, "e31_diff32", two(span=100, edit=lambda r, mid: mid[:40] + mid[72:]), Lb=100, Ed=31, classes=["FAR"], skipped=1, **stays)
    ends_case(19, "e31_diff1", two(span=100, edit=lambda r, mid: insert(r, mid, 50), want=1), Lb=101, Ed=31, eds=[1], **one)
    # (31 edits of which 30 are substitutions at every third place, and one more)
    ends_case(20, "e31_ed31", two(span=100, edit=lambda r, mid: mutate(r, delete(mid, 99), range(0, 90, 3)), want=31), Lb=100, Ed=31, eds=[31], **one)
    ends_case(21, "e31_ed32", two(span=100, edit=lambda r, mid: mutate(r, delete(mid, 99), range(0, 93, 3)), want=32), Lb=100, Ed=31, eds=[32],
              classes=["KEPT_EDITS"], kept=1, **stays)
    # 5: ed * 1000 against De * min(bases): both arms one read; 1000 == 1 * 1000 goes, 1000 > 1 * 999 stays
    ends_case(22, "at_permille", two(span=951, edit=lambda r, mid: delete(mid, 500), want=1), Lb=1000, Ed=4, De=1, eds=[1], **one)
    ends_case(23, "above_permille", two(span=950, edit=lambda r, mid: delete(mid, 500), want=1), Lb=1000, Ed=4, De=1, eds=[1],
              classes=["KEPT_PERMILLE"], kept=1, **stays)
    ends_case(24, "permille_0", two(), Ed=4, De=0, eds=[1], classes=["KEPT_PERMILLE"], kept=1, **stays)
    # 6: the smallest windows: 1 against 2, 1 against 1 + E, 2 against 1 (the winner longer and the winner shorter)
    ends_case(25, "span_1_2", two(span=1, edit=lambda r, mid: insert(r, mid, 1), want=1), Ed=1, eds=[1], **one)
    ends_case(26, "span_2_1", two(span=2, edit=lambda r, mid: delete(mid, 0), want=1), Ed=1, eds=[1], **one)
    ends_case(27, "span_1_4", two(span=1, edit=lambda r, mid: mid + bases(r, 3), want=3), Ed=3, eds=[3], **one)
    ends_case(28, "span_1_5", two(span=1, edit=lambda r, mid: mid + bases(r, 4)), Ed=3, classes=["FAR"], skipped=1, **stays)
    # 7: the window at a wave's width
    for k, span in enumerate((63, 64, 65)):
        ends_case(29 + k, "span_%d" % span, two(span=span, edit=lambda r, mid: mutate(r, insert(r, mid, len(mid)), (0,)), want=2), Lb=70, Ed=2,
                  eds=[2], **one)
    # 8: span at Lb and above it: an arm beyond Lb takes no part
    ends_case(32, "winner_at_lb", two(span=40, edit=lambda r, mid: delete(mid, 3), want=1), eds=[1], **one)
    ends_case(33, "loser_above_lb", two(span=40, edit=lambda r, mid: insert(r, mid, 3)), **stays)

    # 9: the staging limit: windows of 4095 and 4096 bytes over arms of several reads, the winner the longer and the shorter one
    def long_arms(span_w, span_x, pieces_w, pieces_x, flips=False):
        def build(cs, r):
            mid = bases(r, max(span_w, span_x))
            short = mutate(r, delete(mid, 2000), (0, len(mid) - 2))
            mw, mx = (mid, short) if span_w > span_x else (short, mid)
            fl = lambda k: [flips and i % 3 == 1 for i in range(k)]  # noqa: E731
            w = plant_chain(cs, r, cs["p"], cs["q"], mw, o1=25, o2=27, pieces=pieces_w, flips=fl(pieces_w))
            x = plant_chain(cs, r, cs["p"], cs["q"], mx, o1=31, o2=22, pieces=pieces_x, flips=fl(pieces_x))
            return {"w0": w[0], "w1": w[-1], "x0": x[0], "x1": x[-1]}
        return build

    big = dict(popped=1, ind_rounds=1, rounds=1, unitigs=1, eds=[3], flagged={"x0": 1, "x1": 1}, kept_ids=["w0", "w1"])
    ends_case(34, "span_4096_winner", long_arms(4096, 4095, 40, 39), Lb=4096, Ed=3, De=50, ind_reads=39, **big)
    ends_case(35, "span_4096_loser", long_arms(4095, 4096, 40, 39, flips=True), Lb=4096, Ed=3, De=50, ind_reads=39, **big)

    # 10: arm and winner entered through the left or the right end, all four ways (p > q in two of them)
    def entered(swap_ends, w_right, x_right):
        def build(cs, r):
            mid = bases(r, 30)
            other = mutate(r, insert(r, mid, 0), (29,))
            if swap_ends:
                cs["p"], cs["q"] = max(cs["p"], cs["q"]), min(cs["p"], cs["q"])
            p, q = cs["p"], cs["q"]
            put = lambda s, right: plant_arm(cs, r, q, p, uc.revcomp(s)) if right else plant_arm(cs, r, p, q, s)  # noqa: E731
            return {"w": put(mid, w_right), "x": put(other, x_right)}
        return build

    for k, (sw, wr, xr) in enumerate(((False, False, True), (False, True, False), (True, True, True), (True, False, False))):
        ends_case(36 + k, "entered_%d%d%d" % (sw, wr, xr), entered(sw, wr, xr), Ed=2, eds=[2], **one)

    # 11: U(p) == U(q): a bubble from the E end of a chain back to its B end
    g = tc._Grow(140)
    a = g.chain(4, lens=[60] * 4, ovs=[22] * 3)
    pe, pb = cc._end(g, a[3], E), cc._end(g, a[0], B)

    def loop_back(cs, r):
        mid = bases(r, 30)
        return {"w": plant_arm(cs, r, pe, pb, mid), "x": plant_arm(cs, r, pe, pb, delete(mid, 12), flip=True)}

    add(g, "same_unitig", loop_back, popped=1, eds=[1], flagged={"x": 1}, kept_ids=a + ["w"], unitigs=1)

    # 12: three arms of spans s, s, s + 1: the bubble step takes the equal-span one first, or keeps it and this step leaves it alone
    def three(subs):
        def build(cs, r):
            mid = bases(r, 30)
            return {"w": plant_arm(cs, r, cs["p"], cs["q"], mid), "x": plant_arm(cs, r, cs["p"], cs["q"], mutate(r, mid, subs)),
                    "y": plant_arm(cs, r, cs["p"], cs["q"], insert(r, mid, 17), flip=True)}
        return build

    ends_case(40, "three_bubble_pops", three((4,)), bub=1, popped=1, eds=[1], classes=["POPPED"], flagged={"y": 1}, kept_ids=["w"], rounds=1, unitigs=1)
    # (round 2 judges x again: not compared is summed over the rounds that ran)
    ends_case(41, "three_bubble_keeps", three((4, 9, 20)), bub=0, popped=1, eds=[1], classes=["POPPED", "SAME_SPAN"], skipped=2, flagged={"y": 1},
              kept_ids=["w", "x"], rounds=1)

    # 13: 130 arms of mixed spans in one group, no two alike: more than two waves of losers; popped, far, same span and kept on edits.
    # D = 0: the bubble step, which meets the arms of one span first, pops none of them
    def many(cs, r):
        mid = bases(r, 30)
        ids, seen = {"w": plant_arm(cs, r, cs["p"], cs["q"], mid)}, {mid}
        for i in range(1, 130):
            kind = i % 5
            while True:
                m2 = (mutate(r, delete(mid, r.randrange(30)), (r.randrange(29),)) if kind == 0 else
                      mutate(r, insert(r, mid, r.randrange(31)), (r.randrange(31),)) if kind == 1 else
                      mutate(r, mid[:10] + mid[13:], (r.randrange(27),)) if kind == 2 else
                      mutate(r, mid, r.sample(range(30), 4)) if kind == 3 else mutate(r, delete(mid, 29), r.sample(range(29), 3)))
                if m2 not in seen and (kind != 4 or lev(m2, mid) > 2):
                    break
            seen.add(m2)
            ids["x%d" % i] = plant_arm(cs, r, cs["p"], cs["q"], m2, flip=i % 3 == 0)
        return ids

    # kinds 0 and 1 go (25 + 26); kind 2 is FAR and kind 3 SAME_SPAN (26 + 26, judged in both rounds); kind 4 has ed > E (26, both rounds)
    ends_case(42, "arms130", many, Ed=2, D=0, bub=0, popped=51, ind_reads=51, ind_rounds=1, kept=52, skipped=104, rounds=1,
              kept_ids=["w", "x2", "x3", "x4"], flagged={"x1": 1, "x5": 1, "x125": 1})

    # 14: N and lower case inside the windows: bytes are compared as bytes
    def letters(in_w, in_x):
        def build(cs, r):
            mid = bytearray(bases(r, 30))
            other = bytearray(delete(bytes(mid), 25))
            for at, ch in ((11, ord("N")), (5, ord("a"))):
                if in_w:
                    mid[at] = ch
                if in_x:
                    other[at] = ch
            return {"w": plant_arm(cs, r, cs["p"], cs["q"], bytes(mid)), "x": plant_arm(cs, r, cs["p"], cs["q"], bytes(other), flip=in_w and in_x)}
        return build

    ends_case(43, "letters_in_one", letters(False, True), Ed=2, eds=[3], classes=["KEPT_EDITS"], kept=1, **stays)
    ends_case(44, "letters_in_one_e3", letters(True, False), Ed=3, eds=[3], **one)
    ends_case(45, "letters_in_both", letters(True, True), Ed=1, eds=[1], **one)

    # 15: a bubble that exists only after the trim steps of rounds 1 and 2 (bubble_cases' second_round with a deletion)
    def late(cs, r):
        mid = bases(r, 30)
        w = plant_arm(cs, r, cs["p"], cs["q"], mid)
        x = plant_arm(cs, r, cs["p"], cs["q"], delete(mid, 5))
        t = cc.plant(cs, r, 2 * x + E, o1=22, mid=18)
        return {"w": w, "x": x, "t": t, "t1": cc.plant(cs, r, 2 * t + E, o1=22, mid=18), "t2": cc.plant(cs, r, 2 * t + E, o1=24, mid=16)}

    ends_case(46, "second_round", late, L=45, popped=1, ind_rounds=1, rounds=2, flagged={"x": 2}, kept_ids=["w"], unitigs=1)

    # 16: the winner (two reads) is what the chimeric step would take; with this step the loser goes first and the winner survives
    def thin_winner(cs, r):
        mid = bases(r, 30)
        x = plant_arm(cs, r, cs["p"], cs["q"], insert(r, mid, 6), o1=40, o2=40)
        w = plant_chain(cs, r, cs["p"], cs["q"], mid, o1=22, o2=22, pieces=2, ov=30)
        return {"x": x, "w0": w[0], "w1": w[1]}

    ends_case(47, "chimeric_winner", thin_winner, Lc=100, popped=1, eds=[1], flagged={"x": 1}, kept_ids=["w0", "w1"], unitigs=1, chim=0)
    return cases


def case_named(name):
    return next(c for c in hand_built() if c["name"] == name)


KEYS = bc.KEYS + ("Ed", "De")


def run(fn, case, max_rounds=None, **over):
    kw = {k: case[k] for k in KEYS}
    kw.update(over)
    return fn(case["reads"], case["edges"], case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"], **kw)


@functools.lru_cache(maxsize=None)
def expected_of(name, max_rounds=None):
    return run(expected_indel, case_named(name), max_rounds)


def with_indel_keys(case, Ed=0, De=50):
    """a case of bubble_cases as one of these"""
    c = dict(case)
    c.update(Ed=Ed, De=De)
    return c


def shuffled(case, seed, fixed_from):
    """the same graph with its records in another order and the reads below `fixed_from` (the neighbours' chains) renumbered among
    themselves: lo and hi change, and with them the frames; the arms keep their ids, and so the ties on K their winners
    -> (case, new id of every old read)"""
    rng = random.Random(seed)
    new = list(range(fixed_from))
    rng.shuffle(new)
    new += list(range(fixed_from, len(case["reads"])))
    reads = [None] * len(new)
    for old, r in enumerate(case["reads"]):
        reads[new[old]] = r
    edges = [(new[q], new[t], ln, fl) for q, t, ln, fl in case["edges"]]
    rng.shuffle(edges)
    return dict(case, name=case["name"] + "_shuffled", reads=reads, edges=edges), new


# ---- seeded random graphs: prune_cases.random_case with one or two bubbles planted, their arms apart by substitutions and indels ----
@functools.lru_cache(maxsize=None)
def random_case(seed):
    base = pc.random_case(seed)
    rng = random.Random(600000 + seed)
    case = dict(base, name="indel_random%d" % seed, reads=list(base["reads"]), edges=list(base["edges"]))
    n0 = len(case["reads"])
    for _ in range(rng.randint(1, 2)):
        left, right = rng.randrange(2 * n0), rng.randrange(2 * n0)
        span = rng.randint(4, 40)
        mid = bases(rng, span)
        for k in range(rng.randint(2, 4)):
            m2 = mid
            if k > 0:
                for _e in range(rng.choice((0, 1, 1, 1, 2, 3, 6))):
                    kind, at = rng.randrange(3), rng.randrange(len(m2))
                    m2 = mutate(rng, m2, (at,)) if kind == 0 else insert(rng, m2, at) if kind == 1 or len(m2) < 3 else delete(m2, at)
            if rng.random() < 0.25 and len(m2) >= 30:
                plant_chain(case, rng, left, right, m2, o1=rng.randint(20, 35), o2=rng.randint(20, 35), pieces=2,
                            flips=[rng.random() < 0.5, rng.random() < 0.5], ov=rng.randint(20, 26))
            else:
                plant_arm(case, rng, left, right, m2, o1=rng.randint(20, 35), o2=rng.randint(20, 35), flip=rng.random() < 0.5)
    case.update(Lc=rng.choice((0, 0, 90)), Ac=None, delta_c=0, Tc=3.0, Lb=rng.choice((20, 40, 40, 60)), D=rng.choice((0, 50, 100, 300, None)),
                L=rng.choice((30, 30, 30, 50)), Ed=rng.choice((1, 2, 2, 4, 8)), De=rng.choice((0, 10, 30, 50, 50, 1000)))
    if rng.random() < 0.75:
        case["delta"] = 0
    return case


# ---- many small bubbles at once: every counter the sum of slots that more than one wave added to ----
@functools.lru_cache(maxsize=None)
def many_bubbles(indels=44, plain=40, fillers=420):
    """-> (case, expected_indel's dict of it): `indels` bubbles apart by one deleted base and `plain` apart by one substitution, each
    between two chains of its own, and `fillers` chains of four short reads, every fourth with a tip: more than 2048 reads, so the
    256-lane kernels run more than 32 waves, and more than 32 pairs compared in round 1, one workgroup of one wave each"""
    g = tc._Grow(4100)
    pairs = [(g.chain(2, lens=[60] * 2, ovs=[22]), g.chain(2, lens=[60] * 2, ovs=[22])) for _ in range(indels + plain)]
    fill = [g.chain(4, lens=[50] * 4, ovs=[22] * 3) for _ in range(fillers)]
    case = _case(g, "many_bubbles", x=10, L=45, Lb=40, D=50, Ed=2, De=1000)
    case["N"] = None  # (the reads given: the call refuses a smaller number)
    rng = random.Random(4101)
    for k, (a, c) in enumerate(pairs):
        p, q = cc._end(g, a[1], E), cc._end(g, c[0], B)
        mid = bases(rng, 30)
        plant_arm(case, rng, p, q, mid, flip=k % 3 == 1)
        plant_arm(case, rng, p, q, delete(mid, k % 30) if k < indels else mutate(rng, mid, (k % 30,)), flip=k % 2 == 1)
    for chain in fill[::4]:
        cc.plant(case, rng, cc._end(g, chain[1], E), o1=22, mid=18)
    exp = run(expected_indel, case)
    assert len(case["reads"]) == 4 * (indels + plain) + 2 * (indels + plain) + 4 * fillers + (fillers + 3) // 4 > 2048
    assert sum(1 for e in exp["indel_log"] if e["round"] == 1 and e["ed"] is not None) >= 40
    st = exp["status"]
    assert st[8] == (fillers + 3) // 4 and st[20] == plain and st[24] == indels, st  # tips, bubbles, indel bubbles: all taken
    return case, exp


# ---- end to end: reads that tile two haplotypes of a small genome, apart by substitutions and short indels ----
E2E_SEED, E2E_GENOME, E2E_READS, E2E_LEN, E2E_M, E2E_EVERY = 37, 6000, 2400, 100, 40, 1000
E2E_X, E2E_L, E2E_LB, E2E_D, E2E_ED, E2E_DE = 10, 150, 100, 1000, 4, 1000


@functools.lru_cache(maxsize=None)
def end_to_end():
    """-> (names, reads): 2 400 error-free reads of 100, half each from a 6 000-base random genome and from a copy of it with, every 1 000
    bases in turn, a substitution, a deleted base and three inserted bases"""
    rng = random.Random(E2E_SEED)
    g = bases(rng, E2E_GENOME)
    h, kind = g, 0
    for at in range(E2E_GENOME - E2E_EVERY // 2, 0, -E2E_EVERY):  # (from the far end: earlier places keep their offsets)
        h = mutate(rng, h, (at,)) if kind % 3 == 0 else delete(h, at) if kind % 3 == 1 else h[:at] + bases(rng, 3) + h[at:]
        kind += 1
    reads = []
    seen = set()
    while len(reads) < E2E_READS:
        src = g if rng.random() < 0.5 else h
        at, rev = rng.randrange(len(src) - E2E_LEN + 1), rng.random() < 0.5
        w = src[at:at + E2E_LEN]
        if w in seen:  # (no read twice: no containments)
            continue
        seen.add(w)
        reads.append(uc.revcomp(w) if rev else w)
    return ["r%d" % i for i in range(len(reads))], reads
