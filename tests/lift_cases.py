"""A small case of `siga unitig --scaffold --join-overlaps` or `--gapfill` lifted behind ballast, so that its offsets, its sources
and its status carry a high word -- beyond 2^32 in tests/test_gpu_gapfill_join_wide.py -- while its expected result follows from
the small case's by shifting.  No tests here (tests/test_lift_cases.py holds the shift rule against the restatements with small
ballast of explicit bytes; the GPU test uses it where no restatement can run).

The ballast has two forms.
  front   ballast scaffolds laid before the case's scaffolds, their unitigs before the case's unitigs.  An int X is one unitig of
          X bases alone in its scaffold.  For join, (lu, lv, v, G) is two unitigs in one scaffold, G bytes of N between them, the
          second beginning with the first's last v bytes: with v >= k - 1 there is no window across the junction, so the gap is
          JOINED whatever the reads hold (given that v is the only match, which the caller checks on the bytes).  For gapfill,
          (lu, lv, G, rev) is two unitigs of random bytes, the second placed reversed when rev is set: no read holds their ends,
          so both walks are DEAD_END at their first step and the gap stays as laid.
  grow    Y ballast bases in front of the first unitig of the case's first scaffold, which must lie at offset 0: the unitig is
          that much longer, and the case's first gap has a left neighbour of more than Y bases.  For gapfill the unitig must be
          placed forward (its stored bytes begin with the ballast); grow_rev is the same for a unitig stored
          reverse-complemented and placed with SIGAX_PLACED_REV: the ballast lies BEHIND its stored bytes in useqs and comes
          out reverse-complemented in front (flip_first() turns a case into the other kind).

The shift rule.  With kb ballast unitigs, sb ballast scaffolds, Bu the ballast unitigs' bases, Bi and Bo the ballast scaffolds'
bases in the input and in the output, u0 the case's first placed unitig and ng the ballast gaps:
  input    unitig ids + kb; seq_offs + Bu, and + Y behind u0; sc_lay_offs + kb; sc_offs (join) + Bi, and + Y from entry 1 on;
           the offsets of the first scaffold's placements behind the first + Y; the bytes as the plans below say.
  output   sc_offs' + Bo, and + Y from entry 1 on; sc_lay_offs + kb; layout' ids + kb, the first scaffold's offsets behind the
           first placement + Y; records: scaffold + sb, left and right + kb, offset + Y in the first scaffold, numbered behind
           the ballast's.
  join     a ballast gap's record is (scaffold, u, u + 1, G, v, JOINED, 1, 0, lu - v); everything behind it moves down by G + v,
           so its scaffold has lu + lv - v bases.  status: 0 and 1 + ng; 9 + sum v; 10 + sum G; 11 + Bo + Y; 12 + the ballast
           gaps' hi - lo + 1, hi = min(max_overlap, lu - 1, lv - 1); 15 + sb.  grow: a first gap that comes to the match has
           hi = min(max_overlap, |L| - 1 + Y, |R| - 1), so status 12 rises by the difference; a candidate above the old hi compares
           ballast with R, and lift_join refuses a case in which the case's own bytes would let one match (L == R[v - |L| : v]),
           one whose first gap is SHORT only for its L, and one whose junction windows would reach into the ballast (|L| < k - 1).
  gapfill  a ballast gap's record is (scaffold, u, u + 1, G, 0, DEAD_END, DEAD_END, DEAD_END, 0, lu).  status: 0 + ng; 1 +
           DEAD_END + ng; 15 + sum G; 16 + Bo + Y; 17 + 2 ng (one step a walk), 18 = 8 x 17; 22 + sb.  The ballast gaps come
           first and take G + slack bytes of walk scratch each: max_walk_bases rises by that much.  grow needs |L| >= k.
Entry 14 (join) and 20 (gapfill) follow from the capacity.

Bytes are described, not held: a plan is a list of pieces
  ("rand", n)  n random ACGT of the ballast      ("N", n)           ("bytes", b)  the case's own
  ("same", at, n)  a copy of the n bytes at `at` of the same buffer (join's overlap)
and an expected output is a list of
  ("in", at, n)  the input's bytes [at, at + n)   ("inrc", at, n)  their reverse complement   ("N", n)   ("bytes", b)
materialise() and expected_bytes() turn both into bytes for small ballast."""
from tests import gapfill_cases as gc
from tests import join_cases as jc
from tests import unitig_cases as uc

REV = uc.PLACED_REV


def _cum(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def plan_bytes(plan):
    return sum(len(p[1]) if p[0] == "bytes" else p[-1] for p in plan)


def materialise(plan, rng):
    """a plan as bytes, the ballast drawn from rng (small ballast only)"""
    out = bytearray()
    for p in plan:
        if p[0] == "rand":
            out += bytes(rng.choice(b"ACGT") for _ in range(p[1]))
        elif p[0] == "N":
            out += b"N" * p[1]
        elif p[0] == "same":
            assert p[1] + p[2] <= len(out)
            out += out[p[1]:p[1] + p[2]]
        else:
            out += p[1]
    return bytes(out)


def expected_bytes(out_plan, inp):
    out = bytearray()
    for p in out_plan:
        if p[0] == "in":
            out += inp[p[1]:p[1] + p[2]]
        elif p[0] == "inrc":
            out += uc.revcomp(inp[p[1]:p[1] + p[2]])
        elif p[0] == "N":
            out += b"N" * p[1]
        else:
            out += p[1]
    return bytes(out)


def _tables(scaf):
    lay = [tuple(int(x) for x in p) for p in scaf["layout"]]
    return lay, [int(x) for x in scaf["sc_lay_offs"]], [int(x) for x in scaf["sc_flags"]]


def _grown_tables(so, lay, slo, Y):
    """Y bases more in the first placed unitig -> (u0, seq_offs, layout)"""
    assert len(slo) >= 2 and slo[0] == 0 and slo[1] >= 1 and lay[0][2] == 0, "grow: the first scaffold's first placement lies at offset 0"
    u0 = lay[0][0]
    assert all(p[0] != u0 for p in lay[1:]), "grow: the first unitig is placed once"
    so2 = [x + (Y if i > u0 else 0) for i, x in enumerate(so)]
    lay2 = [(u, fl, off + (Y if 0 < p < slo[1] else 0)) for p, (u, fl, off) in enumerate(lay)]
    return u0, so2, lay2


# ---- join ------------------------------------------------------------------------------------------------------------------------------
def lift_join(res, scaf, opts, front=(), grow=0):
    """-> dict(res: seq_offs; scaf: sc_offs, sc_lay_offs, sc_flags, layout, seqs_plan; opts; and what shifted_join needs)"""
    o = dict(jc.DEFAULT_OPTS, **(opts or {}))
    lo, mx, slack, k = o["min_overlap"], o["max_overlap"], o["slack"], o["k"]
    so = [int(x) for x in res["seq_offs"]]
    sco = [int(x) for x in scaf["sc_offs"]]
    lay, slo, flags = _tables(scaf)
    seqs = bytes(scaf["seqs"])
    assert len(sco) == len(slo) and slo[-1] == len(lay) and sco[-1] == len(seqs), "lift_join: tables as a scaffold call leaves them"
    dhi = 0
    if grow:
        u0, so2, lay2 = _grown_tables(so, lay, slo, grow)
        if slo[1] >= 2:  # the first gap: its L grows
            lenl, (u1, _, off1) = so[u0 + 1] - so[u0], lay[1]
            lenr = so[u1 + 1] - so[u1]
            G = off1 - lenl
            hi_old, hi_new = min(mx, lenl - 1, lenr - 1), min(mx, lenl + grow - 1, lenr - 1)
            if 0 < G <= slack and seqs[lenl:lenl + G] == b"N" * G:  # it comes to SHORT or to the match
                assert not (hi_old < lo <= hi_new), "grow: the first gap is SHORT for its L alone"
                if hi_old >= lo:
                    dhi = hi_new - hi_old
                    L, R = seqs[:lenl], seqs[off1:off1 + lenr]
                    assert not any(R[v - lenl:v] == L for v in range(hi_old + 1, hi_new + 1)), "grow: a new candidate could match"
                    assert lenl >= k - 1, "grow: the junction windows would reach into the ballast"
        so, lay = so2, lay2
        sco = [0] + [x + grow for x in sco[1:]]
    bl, bsc, bpl, blay, gaps, plan, at = [], [], [], [], [], [], 0
    for it in front:
        u = len(bl)
        if isinstance(it, int):
            bl.append(it)
            bsc.append(it)
            bpl.append(1)
            blay.append((u, 0, 0))
            plan.append(("rand", it))
            at += it
        else:
            lu, lv, v, G = it
            hi = min(mx, lu - 1, lv - 1)
            assert lo <= v <= hi and v >= k - 1 and 0 < G <= slack, "a ballast gap that is JOINED without read support"
            bl += [lu, lv]
            bsc.append(lu + G + lv)
            bpl.append(2)
            blay += [(u, 0, 0), (u + 1, 0, lu + G)]
            plan += [("rand", lu), ("N", G), ("same", at + lu - v, v), ("rand", lv - v)]
            gaps.append({"scaffold": len(bsc) - 1, "u": u, "lu": lu, "lv": lv, "v": v, "G": G, "cand": hi - lo + 1, "at": at})
            at += lu + G + lv
    kb, Bu, Bi = len(bl), sum(bl), sum(bsc)
    if grow:
        plan.append(("rand", grow))
    plan.append(("bytes", seqs))
    out = {"res": {"seq_offs": _cum(bl)[:-1] + [x + Bu for x in so]},
           "scaf": {"sc_offs": _cum(bsc)[:-1] + [x + Bi for x in sco], "sc_lay_offs": _cum(bpl)[:-1] + [x + kb for x in slo],
                    "sc_flags": [0] * len(bsc) + flags, "layout": blay + [(u + kb, fl, off) for u, fl, off in lay], "seqs_plan": plan},
           "opts": o, "front": list(front), "grow": grow, "dhi": dhi, "kb": kb, "sb": len(bsc), "gaps": gaps, "first": slo[1] if grow else 0, "bpl": bpl}
    assert plan_bytes(plan) == out["scaf"]["sc_offs"][-1]
    return out


def shifted_join(exp, lf, capacity=None):
    """join_cases.expected_join's dict of the small case (capacity: exactly enough) -> that of the lifted one; seqs_plan for the bytes"""
    Y, kb, sb, gaps = lf["grow"], lf["kb"], lf["sb"], lf["gaps"]
    first = lf["first"]  # the placements of the case's first scaffold, when it grows
    lay = [(u, fl, off + (Y if 0 < p < first else 0)) for p, (u, fl, off) in enumerate(exp["layout"])]
    sco = [exp["sc_offs"][0]] + [x + Y for x in exp["sc_offs"][1:]]
    joins = [j[:8] + (j[8] + (Y if j[0] == 0 else 0),) for j in exp["joins"]]
    # the ballast in front
    bsc, blay, brec, plan = [], [], [], []
    at, gi = 0, 0
    for it in lf["front"]:
        if isinstance(it, int):
            bsc.append(it)
            blay.append((len(blay), 0, 0))
            plan.append(("in", at, it))
            at += it
        else:
            g = gaps[gi]
            gi += 1
            lu, lv, v, G = it
            bsc.append(lu + lv - v)
            blay += [(g["u"], 0, 0), (g["u"] + 1, 0, lu - v)]
            brec.append((g["scaffold"], g["u"], g["u"] + 1, G, v, jc.C["JOINED"], 1, 0, lu - v))
            plan += [("in", at, lu), ("in", at + lu + G + v, lv - v)]
            at += lu + G + lv
    Bo = sum(bsc)
    if Y:
        plan.append(("in", at, Y))
    if exp["seqs"] is not None:
        plan.append(("bytes", exp["seqs"]))
    st = list(exp["status"])
    st[0] += len(gaps)
    st[1] += len(gaps)
    st[9] += sum(g["v"] for g in gaps)
    st[10] += sum(g["G"] for g in gaps)
    st[11] += Bo + Y
    st[12] += sum(g["cand"] for g in gaps) + lf["dhi"]
    st[14] = 1 if capacity is not None and st[11] > capacity else 0
    st[15] += sb
    return {"status": st, "sc_offs": _cum(bsc)[:-1] + [x + Bo for x in sco], "sc_lay_offs": _cum(lf["bpl"])[:-1] + [x + kb for x in exp["sc_lay_offs"]],
            "sc_flags": [0] * sb + list(exp["sc_flags"]), "layout": blay + [(u + kb, fl, off) for u, fl, off in lay],
            "joins": brec + [(j[0] + sb, j[1] + kb, j[2] + kb) + j[3:] for j in joins], "seqs_plan": plan, "case_at": Bo + Y}


# ---- gapfill ---------------------------------------------------------------------------------------------------------------------------
def flip_first(res, scaf):
    """the same case with the first placed unitig stored the other way round and its placement's strand turned: what it reads
    like as placed does not change"""
    so, useqs = [int(x) for x in res["seq_offs"]], bytes(res["useqs"])
    lay = [tuple(int(x) for x in p) for p in scaf["layout"]]
    u0, fl, off = lay[0]
    a, b = so[u0], so[u0 + 1]
    return (dict(res, useqs=useqs[:a] + uc.revcomp(useqs[a:b]) + useqs[b:]), dict(scaf, layout=[(u0, fl ^ REV, off)] + lay[1:]))


def lift_gapfill(res, scaf, opts, front=(), grow=0, grow_rev=0, max_walk_bases=None):
    """-> dict(res: seq_offs, useqs_plan; scaf: sc_lay_offs, sc_flags, layout; opts; max_walk_bases; and what shifted_gapfill
    needs)"""
    o = dict(gc.DEFAULT_OPTS, **(opts or {}))
    k, slack, max_fill = o["k"], o["slack"], o["max_fill"]
    so = [int(x) for x in res["seq_offs"]]
    useqs = bytes(res["useqs"])
    lay, slo, flags = _tables(scaf)
    assert so[-1] == len(useqs) and slo[-1] == len(lay) and not (grow and grow_rev)
    Y = grow or grow_rev
    case_plan, grow_at = [("bytes", useqs)], None
    if Y:
        u0, so2, lay2 = _grown_tables(so, lay, slo, Y)
        assert bool(lay[0][1] & REV) == bool(grow_rev), "grow: a first unitig placed forward; grow_rev: one placed reversed"
        assert so[u0 + 1] - so[u0] >= k, "grow: a first unitig that is SHORT"
        cut = so[u0 + 1] if grow_rev else so[u0]
        case_plan, grow_at = [("bytes", useqs[:cut]), ("rand", Y), ("bytes", useqs[cut:])], cut
        so, lay = so2, lay2
    bl, bsc, bpl, blay, gaps, plan = [], [], [], [], [], []
    for it in front:
        u = len(bl)
        if isinstance(it, int):
            bl.append(it)
            bsc.append(it)
            bpl.append(1)
            blay.append((u, 0, 0))
            plan.append(("rand", it))
        else:
            lu, lv, G, rev = it
            assert lu >= k and lv >= k and 0 < G <= max_fill
            gaps.append({"scaffold": len(bsc), "u": u, "lu": lu, "lv": lv, "G": G, "rev": bool(rev), "at": sum(bl)})
            bl += [lu, lv]
            bsc.append(lu + G + lv)
            bpl.append(2)
            blay += [(u, 0, 0), (u + 1, REV if rev else 0, lu + G)]
            plan += [("rand", lu), ("rand", lv)]
    kb, Bu = len(bl), sum(bl)
    mw = None if max_walk_bases is None else max_walk_bases + sum(g["G"] + slack for g in gaps)
    return {"res": {"seq_offs": _cum(bl)[:-1] + [x + Bu for x in so], "useqs_plan": plan + case_plan},
            "scaf": {"sc_lay_offs": _cum(bpl)[:-1] + [x + kb for x in slo], "sc_flags": [0] * len(bsc) + flags,
                     "layout": blay + [(u + kb, fl, off) for u, fl, off in lay]},
            "opts": o, "max_walk_bases": mw, "front": list(front), "grow": Y, "grow_rev": bool(grow_rev), "grow_at": None if grow_at is None else Bu + grow_at,
            "kb": kb, "sb": len(bsc), "gaps": gaps, "first": slo[1] if Y else 0, "bpl": bpl}


def shifted_gapfill(exp, lf, capacity=None):
    """gapfill_cases.expected_gapfill's dict of the small case (capacity: exactly enough; its max_walk_bases the one lift_gapfill
    was given) -> that of the lifted one; seqs_plan for the bytes, over the lifted useqs as the input"""
    Y, kb, sb, gaps, first = lf["grow"], lf["kb"], lf["sb"], lf["gaps"], lf["first"]
    DE = gc.C["DEAD_END"]
    lay = [(u, fl, off + (Y if 0 < p < first else 0)) for p, (u, fl, off) in enumerate(exp["layout"])]
    sco = [exp["sc_offs"][0]] + [x + Y for x in exp["sc_offs"][1:]]
    recs = [g[:9] + (g[9] + (Y if g[0] == 0 else 0),) for g in exp["gaps"]]
    bsc, blay, brec, plan = [], [], [], []
    at, gi = 0, 0
    for it in lf["front"]:
        if isinstance(it, int):
            bsc.append(it)
            blay.append((len(blay), 0, 0))
            plan.append(("in", at, it))
            at += it
        else:
            g = gaps[gi]
            gi += 1
            lu, lv, G, rev = it
            bsc.append(lu + G + lv)
            blay += [(g["u"], 0, 0), (g["u"] + 1, REV if rev else 0, lu + G)]
            brec.append((g["scaffold"], g["u"], g["u"] + 1, G, 0, DE, DE, DE, 0, lu))
            plan += [("in", at, lu), ("N", G), ("inrc" if rev else "in", at + lu, lv)]
            at += lu + lv
    Bo = sum(bsc)
    if Y:
        plan.append(("inrc" if lf["grow_rev"] else "in", lf["grow_at"], Y))
    if exp["seqs"] is not None:
        plan.append(("bytes", exp["seqs"]))
    st = list(exp["status"])
    ng = len(gaps)
    st[0] += ng
    st[1 + DE] += ng
    st[15] += sum(g["G"] for g in gaps)
    st[16] += Bo + Y
    st[17] += 2 * ng
    st[18] = 8 * st[17]
    st[20] = 1 if capacity is not None and st[16] > capacity else 0
    st[22] += sb
    return {"status": st, "sc_offs": _cum(bsc)[:-1] + [x + Bo for x in sco], "sc_lay_offs": _cum(lf["bpl"])[:-1] + [x + kb for x in exp["sc_lay_offs"]],
            "sc_flags": [0] * sb + list(exp["sc_flags"]), "layout": blay + [(u + kb, fl, off) for u, fl, off in lay],
            "gaps": brec + [(g[0] + sb, g[1] + kb, g[2] + kb) + g[3:] for g in recs], "seqs_plan": plan, "case_at": Bo + Y,
            "fills": {i + ng: f for i, f in exp["fills"].items()}}


# ---- the small cases both test files use ----------------------------------------------------------------------------------------------
def join_small(which):
    """"three": three_joins_in_a_row, k = 31; "random": the first random case with a fill (a CLOSED gap of non-N bytes), an
    UNSUPPORTED gap, slack for the ballast's gap and a max_overlap that holds the ballast's overlap of 1000"""
    if which == "three":
        return next(c for c in jc.hand_built(31) if c["kind"] == "three_joins_in_a_row")
    for seed in range(100):
        c = jc.random_case(seed)
        if c["opts"]["max_overlap"] < 1000 or c["opts"]["slack"] < 5 or c["opts"]["k"] > 64:
            continue
        exp = jc.case_expected(c)
        if exp["status"][1 + jc.C["UNSUPPORTED"]] and exp["status"][1] and any(
                j[5] == jc.C["CLOSED"] and 0 < j[3] <= c["opts"]["slack"] for j in exp["joins"]):
            return c
    raise AssertionError("no random case with a fill and an UNSUPPORTED gap")


def gapfill_small(flipped=None):
    """k = 31, four scaffolds: three gaps filled forward between pieces on both strands; a gap with a fork of min_count reads at
    its forward start, filled by the reverse walk alone; a gap over a hole in the reads, DEAD_END both ways; a unitig on its
    own.  flipped: None or False as it is (the first unitig placed forward), True with it stored the other way round and placed
    reversed"""
    k = 31
    n, a0 = 2 * k + 40, 200
    g = gc.genome(k, 1, 3000)
    reads = tuple(gc.tile(g, k, seed=k, drop=1612) + gc.fork_reads(g, k, 1000 + n, 3, seed=k))
    scaffolds = [[(a0, a0 + n, False, 30), (a0 + n + 25, a0 + 2 * n + 25, True, 9), (a0 + 2 * n + 36, a0 + 3 * n + 36, False, 60),
                  (a0 + 3 * n + 36 + 44, a0 + 4 * n + 36 + 44, True, None)],
                 [(1000, 1000 + n, False, 42), (1000 + n + 37, 1000 + 2 * n + 37, True, None)],
                 [(1500, 1500 + n, True, 20), (1500 + n + 23, 1500 + 2 * n + 23, False, None)],
                 [(2000, 2000 + n, True, None)]]
    c = gc.case("lifted", k, g, reads, scaffolds, seed=5)
    if flipped:
        res, scaf = flip_first(c["res"], c["scaf"])
        c = dict(c, res=res, scaf=scaf)
    return c
