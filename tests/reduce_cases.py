"""Cases and the serial restatement for the transitive reduction in the rounds of `siga unitig` (sigax_unitigs_reduce_*, the rules in
include/sigax.h); no tests here (tests/test_reduce_cases.py, tests/test_gpu_unitig_reduce.py).

expected_reduce()  the rules, serially: a pass (reduce_pass) before every round and once more before the final unitigs, and between the
                   passes one round of indel_cases.expected_indel at a time over what is there -- the alive reads and the records that
                   are neither cut nor flagged.  A round's removals and cuts are stamped with the round's number; reads and records
                   keep their order in every sub-call, so every tie on a smallest id falls as it does over the whole set.
reduce_pass()      the TRANSITIVE rule as written: for a participant a-b and either of its ends, every participant a-w to a third read
                   and every participant (w ^ 1)-b, the three extensions added up.  No table, no sorting, no shortcut on the lengths.
The reference has no such step (TransitiveReductionVisitor is empty); the yardstick from the reference is its irreducible overlap run:
oracle_sets() holds five read sets on which "exhaustive records, reduced" must be that run's records exactly.

A case: indel_cases' dict plus reduce (bool)."""
import functools
import random

import numpy as np

from tests import chimeric_cases as cc
from tests import indel_cases as ic
from tests import trim_cases as tc
from tests import unitig_cases as uc

B, E = uc.B, uc.E
TRANSITIVE = 0x80000000  # SIGAX_CUT_TRANSITIVE
ROUND_BITS = 0x1FFFFFFF  # removed[]: what is left beside the three flag bits
KEYS = ic.KEYS


# ---- the rules, serially ----
def participants(lens, edges, m, removed, cut):
    """[(index, state a, state b, overlap)] of a pass over the state (removed, cut)"""
    out = []
    for i, rec in enumerate(edges):
        c = uc.classify(rec, lens, m)
        if c in ("bad", "low"):
            continue
        a, b, contain, self_edge = c
        if contain or self_edge or (cut[i] & ~TRANSITIVE) or removed[a >> 1] or removed[b >> 1]:
            continue
        out.append((i, a, b, rec[2]))
    return out


def reduce_pass(lens, edges, m, removed, cut):
    """-> (the indices of the records that are transitive in this pass, the number of participants)"""
    part = participants(lens, edges, m, removed, cut)
    at, between = {}, {}  # state -> [(other state, ext towards it, record)]; (state, state) -> [overlap]
    for i, a, b, ln in part:
        at.setdefault(a, []).append((b, lens[b >> 1] - ln, i))
        at.setdefault(b, []).append((a, lens[a >> 1] - ln, i))
        between.setdefault((a, b), []).append(ln)
        between.setdefault((b, a), []).append(ln)
    flagged = set()
    for i, s, t, ln in part:
        for a, b in ((s, t), (t, s)):
            ext_ab = lens[b >> 1] - ln
            for w, ext_aw, j in at[a]:
                if j == i or w >> 1 in (a >> 1, b >> 1):
                    continue
                if any(ext_aw + (lens[b >> 1] - lk) == ext_ab for lk in between.get((w ^ 1, b), [])):
                    flagged.add(i)
    return flagged, len(part)


def expected_reduce(reads, edges, m, max_rounds, L, C=None, reduce=True, **kw):
    """-> indel_cases.expected_indel's dict with status [40]; cut carries TRANSITIVE on the records flagged in the final graph;
    first_flags: the records the first pass flagged; pass_flags: [(round, or 0 for the final pass, flagged records)] of the passes that ran.
    tables_only = True (among kw): as unitig_cases.expected's"""
    if not reduce:
        res = ic.expected_indel(reads, edges, m, max_rounds, L, C, **kw)
        res["status"] = res["status"] + [0] * 8
        res["first_flags"], res["pass_flags"] = set(), []
        return res
    n = len(reads)
    lens = [uc.nbases(r) for r in reads]
    kw = dict(kw)
    if kw.get("N") is None:
        kw["N"] = n
    kept, bad, low = tc._kept(edges, lens, m)
    removed, cut = [0] * n, [0] * len(edges)
    flagged, first_flags, pass_flags = set(), None, []
    acc = [0] * 32  # the counts of the rounds, summed where they are sums
    passes = last_part = 0

    def run_pass(rnd):
        nonlocal flagged, first_flags, passes, last_part
        flagged, last_part = reduce_pass(lens, edges, m, removed, cut)
        passes += 1
        pass_flags.append((rnd, set(flagged)))
        if first_flags is None:
            first_flags = set(flagged)

    def sub_problem():
        alive = [r for r in range(n) if not removed[r]]
        new = {r: k for k, r in enumerate(alive)}
        idx = [i for i, _ in kept if not cut[i] and i not in flagged and not removed[edges[i][0]] and not removed[edges[i][1]]]
        sub = [(new[edges[i][0]], new[edges[i][1]], edges[i][2], edges[i][3]) for i in idx]
        return alive, idx, [reads[r] for r in alive], sub

    rounds, changed = 0, True
    for rnd in range(1, max_rounds + 1):
        run_pass(rnd)  # (a round runs only when the one before changed something: its pass is never idle here)
        alive, idx, sub_reads, sub = sub_problem()
        one = ic.expected_indel(sub_reads, sub, m, 1, L, C, **kw)
        for k, x in enumerate(one["removed"]):
            if x:
                assert x & ROUND_BITS == 1
                removed[alive[k]] = (x & ~ROUND_BITS) | rnd
        for j, x in enumerate(one["cut"]):
            if x:
                cut[idx[j]] = rnd
        st = one["status"]
        for k in (7, 8, 13, 16, 17, 18, 20, 21, 22, 23, 24, 25, 26, 27, 28):
            acc[k] += st[k]
        if rnd == 1:
            acc[14] = st[14]
        changed = st[6] == 1
        if not changed:
            break
        rounds += 1
    if max_rounds == 0 or changed:  # the final pass is idle behind a round that changed nothing: the flags of the pass before hold
        run_pass(0)
    alive, idx, sub_reads, sub = sub_problem()
    res = ic.expected_indel(sub_reads, sub, m, 0, L, C, **kw)
    res["layout"] = [(alive[r], fl, off) for r, fl, off in res["layout"]]
    dropped = sum(1 for i, _ in kept if not cut[i] and i not in flagged and (removed[edges[i][0]] or removed[edges[i][1]]))
    st = res["status"]
    res["status"] = ([st[0], st[1], bad, low, st[4], st[5], rounds, acc[7], acc[8], sum(1 for x in removed if x), dropped, len(res["uedges"]),
                      sum(1 for x in cut if x), acc[13], acc[14], 0] + acc[16:32] +
                     [len(first_flags or ()), len(flagged), passes, last_part, 0, 0, 0, 0])
    res["removed"] = removed
    res["cut"] = [x | (TRANSITIVE if i in flagged else 0) for i, x in enumerate(cut)]
    res["first_flags"], res["pass_flags"] = first_flags or set(), pass_flags
    return res


def run(fn, case, max_rounds=None, **over):
    kw = {k: case[k] for k in KEYS}
    kw["reduce"] = case.get("reduce", True)
    kw.update(over)
    return fn(case["reads"], case["edges"], case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"], **kw)


def unit_of(res):
    """read -> the unitig it lies in"""
    out = {}
    for u in range(len(res["uflags"])):
        for p in res["layout"][int(res["lay_offs"][u]):int(res["lay_offs"][u + 1])]:
            out[int(p[0])] = u
    return out


# ---- reads on a line: every record a real overlap of the stored bytes ----
class _Line:
    def __init__(self, seed, m=20):
        self.rng = random.Random(seed)
        self.m, self.reads, self.edges = m, [], []
        self.pos, self.rc = [], []

    def genome(self, n):
        return bytes(self.rng.choice(b"ACGT") for _ in range(n))

    def place(self, g, spans, rc=None):
        """reads g[p:p + ln] for (p, ln) in spans, stored reverse-complemented where rc[i] -> their ids"""
        ids = []
        for k, (p, ln) in enumerate(spans):
            r = self.rng.random() < 0.5 if rc is None else rc[k]
            w = g[p:p + ln]
            assert len(w) == ln
            self.reads.append(uc.revcomp(w) if r else w)
            self.pos.append((p, ln))
            self.rc.append(r)
            ids.append(len(self.reads) - 1)
        return ids

    def record(self, x, y, ov=None, qfirst=None):
        """the record of x, which lies left of y on the line, and y; ov: the length it names (the true one unless given)"""
        (px, lx), (py, _) = self.pos[x], self.pos[y]
        ov = px + lx - py if ov is None else ov
        rx, ry = self.rc[x], self.rc[y]
        if self.rng.random() < 0.5 if qfirst is None else qfirst:
            q, t, af = x, y, (1 if rx else 0) | (2 if ry else 0)
        else:
            q, t, af = y, x, (0 if ry else 1) | (0 if rx else 2)
        self.edges.append((q, t, ov, af | (((af ^ (af >> 1)) & 1) << 2)))
        return len(self.edges) - 1

    def all_records(self, ids):
        """every pair of `ids` that overlaps by m or more without one containing the other"""
        out = []
        for x in ids:
            for y in ids:
                (px, lx), (py, ly) = self.pos[x], self.pos[y]
                if (px, x) < (py, y) and px + lx - py >= self.m and px + lx < py + ly and px < py:
                    out.append(self.record(x, y))
        return out

    def case(self, name, x=0, L=30, shuffle=True, **claims):
        order = list(range(len(self.edges)))
        if shuffle:
            self.rng.shuffle(order)  # records in any order
        where = {old: new for new, old in enumerate(order)}
        c = {"name": name, "reads": list(self.reads), "edges": [self.edges[i] for i in order], "m": self.m, "x": x, "L": L, "C": None,
             "delta": 0, "careful": False, "N": 1000, "G": 10000, "T": 10.0, "Lc": 0, "Ac": None, "delta_c": 0, "Tc": 3.0, "Lb": 0, "D": 50,
             "Ed": 0, "De": 50, "reduce": True, "claims": claims}
        for key in ("flagged", "first"):
            if key in claims:
                claims[key] = sorted(where[i] for i in claims[key])
        c["where"] = where
        return c


def _triple(seed, rc=None, qfirst=None):
    """A, B, C of 50 bases at 0, 15, 30: A-B 35, B-C 35, A-C 20 -> (line, ids, the index of the A-C record)"""
    ln = _Line(seed)
    ids = ln.place(ln.genome(80), [(0, 50), (15, 50), (30, 50)], rc)
    q = qfirst or [None] * 3
    ln.record(ids[0], ids[1], qfirst=q[0])
    ln.record(ids[1], ids[2], qfirst=q[1])
    return ln, ids, ln.record(ids[0], ids[2], qfirst=q[2])


@functools.lru_cache(maxsize=None)
def hand_built():
    """claims: flagged (the records with bit 31 in the final graph, by index), first (those of the first pass; = flagged unless given),
    unitigs (status[0]), rounds (status[6]), passes (status[34]), together (reads that lie in one unitig), apart (reads that do not)"""
    cases = []
    # triple: A -> B -> C and A -> C
    ln, ids, ac = _triple(1)
    cases.append(ln.case("triple", flagged=[ac], unitigs=1, passes=1, together=ids))
    # ... among malformed records and records below m: none of them is a participant, a witness or flagged
    ln, ids, ac = _triple(11)
    ln.edges += [(3, ids[0], 25, 0), (ids[0], 3, 25, 0), (0xFFFFFFFF, 0xFFFFFFFF, 25, 0), (ids[0], ids[1], 25, 1), (ids[0], ids[2], 20, 7),
                 (ids[0], ids[2], 0, 0), (ids[1], ids[2], 1000, 0), (ids[0], ids[2], 19, 0), (ids[0], ids[2], 20, 0x80000000)]
    cases.append(ln.case("triple_malformed", shuffle=False, flagged=[ac], unitigs=1, passes=1, together=ids))
    # the same three reads under all 8 strand flips, each with the records' query / target order as given and swapped
    k = 0
    for flips in range(8):
        rc = [bool(flips >> b & 1) for b in range(3)]
        for qf in (True, False):
            ln, ids, ac = _triple(1, rc, [qf, qf, qf])
            cases.append(ln.case("triple_strands_%d" % k, shuffle=False, flagged=[ac], unitigs=1, passes=1, together=ids))
            k += 1
    # fork: w and x both begin inside a and diverge; no record between them
    ln = _Line(2)
    g = ln.genome(50)
    a, = ln.place(g, [(0, 50)])
    w, = ln.place(g[20:] + ln.genome(25), [(0, 55)])
    x, = ln.place(g[25:] + ln.genome(30), [(0, 55)])
    ln.pos[w], ln.pos[x] = (20, 55), (25, 55)
    ln.record(a, w)
    ln.record(a, x)
    cases.append(ln.case("fork", flagged=[], unitigs=3, apart=[a, w, x]))
    # off_by_one: the B-C record names 36 bases where the sum asks for 35 (the same two reads at another offset, as inside a repeat)
    for name, ov, hit in (("off_by_one", 36, False), ("off_by_one_short", 34, False), ("off_by_none", 35, True)):
        ln = _Line(3)
        ids = ln.place(ln.genome(80), [(0, 50), (15, 50), (30, 50)])
        ln.record(ids[0], ids[1])
        ln.record(ids[1], ids[2], ov=ov)
        ac = ln.record(ids[0], ids[2])
        cases.append(ln.case(name, flagged=[ac] if hit else [], unitigs=1 if hit else 3))
    # parallel: A-C twice, at 20 (explained by B) and at 23 (by nothing)
    ln, ids, ac = _triple(4)
    ln.record(ids[0], ids[2], ov=23)
    cases.append(ln.case("parallel", flagged=[ac], unitigs=3))
    ln, ids, ac = _triple(4)
    twice = ln.record(ids[0], ids[2])  # ... and the same record twice: both explained
    cases.append(ln.case("parallel_same", flagged=[ac, twice], unitigs=1))
    # special_witness: the read between A and C is contained in A, so its record with A is a containment: no witness, and never flagged
    ln = _Line(5)
    g = ln.genome(80)
    a, c = ln.place(g, [(0, 50), (30, 50)])
    w, = ln.place(g, [(15, 35)])
    aw = ln.record(a, w)  # 35 bases, all of w: were it a witness, 0 + ext(w -> c) = 30 = ext(a -> c) would flag a-c
    assert ln.edges[aw][2] == len(ln.reads[w])
    ln.record(w, c)
    ln.record(a, c)
    cases.append(ln.case("special_witness_containment", flagged=[]))
    # ... and where B's place is taken by self edges of B and of C
    ln, ids, ac = _triple(6, rc=[False, False, False])
    ln.edges[1] = (ids[1], ids[1], 35, 0)  # B.E - B.B in place of B-C
    ln.edges.append((ids[2], ids[2], 35, 6))  # C.B - C.B
    cases.append(ln.case("special_witness_self", flagged=[]))
    # dead_witness_cut: A-B is cut by -d in round 1 (A-D at the same end of A is 10 bases longer; the records D-B and D-C are left
    # out), so from round 2 on nothing explains A-C
    ln = _Line(7)
    ids = ln.place(ln.genome(90), [(0, 50), (15, 50), (30, 50), (5, 60)])
    ab = ln.record(ids[0], ids[1])
    ln.record(ids[1], ids[2])
    ac = ln.record(ids[0], ids[2])
    ad = ln.record(ids[0], ids[3])
    assert ln.edges[ad][2] == 45 and ln.edges[ab][2] == 35
    c = ln.case("dead_witness_cut", x=10, shuffle=False, first=[ac], flagged=[])
    c.update(delta=10, G=1000)  # (one read of 50 bases scores as unique in a genome of 1000)
    c["claims"]["cut_in_1"] = [ab]
    cases.append(c)
    # chain5: five reads of 60 every 10 bases, all ten overlaps: the six that are not between neighbours are flagged
    ln = _Line(8)
    ids = ln.place(ln.genome(100), [(10 * k, 60) for k in range(5)])
    recs = ln.all_records(ids)
    assert len(recs) == 10
    far = [i for i in recs if abs(ln.edges[i][0] - ln.edges[i][1]) > 1]
    cases.append(ln.case("chain5", flagged=far, unitigs=1, passes=1, together=ids))
    # revive (and dead_witness_read: the witness read is not alive): a0 a1 a2 A B C c1 c2 c3 on one line, A-C explained by B alone; A's
    # E end and C's B end are branched by two bridges of 60 bases to other chains, Y and Z.  Round 1 flags A-C; its chimeric step takes B
    # (50 bases: Y and Z are longer) and Y and Z (through their hubs).  Round 2's pass finds A-C alone at both its ends.
    cases.append(_revive(True))
    cases.append(_revive(False))
    # wide_end: 300 participants at one read end (synthetic records over reads of 100 random bases)
    cases.append(_wide_end())
    for want in (0, 1, 63, 64, 65, 255, 256, 257):
        cases.append(sized_case(want))
    return cases


def _revive(with_ac):
    ln = _Line(9)
    lens = [60, 60, 60, 60, 50, 60, 60, 60, 60]
    ovs = [22, 22, 22, 40, 40, 22, 22, 22]
    pos = [0]
    for k in range(8):
        pos.append(pos[-1] + lens[k] - ovs[k])
    ids = ln.place(ln.genome(pos[-1] + 60), list(zip(pos, lens)))
    for k in range(8):
        ln.record(ids[k], ids[k + 1])
    a, b, c = ids[3], ids[4], ids[5]
    ac = ln.record(a, c)
    assert ln.edges[ac][2] == 30
    hubs = []
    for _ in range(2):  # two chains of four reads of 60 over 22
        p = [0, 38, 76, 114]
        h = ln.place(ln.genome(174), [(q, 60) for q in p])
        for k in range(3):
            ln.record(h[k], h[k + 1])
        hubs.append(h)
    case = ln.case("revive" if with_ac else "revive_irreducible", x=10, shuffle=False, **(dict(first=[ac], flagged=[]) if with_ac else {}))
    if not with_ac:  # the same reads and records without A-C: what an irreducible overlap run gives
        del case["edges"][ac]
    rng = random.Random(90)
    end = lambda r, e: 2 * r + (e ^ int(ln.rc[r]))  # noqa: E731
    y = cc.plant(case, rng, end(a, E), end(hubs[0][2], B), o1=25, o2=25, mid=10)
    z = cc.plant(case, rng, end(hubs[1][1], E), end(c, B), o1=25, o2=25, mid=10)
    case.update(Lc=60, reduce=with_ac)
    cl = case["claims"]
    cl.update(chimeric={b: 1, y: 1, z: 1}, rounds=1, abc=(a, b, c))
    if with_ac:
        cl.update(together=[a, c], passes=2, ac=ac)
    else:
        cl.update(apart=[a, c])
    return case


def _wide_end():
    rng = random.Random(10)
    reads = [bytes(rng.choice(b"ACGT") for _ in range(100)) for _ in range(301)]
    d = [0] + [rng.randint(1, 80) for _ in range(300)]  # where read i begins behind read 0, the hub
    edges = [(0, i, 100 - d[i], 0) for i in range(1, 301)]
    for _ in range(900):
        i, j = rng.randrange(1, 301), rng.randrange(1, 301)
        if d[i] < d[j]:
            edges.append((i, j, 100 - (d[j] - d[i]) - (1 if rng.random() < 0.2 else 0), 0))
    rng.shuffle(edges)
    return {"name": "wide_end", "reads": reads, "edges": edges, "m": 20, "x": 0, "L": 30, "C": None, "delta": 0, "careful": False, "N": 1000,
            "G": 10000, "T": 10.0, "Lc": 0, "Ac": None, "delta_c": 0, "Tc": 3.0, "Lb": 0, "D": 50, "Ed": 0, "De": 50, "reduce": True,
            "claims": {"hub_degree": 300}}


@functools.lru_cache(maxsize=None)
def every_step():
    """-> (case, expected_reduce's dict of it): one graph of a few dozen reads in which, in one call, every step of the rounds takes
    something -- a transitive triple, a fork whose shorter overlap the cut step takes, a tip, a bubble apart by a substitution, one
    apart by a deleted base and a bridge between two chains.  That each step does is asserted here, on the restatement's own output."""
    g = tc._Grow(77)
    abc = g.chain(3, lens=[50] * 3, ovs=[35] * 2)
    g._record(abc[0], abc[2], 20)  # A's last 20 bases begin C
    f = g.start(60)  # the fork: 45 bases against 33 at one end
    g.grow(f, 1, lens=[60], ovs=[45])
    g.grow(f, 1, lens=[60], ovs=[33])
    chains = [g.chain(4, lens=[60] * 4, ovs=[22] * 3) for _ in range(7)]
    case = ic._case(g, "every_step", x=10, L=45, Lb=40, D=50, Lc=60, Ed=2, De=1000)
    case.update(delta=10, G=1000, reduce=True)
    rng = random.Random(78)
    end = lambda r, e: cc._end(g, r, e)  # noqa: E731
    cc.plant(case, rng, end(chains[0][1], E), o1=22, mid=18)  # a tip of 40 bases
    mid = ic.bases(rng, 30)
    for edit, (a, c) in ((ic.mutate(rng, mid, (4,)), chains[1:3]), (ic.delete(mid, 7), chains[3:5])):
        ic.plant_arm(case, rng, end(a[3], E), end(c[0], B), mid)
        ic.plant_arm(case, rng, end(a[3], E), end(c[0], B), edit, flip=True)
    cc.plant(case, rng, end(chains[5][1], E), end(chains[6][2], B), o1=25, o2=25, mid=10)  # a bridge of 60 bases
    exp = run(expected_reduce, case)
    marks = [x & ~ROUND_BITS for x in exp["removed"] if x]
    assert all(marks.count(bit) >= 1 for bit in (0, ic.CHIMERIC, ic.BUBBLE, ic.INDEL)), marks
    assert any(x & ~TRANSITIVE for x in exp["cut"]) and any(x & TRANSITIVE for x in exp["cut"]) and exp["first_flags"]
    st = exp["status"]
    assert st[8] >= 1 and st[12] >= 1 and st[16] >= 1 and st[20] >= 1 and st[24] >= 1 and st[33] >= 1, st
    return case, exp


def random_case(seed, want=None):
    """reads of 40 to 60 bases at random places of a random genome, either strand, and every overlap of 20 or more between them that is
    no containment; want: exactly that many records (the first `want` of a shuffle; every one of them is a participant)"""
    ln = _Line(700 + seed)
    n = 24 + (want or 0) // 2
    g = ln.genome(12 * n + 60)
    spans = []
    while len(spans) < n:
        p, k = ln.rng.randrange(len(g) - 60), ln.rng.randint(40, 60)
        if not any(q <= p and p + k <= q + j or p <= q and q + j <= p + k for q, j in spans):
            spans.append((p, k))
    ids = ln.place(g, spans)
    ln.all_records(ids)
    ln.rng.shuffle(ln.edges)
    if want is not None:
        assert len(ln.edges) >= want, (len(ln.edges), want)
        del ln.edges[want:]
    return ln.case("reduce_random%d" % seed if want is None else "participants_%d" % want, x=ln.rng.choice((0, 0, 3)), L=30)


def sized_case(want):
    return random_case(want, want)


def case_named(name):
    return next(c for c in hand_built() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected_of(name, max_rounds=None):
    return run(expected_reduce, case_named(name), max_rounds)


# ---- five read sets whose exhaustive and irreducible records come from the CPU oracle ----
ORACLE_SETS = (  # name, seed, genome, read length (or a range), reads drawn, m, planted repeat
    ("g6000_600", 11, 6000, 60, 600, 25, 0),
    ("g6000_1500", 12, 6000, 60, 1500, 25, 0),
    ("g6000_1500_repeat200", 13, 6000, 60, 1500, 25, 200),
    ("g3000_1500_repeat80", 14, 3000, 100, 1500, 30, 80),
    ("g6000_40to60", 15, 6000, (40, 60), 700, 25, 0),
)


def _oracle_reads(seed, glen, rlen, n, repeat):
    rng = random.Random(seed)
    g = bytearray(rng.choice(b"ACGT") for _ in range(glen))
    if repeat:  # one stretch copied forward and once more reverse-complemented
        src = bytes(g[500:500 + repeat])
        g[glen // 2:glen // 2 + repeat] = src
        g[glen - 700:glen - 700 + repeat] = uc.revcomp(src)
    g = bytes(g)
    reads, seen = [], set()
    while len(reads) < n:
        k = rlen if isinstance(rlen, int) else rng.randint(*rlen)
        p = rng.randrange(glen - k + 1)
        w = g[p:p + k]
        w = uc.revcomp(w) if rng.random() < 0.5 else w
        if w in seen or uc.revcomp(w) in seen:  # no duplicate, on either strand
            continue
        seen.add(w)
        reads.append(w)
    if not isinstance(rlen, int):  # no read that lies inside another, on either strand
        reads = [r for r in reads if not any(o is not r and (r in o or uc.revcomp(r) in o) for o in reads)]
    return reads


@functools.lru_cache(maxsize=None)
def oracle_sets():
    """-> [dict(name, reads, m, exhaustive, irreducible)]: the two record lists [(query, target, length, af)] of oracle/pyoracle.py's
    overlap run over the reads, in the order the run gives them"""
    from oracle import pyoracle as po
    from siga_amd.overlap import name_ranks
    from tests.bigcheck import expected_edges
    out = []
    for name, seed, glen, rlen, n, m, repeat in ORACLE_SETS:
        reads = _oracle_reads(seed, glen, rlen, n, repeat)
        seqs = [r.decode() for r in reads]
        names = ["r%d" % i for i in range(len(reads))]
        fwd, rev = po.Index.build(seqs), po.Index.build(seqs, reverse=True)
        lengths = np.array([len(r) for r in reads], dtype=np.uint32)
        recs = {}
        for irreducible in (False, True):
            got = po.overlap_batch(fwd, rev, seqs, m, irreducible=irreducible)
            e = expected_edges(got["blocks"], got["block_offs"], fwd.sai(), rev.sai(), lengths, np.asarray(name_ranks(names)))
            recs[irreducible] = [tuple(int(x) for x in rec) for rec in e.tolist()]
        out.append({"name": name, "reads": reads, "m": m, "exhaustive": recs[False], "irreducible": recs[True]})
    return out


def record_key(rec):
    """a record as the unordered pair of the read ends it joins, with its length: the same overlap written from either read is one key"""
    q, t, ln, af = rec
    a, b = 2 * q + (B if af & 1 else E), 2 * t + (E if af & 2 else B)
    return (min(a, b), max(a, b), ln)
