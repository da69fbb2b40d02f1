"""Cases that put the later steps of the unitig rounds -- cut (-d), chimeric (-l), bubble (-b), indel (--bubble-edits), reduce
(--reduce) -- beyond 2^32 bases and at the limits of their u32 options.  No tests here (tests/test_giant_cases.py holds the claims on
the CPU, tests/test_gpu_unitig_rounds_wide.py runs the cases on the device).  The reference is always the serial restatement of the
step, in its tables-only mode (unitig_cases.expected): reads that no step looks into are given as bare lengths.

(a) behind()     a hand-built case of the step's own module behind ballast reads (ballast_cases.Ballast) given as lengths.
(b) giant_*      unitigs of 2^32 + 101 bases that take part in a decision: a joined chain of three reads (2^31 + 40, 2^31 + 45, 70 over
                 33 and 21), small reads of real bytes attached to its outer ends -- the B end of its first read, the E end of its
                 third -- by synthetic records (no kernel compares a record with the bytes).  truncated() is the same case with the
                 giant's bases & 0xFFFFFFFF = 101: a decision that differs there is one a dropped high word would change.
(c) *_no_wrap    option values near 2^32 on small graphs: a sum or a product that differs between u64 and u32.

A case: reduce_cases' dict (every key of the five steps; full() fills in the neutral values), plus `step`, the entry it runs through,
`watch`, the one decision it was built for -- ("cut", record), ("removed", read) -> decision() -- and `want`, what that decision is.
Every score any of these cases evaluates lies at least MARGIN from its threshold: restate() asserts it."""
import functools
import random

from tests import ballast_cases as blc
from tests import bubble_cases as bc
from tests import chimeric_cases as cc
from tests import indel_cases as ic
from tests import prune_cases as pc
from tests import reduce_cases as rc
from tests import trim_cases as tc
from tests import unitig_cases as uc

B, E = uc.B, uc.E
G30, G31, G32 = 1 << 30, 1 << 31, 1 << 32
U32 = 0xFFFFFFFF
MARGIN = 1.0
# tests/test_gpu_unitig_wide.py's shapes a and c: 2^32 - 37 bases (the case's first read straddles 2^32) and 2^32 + 2^31 + 1 bases
# (everything of the case beyond 2^32, odd-aligned)
SHAPES = {"a": [G30 + 5, G30 - 9, G30 + 3, G30 - 36], "c": [G31 + 1, G31 - 6, G31 + 6]}
GIANT = (G31 + 40, G31 + 45, 70, 33, 21)  # test_gpu_unitig_wide.py's shape d
GIANT_BASES = G32 + 101
LOW = (40, 45, 70, 33, 21)  # the same chain without bit 31 of its lengths: 101 bases, GIANT_BASES & 0xFFFFFFFF
assert sum(GIANT[:3]) - 54 == GIANT_BASES and sum(LOW[:3]) - 54 == GIANT_BASES & U32

NEUTRAL = dict(C=None, delta=0, careful=False, N=None, G=None, T=13.0, Lc=0, Ac=None, delta_c=0, Tc=0.0, Lb=0, D=50, Ed=0, De=50, reduce=False)
# step -> (the module of its cases and restatement, the restatement, the words of its status)
STEPS = {"trim": (tc, tc.expected_trim, 12), "cut": (pc, pc.expected_prune, 16), "chimeric": (cc, cc.expected_chimeric, 20),
         "bubble": (bc, bc.expected_bubble, 24), "indel": (ic, ic.expected_indel, 32), "reduce": (rc, rc.expected_reduce, 40)}
TABLES = ("status", "seq_offs", "lay_offs", "uflags", "layout", "removed", "cut", "uedges")


def full(case):
    c = dict(NEUTRAL)
    c.update(case)
    return c


def restate(step, case, margin=None, **over):
    """the step's restatement over the case, tables only; margin: every score evaluated lies that far from its threshold"""
    mod, fn, words = STEPS[step]
    pc.SCORES = cc.SCORES = []
    try:
        if step == "trim":
            res = fn(case["reads"], case["edges"], case["m"], case["x"], case["L"], case["C"], tables_only=True)
        else:
            res = mod.run(fn, case, tables_only=True, **over)
        scores = list(pc.SCORES)
    finally:
        pc.SCORES = cc.SCORES = None
    assert len(res["status"]) == words and res["useqs"] is None
    if margin is not None:
        near = [(s, t) for s, t in scores if abs(s - t) < margin]
        assert not near, "%s: scores %r within %r of their thresholds" % (case["name"], near, margin)
    return res


# ---- (a) behind ballast ----
BEHIND_NAMES = {
    "bubble": ["two_arms", "mismatch_last_flipped", "loser_flipped", "winner_flipped", "at_divergence", "above_divergence", "n_in_reversed",
               "chains_all_flipped", "entered_right", "second_round"],
    "indel": ["deleted_flipped", "span_4096_winner", "e31_ed31", "e31_ed32", "at_permille", "above_permille", "span_4096_loser", "entered_111",
              "arms130", "second_round"],
    "cut": ["fork", "parallel_careful", "hub300"],
    "chimeric": ["bridge_flipped", "good_by_reads", "second_round"],
    "reduce": ["revive", "chain5", "wide_end"],
}
# every case behind shape a, the first two of every step also behind shape c
BEHIND = [(step, name, shape) for step, names in BEHIND_NAMES.items() for k, name in enumerate(names) for shape in ("a", "c")[:2 if k < 2 else 1]]


@functools.lru_cache(maxsize=None)
def behind(step, name, shape):
    """-> (the case behind the ballast, its reads lengths; the Ballast; the restatement's tables over it; the small case's result)"""
    mod = STEPS[step][0]
    case = full(mod.case_named(name))
    assert case["N"] is not None, "behind ballast N would default to another read count"
    bal = blc.Ballast(SHAPES[shape])
    assert all(b > max(case["L"], case["Lc"]) for b, _ in bal.units), "ballast that a step removes"
    big = dict(case, name="%s %s behind %s" % (step, name, shape), reads=list(bal.lens) + list(case["reads"]), edges=blc.concat_tables(case, bal)[0])
    return big, bal, restate(step, big), mod.expected_of(name)


# ---- (b) giant unitigs that take part ----
def _assemble(name, step, n_giants, small_reads, small_edges, synthetic, seed, **keys):
    """giants first (ids 0 .. 3 n_giants - 1, given as lengths), then the small reads; synthetic: records in the final ids"""
    bal = blc.Ballast([GIANT] * n_giants)
    k = bal.k
    edges = list(bal.edges) + [(q + k, t + k, ln, af) for q, t, ln, af in small_edges] + list(synthetic)
    random.Random(seed).shuffle(edges)  # records in any order
    # third: where the first giant's third read is placed in the final layout, unless a case says otherwise: 2^32 + 31 into its unitig
    return full(dict(name=name, step=step, reads=list(bal.lens) + list(small_reads), edges=edges, m=20, giants=n_giants,
                     third=(2, 0, G32 + 31), **keys))


def giant_left(i):
    return 2 * (3 * i) + B


def giant_right(i):
    return 2 * (3 * i + 2) + E


def truncated(case):
    """the case with every giant's bases & 0xFFFFFFFF: what a unitig's low word alone says"""
    reads = list(case["reads"])
    for i in range(case["giants"]):
        assert tuple(reads[3 * i:3 * i + 3]) == GIANT[:3]
        reads[3 * i:3 * i + 3] = LOW[:3]
    return dict(case, reads=reads, name=case["name"] + ", low word")


def decision(case, res):
    kind, what = case["watch"]
    return bool(res["cut"][what] if kind == "cut" else res["removed"][what])


def _small_end(g, k, read, w_end):
    """the state, in the final ids, of a _Grow read's end named in the shared orientation"""
    return 2 * (read + k) + (w_end ^ int(g.rc[read]))


def _between(s, t, ln, rng):
    return cc._record(rng, s >> 1, s & 1, t >> 1, t & 1, ln)


# N, G, T, and whether a unitig of GIANT_BASES is unique under them.  The scores for b = 2^32 + 101 and for b & 0xFFFFFFFF = 101:
#   beyond_genome     b >= G: not unique                                    -2.079 >= -5: unique
#   third_of_genome   693143.02 >= 13: unique                               -2.072: not unique
#   over_half_genome  28308.05 (b < G <= 2 b, the log(0.001) branch)        -2.079: not unique
GENOMES = {"beyond_genome": (1000, G32 + 50, -5.0, False), "third_of_genome": (10 ** 6, 3 * GIANT_BASES, 13.0, True),
           "over_half_genome": (1000, G32 + G31, 13.0, True)}
GIANT_SCORE = 693143.02  # third_of_genome's


def _giant_fork(name, genome, left=False, careful=False):
    """prune_cases' fork at a giant's end: w (three reads) over 40 and lo (two reads of 50, 78 bases) over 25, delta = 10; lo's far
    end forks again.  The record over 25 is cut iff the giant scores as unique.  careful: lo's near end also carries a record over
    45 to a further read, so that the record is non-maximal at both its ends and careful mode does not hold it back"""
    N, G, T, unique = GENOMES[genome]
    g = tc._Grow(9100 + len(name))
    w = g.chain(3, lens=[60] * 3, ovs=[22, 22])
    lo = g.chain(2, lens=[50, 50], ovs=[22])
    g.grow(lo[1], 3, lens=[60] * 3, ovs=[22, 22, 22])
    g.grow(lo[1], 3, lens=[60] * 3, ovs=[24, 22, 22])
    if careful:
        g.grow(lo[0], 1, side=B, lens=[70], ovs=[45])
    small = g.case(name, 10, 30 if careful else 100)
    rng = random.Random(9200 + len(name))
    end = giant_left(0) if left else giant_right(0)
    syn = [_between(end, _small_end(g, 3, w[0], B), 40, rng), _between(end, _small_end(g, 3, lo[0], B), 25, rng)]
    case = _assemble(name, "reduce", 1, small["reads"], small["edges"], syn, 1, x=10, L=small["L"], delta=10, careful=careful, N=N, G=G, T=T)
    case["watch"], case["want"] = ("cut", pc.rec_between(case, end >> 1, lo[0] + 3)), unique
    if left and unique:  # w merges at the giant's left end: the unitig begins at the giant's third read, the smaller id of its two ends
        case["third"] = (2, uc.PLACED_REV, 0)
    return case


def _giant_other(name, delta_c, want):
    """chimeric_cases' bridge_simple, where the bridge is merged away because p and q have degree 1 -- with a giant's two outer ends
    attached at p and at q.  Now both have degree 2 and the only other unitig at either is the giant: 3 reads, never more than K + 3,
    so good() holds by bases alone: min(bases(giant), 2^32 - 1) > 60 + delta_c"""
    g, a, c, p, q = cc._two_chains(4, at_a=3, at_c=0)
    small = cc._case(g, name)
    x = cc.plant(small, random.Random(9300), p, q)
    assert len(small["reads"][x]) == 60
    rng = random.Random(9301)
    syn = [_between(giant_left(0), p + 6, 30, rng), _between(giant_right(0), q + 6, 30, rng)]
    case = _assemble(name, "reduce", 1, small["reads"], small["edges"], syn, 2, x=10, L=30, N=1000, G=10000, T=10.0, Lc=60, delta_c=delta_c, Tc=3.0)
    case["watch"], case["want"] = ("removed", x + 3), want
    if want:  # a + giant + c are one unitig: the giant begins where a's 174 bases end, less the record's 30
        case["third"] = (2, 0, 174 - 30 + G32 + 31)
    return case


def _giant_neighbour(name, Tc, want):
    """a bridge of 60 bases from a giant's right end p to the middle of a chain c.  The other unitig at p is a chain d of 98 bases:
    longer than the bridge.  U(q), two reads, is not unique under third_of_genome's N and G (score -1.39), so the giant's score decides"""
    N, G, _, _ = GENOMES["third_of_genome"]
    g = tc._Grow(9400)
    c = g.chain(4, lens=[60] * 4, ovs=[22] * 3)
    d = g.chain(2, lens=[60, 60], ovs=[22])
    small = cc._case(g, name)
    x = cc.plant(small, random.Random(9401), cc._end(g, c[2], B), o1=25, mid=35)  # its B end at q; its E end is free
    rng = random.Random(9402)
    p = giant_right(0)
    syn = [_between(p, 2 * (x + 3) + E, 25, rng), _between(p, _small_end(g, 3, d[0], B), 30, rng)]
    case = _assemble(name, "reduce", 1, small["reads"], small["edges"], syn, 3, x=10, L=30, N=N, G=G, T=13.0, Lc=60, Tc=Tc)
    case["watch"], case["want"] = ("removed", x + 3), want
    return case


def _giant_tip():
    """a ring of four reads; one of its read ends carries the ring's own record, a tip of 40 bases and a giant's left end.  The giant's
    right end is free: a dead end.  -x 1 with L = 2^32 - 1: the tip goes, the giant has more than L bases and stays"""
    g = tc._Grow(9500)
    ring = g.ring(4)
    tip = g.grow(ring[1], 1, lens=[40])
    small = g.case("giant_tip", 1, U32)
    syn = [_between(giant_left(0), _small_end(g, 3, ring[1], E), 25, random.Random(9501))]
    case = _assemble("giant_tip", "reduce", 1, small["reads"], small["edges"], syn, 4, x=1, L=U32, N=1000, G=10000)
    case["watch"], case["want"], case["tip"] = ("removed", 0), False, tip[0] + 3
    return case


def _giant_indel():
    """indel_cases' at_permille: two arms of one read each, 1001 and 1000 bases, one deleted base, De = 1 -- between the right end
    of one giant and the left end of another.  The per-mille test takes the arms' own bases, never the neighbours'"""
    src = ic.case_named("at_permille")
    w, x = src["claims"]["kept_ids"][0], next(iter(src["claims"]["flagged"]))
    arms = [src["reads"][w], src["reads"][x]]
    assert (w, x) == (6, 7) and [len(r) for r in arms] == [1001, 1000]
    rng = random.Random(9600)
    syn = []
    for arm in (6, 7):  # (the small case plants both arms forward: B end at p, E end at q)
        syn += [_between(giant_right(0), 2 * arm + B, 25, rng), _between(2 * arm + E, giant_left(1), 25, rng)]
    keys = {k: src[k] for k in ic.KEYS}
    case = _assemble("giant_indel_permille", "indel", 2, arms, [], syn, 5, x=src["x"], L=src["L"], C=src["C"], **keys)
    case["watch"], case["want"], case["small"] = ("removed", 7), True, "at_permille"
    return case


@functools.lru_cache(maxsize=None)
def giants():
    cases = [_giant_fork("giant_fork_" + v, v) for v in GENOMES]
    cases.append(_giant_fork("giant_fork_left", "third_of_genome", left=True))
    cases.append(_giant_fork("giant_fork_careful", "third_of_genome", careful=True))
    cases.append(_giant_other("giant_other", 50, True))  # (with the low word: 101 > 60 + 50 fails)
    # bases + delta_c = 2^32 - 1: the clamp says "not longer", although the giant is; and one less
    cases.append(_giant_other("giant_other_saturated", U32 - 60, False))
    cases.append(_giant_other("giant_other_below_saturation", U32 - 61, True))
    cases.append(_giant_neighbour("giant_neighbour_unique", 3.0, True))
    cases.append(_giant_neighbour("giant_neighbour_not_unique", GIANT_SCORE + 8.0, False))
    cases.append(_giant_tip())
    cases.append(_giant_indel())
    return cases


# the cases whose decision must differ under truncated(): the clamp's two (the low word, 101, is below 2^32 - 1 either way) and the
# indel pair (its test never takes the giants' bases) are exempt, and so is the raised Tc, which no score of either length reaches
LOW_WORD_DIFFERS = ("giant_fork_beyond_genome", "giant_fork_third_of_genome", "giant_fork_over_half_genome", "giant_fork_left",
                    "giant_fork_careful", "giant_other", "giant_neighbour_unique", "giant_tip")


def giant_named(name):
    return next(c for c in giants() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def giant_expected(name, reduce=None):
    """the restatement over a (b) case; reduce: through the reduce restatement with reduce = 0 or 1"""
    case = giant_named(name)
    if reduce is None:
        return restate(case["step"], case, MARGIN)
    return restate("reduce", dict(case, reduce=bool(reduce)), MARGIN)


# ---- (c) option values near 2^32 on small graphs ----
def _bridge_case(name, lens_a, lens_c, **kw):
    g = tc._Grow(9700)
    a = g.chain(4, lens=lens_a, ovs=[22] * 3)
    c = g.chain(4, lens=lens_c, ovs=[22] * 3)
    case = cc._case(g, name, **kw)
    return case, cc._end(g, a[1], E), cc._end(g, c[2], B)


@functools.lru_cache(maxsize=None)
def no_wrap():
    """-> the cases; each names its expression as expr(wrap) -> the decision with the expression taken in u64 or wrapped to 32 bits"""
    cases = []
    # delta_c_no_wrap: bases(U) + delta_c = 60 + (2^32 - 30) = 2^32 + 30 in u64, 30 wrapped to 32 bits; the others at p and at q have
    # 100 bases and two reads: not longer than 2^32 + 30 (longer than 30), and not more than K + 3 reads: not chimeric
    case, p, q = _bridge_case("delta_c_no_wrap", [60, 60, 61, 61], [61, 61, 60, 60], delta_c=G32 - 30)
    x = cc.plant(case, random.Random(9701), p, q)
    assert len(case["reads"][x]) == 60
    case.update(step="chimeric", watch=("removed", x), want=False, expr=lambda wrap: 100 > ((60 + G32 - 30) & U32 if wrap else 60 + G32 - 30))
    cases.append(case)
    # chim_size_no_wrap: a bridge of K = 3 reads and 128 bases under Lc = 2^31 + 7.  (K - 1) * Lc = 2^32 + 14 in u64, 14 wrapped;
    # (Ac - 1) * bases = 2^26 * 128 = 2^33 in u64, 0 wrapped: 2^32 + 14 <= 2^33 holds, 14 <= 0 fails
    # chim_size_no_wrap_twin: Ac = 2: (Ac - 1) * bases = 128 either way: 2^32 + 14 <= 128 fails, 14 <= 128 holds
    for name, Ac, want in (("chim_size_no_wrap", (1 << 26) + 1, True), ("chim_size_no_wrap_twin", 2, False)):
        # (the others at p and at q have 178 bases: longer than the bridge)
        case, p, q = _bridge_case(name, [60, 60, 100, 100], [100, 100, 60, 60], Lc=G31 + 7, Ac=Ac)
        ids = bc.plant_chain(case, random.Random(9702), p, q, bc.bases(random.Random(9703), 78), pieces=3)
        case.update(step="chimeric", watch=("removed", ids[1]), want=want,
                    expr=lambda wrap, Ac=Ac: (2 * (G31 + 7)) & U32 <= ((Ac - 1) * 128) & U32 if wrap else 2 * (G31 + 7) <= (Ac - 1) * 128)
        cases.append(case)
    # trim_size_no_wrap and its twin: the same numbers as L and C, on a tip of three reads and 128 bases at a ring.  -x 1
    for name, C, want in (("trim_size_no_wrap", (1 << 26) + 1, True), ("trim_size_no_wrap_twin", 2, False)):
        g = tc._Grow(9704)
        ring = g.ring(4)
        tip = g.grow(ring[1], 3, lens=[60, 56, 56], ovs=[22, 22, 22])
        case = g.case(name, 1, G31 + 7, C)
        case.update(step="trim", watch=("removed", tip[1]), want=want,
                    expr=lambda wrap, C=C: (2 * (G31 + 7)) & U32 <= ((C - 1) * 128) & U32 if wrap else 2 * (G31 + 7) <= (C - 1) * 128)
        cases.append(case)
    return cases


def no_wrap_named(name):
    return next(c for c in no_wrap() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def no_wrap_expected(name, tables_only=False):
    case = no_wrap_named(name)
    if tables_only:
        return restate(case["step"], case, MARGIN)
    if case["step"] == "trim":
        return tc.expected_trim(case["reads"], case["edges"], case["m"], case["x"], case["L"], case["C"])
    return cc.run(cc.expected_chimeric, case)
