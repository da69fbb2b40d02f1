"""Cases and the serial restatement for `siga unitig --scaffold --join-overlaps` (csrc/sigax_join.hip); no tests here
(tests/test_join_cases.py, tests/test_gpu_join.py).

expected_join()  the rules of include/sigax.h (the `--join-overlaps` block), serially, with Python integers, over a dictionary of
                 the reads' k-mers: every pair of neighbouring placements is classed, every overlap length tried byte by byte, the
                 junction windows counted, and the new tables and bases laid out by deleting bytes from the old ones.
A case is a random genome, reads that tile it, and scaffold tables whose placed pieces are cut from the genome so that neighbours
overlap by a chosen v with N laid between them: the genome itself is then the one right join."""
import functools
import random

from tests import gapfill_cases as gc
from tests import unitig_cases as uc

M64 = (1 << 64) - 1
REV = uc.PLACED_REV
CLASSES = ("JOINED", "CLOSED", "FAR", "SHORT", "NONE", "AMBIGUOUS", "UNSUPPORTED", "MALFORMED")
C = {name: i for i, name in enumerate(CLASSES)}
DEFAULT_OPTS = {"min_overlap": 16, "max_overlap": 1000, "slack": 100, "k": 31, "min_count": 3}
KS = (15, 31, 64, 128)
ACGT = frozenset(b"ACGT")
genome, tile, tables, kmer_count, read_len = gc.genome, gc.tile, gc.tables, gc.kmer_count, gc.read_len


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def matches_of(L, R, lo, hi):
    """M: every v in [lo, hi] with the last v bytes of L the first v of R, all of them upper-case ACGT"""
    return [v for v in range(lo, hi + 1) if L[len(L) - v:] == R[:v] and ACGT.issuperset(R[:v])]


def junction_windows(L, R, v, k):
    """the k-byte windows of J = L ++ R[v:] that lie neither wholly in L nor wholly in R"""
    J = L + R[v:]
    first, last = max(len(L) - k + 1, 0), min(len(L) - v - 1, len(J) - k)
    return [J[s:s + k] for s in range(first, last + 1)]


def expected_join(reads, res, scaf, opts=None, n_unitigs=None, n_scaffolds=None, sseqs_capacity=None, sseqs_bytes=None, bases=True):
    """reads: the indexed reads (bytes); res: seq_offs of a unitig call; scaf: sc_offs, sc_lay_offs, sc_flags, layout [(unitig,
    flags, offset)] and seqs of a scaffold or gapfill call; opts over DEFAULT_OPTS; n_unitigs, n_scaffolds: the counts the device
    form is given when they are not the tables' sizes (the capacity is len(seq_offs) - 1); sseqs_capacity: the room for the bases
    (None: exactly enough); sseqs_bytes: None = len(seqs); bases: False leaves the bases out (tables whose bases are not restated)
    -> dict(status [16], sc_offs, sc_lay_offs, sc_flags, layout, seqs bytes or None, joins [(scaffold, left, right, laid, overlap,
    cls, matches, windows, offset)])"""
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    lo, mx, slack, k, mc = o["min_overlap"], o["max_overlap"], o["slack"], o["k"], o["min_count"]
    assert 8 <= lo <= mx <= 4096 and slack < 1 << 31 and 8 <= k <= 128 and mc >= 1
    reads = reads if isinstance(reads, tuple) else tuple(bytes(r) for r in reads)
    so = [int(x) for x in res["seq_offs"]]
    seqs = bytes(scaf["seqs"])
    sb = len(seqs) if sseqs_bytes is None else sseqs_bytes
    n = len(so) - 1
    nu = min(n if n_unitigs is None else n_unitigs, n)
    lay_offs = [int(x) for x in scaf["sc_lay_offs"]]
    sco = [int(x) for x in scaf["sc_offs"]]
    S = min(len(lay_offs) - 1 if n_scaffolds is None else n_scaffolds, n)
    lay = [tuple(int(x) for x in p) for p in (scaf["layout"].tolist() if hasattr(scaf["layout"], "tolist") else scaf["layout"])]
    lay_offs += [0] * (n + 1 - len(lay_offs))  # the device form's tables have the capacity's entries: zeros beyond what is given
    sco += [0] * (n + 1 - len(sco))
    lay += [(0, 0, 0)] * (n - len(lay))
    P = min(lay_offs[S], n) if S else 0
    sof = [gc._scaffold_of(lay_offs, S, p) for p in range(P)]

    def placed(p):
        """-> (bad, where its bases lie in seqs, its bases)"""
        u, _, off = lay[p]
        base, top = sco[sof[p]], sco[sof[p] + 1]
        if u >= nu or so[u + 1] < so[u] or top < base or top > sb:
            return True, 0, 0
        ln, length = so[u + 1] - so[u], top - base
        if off > length or ln > length - off:
            return True, 0, 0
        return False, base + off, ln

    status = [0] * 16
    joins, cut = [], {}
    E = [0] * (P + 1)  # E[p]: the bytes the joined gaps before placement p take out
    for p in range(P):
        E[p + 1] = E[p]
        if not (p + 1 < P and sof[p + 1] == sof[p]):
            continue
        badl, atl, lenl = placed(p)
        badr, atr, lenr = placed(p + 1)
        G = (lay[p + 1][2] - lay[p][2] - lenl) & M64
        v, nm, nw = 0, 0, 0
        if badl or badr:
            cls = "MALFORMED"
        elif G == 0:
            cls = "CLOSED"
        elif G > slack:
            cls = "FAR"
        elif seqs[atl + lenl:atl + lenl + G] != b"N" * G:
            cls = "CLOSED"
        else:
            hi = min(mx, lenl - 1, lenr - 1)
            if hi < lo:
                cls = "SHORT"
            else:
                L, R = seqs[atl:atl + lenl], seqs[atr:atr + lenr]
                status[12] += hi - lo + 1
                M = matches_of(L, R, lo, hi)
                nm = min(len(M), 255)
                if not M:
                    cls = "NONE"
                elif len(M) >= 2:
                    cls = "AMBIGUOUS"
                else:
                    v = M[0]
                    wins = junction_windows(L, R, v, k)
                    nw = len(wins)
                    ok = all(ACGT.issuperset(w) and kmer_count(reads, k, w) >= mc for w in wins)
                    cls = "JOINED" if ok else "UNSUPPORTED"
        status[1 + C[cls]] += 1
        status[13] += nw
        if cls == "JOINED":
            status[9] += v
            status[10] += G
            E[p + 1] = E[p] + G + v
            cut[p] = (G, v)
        joins.append([sof[p], lay[p][0], lay[p + 1][0], min(G, 0xFFFFFFFF), v, C[cls], nm, nw, p])
    # the new tables
    head_of = [min(lay_offs[s], P) for s in range(S + 1)]
    new_off = [(lay[p][2] - (E[p] - E[head_of[sof[p]]])) & M64 for p in range(P)]
    lens = []
    for s in range(S):
        h, e = head_of[s], head_of[s + 1]
        lens.append((sco[s + 1] - sco[s] - (E[e] - E[h] if e > h else 0)) & M64)
    sc_offs = [0]
    for x in lens:
        sc_offs.append((sc_offs[-1] + x) & M64)
    for rec in joins:
        p = rec[8]
        rec[8] = new_off[p + 1] if rec[5] == C["JOINED"] else (new_off[p] + placed(p)[2]) & M64
    total = sc_offs[S]
    status[0] = len(joins)
    status[11] = total
    cap = total if sseqs_capacity is None else sseqs_capacity
    status[14] = 1 if total > cap else 0
    status[15] = S
    out = None
    if bases and not status[14]:
        parts = []
        for s in range(S):
            old = seqs[sco[s]:sco[s + 1]]
            at = 0
            for p in range(head_of[s], head_of[s + 1]):
                if p in cut:
                    G, v = cut[p]
                    a, b = lay[p + 1][2] - G, lay[p + 1][2] + v
                    assert at <= a <= b <= len(old), "joined gaps out of order: the bases of such tables are not restated"
                    parts.append(old[at:a])
                    at = b
            parts.append(old[at:])
        out = b"".join(parts)
        assert len(out) == total, "scaffold offsets that wrap: the bases of such tables are not restated"
    return {"status": status, "sc_offs": sc_offs, "sc_lay_offs": lay_offs[:S + 1], "sc_flags": [int(x) for x in scaf["sc_flags"]][:S],
            "layout": [(lay[p][0], lay[p][1], new_off[p]) for p in range(P)], "seqs": out, "joins": [tuple(r) for r in joins]}


def render(exp, seq_offs, filled=None):
    """the FASTA, layout and JN texts `siga unitig --scaffold --join-overlaps --joins` writes for expected_join's dict; seq_offs: the
    unitig call's; filled: per scaffold the gaps --gapfill filled, None without it"""
    fa, lay, jn = [], [], []
    joined = [0] * exp["status"][15]
    for j in exp["joins"]:
        joined[j[0]] += j[5] == C["JOINED"]
        jn.append("JN\tscaffold-%d\tunitig-%d\tunitig-%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (j[0], j[1], j[2], j[3], CLASSES[j[5]], j[4], j[6], j[7], j[8]))
    for s in range(exp["status"][15]):
        a, b = exp["sc_lay_offs"][s], exp["sc_lay_offs"][s + 1]
        head = ">scaffold-%d unitigs=%d gaps=%d" % (s, b - a, b - a - 1)
        if exp["sc_flags"][s] & 1:
            head += " circular=%d" % (exp["sc_flags"][s] >> 1)
        if filled is not None:
            head += " filled=%d" % filled[s]
        head += " joined=%d" % joined[s]
        fa.append(head + "\n" + exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]].decode("latin-1") + "\n")
        for p in range(a, b):
            u, fl, off = exp["layout"][p]
            before = 0
            if p > a:
                v, _, voff = exp["layout"][p - 1]
                before = off - voff - (seq_offs[v + 1] - seq_offs[v])
            lay.append("scaffold-%d\tunitig-%d\t%s\t%d\t%d\n" % (s, u, "-" if fl & REV else "+", off, before))
    return "".join(fa), "".join(lay), "".join(jn)


# ---- tables over pieces of a genome ------------------------------------------------------------------------------------------------
def scaffold_tables(g, scaffolds, seed=0, flags=None, fills=()):
    """scaffolds: per scaffold a list of pieces (a, b, placed reversed, G: the N laid BEHIND the piece, None after the last); a
    piece that begins before the one before it ends overlaps it.  fills: (scaffold, piece) whose gap holds the genome's bytes
    behind the piece for N.  -> (res, scaf) with sc_offs and seqs: every piece reads like the genome as placed"""
    res, scaf, _ = tables(g, scaffolds, seed, flags)
    sc_offs, parts = [0], []
    for i, sc in enumerate(scaffolds):
        ln = 0
        for j, (a, b, _, G) in enumerate(sc):
            parts.append(g[a:b])
            gap = g[b:b + (G or 0)] if (i, j) in fills else b"N" * (G or 0)
            assert len(gap) == (G or 0)
            parts.append(gap)
            ln += b - a + (G or 0)
        sc_offs.append(sc_offs[-1] + ln)
    scaf["sc_offs"] = sc_offs
    scaf["seqs"] = b"".join(parts)
    return res, scaf


def case(name, k, g, reads, scaffolds, opts=None, flags=None, seed=0, reads_key=None, fills=(), clean=True, **extra):
    res, scaf = scaffold_tables(g, scaffolds, seed, flags, fills)
    c = {"name": "%s_k%d" % (name, k), "kind": name, "k": k, "genome": g, "reads": reads, "reads_key": reads_key or ("%s_k%d" % (name, k)), "res": res,
         "scaf": scaf, "opts": dict(DEFAULT_OPTS, k=k, **(opts or {})), "clean": clean}
    c.update(extra)
    return c


def patch(c, scaffold, at, new):
    """bytes of the case's scaffold bases replaced: `at` within the scaffold"""
    s = c["scaf"]["seqs"]
    x = c["scaf"]["sc_offs"][scaffold] + at
    c["scaf"]["seqs"] = s[:x] + new + s[x + len(new):]
    c["clean"] = False
    return c


@functools.lru_cache(maxsize=None)
def clean(k):
    """-> (genome of 4 kb, its tiling): what every case without a special read set shares, so that one index serves them"""
    g = genome(k, 2, 4000)
    return g, tuple(tile(g, k, seed=k))


def two(a, n1, v, n2, G=5, rl=False, rr=False):
    """one scaffold of two pieces of n1 and n2 bases, the second beginning v bases before the first ends (v < 0: that far behind)"""
    return [[(a, a + n1, rl, G), (a + n1 - v, a + n1 - v + n2, rr, None)]]


def hand_built(k):
    """the cases of one k, by name"""
    g, reads = clean(k)
    key = "clean_k%d" % k
    out = []

    def add(name, scaffolds, opts=None, rd=None, rkey=None, gen=None, **kw):
        c = case(name, k, g if gen is None else gen, reads if rd is None else tuple(rd), scaffolds, opts,
                 reads_key=key if rd is None else rkey or "%s_k%d" % (name, k), seed=len(out) + k, **kw)
        out.append(c)
        return c

    n, a0 = 2 * k + 40, 300
    low = lambda v: {"min_overlap": 8} if v < 16 else {}
    for v in sorted({16, 31, 32, 33, 63, 64, 65, k - 2, k - 1, k}):
        m = max(n, v + 20)
        add("v_%d" % v, two(a0, m, v, m + 3), low(v))
    add("v_at_lo", two(a0, n, 20, n), {"min_overlap": 20})
    add("v_below_lo", two(a0, n, 19, n), {"min_overlap": 20})
    add("v_at_hi", two(a0, n, 40, n), {"max_overlap": 40})
    add("v_above_hi", two(a0, n, 41, n), {"max_overlap": 40})
    add("range_over_64", two(a0, 120, 90, 125))
    add("range_over_128", two(a0, 220, 150, 230))
    add("range_over_128_at_the_top", two(a0, 220, 219, 230))
    add("hi_by_left", two(a0, 30, 29, 80))
    add("hi_by_right", two(a0, 80, 29, 30))
    add("left_within_right", two(a0, 30, 30, 80))  # v = |L| is not looked for
    add("piece_of_min_overlap", [[(a0, a0 + n, False, 3), (a0 + n - 15, a0 + n + 1, False, 2), (a0 + n + 1 - 15, a0 + 2 * n, False, None)]])
    add("piece_of_min_overlap_plus_1", [[(a0, a0 + n, False, 3), (a0 + n - 16, a0 + n + 1, False, 2), (a0 + n + 1 - 16, a0 + 2 * n, False, None)]])
    for nm, rl, rr in (("forward_reverse", False, True), ("reverse_forward", True, False), ("reverse_reverse", True, True)):
        add(nm, two(a0, n, 24, n, rl=rl, rr=rr))
    # L's tail at every residue modulo 16 of the scaffold bases
    scs, at = [], 0
    for i in range(16):
        n1 = n + (i - (at + n)) % 16
        scs.append(two(a0 + 7 * i, n1, 20 + i, n, G=1 + i % 3)[0])
        at += n1 + 1 + i % 3 + n
    c = add("residues", scs)
    assert sorted((c["scaf"]["sc_offs"][i] + sc[0][1] - sc[0][0]) % 16 for i, sc in enumerate(scs)) == list(range(16))
    for nm, G in (("g_1", 1), ("g_at_slack", 7), ("g_above_slack", 8)):
        add(nm, two(a0, n, 22, n, G=G), {"slack": 7})
    # gaps that are no gaps any more
    add("filled_by_gapfill", [[(a0, a0 + n, False, 12), (a0 + n + 12, a0 + 2 * n, False, None)]], fills={(0, 0)})
    patch(add("one_base_in_the_gap", two(a0, n, 22, n, G=9)), 0, n + 4, b"A")
    add("g_0", [[(a0, a0 + n, False, 0), (a0 + n, a0 + 2 * n, True, None)]])
    add("no_overlap", two(a0, n, -12, n, G=12))
    # bytes outside ACGT: inside the overlap, in both copies, and just outside it, in one
    v = 22
    for nm, ch in (("n", b"N"), ("lower_case", None)):
        for where, at in (("first", n - v), ("last", n - 1)):
            c = add("%s_inside_overlap_%s" % (nm, where), two(a0, n, v, n, G=4))
            b = ch or c["scaf"]["seqs"][at:at + 1].lower()
            patch(patch(c, 0, at, b), 0, n + 4 + at - (n - v), b)
        c = add("%s_before_overlap" % nm, two(a0, n, v, n, G=4))
        patch(c, 0, n - v - 1, ch or c["scaf"]["seqs"][n - v - 1:n - v].lower())
        c = add("%s_behind_overlap" % nm, two(a0, n, v, n, G=4))
        patch(c, 0, n + 4 + v, ch or c["scaf"]["seqs"][n + 4 + v:n + 5 + v].lower())
    # repeats across the junction: more than one v fits, and the estimate cannot choose
    x = a0 + n - 45
    gt = g[:x] + b"ACG" * 20 + g[x + 60:]
    c = add("tandem_repeat", [[(a0, x + 45, False, 6), (x + 15, x + 15 + n, False, None)]], gen=gt, clean=False)
    c["matches"] = 10  # v = 18, 21, .. 45
    gh = g[:x] + b"A" * 60 + g[x + 60:]
    c = add("homopolymer", [[(a0, x + 45, False, 6), (x + 15, x + 15 + n, False, None)]], gen=gh, clean=False)
    c["matches"] = 30  # v = 16 .. 45
    # the reads themselves: b = where L ends in the genome; the windows across the junction all hold g[b - 1]
    b = a0 + n
    add("one_window_in_a_hole", two(a0, n, k - 2, n), low(k - 2), rd=tile(g, k, seed=k, drop=b - 1), rkey="hole_k%d" % k)
    add("four_windows_in_a_hole", two(a0, n, k - 5, n), low(k - 5), rd=tile(g, k, seed=k, drop=b - 1), rkey="hole_k%d" % k)
    add("hole_behind_the_junction_windows", two(a0, n, k - 1, n), low(k - 1), rd=tile(g, k, seed=k, drop=b - 1), rkey="hole_k%d" % k)
    add("minus_strand_only", two(a0, n, k - 5, n), low(k - 5), rd=tile(g, k, seed=k, minus=(b - 2 * k, b + 2 * k)))
    rng = random.Random(k)
    over = g[b - k - 4:b - k - 4 + read_len(k)]  # a read over both windows of v = k - 3
    for copies, nm in ((3, "windows_at_min_count"), (2, "windows_below_min_count")):
        rd = tile(g, k, seed=k, drop=b - 1) + [uc.revcomp(over) if rng.random() < 0.5 else over for _ in range(copies)]
        add(nm, two(a0, n, k - 3, n), low(k - 3), rd=rd)
    # joins that chain: the second overlap reaches back into the first
    m = 40
    p1 = a0 + n - 25
    p2 = p1 + m - 25
    p3 = p2 + n - 30
    add("three_joins_in_a_row", [[(a0, a0 + n, False, 3), (p1, p1 + m, True, 1), (p2, p2 + n, False, 60), (p3, p3 + n, True, None)]])
    b0 = a0 + 5 * n
    add("ring_and_single", [[(b0, b0 + n, False, None)], two(a0, n, 21, n, G=2)[0], [(b0 + n + 50, b0 + 2 * n + 50, True, None)]], flags=[0, 1 | (17 << 1), 0])
    # a placement beyond the unitigs
    c = add("bad_placement", [[(a0, a0 + n, False, 3), (a0 + n - 20, a0 + 2 * n, False, 4), (a0 + 2 * n - 40, a0 + 3 * n, False, None)]])
    c["scaf"]["layout"][1] = (0xFFFFFFF0,) + tuple(c["scaf"]["layout"][1][1:])
    c["clean"] = False
    return out


@functools.lru_cache(maxsize=None)
def many_gaps(count, k=15, step=4, depth=3, min_count=3, hole_under=None):
    """`count` gaps in one scaffold and a second scaffold behind it: pieces of 20 .. 60 bases, overlaps of 8 .. 19, now and then a
    true gap.  step, depth: the tiling; min_count: the support asked for; hole_under = i: no read holds the last base of piece i,
    which every window across the junction of gap i holds.  The pieces and the genome do not depend on the four"""
    rng = random.Random(count)
    at, pieces = 50, []
    for i in range(count + 1):
        ln = 20 + rng.randrange(41)
        over = -rng.randrange(8, 20) if rng.random() < 0.8 else rng.randrange(0, 6)
        pieces.append((at, at + ln, rng.random() < 0.5, max(1, over + rng.randrange(0, 4)) if i < count else None))
        at += ln + over
    g = genome(k, 200 + count, at + 400)
    tail = two(at + 100, 50, 17, 50)[0]
    drop = None if hole_under is None else pieces[hole_under][1] - 1
    opts = {"min_overlap": 8, "slack": 10}
    if min_count != 3:
        opts["min_count"] = min_count
    return case("gaps_%d" % count, k, g, tuple(tile(g, k, seed=count, step=step, depth=depth, drop=drop)), [pieces, tail], opts)


MATCH_CLASSES = ("JOINED", "NONE", "AMBIGUOUS", "UNSUPPORTED")


def came_to_the_match(exp):
    """the gap numbers of expected_join's dict that came to the match, in the order k_join_list gives them to the match waves"""
    return [i for i, j in enumerate(exp["joins"]) if CLASSES[j[5]] in MATCH_CLASSES]


@functools.lru_cache(maxsize=None)
def beyond_the_grid(n_cu):
    """more open gaps than the 16 * n_cu one-wave workgroups of the match and support launches, sparsely tiled, with a hole in the
    reads under one junction more than 100 open gaps beyond the grid -> (case, its expected result, the gap over the hole)"""
    grid = 16 * n_cu
    count = grid + 300
    kw = dict(step=30, depth=1, min_count=1)
    exp = case_expected(many_gaps(count, 15, **kw))
    opened = came_to_the_match(exp)
    assert len(opened) > grid + 100
    at = next(i for i in opened[grid + 100:] if exp["joins"][i][5] == C["JOINED"] and exp["joins"][i][7] > 0 and i < count)
    c = many_gaps(count, 15, hole_under=at, **kw)
    return c, case_expected(c), at


# ---- the match at its limits: ranges of up to 4096 candidates, every LDS word, |M| beyond 255 -----------------------------------------
@functools.lru_cache(maxsize=None)
def long_overlaps(k=31):
    """overlaps of thousands of bases over a genome of 30 kb, sparsely tiled (min_count 1; with v >= k - 1 there are no junction
    windows, so the reads hardly matter): hi = 4096 by both lengths and by max_overlap, v at, just above and far below hi, v either
    side of 2048 (where a lane of k_join_match begins to pack a second word), 66 words, a byte outside ACGT deep in a long range,
    |M| beyond 255 and a tandem repeat whose M has stride 3 over ten turns of the wave"""
    g = genome(k, 77, 30000)
    reads = tuple(tile(g, k, seed=1000 + k, step=20, depth=1))
    key = "long_k%d" % k
    out = []

    def add(name, scaffolds, opts=None, gen=None, rd=None, **kw):
        o = dict({"max_overlap": 4096, "min_count": 1}, **(opts or {}))
        c = case(name, k, g if gen is None else gen, reads if rd is None else rd, scaffolds, o, reads_key=key if rd is None else "%s_k%d" % (name, k),
                 seed=len(out) + 7 * k, **kw)
        out.append(c)
        return c

    a0 = 500
    add("hi_4096_by_both_lengths", two(a0, 4097, 4096, 4097), v=4096)
    add("hi_66_words", two(a0, 2200, 2100, 2200), {"max_overlap": 2112}, v=2100)
    add("last_word_partly_filled", two(a0, 4097, 4095, 4200), v=4095)
    add("hi_by_max_overlap", two(a0, 6000, 4096, 6000), v=4096)
    add("v_just_above_hi", two(a0, 6000, 4097, 6000), v=None)
    for v in (2049, 2048, 2047):
        add("v_%d" % v, two(a0, 5000, v, 6000), v=v)
    add("v_in_the_middle", two(a0, 4097, 3000, 4097), v=3000)
    # a byte outside ACGT at the same place in both copies of the overlap, 3000 bases before L's end and at R's base 3000: the
    # two ends still agree byte for byte (and both pack to T's code), so only the run of ACGT, found in a far word, keeps v = 4096
    # from matching.  L's overlap base i lies at 1 + i of the scaffold, R's at 4097 + 5 + i
    i = 4096 - 3000
    patch(patch(add("n_far_in_the_tail", two(a0, 4097, 4096, 4097), v=None), 0, 1 + i, b"N"), 0, 4102 + i, b"N")
    c = add("lower_case_far_in_the_head", two(a0, 4097, 4096, 4097), v=None)
    low = c["scaf"]["seqs"][4102 + 3000:4103 + 3000].lower()
    patch(patch(c, 0, 1 + 3000, low), 0, 4102 + 3000, low)
    # L ends and R begins with 600 bases of one letter: every v in 16 .. 600 matches
    x = a0 + 700
    other = lambda b: bytes([next(c for c in b"CGT" if c != b)])
    gh = g[:x - 1] + other(g[x - 1]) + b"A" * 600 + other(g[x + 600]) + g[x + 601:]
    rd = tuple(tile(gh, k, seed=1001 + k, step=20, depth=1))
    add("matches_saturate", [[(a0, x + 600, False, 6), (x, x + 600 + 150, False, None)]], gen=gh, rd=rd, clean=False, matches=255, v=None)
    # (ACG) x 500: L ends 600 bases into it, R begins 600 bases before its end, so v = 18, 21 .. 600 match and no other
    gt = g[:x - 1] + (b"T" if g[x - 1:x] != b"T" else b"A") + b"ACG" * 500 + (b"T" if g[x + 1500:x + 1501] != b"T" else b"C") + g[x + 1501:]
    rd = tuple(tile(gt, k, seed=1002 + k, step=20, depth=1))
    add("long_tandem_repeat", [[(a0, x + 600, False, 6), (x + 900, x + 1500 + 150, False, None)]], gen=gt, rd=rd, clean=False, matches=195, v=None)
    return out


# ---- random cases: ten read sets, ten cases over each ---------------------------------------------------------------------------------
RANDOM_SIZE = 3000


@functools.lru_cache(maxsize=None)
def random_reads(j):
    """-> (k, genome with a tandem repeat and a homopolymer planted, its tiling with two holes, where the four lie)"""
    rng = random.Random(7000 + j)
    k = KS[j % len(KS)]
    g = bytearray(genome(k, 3000 + j, RANDOM_SIZE))
    rep, hom = rng.randrange(600, 900), rng.randrange(1500, 1800)
    unit = bytes(rng.sample(list(b"ACGT"), 3))
    g[rep:rep + 60] = unit * 20
    g[hom:hom + 50] = bytes([rng.choice(b"ACGT")]) * 50
    g = bytes(g)
    holes = (rng.randrange(1000, 1300), rng.randrange(2200, 2500))
    rl = read_len(k)
    starts = list(range(0, len(g) - rl + 1, 4))
    if starts[-1] != len(g) - rl:
        starts.append(len(g) - rl)
    reads = []
    for s in starts:
        if any(s <= h < s + rl for h in holes):
            continue
        for _ in range(3):
            r = g[s:s + rl]
            reads.append(uc.revcomp(r) if rng.random() < 0.5 else r)
    return k, g, tuple(reads), {"repeat": rep, "homopolymer": hom, "holes": holes}


def random_case(seed):
    rng = random.Random(seed)
    k, g, reads, where = random_reads(seed % 10)
    lo = rng.choice((8, 12, 16, 16, 20))
    opts = {"min_overlap": lo, "max_overlap": rng.choice((lo, 40, 100, 1000, 4096)), "slack": rng.choice((3, 10, 100)),
            "min_count": rng.choice((1, 2, 3, 3, 4))}
    spots = [where["repeat"] + 45, where["homopolymer"] + 35, where["holes"][0], where["holes"][1]]
    scaffolds, fills, at = [], set(), rng.randrange(0, 40)
    while True:
        sc = []
        for j in range(rng.choice((1, 2, 2, 3, 4, 6))):
            ln = rng.choice((lo, lo + 1, lo + rng.randrange(2, 60), 2 * k + rng.randrange(40), 150 + rng.randrange(100)))
            near = [s for s in spots if at + lo < s <= at + ln + 60]
            if near and rng.random() < 0.7:  # a piece that ends in a repeat or at a hole
                ln = near[0] - at
            if at + ln + 300 > len(g):
                break
            step = rng.choice((-rng.randrange(lo, 3 * lo), -rng.randrange(8, 80), -rng.randrange(max(8, k - 6), k + 2), 0, rng.randrange(1, 12), -lo, 1 - lo))
            step = max(step, 1 - ln)
            G = rng.choice((0, 1, 2, 5, rng.randrange(1, 15), opts["slack"], opts["slack"] + 1))
            if step > 0 and rng.random() < 0.5:
                G = step
                if rng.random() < 0.5:
                    fills.add((len(scaffolds), len(sc)))
            sc.append([at, at + ln, rng.random() < 0.5, G])
            at = at + ln + step
        if not sc:
            break
        fills.discard((len(scaffolds), len(sc) - 1))
        sc[-1][3] = None
        scaffolds.append([tuple(p) for p in sc])
        at += rng.randrange(5, 30)
    c = case("random_%d" % seed, k, g, reads, scaffolds, opts, seed=seed, reads_key="random_reads_%d" % (seed % 10), fills=fills, clean=False)
    if rng.random() < 0.3:  # now and then a byte outside ACGT somewhere
        x = rng.randrange(len(c["scaf"]["seqs"]))
        s = c["scaf"]["seqs"]
        c["scaf"]["seqs"] = s[:x] + (b"N" if rng.random() < 0.5 else s[x:x + 1].lower()) + s[x + 1:]
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    out = [c for k in KS for c in hand_built(k)]
    out += [many_gaps(70, 15), many_gaps(300, 15)]
    out += long_overlaps(31)
    out += [random_case(s) for s in range(100)]
    return out


def case_expected(c, **kw):
    return expected_join(c["reads"], c["res"], c["scaf"], c["opts"], **kw)


def joined_again(c, exp):
    """the case with the tables a join returned: what a second join is given"""
    scaf = {"sc_offs": exp["sc_offs"], "sc_lay_offs": exp["sc_lay_offs"], "sc_flags": exp["sc_flags"], "layout": exp["layout"], "seqs": exp["seqs"]}
    return dict(c, scaf=scaf, name=c["name"] + "_again")
