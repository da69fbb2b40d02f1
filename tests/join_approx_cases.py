"""Cases and the serial restatement for `siga unitig --scaffold --join-overlaps --join-mismatches` (csrc/sigax_join.hip); no tests
here (tests/test_join_approx_cases.py, tests/test_gpu_join_approx.py).

expected_join_approx()  the rules of include/sigax.h (the `--join-mismatches` block) serially, with Python integers, over the
                        helpers of tests/join_cases.py: the exact match first, then the second match column by column, the choice
                        and the support test over a dictionary of the reads' k-mers, the compaction, the patches.
A case is join_cases' kind -- a random genome, reads that tile it, scaffold pieces cut from it so that neighbours overlap by a
chosen v -- with substitutions planted in the two copies of the overlap: the genome itself is then the one right join."""
import functools
import random

from tests import gapfill_cases as gc
from tests import join_cases as jc

M64, C, CLASSES, ACGT = jc.M64, jc.C, jc.CLASSES, jc.ACGT
genome, tile, tables, kmer_count, scaffold_tables = jc.genome, jc.tile, jc.tables, jc.kmer_count, jc.scaffold_tables
DEFAULT_OPTS = dict(jc.DEFAULT_OPTS, max_mismatches=0, mismatch_permille=50)
KS = jc.KS
APPROX = 1 << 16


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def budget(v, max_mismatches, permille):
    return min(max_mismatches, v * permille // 1000)


def columns(L, R, v):
    """the j in [0, v) where the last v bytes of L and the first v of R differ, or None when one of the 2 v bytes is not ACGT"""
    a, b = L[len(L) - v:], R[:v]
    if not (ACGT.issuperset(a) and ACGT.issuperset(b)):
        return None
    return [j for j in range(v) if a[j] != b[j]]


def second_match(L, R, lo, hi, max_mismatches, permille):
    """-> (hi', [(v, its columns)] for the v of M1)"""
    hi2 = min(hi, len(L) // 2, len(R) // 2)
    out = []
    for v in range(lo, hi2 + 1):
        cols = columns(L, R, v)
        if cols is not None and len(cols) <= budget(v, max_mismatches, permille):
            out.append((v, cols))
    return hi2, out


def count(reads, k, w):
    return kmer_count(reads, k, w) if ACGT.issuperset(w) else 0


def choose(reads, k, L, R, v, cols):
    """-> (J*, the columns that took R's base); |J| >= k"""
    JL, JR = L + R[v:], L[:len(L) - v] + R
    assert len(JL) == len(JR) and [x for x in range(len(JL)) if JL[x] != JR[x]] == [len(L) - v + j for j in cols]
    star, right = bytearray(JL), []
    for j in cols:
        x = len(L) - v + j
        w = min(max(x, k // 2) - k // 2, len(JL) - k)
        if count(reads, k, JR[w:w + k]) > count(reads, k, JL[w:w + k]):
            star[x] = R[j]
            right.append(j)
    return bytes(star), right


def expected_join_approx(reads, res, scaf, opts=None, n_unitigs=None, n_scaffolds=None, sseqs_capacity=None, sseqs_bytes=None, bases=True):
    """As join_cases.expected_join, with opts over DEFAULT_OPTS (max_mismatches, mismatch_permille) -> its dict with status [24] and
    mm [per gap: mismatches | taken_right << 8 | APPROX, or 0]"""
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    lo, mx, slack, k, mc = o["min_overlap"], o["max_overlap"], o["slack"], o["k"], o["min_count"]
    mmx, pm = o["max_mismatches"], o["mismatch_permille"]
    assert 8 <= lo <= mx <= 4096 and slack < 1 << 31 and 8 <= k <= 128 and mc >= 1 and 0 <= mmx <= 16 and 1 <= pm <= 250
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
    lay_offs += [0] * (n + 1 - len(lay_offs))
    sco += [0] * (n + 1 - len(sco))
    lay += [(0, 0, 0)] * (n - len(lay))
    P = min(lay_offs[S], n) if S else 0
    sof = [gc._scaffold_of(lay_offs, S, p) for p in range(P)]

    def placed(p):
        u, _, off = lay[p]
        base, top = sco[sof[p]], sco[sof[p] + 1]
        if u >= nu or so[u + 1] < so[u] or top < base or top > sb:
            return True, 0, 0
        ln, length = so[u + 1] - so[u], top - base
        if off > length or ln > length - off:
            return True, 0, 0
        return False, base + off, ln

    status = [0] * 24
    joins, mm, cut, patches = [], [], {}, []
    E = [0] * (P + 1)
    for p in range(P):
        E[p + 1] = E[p]
        if not (p + 1 < P and sof[p + 1] == sof[p]):
            continue
        badl, atl, lenl = placed(p)
        badr, atr, lenr = placed(p + 1)
        G = (lay[p + 1][2] - lay[p][2] - lenl) & M64
        v, nm, nw, info, right, R = 0, 0, 0, 0, [], b""
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
                M = jc.matches_of(L, R, lo, hi)
                nm = min(len(M), 255)
                if len(M) >= 2:
                    cls = "AMBIGUOUS"
                elif len(M) == 1:  # rule 1: the exact join
                    v = M[0]
                    wins = jc.junction_windows(L, R, v, k)
                    nw = len(wins)
                    cls = "JOINED" if all(count(reads, k, w) >= mc for w in wins) else "UNSUPPORTED"
                elif mmx == 0:
                    cls = "NONE"
                else:  # rule 2
                    hi2, M1 = second_match(L, R, lo, hi, mmx, pm)
                    status[19] += max(0, hi2 - lo + 1)
                    nm = min(len(M1), 255)
                    if not M1:
                        cls = "NONE"
                    elif len(M1) >= 2:
                        cls = "AMBIGUOUS"
                    else:
                        v, cols = M1[0]
                        assert 1 <= len(cols) <= 16
                        lenj = lenl + lenr - v
                        if lenj < k:  # rule 3
                            cls = "UNSUPPORTED"
                        else:
                            star, right = choose(reads, k, L, R, v, cols)
                            status[20] += 2 * len(cols)
                            first, last = max(0, lenl - v - k + 1), min(lenl - 1, lenj - k)  # rule 4
                            nw = last - first + 1
                            cls = "JOINED" if all(count(reads, k, star[s:s + k]) >= mc for s in range(first, last + 1)) else "UNSUPPORTED"
                        info = len(cols) | len(right) << 8 | APPROX
        status[1 + C[cls]] += 1
        status[13] += nw
        if cls == "JOINED":
            status[9] += v
            status[10] += G
            E[p + 1] = E[p] + G + v
            cut[p] = (G, v)
            if info:
                status[16] += 1
                status[17] += info & 0xFF
                status[18] += len(right)
                patches += [(p, j, R[j]) for j in right]
        joins.append([sof[p], lay[p][0], lay[p + 1][0], min(G, 0xFFFFFFFF), v, C[cls], nm, nw, p])
        mm.append(info)
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
        out = bytearray(b"".join(parts))
        assert len(out) == total, "scaffold offsets that wrap: the bases of such tables are not restated"
        written = set()
        for p, j, b in patches:  # rule 5
            at = sc_offs[sof[p]] + new_off[p + 1] + j
            assert at not in written
            written.add(at)
            out[at] = b
        out = bytes(out)
    return {"status": status, "sc_offs": sc_offs, "sc_lay_offs": lay_offs[:S + 1], "sc_flags": [int(x) for x in scaf["sc_flags"]][:S],
            "layout": [(lay[p][0], lay[p][1], new_off[p]) for p in range(P)], "seqs": out, "joins": [tuple(r) for r in joins], "mm": mm}


def render(exp, seq_offs):
    """the FASTA and JN texts `siga unitig --scaffold --join-overlaps --join-mismatches N --joins` writes for the dict above"""
    fa, jn = [], []
    joined, corrected = [0] * exp["status"][15], [0] * exp["status"][15]
    for j, m in zip(exp["joins"], exp["mm"]):
        joined[j[0]] += j[5] == C["JOINED"]
        corrected[j[0]] += (m >> 8 & 0xFF) if j[5] == C["JOINED"] else 0
        jn.append("JN\tscaffold-%d\tunitig-%d\tunitig-%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
            j[0], j[1], j[2], j[3], CLASSES[j[5]], j[4], j[6], j[7], j[8], m & 0xFF, m >> 8 & 0xFF))
    for s in range(exp["status"][15]):
        a, b = exp["sc_lay_offs"][s], exp["sc_lay_offs"][s + 1]
        head = ">scaffold-%d unitigs=%d gaps=%d" % (s, b - a, b - a - 1)
        if exp["sc_flags"][s] & 1:
            head += " circular=%d" % (exp["sc_flags"][s] >> 1)
        head += " joined=%d corrected=%d" % (joined[s], corrected[s])
        fa.append(head + "\n" + exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]].decode("latin-1") + "\n")
    return "".join(fa), "".join(jn)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def other(b, turn=1):
    """a base that is not b"""
    return b"ACGT"[(b"ACGT".index(b) + turn) % 4]


def sub(c, at, turn=1, scaffold=0):
    """the case with the base at `at` of the scaffold's bases replaced by another one"""
    b = c["scaf"]["seqs"][c["scaf"]["sc_offs"][scaffold] + at]
    return jc.patch(c, scaffold, at, bytes([other(b, turn)]))


@functools.lru_cache(maxsize=None)
def planted(k):
    """the planted cases of one k over join_cases.clean(k) (one index serves them), each with `want`: per gap the class, and
    `genome_out`: whether the joined scaffold must read like the genome"""
    g, reads = jc.clean(k)
    key = "clean_k%d" % k
    out = []
    a0, G = 300, 5

    def add(name, n1, v, n2, opts=None, left=(), right=(), want="JOINED", rd=None, rkey=None, turn=1, genome_out=None, **kw):
        """two pieces that overlap by v, substitutions at the columns `left` of L's copy of the overlap and `right` of R's"""
        o = dict({"max_mismatches": 16, "mismatch_permille": 250}, **(opts or {}))
        c = jc.case(name, k, g, reads if rd is None else tuple(rd), jc.two(a0, n1, v, n2, G=G), o, reads_key=key if rd is None else rkey,
                    seed=len(out) + k, **kw)
        for j in left:
            sub(c, n1 - v + j, turn)
        for j in right:
            sub(c, n1 + G + j, turn + 1)
        c.update(want=[want], genome_out=(want == "JOINED") if genome_out is None else genome_out, v=v, span=(a0, a0 + n1 + n2 - v))
        c["clean"] = False
        out.append(c)
        return c

    n = 2 * k + 200
    v = k + 70  # two columns more than k apart fit, and lane v - lo takes a second stride (v >= lo + 65)
    # choice
    add("one_in_left", n, v, n, left=[30])
    add("one_in_right", n, v, n, right=[30])
    add("one_in_each_far_apart", n, v, n, left=[5], right=[k + 40])
    add("one_in_each_within_half_k", n, v, n, left=[30], right=[30 + k // 2 - 2], want="UNSUPPORTED")
    add("neither_base_supported", n, v, n, left=[30], right=[30], want="UNSUPPORTED")
    # budget: B(60) = 3 at 50 permille; B(100) = 2 by max_mismatches; the floor at v = 19 and v = 20
    p50 = {"mismatch_permille": 50}
    add("d_at_budget", 200, 60, 200, p50, left=[3, 20, 41])
    add("d_above_budget", 200, 60, 200, p50, left=[3, 20, 41, 55], want="NONE")
    add("d_at_max_mismatches", 300, 100, 300, {"max_mismatches": 2}, left=[10], right=[80])
    add("d_above_max_mismatches", 300, 100, 300, {"max_mismatches": 2}, left=[10, 50], right=[80], want="NONE")
    add("v_19_floor", 100, 19, 100, p50, left=[7], want="NONE")
    add("v_20_floor", 100, 20, 100, p50, left=[7])
    add("sixteen_columns", 500, 200, 500, {"mismatch_permille": 100}, left=[3 + 12 * i for i in range(16)])
    add("seventeen_columns", 500, 200, 500, {"mismatch_permille": 100}, left=[3 + 11 * i for i in range(17)], want="NONE")
    # word boundaries of the packed ends; the funnel shift (hi - v) & 31; a lane's second stride
    w = 100
    edge = [0, 31, 32, 63, 64, w - 1]
    add("columns_at_word_edges_left", 300, w, 300, left=edge)
    add("columns_at_word_edges_right", 300, w, 300, right=edge)
    add("columns_at_word_edges_both", 300, w, 300, left=edge[::2], right=edge[1::2], want="UNSUPPORTED")  # 31 | 32 and 63 | 64
    for s in (0, 1, 31, 32):
        add("shift_%d" % s, 300, w, 300, {"max_overlap": w + s}, left=[0, 33], right=[w - 1])
    # the half rule
    add("v_half_of_right", 200, 40, 81, left=[11])
    add("v_half_of_right_plus_1", 200, 41, 81, left=[11], want="NONE")
    add("v_half_of_left", 81, 40, 200, right=[11])
    add("v_half_of_left_plus_1", 81, 41, 200, right=[11], want="NONE")
    # bytes
    c = add("n_inside_overlap", n, v, n, left=[30], want="NONE")
    jc.patch(c, 0, n + G + 50, b"N")
    c = add("lower_case_inside_overlap", n, v, n, left=[30], want="NONE")
    at = n - v + 50
    jc.patch(c, 0, at, c["scaf"]["seqs"][at:at + 1].lower())
    c = add("n_just_behind_overlap", n, v, n, left=[30], want="UNSUPPORTED")  # matched, but a window of J* holds the N
    jc.patch(c, 0, n + G + v, b"N")
    if k >= 64:
        add("j_shorter_than_k", 40, 20, 40, left=[7], want="UNSUPPORTED")  # |J| = 60
    b = a0 + n
    add("minus_strand_only", n, v, n, left=[30], right=[v - 9], rd=tile(g, k, seed=k, minus=(b - 3 * k - v, b + 3 * k)), rkey="minus_k%d" % k)
    add("hole_in_the_overlap", n, v, n, left=[30], rd=tile(g, k, seed=k, drop=b - 20), rkey="hole_k%d" % k, want="UNSUPPORTED")
    # exact first: L ends A' B A, R begins A B A (A, B 20 bases each): v = 20 matches exactly, v = 60 with one mismatch
    rng = random.Random(900 + k)
    A, B = (bytes(rng.choice(b"ACGT") for _ in range(20)) for _ in range(2))
    A1 = A[:9] + bytes([other(A[9])]) + A[10:]
    c = add("exact_and_approximate", 200, 60, 200, want=None, genome_out=False)
    jc.patch(jc.patch(c, 0, 200 - 60, A1 + B + A), 0, 200 + G, A + B + A)
    c["exact_v"] = 20
    # ambiguity: L ends U U, R begins U* U (U 40 bases, U* one substitution): v = 40 and v = 80 with one mismatch each
    U = bytes(rng.choice(b"ACGT") for _ in range(40))
    U1 = U[:17] + bytes([other(U[17])]) + U[18:]
    c = add("tandem_repeat_one_substitution", 300, 80, 300, p50, want="AMBIGUOUS", genome_out=False)
    jc.patch(jc.patch(c, 0, 300 - 80, U + U), 0, 300 + G, U1 + U)
    c["matches"] = 2
    # three pieces, the middle one joined approximately on both sides with v0 + v1 = |U|
    c = jc.case("middle_joined_on_both_sides", k, g, reads, [[(a0, a0 + 200, False, 3), (a0 + 160, a0 + 240, False, 4), (a0 + 200, a0 + 400, False, None)]],
                {"max_mismatches": 16, "mismatch_permille": 250}, reads_key=key, seed=len(out) + k)
    # one in the first piece's tail and one in the middle piece's tail, both patched; the latter lies in J of the first gap too, and
    # only from column k - 1 on beyond its windows, so for the larger k it is planted in the last piece's head instead
    sub(sub(c, 200 - 40 + 13), 200 + 3 + 80 - 40 + 35 if k <= 31 else 200 + 3 + 80 + 4 + 21)
    c.update(want=["JOINED", "JOINED"], genome_out=True, span=(a0, a0 + 400), clean=False)
    out.append(c)
    c = jc.case("middle_one_base_too_short", k, g, reads, [[(a0, a0 + 200, False, 3), (a0 + 160, a0 + 239, False, 4), (a0 + 199, a0 + 400, False, None)]],
                {"max_mismatches": 16, "mismatch_permille": 250}, reads_key=key, seed=len(out) + k)
    sub(sub(c, 200 - 40 + 13), 200 + 3 + 79 - 40 + 21)
    c.update(want=["NONE", "NONE"], genome_out=False, span=(a0, a0 + 400), clean=False)  # |U| / 2 = 39 < 40
    out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def long_overlap(k=31):
    """max_overlap = 4096 and v = 4090 = |L| / 2 over a genome of 13 kb, sparsely tiled (min_count 1): all 128 LDS words of each end,
    4120 support windows; columns in the first word, the last one and in between, from either side"""
    g = genome(k, 78, 13000)
    reads = tuple(tile(g, k, seed=2000 + k, step=20, depth=1))
    v, n1, a0, G = 4090, 8180, 200, 5
    c = jc.case("v_4090", k, g, reads, jc.two(a0, n1, v, n1 + 100, G=G), {"max_overlap": 4096, "min_count": 1, "max_mismatches": 16, "mismatch_permille": 50},
                reads_key="long_approx_k%d" % k, seed=5)
    for j in (0, 2047, 4089):
        sub(c, n1 - v + j)
    for j in (31, 3000, 4064):
        sub(c, n1 + G + j, 2)
    c.update(want=["JOINED"], genome_out=True, v=v, span=(a0, a0 + 2 * n1 + 100 - v), clean=False)
    return c


RANDOM_SIZE = 3000


@functools.lru_cache(maxsize=None)
def random_reads(j):
    k = KS[j % len(KS)]
    g = genome(k, 4000 + j, RANDOM_SIZE)
    return k, g, tuple(tile(g, k, seed=4000 + j))


def random_case(seed):
    """small random scaffolds over a clean tiling, substitutions at 0-3 % in the first and last 120 bases of every piece"""
    rng = random.Random(50000 + seed)
    k, g, reads = random_reads(seed % 8)
    lo = rng.choice((8, 16, 16, 20))
    opts = {"min_overlap": lo, "max_overlap": rng.choice((60, 100, 1000, 4096)), "slack": rng.choice((3, 10, 100)), "min_count": rng.choice((1, 2, 3, 3)),
            "max_mismatches": rng.choice((1, 2, 2, 4, 16)), "mismatch_permille": rng.choice((20, 50, 50, 100, 250))}
    scaffolds, at = [], rng.randrange(0, 40)
    while True:
        sc = []
        for _ in range(rng.choice((1, 2, 2, 3, 4))):
            ln = rng.choice((2 * lo, 2 * lo + 1, 40 + rng.randrange(60), 2 * k + rng.randrange(80), 200 + rng.randrange(100)))
            if at + ln + 300 > len(g):
                break
            step = -rng.choice((lo, rng.randrange(lo, 3 * lo), rng.randrange(20, 100), ln // 2, ln // 2 + 1))
            step = max(step, 1 - ln)
            sc.append([at, at + ln, rng.random() < 0.5, rng.choice((1, 2, 5, opts["slack"], opts["slack"] + 1))])
            at = at + ln + step
        if not sc:
            break
        sc[-1][3] = None
        scaffolds.append([tuple(p) for p in sc])
        at += rng.randrange(5, 30)
    c = jc.case("random_approx_%d" % seed, k, g, reads, scaffolds, opts, seed=seed, reads_key="random_approx_reads_%d" % (seed % 8), clean=False)
    rate = rng.choice((0.0, 0.01, 0.02, 0.03))
    s = bytearray(c["scaf"]["seqs"])
    x = 0
    for sc in scaffolds:
        for a, b, _, G in sc:
            for i in range(b - a):
                if (i < 120 or b - a - i <= 120) and rng.random() < rate:
                    s[x + i] = other(s[x + i], rng.randrange(1, 4))
            x += b - a + (G or 0)
    if rng.random() < 0.2:
        y = rng.randrange(len(s))
        s[y] = ord("N") if rng.random() < 0.5 else ord(chr(s[y]).lower())
    c["scaf"]["seqs"] = bytes(s)
    return c


RANDOM_SEEDS = range(48)


def case_expected(c, **kw):
    return expected_join_approx(c["reads"], c["res"], c["scaf"], c["opts"], **kw)
