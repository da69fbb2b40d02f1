"""Cases and the serial restatement for `siga unitig --scaffold --gapfill` (csrc/sigax_gapfill.hip); no tests here
(tests/test_gapfill_cases.py, tests/test_gpu_gapfill.py).

expected_gapfill()  the rules of include/sigax.h (the `--gapfill` block), serially, with Python integers, over a dictionary of the
                    reads' k-mers: every pair of neighbouring placements is classed, walked forward and, where the rules say so,
                    in reverse, and the new tables and bases are laid out gap by gap.
A case is a random genome, reads that tile it, and hand-made unitig and scaffold tables over pieces of it: the unitig of a piece
is stored so that the piece AS PLACED reads like the genome, which makes the genome between two pieces the one right fill."""
import functools
import random

from tests import unitig_cases as uc

M64 = (1 << 64) - 1
REV = uc.PLACED_REV
CLASSES = ("FILLED", "SHORT", "NON_ACGT", "FAR", "NO_ROOM", "DEAD_END", "BRANCH", "TOO_LONG", "OVERLAP", "OFF_ESTIMATE", "MALFORMED")
C = {name: i for i, name in enumerate(CLASSES)}
NOT_RUN = 255
DEFAULT_OPTS = {"k": 31, "min_count": 3, "slack": 100, "max_fill": 10000}
KS = (15, 31, 32, 33, 63, 64, 65, 128)
revcomp = uc.revcomp


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _kmers(reads, k):
    """every window of k bytes of every read -> how often it occurs (a window with a byte outside ACGT is never asked for)"""
    d = {}
    for r in reads:
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            d[w] = d.get(w, 0) + 1
    return d


def kmer_count(reads, k, w):
    """count(w) = occ(w) + occ(revcomp(w)): a reverse-palindromic w counts twice"""
    d = _kmers(reads if isinstance(reads, tuple) else tuple(reads), k)
    return d.get(w, 0) + d.get(revcomp(w), 0)


def _walk(d, min_count, src, dst, limit):
    """d: the reads' k-mers -> (outcome, t, the appended bases, extension steps made)"""
    w, out = src, bytearray()
    for t in range(1, limit + 1):
        cand = [b for b in b"ACGT" if d.get(w[1:] + bytes([b]), 0) + d.get(revcomp(w[1:] + bytes([b])), 0) >= min_count]
        if not cand:
            return "DEAD_END", t, bytes(out), t
        if len(cand) >= 2:
            return "BRANCH", t, bytes(out), t
        out.append(cand[0])
        w = w[1:] + bytes(cand[:1])
        if w == dst:
            return "REACHED", t, bytes(out), t
    return "TOO_LONG", limit, bytes(out), limit


def _judge(outcome, t, appended, k, slack, G):
    """a walk's outcome as a class -> (class, fill or None)"""
    if outcome != "REACHED":
        return outcome, None
    if t < k:
        return "OVERLAP", None
    f = t - k
    if f + slack < G:
        return "OFF_ESTIMATE", None
    return "FILLED", appended[:f]


def _scaffold_of(lay_offs, S, p):
    lo, hi = 0, S
    for _ in range(32):
        if hi - lo <= 1:
            break
        mid = (lo + hi) >> 1
        if lay_offs[mid] <= p:
            lo = mid
        else:
            hi = mid
    return lo


def expected_gapfill(reads, res, scaf, opts=None, n_unitigs=None, n_scaffolds=None, max_walk_bases=None, sseqs_capacity=None,
                     useqs_bytes=None):
    """reads: the indexed reads (bytes); res: seq_offs and useqs of a unitig call; scaf: sc_lay_offs, sc_flags and layout
    [(unitig, flags, offset)] of the scaffold call; opts over DEFAULT_OPTS; n_unitigs, n_scaffolds: the counts the device form is
    given when they are not the tables' sizes (the capacity is len(seq_offs) - 1); max_walk_bases: the walk scratch (None: room
    for every gap); sseqs_capacity: the room for the bases (None: exactly enough); useqs_bytes: None = len(useqs)
    -> dict(status [24] with None for the sectors, sc_offs, sc_lay_offs, sc_flags, layout, seqs bytes or None, gaps [(scaffold,
    left, right, laid, fill, cls, fwd, rev, dir, offset)], fills {gap number: bytes})"""
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    k, mc, slack, max_fill = o["k"], o["min_count"], o["slack"], o["max_fill"]
    assert 8 <= k <= 128 and mc >= 1 and slack < 1 << 31 and max_fill < 1 << 31
    d = _kmers(reads if isinstance(reads, tuple) else tuple(bytes(r) for r in reads), k)
    so = [int(x) for x in res["seq_offs"]]
    useqs = bytes(res["useqs"])
    ub = len(useqs) if useqs_bytes is None else useqs_bytes
    n = len(so) - 1
    nu = min(n if n_unitigs is None else n_unitigs, n)
    lay_offs = [int(x) for x in scaf["sc_lay_offs"]]
    S = min(len(lay_offs) - 1 if n_scaffolds is None else n_scaffolds, n)
    lay = [tuple(int(x) for x in p) for p in (scaf["layout"].tolist() if hasattr(scaf["layout"], "tolist") else scaf["layout"])]
    lay_offs += [0] * (n + 1 - len(lay_offs))  # the device form's tables have the capacity's entries: zeros beyond what is given
    lay += [(0, 0, 0)] * (n - len(lay))
    P = min(lay_offs[S], n) if S else 0

    def unitig(p):
        """-> (bad, where it lies, its bases, placed reversed)"""
        u, fl, _ = lay[p]
        if u >= nu or so[u + 1] < so[u] or so[u + 1] > ub:
            return True, 0, 0, bool(fl & REV)
        return False, so[u], so[u + 1] - so[u], bool(fl & REV)

    def placed(p):
        _, at, ln, rev = unitig(p)
        b = useqs[at:at + ln]
        return revcomp(b) if rev else b

    sof = [_scaffold_of(lay_offs, S, p) for p in range(P)]
    status = [0] * 24
    gaps, fills, walk_rev = [], {}, {}
    D = [0] * (P + 1)  # D[p]: what the filled gaps before placement p add
    scratch = 0
    for p in range(P):
        D[p + 1] = D[p]
        if not (p + 1 < P and sof[p + 1] == sof[p]):
            continue
        badl, _, lenl, _ = unitig(p)
        badr, _, lenr, _ = unitig(p + 1)
        G = (lay[p + 1][2] - lay[p][2] - lenl) & M64
        cls, fwd, rv, dr, fill = None, NOT_RUN, NOT_RUN, 0, b""
        if badl or badr:
            cls = "MALFORMED"
        elif lenl < k or lenr < k:
            cls = "SHORT"
        else:
            tail, head = placed(p)[-k:], placed(p + 1)[:k]
            if any(c not in b"ACGT" for c in tail + head):
                cls = "NON_ACGT"
            elif G > max_fill:
                cls = "FAR"
            else:
                need = G + slack
                room = max_walk_bases is None or scratch + need <= max_walk_bases
                scratch += need
                if not room:
                    cls = "NO_ROOM"
                else:
                    limit = k + G + slack
                    out, t, app, steps = _walk(d, mc, tail, head, limit)
                    status[17] += steps
                    cls, f = _judge(out, t, app, k, slack, G)
                    fwd = C[cls]
                    if cls == "FILLED":
                        fill = f
                    elif cls in ("DEAD_END", "BRANCH", "TOO_LONG"):
                        out, t, app, steps = _walk(d, mc, revcomp(head), revcomp(tail), limit)
                        status[17] += steps
                        rcls, f = _judge(out, t, app, k, slack, G)
                        rv = C[rcls]
                        if rcls == "FILLED":
                            cls, dr, fill = "FILLED", 1, revcomp(f)
        g = len(gaps)
        status[1 + C[cls]] += 1
        if cls == "FILLED":
            status[12 + dr] += 1
            status[14] += len(fill)
            fills[g] = fill
            D[p + 1] = (D[p] + len(fill) - G) & M64
        else:
            status[15] = (status[15] + G) & M64
        gaps.append([sof[p], lay[p][0], lay[p + 1][0], min(G, 0xFFFFFFFF), len(fill), C[cls], fwd, rv, dr, p])
        walk_rev[p] = fill if cls == "FILLED" else None
    # the new tables
    head_of = [min(lay_offs[s], P) for s in range(S + 1)]
    new_off = [(lay[p][2] + D[p] - D[head_of[sof[p]]]) & M64 for p in range(P)]
    lens = []
    for s in range(S):
        h, e = head_of[s], head_of[s + 1]
        lens.append((new_off[e - 1] + unitig(e - 1)[2]) & M64 if e > h else 0)
    sc_offs = [0]
    for x in lens:
        sc_offs.append((sc_offs[-1] + x) & M64)
    for rec in gaps:
        p = rec[9]
        rec[9] = (new_off[p] + unitig(p)[2]) & M64
    total = sc_offs[S]
    status[0] = len(gaps)
    status[16] = total
    status[18] = status[17] * 8
    status[19] = None
    cap = total if sseqs_capacity is None else sseqs_capacity
    status[20] = 1 if total > cap else 0
    status[21] = 1 if status[1 + C["NO_ROOM"]] else 0
    status[22] = S
    seqs = None
    if not status[20]:
        parts = []
        for s in range(S):
            at = 0
            for p in range(head_of[s], head_of[s + 1]):
                assert new_off[p] >= at, "placements out of order: the bases of such tables are not restated"
                parts.append(b"N" * (new_off[p] - at))
                parts.append(placed(p))
                at = new_off[p] + len(parts[-1])
                if walk_rev.get(p) is not None:
                    parts.append(walk_rev[p])
                    at += len(walk_rev[p])
            assert at == lens[s]
        seqs = b"".join(parts)
    return {"status": status, "sc_offs": sc_offs, "sc_lay_offs": lay_offs[:S + 1], "sc_flags": [int(x) for x in scaf["sc_flags"]][:S],
            "layout": [(lay[p][0], lay[p][1], new_off[p]) for p in range(P)], "seqs": seqs, "gaps": [tuple(r) for r in gaps], "fills": fills}


def render(exp, seq_offs):
    """the FASTA, layout and gap texts `siga unitig --scaffold --gapfill --gaps` writes for expected_gapfill's dict; seq_offs: the
    unitig call's"""
    name = lambda c: "NOT_RUN" if c == NOT_RUN else CLASSES[c]
    fa, lay, gp = [], [], []
    filled = [0] * exp["status"][22]
    for g in exp["gaps"]:
        filled[g[0]] += g[5] == C["FILLED"]
        gp.append("GP\tscaffold-%d\tunitig-%d\tunitig-%d\t%d\t%s\t%s\t%s\t%s\t%d\t%d\n" % (
            g[0], g[1], g[2], g[3], name(g[5]), name(g[6]), name(g[7]), "-" if g[8] else "+", g[4], g[9]))
    for s in range(exp["status"][22]):
        a, b = exp["sc_lay_offs"][s], exp["sc_lay_offs"][s + 1]
        head = ">scaffold-%d unitigs=%d gaps=%d" % (s, b - a, b - a - 1)
        if exp["sc_flags"][s] & 1:
            head += " circular=%d" % (exp["sc_flags"][s] >> 1)
        head += " filled=%d" % filled[s]
        fa.append(head + "\n" + exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]].decode("latin-1") + "\n")
        for p in range(a, b):
            u, fl, off = exp["layout"][p]
            before = 0
            if p > a:
                v, _, voff = exp["layout"][p - 1]
                before = off - voff - (seq_offs[v + 1] - seq_offs[v])
            lay.append("scaffold-%d\tunitig-%d\t%s\t%d\t%d\n" % (s, u, "-" if fl & REV else "+", off, before))
    return "".join(fa), "".join(lay), "".join(gp)


# ---- genomes and reads ---------------------------------------------------------------------------------------------------------------
def read_len(k):
    return max(60, k + 20)


@functools.lru_cache(maxsize=None)
def genome(k, seed, size):
    rng = random.Random(seed * 1000 + k)
    return bytes(rng.choice(b"ACGT") for _ in range(size))


def tile(g, k, seed, step=4, depth=3, minus=None, drop=None, n_at=None):
    """reads of read_len(k) bases every `step` bases of g, `depth` copies each, every copy on a random strand.
    minus = (a, b): the reads that touch g[a:b] all lie on the minus strand; drop = x: no read holds g[x]; n_at = x: every read
    that holds g[x] has N there."""
    rng = random.Random(seed)
    rl = read_len(k)
    starts = list(range(0, len(g) - rl + 1, step))
    if starts[-1] != len(g) - rl:
        starts.append(len(g) - rl)
    reads = []
    for s in starts:
        if drop is not None and s <= drop < s + rl:
            continue
        r = g[s:s + rl]
        if n_at is not None and s <= n_at < s + rl:
            r = r[:n_at - s] + b"N" + r[n_at - s + 1:]
        for _ in range(depth):
            rev = rng.random() < 0.5
            if minus is not None and s < minus[1] and s + rl > minus[0]:
                rev = True
            reads.append(revcomp(r) if rev else r)
    return reads


def fork_reads(g, k, at, copies, seed, into=False, base=None):
    """`copies` reads that leave the genome at g[at] for a base the genome does not have there and go on at random (into: that
    arrive from random bases and join the genome behind g[at - 1]); base: the odd base, when it must be a given one"""
    rng = random.Random(seed)
    rl = read_len(k)
    half = rl - k // 2 - 1 if rl - k // 2 - 1 >= k - 1 else k - 1
    rest = rl - half - 1
    if into:
        odd = base or rng.choice([b for b in b"ACGT" if b != g[at - 1]])
        r = bytes(rng.choice(b"ACGT") for _ in range(rest)) + bytes([odd]) + g[at:at + half]
    else:
        odd = base or rng.choice([b for b in b"ACGT" if b != g[at]])
        r = g[at - half:at] + bytes([odd]) + bytes(rng.choice(b"ACGT") for _ in range(rest))
    return [revcomp(r) if rng.random() < 0.5 else r for _ in range(copies)]


# ---- tables over pieces of a genome ------------------------------------------------------------------------------------------------
def tables(g, scaffolds, seed=0, flags=None):
    """scaffolds: per scaffold a list of pieces (a, b, placed reversed, G: the gap laid BEHIND the piece, None after the last).
    Unitig ids are shuffled.  -> (res, scaf, truth): truth[gap number] = the genome between the two pieces, None when they overlap"""
    rng = random.Random(seed)
    pieces = [pc for sc in scaffolds for pc in sc]
    ids = list(range(len(pieces)))
    rng.shuffle(ids)
    by_id = sorted(range(len(pieces)), key=lambda i: ids[i])
    so, useqs = [0], []
    for i in by_id:
        a, b, rev, _ = pieces[i]
        useqs.append(revcomp(g[a:b]) if rev else g[a:b])
        so.append(so[-1] + b - a)
    lay, lay_offs, truth = [], [0], []
    i = 0
    for sc in scaffolds:
        off = 0
        for j, (a, b, rev, G) in enumerate(sc):
            lay.append((ids[i], REV if rev else 0, off))
            off += (b - a) + (G or 0)
            if j + 1 < len(sc):
                nxt = sc[j + 1][0]
                truth.append(g[b:nxt] if nxt >= b else None)
            i += 1
        lay_offs.append(len(lay))
    res = {"seq_offs": so, "useqs": b"".join(useqs)}
    scaf = {"sc_lay_offs": lay_offs, "sc_flags": list(flags) if flags else [0] * len(scaffolds), "layout": lay}
    return res, scaf, truth


def case(name, k, g, reads, scaffolds, opts=None, flags=None, seed=0, reads_key=None, **extra):
    res, scaf, truth = tables(g, scaffolds, seed, flags)
    c = {"name": "%s_k%d" % (name, k), "kind": name, "k": k, "genome": g, "reads": reads, "reads_key": reads_key or ("%s_k%d" % (name, k)), "res": res,
         "scaf": scaf, "truth": truth, "opts": dict(DEFAULT_OPTS, k=k, **(opts or {})), "max_walk_bases": None}
    c.update(extra)
    return c


@functools.lru_cache(maxsize=None)
def clean(k):
    """-> (genome of 3 kb, its tiling): what every case without a special read set shares, so that one index serves them"""
    g = genome(k, 1, 3000)
    return g, tuple(tile(g, k, seed=k))


def hand_built(k):
    """the cases of one k, by name"""
    g, reads = clean(k)
    key = "clean_k%d" % k
    out = []

    def add(name, scaffolds, opts=None, rd=None, rkey=None, **kw):
        out.append(case(name, k, g, reads if rd is None else tuple(rd), scaffolds, opts, reads_key=key if rd is None else rkey or "%s_k%d" % (name, k),
                        seed=len(out) + k, **kw))

    n, f = 2 * k + 40, 37  # a piece's bases, the usual fill
    a0 = 200
    two = lambda rl, rr, fill=f, G=None, a=a0: [[(a, a + n, rl, fill + 5 if G is None else G), (a + n + fill, a + 2 * n + fill, rr, None)]]
    add("plain", two(False, False))
    add("right_reversed", two(False, True))
    add("left_reversed", two(True, False))
    add("both_reversed", two(True, True))
    three = [(a0, a0 + n, False, 30), (a0 + n + 25, a0 + 2 * n + 25, True, 9), (a0 + 2 * n + 36, a0 + 3 * n + 36, False, 60),
             (a0 + 3 * n + 36 + 44, a0 + 4 * n + 36 + 44, True, None)]
    add("three_gaps", [three])
    b0 = a0 + 4 * n + 200
    add("circular_and_single", [[(b0, b0 + n, False, None)], [(a0, a0 + n, False, 20), (a0 + n + 22, a0 + 2 * n + 22, True, None)],
                                [(b0 + n + 50, b0 + 2 * n + 50, True, None)]], flags=[0, 1 | (17 << 1), 0])
    for fill in (0, 1, k - 1, k, k + 1):
        add("fill_%s" % {0: "0", 1: "1", k - 1: "k_minus_1", k: "k", k + 1: "k_plus_1"}[fill], two(False, fill % 2 == 1, fill, G=max(1, fill)))
    sl, ff = 7, 30
    for nm, G in (("g_at_fill_minus_slack_minus_1", ff - sl - 1), ("g_at_fill_minus_slack", ff - sl), ("g_at_fill_plus_slack", ff + sl),
                  ("g_at_fill_plus_slack_plus_1", ff + sl + 1)):
        add(nm, two(False, False, ff, G=G), {"slack": sl})
    for ov in (1, k - 1):
        add("overlap_%s" % ("1" if ov == 1 else "k_minus_1"), [[(a0, a0 + n, False, 1), (a0 + n - ov, a0 + 2 * n - ov, ov == 1, None)]])
    add("unitig_of_k", [[(a0, a0 + k, False, 12), (a0 + k + 10, a0 + 2 * k + 10, False, 3), (a0 + 2 * k + 14, a0 + 2 * k + 14 + n, True, None)]])
    add("unitig_of_k_minus_1", [[(a0, a0 + n, False, 12), (a0 + n + 10, a0 + n + 10 + k - 1, False, 3), (a0 + n + k + 12, a0 + 2 * n + k + 12, False, None)]])
    add("far", two(False, False, f, G=f + 1), {"max_fill": f})
    add("far_not", two(False, False, f, G=f), {"max_fill": f})
    # N in an anchor: the last byte but two of L as placed
    sc = two(False, True)
    c = case("n_in_anchor", k, g, reads, sc, reads_key=key, seed=3)
    u = c["scaf"]["layout"][0][0]
    at = c["res"]["seq_offs"][u + 1] - 3
    c["res"]["useqs"] = c["res"]["useqs"][:at] + b"N" + c["res"]["useqs"][at + 1:]
    out.append(c)
    c = case("lower_case_in_anchor", k, g, reads, two(False, False), reads_key=key, seed=4)
    u = c["scaf"]["layout"][1][0]
    at = c["res"]["seq_offs"][u] + k - 1
    c["res"]["useqs"] = c["res"]["useqs"][:at] + c["res"]["useqs"][at:at + 1].lower() + c["res"]["useqs"][at + 1:]
    out.append(c)
    # the reads themselves
    mid = a0 + n + f // 2
    add("n_in_reads", two(False, False), rd=tile(g, k, seed=k, n_at=mid))
    add("coverage_hole", two(False, True), rd=tile(g, k, seed=k, drop=mid))
    add("minus_strand_only", two(False, False), rd=tile(g, k, seed=k, minus=(a0 + n - k, a0 + n + f + k)))
    end_l, start_r = a0 + n, a0 + n + f
    for nm, rl, rr in (("", False, False), ("_left_reversed", True, False), ("_both_reversed", True, True)):
        add("fork_at_min_count" + nm, two(rl, rr), rd=list(reads) + fork_reads(g, k, end_l, 3, seed=k), rkey="fork3_k%d" % k)
    add("fork_below_min_count", two(False, False), rd=list(reads) + fork_reads(g, k, end_l, 2, seed=k))
    add("forks_at_both_ends", two(False, True), rd=list(reads) + fork_reads(g, k, end_l, 3, seed=k) + fork_reads(g, k, start_r, 4, seed=k + 1, into=True))
    if k % 2 == 0:
        # L ends in a reverse palindrome less its last base; two reads carry that base: 2 occurrences, counted twice
        gp = bytearray(g)
        h = bytes(random.Random(k).choice(b"ACGT") for _ in range(k // 2))
        pal = h + revcomp(h)
        odd = pal[-1]
        gp[end_l - (k - 1):end_l] = pal[:-1]
        if gp[end_l] == odd:
            gp[end_l] = next(b for b in b"ACGT" if b != odd)
        gp = bytes(gp)
        rd = tile(gp, k, seed=k)
        for copies, nm in ((2, "palindrome_doubled_crosses"), (1, "palindrome_doubled_below")):
            out.append(case(nm, k, gp, tuple(rd + fork_reads(gp, k, end_l, copies, seed=k, base=odd)), two(False, False), seed=5))
    # scratch and capacity
    add("scratch_one_byte_short", [three], short_scratch=1)
    add("scratch_exact", [three], short_scratch=0)
    return out


@functools.lru_cache(maxsize=None)
def many_gaps(count, k=15):
    """`count` gaps in one scaffold and a second scaffold behind it: pieces of k + 1 .. k + 8 bases, fills of 0 .. 6"""
    rng = random.Random(count)
    at, pieces = 50, []
    for i in range(count + 1):
        ln, fill = k + 1 + rng.randrange(8), rng.randrange(7)
        pieces.append((at, at + ln, rng.random() < 0.5, max(1, fill + rng.randrange(-2, 3)) if i < count else None))
        at += ln + fill
    g = genome(k, 100 + count, at + 400)
    tail = [(at + 100, at + 100 + 2 * k, False, 5), (at + 100 + 2 * k + 9, at + 100 + 4 * k + 9, True, None)]
    return case("gaps_%d" % count, k, g, tuple(tile(g, k, seed=count)), [pieces, tail], {"slack": 10})


@functools.lru_cache(maxsize=None)
def long_fill(k):
    """two gaps of 5000 true bases laid as 4950 (max_fill 10000, slack 100): the first filled forward; at the second a fork of
    min_count reads at the forward start, so that only the reverse walk fills it.  A walk writes, and the bases pass copies, a fill
    over hundreds of 16-byte pieces"""
    n, f = 2 * k + 40, 5000
    a0 = 200
    g = genome(k, 9, a0 + 3 * n + 2 * f + 400)
    b1, b2 = a0 + n + f, a0 + 2 * n + 2 * f
    reads = tuple(tile(g, k, seed=50 + k, step=10) + fork_reads(g, k, b1 + n, 3, seed=k))
    return case("long_fill", k, g, reads, [[(a0, a0 + n, False, f - 50), (b1, b1 + n, True, f - 50), (b2, b2 + n, False, None)]], seed=k)


def random_case(seed):
    rng = random.Random(seed)
    k = rng.choice(KS)
    size = rng.randrange(1000, 3001)
    g = genome(k, 1000 + seed, size)
    reads = tile(g, k, seed=seed, step=rng.choice((3, 4, 5)), drop=rng.randrange(size) if rng.random() < 0.3 else None,
                 n_at=rng.randrange(size) if rng.random() < 0.2 else None)
    scaffolds, at = [], rng.randrange(0, 40)
    while True:
        sc = []
        for j in range(rng.choice((1, 2, 2, 3, 4))):
            ln = rng.choice((k - 1, k, k + 1, k + rng.randrange(2, 60), 2 * k + rng.randrange(40)))
            if at + ln > size:
                break
            fill = rng.choice((0, 1, rng.randrange(2, 25), rng.randrange(2, 90), -rng.randrange(1, k)))
            G = max(1, fill + rng.choice((0, 0, 1, -3, 7, rng.randrange(-30, 30), 60)))
            sc.append([at, at + ln, rng.random() < 0.5, G])
            at = max(at + ln + fill, at + 1)
        if not sc:
            break
        sc[-1][3] = None
        scaffolds.append([tuple(p) for p in sc])
        at += rng.randrange(0, 30)
    for sc in scaffolds:  # now and then a fork out of a piece's end or into a piece's start
        for a, b, _, G in sc:
            if G is not None and rng.random() < 0.25 and read_len(k) <= b <= size - read_len(k):
                reads += fork_reads(g, k, b, rng.choice((2, 3, 4)), seed=seed + b)
            if rng.random() < 0.1 and read_len(k) <= a <= size - read_len(k):
                reads += fork_reads(g, k, a, rng.choice((2, 3)), seed=seed + a, into=True)
    opts = {"slack": rng.choice((0, 5, 20, 100)), "max_fill": rng.choice((40, 200, 10000)), "min_count": rng.choice((1, 2, 3, 3, 4))}
    return case("random_%d" % seed, k, g, tuple(reads), scaffolds, opts, seed=seed)


@functools.lru_cache(maxsize=None)
def all_cases():
    out = [c for k in KS for c in hand_built(k)]
    out += [many_gaps(70, 15), many_gaps(300, 15), many_gaps(70, 31)]
    out += [long_fill(31), long_fill(128)]
    out += [random_case(s) for s in range(100)]
    return out


def case_expected(c, **kw):
    """expected_gapfill of a case; short_scratch: the walk scratch that many bytes below what the case's gaps need"""
    mw = c.get("max_walk_bases")
    if c.get("short_scratch") is not None and "max_walk_bases" not in kw:
        mw = scratch_needed(c) - c["short_scratch"]
    kw.setdefault("max_walk_bases", mw)
    return expected_gapfill(c["reads"], c["res"], c["scaf"], c["opts"], **kw)


def scratch_needed(c):
    """the bytes of walk scratch with which no gap of the case is NO_ROOM: G + slack over the gaps that come to a walk"""
    exp = expected_gapfill(c["reads"], c["res"], c["scaf"], c["opts"])
    walked = [g for g in exp["gaps"] if g[6] != NOT_RUN]
    return sum(g[3] + c["opts"]["slack"] for g in walked)
