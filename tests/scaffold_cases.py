"""Cases and the serial restatement for `siga unitig --scaffold` (csrc/sigax_scaffold.hip); no tests here
(tests/test_scaffold_cases.py, tests/test_gpu_scaffold.py).

expected_scaffolds()  the rules of include/sigax.h (the `--scaffold` block), serially, with Python integers: every link is
                      classed, the degrees are counted, and every scaffold is walked unitig by unitig from its first one.
A unitig end is 2 * unitig + end, B = 0, E = 1.  A link is (a, b, count, min_span, sum_span)."""
import functools
import random

import numpy as np

from tests import unitig_cases as uc

B, E = 0, 1
M64 = (1 << 64) - 1
REV = uc.PLACED_REV
DEFAULT_OPTS = {"insert_size": None, "min_pairs": 2, "link_ratio": 0, "min_unitig_bases": 0, "min_gap": 1, "max_gap": 1000000}
CLASSES = ("MALFORMED", "SELF", "CIRCULAR", "SHORT", "THIN")  # status entries 3 .. 7, in precedence order


def insert_from_status(status24):
    return int(status24[15]) // int(status24[14]) if int(status24[14]) else 0


def link_class(link, nu, seq_offs, uflags, o):
    """the first class that applies, or "CANDIDATE" """
    a, b, count = link[0], link[1], link[2]
    if a >= 2 * nu or b >= 2 * nu or a >= b or count == 0:
        return "MALFORMED"
    ua, ub = a >> 1, b >> 1
    if ua == ub:
        return "SELF"
    if (uflags[ua] | uflags[ub]) & uc.CIRCULAR:
        return "CIRCULAR"
    if any(((seq_offs[u + 1] - seq_offs[u]) & M64) < o["min_unitig_bases"] for u in (ua, ub)):
        return "SHORT"
    if count < o["min_pairs"]:
        return "THIN"
    return "CANDIDATE"


def gap_of(link, ins, o):
    """-> (gap, estimate below min_gap, clamped at max_gap)"""
    m = link[4] // link[2]
    if m >= ins:
        return o["min_gap"], True, False
    g = ins - m
    if g < o["min_gap"]:
        return o["min_gap"], True, False
    if g > o["max_gap"]:
        return o["max_gap"], False, True
    return g, False, False


def _plain(links):
    if hasattr(links, "tolist"):
        links = links.tolist()
    return [tuple(int(x) for x in r) for r in links]


def expected_scaffolds(res, links, status24, opts=None, n_unitigs=None, n_links=None, sseqs_capacity=None):
    """res: seq_offs, uflags and (for the bases) useqs of a unitig call; links and status24 of the pairs call; opts over
    DEFAULT_OPTS (insert_size None: from status24); n_unitigs, n_links: the counts the device form is given, when they are not
    len(uflags) and len(links) (the capacities); sseqs_capacity: the room for the bases (None: exactly enough)
    -> dict(sc_offs, sc_lay_offs, sc_flags, layout [(unitig, flags, offset)], gaps [gap before each placement], seqs bytes or None,
    status [16], joins {end: (end, gap)})"""
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    seq_offs = [int(x) for x in res["seq_offs"]]
    uflags = [int(x) for x in res["uflags"]]
    links = _plain(links)
    nu = min(len(uflags) if n_unitigs is None else n_unitigs, len(uflags))
    nl = min(len(links) if n_links is None else n_links, len(links))
    links = links[:nl]
    ins = insert_from_status(status24) if o["insert_size"] is None else o["insert_size"]
    bases = [(seq_offs[u + 1] - seq_offs[u]) & M64 for u in range(nu)]
    st = [0] * 16
    st[2] = nl
    cand = []
    for ln in links:
        c = link_class(ln, nu, seq_offs, uflags, o)
        if c == "CANDIDATE":
            cand.append(ln)
        else:
            st[3 + CLASSES.index(c)] += 1
    best = {}
    for a, b, count, _, _ in cand:
        best[a] = max(best.get(a, 0), count)
        best[b] = max(best.get(b, 0), count)
    strong = []
    for ln in cand:
        a, b, count = ln[:3]
        if o["link_ratio"] > 0 and (count * o["link_ratio"] <= best[a] or count * o["link_ratio"] <= best[b]):
            st[8] += 1
        else:
            strong.append(ln)
    deg = {}
    for a, b, _, _, _ in strong:
        deg[a] = deg.get(a, 0) + 1
        deg[b] = deg.get(b, 0) + 1
    joins = {}
    for ln in strong:
        a, b = ln[:2]
        if deg[a] == 1 and deg[b] == 1:
            g, below, clamped = gap_of(ln, ins, o)
            joins[a], joins[b] = (b, g), (a, g)
            st[13] += below
            st[14] += clamped
        else:
            st[9] += 1
    # the walks: every unitig once, from the smallest id of its component.  A path is [(unitig, the end it is left through)]
    # with the gaps between neighbours; a unitig left through E was entered through B and lies forward.
    def walk(state):
        """from `state` along the joins -> [(unitig, end it is entered through, gap before it)], and whether it came back"""
        out, start = [], state >> 1
        while state in joins:
            nxt, g = joins[state]
            if nxt >> 1 == start:
                return out, g
            out.append((nxt >> 1, nxt & 1, g))
            seen[nxt >> 1] = True
            state = nxt ^ 1
        return out, None

    seen = [False] * nu
    scaffolds = []  # (first unitig, flag, [(unitig, rev, gap before)])
    for u in range(nu):
        if seen[u]:
            continue
        seen[u] = True
        right, closing = walk(2 * u + E)
        path = [(u, E)] + [(x, p ^ 1) for x, p, _ in right]
        between = [g for _, _, g in right]
        flag = 0
        if closing is not None:
            flag = 1 | (closing << 1)
        else:
            left, _ = walk(2 * u + B)
            path = [(x, p) for x, p, _ in reversed(left)] + path
            between = [g for _, _, g in reversed(left)] + between
            if path[-1][0] < path[0][0]:  # a path starts at its terminal of smaller id
                path = [(x, e ^ 1) for x, e in reversed(path)]
                between = between[::-1]
        chain = [(x, e == B, between[i - 1] if i else 0) for i, (x, e) in enumerate(path)]
        scaffolds.append((chain[0][0], flag, chain))
    scaffolds.sort(key=lambda s: s[0])
    useqs = res.get("useqs") if hasattr(res, "get") else None
    if useqs is not None:
        useqs = bytes(np.ascontiguousarray(useqs, dtype=np.uint8)) if not isinstance(useqs, (bytes, bytearray)) else bytes(useqs)
    sc_offs, sc_lay_offs, sc_flags, layout, gaps, parts = [0], [0], [], [], [], []
    for _, flag, chain in scaffolds:
        off = 0
        for i, (x, rev, g) in enumerate(chain):
            if i:
                off = (off + g) & M64
                st[12] += g
                st[10] += 1
                parts.append(b"N" * g if useqs is not None else b"")
            layout.append((x, REV if rev else 0, off))
            gaps.append(g if i else 0)
            if useqs is not None:
                s = useqs[seq_offs[x]:seq_offs[x + 1]]
                parts.append(uc.revcomp(s) if rev else s)
            off = (off + bases[x]) & M64
        sc_offs.append((sc_offs[-1] + off) & M64)
        sc_lay_offs.append(len(layout))
        sc_flags.append(flag)
        st[11] += flag & 1
    st[0], st[1] = len(scaffolds), sc_offs[-1]
    st[15] = int(sseqs_capacity is not None and st[1] > sseqs_capacity)
    return {"sc_offs": sc_offs, "sc_lay_offs": sc_lay_offs, "sc_flags": sc_flags, "layout": layout, "gaps": gaps,
            "seqs": b"".join(parts) if useqs is not None else None, "status": st, "joins": joins}


# ---- hand-built inputs ----
def make_res(lens, circular=(), seed=0, alphabet=b"ACGT"):
    """unitigs of the given lengths over random bases -> the dict a unitig call returns, as far as the scaffold call reads it"""
    rng = random.Random(seed)
    seq_offs = [0]
    for n in lens:
        seq_offs.append(seq_offs[-1] + n)
    useqs = bytes(rng.choice(alphabet) for _ in range(seq_offs[-1]))
    return {"seq_offs": seq_offs, "uflags": [uc.CIRCULAR if u in circular else 0 for u in range(len(lens))], "useqs": useqs}


def link(a, b, count=5, span=100):
    """a link of `count` pairs whose mean span is `span`"""
    a, b = min(a, b), max(a, b)
    return (a, b, count, span, span * count)


def path_links(order, rev, count=5, spans=None):
    """the links that join the unitigs `order` in that order, unitig order[i] lying reversed where rev[i]"""
    out = []
    for i in range(len(order) - 1):
        x, y = order[i], order[i + 1]
        out.append(link(2 * x + (B if rev[i] else E), 2 * y + (E if rev[i + 1] else B), count, spans[i] if spans else 100))
    return out


def cycle_links(order, rev, count=5, span=100):
    x, y = order[-1], order[0]
    return path_links(order, rev, count) + [link(2 * x + (B if rev[-1] else E), 2 * y + (E if rev[0] else B), count, span)]


def shuffled_chain(n, seed, lens=None):
    """n unitigs in one path, ids shuffled and strands mixed -> (res, links, order, rev)"""
    rng = random.Random(seed)
    order = list(range(n))
    rng.shuffle(order)
    rev = [rng.random() < 0.5 for _ in range(n)]
    lens = lens or [rng.randint(1, 40) for _ in range(n)]
    links = path_links(order, rev, spans=[rng.randint(60, 99) for _ in range(n - 1)])
    rng.shuffle(links)
    return make_res(lens, seed=seed), links, order, rev


@functools.lru_cache(maxsize=None)
def hand_built():
    """[(name, res, links, opts)] with insert_size given"""
    cases = []
    o = {"insert_size": 120}
    # the bases pass: unitigs of 1, 15, 16, 17 and 33 bases, gaps of 1, 15, 16 and 17, strands mixed
    lens = [1, 15, 16, 17, 33, 40, 5]
    gaps = [1, 15, 16, 17, 3, 2]
    cases.append(("sizes_forward", make_res(lens, seed=1), path_links(range(7), [False] * 7, spans=[120 - g for g in gaps]), o))
    cases.append(("sizes_mixed", make_res(lens, seed=2), path_links(range(7), [False, True, False, True, True, False, True], spans=[120 - g for g in gaps]), o))
    # a piece that holds the end of one unitig, a whole gap and the start of the next: 20 + 3 + 20, pieces at 16 and 32
    cases.append(("gap_in_a_piece", make_res([20, 20, 9], seed=3), path_links([0, 1, 2], [False, True, False], spans=[117, 119]), o))
    # a reversed unitig whose source start is not 16-byte aligned (it lies behind 7 bases), long enough for whole pieces
    cases.append(("reversed_unaligned", make_res([7, 70, 50], seed=4), path_links([0, 1, 2], [False, True, True], spans=[110, 104]), o))
    # non-ACGT bytes, placed reversed
    cases.append(("non_acgt_reversed", make_res([40, 45], seed=5, alphabet=b"ACGTNRYacgt"), path_links([0, 1], [False, True]), o))
    cases.append(("one_unitig", make_res([37], seed=6), [], o))
    # rings
    cases.append(("cycle3", make_res([30, 31, 32], seed=7), cycle_links([0, 2, 1], [False, True, False], span=90), o))
    rng = random.Random(70)
    order = list(range(70))
    rng.shuffle(order)
    cases.append(("cycle70", make_res([rng.randint(5, 30) for _ in range(70)], seed=8), cycle_links(order, [rng.random() < 0.5 for _ in range(70)]), o))
    # a cycle next to a path, and a circular unitig given links anyway
    cases.append(("cycle_and_path", make_res([20] * 7, seed=9), cycle_links([1, 4, 2], [True, False, False]) + path_links([6, 0, 3, 5], [True, True, False, False]), o))
    cases.append(("circular_unitig", make_res([30, 40, 50], circular=(1,), seed=10), [link(1, 2), link(3, 4), link(1, 4)], o))
    # a path whose smaller terminal is at the far end of the walk from its smallest id
    cases.append(("turned", make_res([10, 20, 30, 40], seed=11), path_links([3, 0, 2, 1], [False, False, True, False]), o))
    return cases


def case_named(name):
    return next(c for c in hand_built() if c[0] == name)


# ---- seeded random inputs ----
@functools.lru_cache(maxsize=None)
def random_links_case(seed):
    """up to 14 unitigs and random links over them: every class, keys given twice, hostile records -> (res, links, status24, opts)"""
    rng = random.Random(90000 + seed)
    nu = rng.randint(1, 14)
    circ = tuple(u for u in range(nu) if rng.random() < 0.1)
    res = make_res([rng.randint(1, 60) for _ in range(nu)], circular=circ, seed=seed)
    links = []
    for _ in range(rng.randint(0, 2 * nu)):
        a, b = rng.randrange(2 * nu + 2), rng.randrange(2 * nu + 2)
        if rng.random() < 0.9:
            a, b = min(a, b), max(a, b)
        count = rng.choice((0, 1, 1, 2, 3, 5, 9))
        links.append((a, b, count, rng.randint(10, 90), rng.randint(10, 200) * max(count, 1)))
    if links and rng.random() < 0.3:
        links.append(rng.choice(links))
    status24 = [0] * 24
    status24[14], status24[15] = rng.choice((0, 3, 7)), rng.randint(300, 1200)
    opts = {"insert_size": rng.choice((None, 0, 100, 150)), "min_pairs": rng.choice((1, 2, 3)), "link_ratio": rng.choice((0, 0, 1, 2, 3)),
            "min_unitig_bases": rng.choice((0, 0, 10, 30)), "min_gap": rng.choice((1, 1, 5)), "max_gap": rng.choice((5, 40, 1000000))}
    return res, links, status24, opts


def pipeline_options(seed):
    """the options of the random graphs that come through the unitig call and the pairs call, varied by seed"""
    return {"insert_size": (None, 150, 400, 90)[seed % 4], "min_pairs": (1, 1, 2)[seed % 3], "link_ratio": (0, 2, 1, 0, 3)[seed % 5],
            "min_unitig_bases": (0, 0, 0, 70)[(seed // 2) % 4], "min_gap": (1, 3)[seed % 2], "max_gap": (1000000, 60)[(seed // 3) % 2]}


def pipeline_extra_links(seed, nu, links):
    """what no pairs call gives, planted behind its links by seed: a link between the two ends of one unitig, a key twice"""
    extra = []
    if nu and seed % 4 == 0:
        u = seed % nu
        extra.append((2 * u, 2 * u + 1, 1 + seed % 2, 50, 50 * (1 + seed % 2)))
    if links and seed % 5 == 0:
        extra.append(tuple(links[0]))
    return extra


def render(exp):
    """the FASTA and layout texts `siga unitig --scaffold` writes for expected_scaffolds' dict"""
    fa, lay = [], []
    for s in range(exp["status"][0]):
        a, b = exp["sc_lay_offs"][s], exp["sc_lay_offs"][s + 1]
        head = ">scaffold-%d unitigs=%d gaps=%d" % (s, b - a, b - a - 1)
        if exp["sc_flags"][s] & 1:
            head += " circular=%d" % (exp["sc_flags"][s] >> 1)
        fa.append(head + "\n" + exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]].decode("latin-1") + "\n")
        for p in range(a, b):
            u, fl, off = exp["layout"][p]
            lay.append("scaffold-%d\tunitig-%d\t%s\t%d\t%d\n" % (s, u, "-" if fl & REV else "+", off, exp["gaps"][p]))
    return "".join(fa), "".join(lay)
