"""Containment records of `siga overlap -e` (rule 9 of the block of overlaps with mismatches in include/sigax.h,
SIGAX_MMO_CONTAINMENTS) restated serially on top of tests/mmoverlap_cases.py and tests/pileup_cases.py, and the cases of
tests/test_contained_cases.py and tests/test_gpu_contained.py.  No tests here.

expected_containments()  rule 9 over the seeds' candidates -> (sorted records, records written: what status[7] gains)
brute_containments()     the same over every read, strand and diagonal, without seeds -> sorted records
containment_lines()      the file `siga overlap -e --containments FILE` writes
placed_text()            the bases a record says the container holds under the contained read, as the contained read reads them
expected_placement()     the placement pass (sigax_contained_place_*), rules 1 to 6 with a plain walk, no doubling
A record is the tuple (query = contained, target = container, length = len(contained), af = 8 | 4 if reversed, num_diff, reserved = o).
"""
from tests import mmoverlap_cases as mc
from tests import pileup_cases as pc
from tests import unitig_cases as uc

CONTAINMENT = 8  # SIGAX_MM_CONTAINMENT


def _record(refs, ranks, i, cand, ell, L, m):
    """rule 9 for one accepted candidate of read i, or None for a dovetail"""
    t, strand, d = cand
    n = len(refs[i])
    cls = mc.classify(n, L, d, ell)
    if cls in ("SUFFIX", "PREFIX"):
        return None
    if cls == "DUP":
        inner_is_q = ranks[i] > ranks[t]
    else:
        inner_is_q = cls == "Q_IN_T"
    af = CONTAINMENT | (4 if strand else 0)
    if inner_is_q:  # found from the contained read: o = d forward, L - d - n against the reverse complement
        return (i, t, n, af, m, (L - d - n) if strand else d)
    return (t, i, L, af, m, -d)  # found from the container, on either strand


def _ordered(records):
    """each (query, target, af, length, reserved) once, ascending"""
    return sorted(set(records), key=lambda r: (r[0], r[1], r[3], r[2], r[5]))


def expected_containments(refs, name_rank, p, first=0, count=None):
    """rules 1-5 and 9 with reads first .. first + count as queries -> (records, the number written before repeats are dropped)"""
    count = len(refs) - first if count is None else count
    records = []
    for i in range(first, first + count):
        q = refs[i]
        if len(q) < p["S"] or len(q) > min(p["max_len"], pc.PILE_MAX_LEN):
            continue
        cands = pc.seed_candidates(refs, q, p)[0]
        if len(cands) > p["K"]:
            continue
        for c in sorted(cands):
            if name_rank[c[0]] == name_rank[i]:
                continue
            x0, x1, text, m = pc.overlap_of(refs, q, c)
            ell = x1 - x0
            if ell < p["M"] or m > (ell * p["P"]) // 1000:
                continue
            rec = _record(refs, name_rank, i, c, ell, len(text), m)
            if rec is not None:
                records.append(rec)
    return _ordered(records), len(records)


def brute_containments(refs, name_rank, p):
    """every read against every read, strand and diagonal on which one of the two is covered whole -> records"""
    records = []
    texts = [(r, pc.revcomp(r)) for r in refs]
    for i, q in enumerate(refs):
        n = len(q)
        for t in range(len(refs)):
            if name_rank[t] == name_rank[i]:
                continue
            for strand in (0, 1):
                text = texts[t][strand]
                L = len(text)
                for d in range(-n + 1, L):
                    x0, x1 = max(0, -d), min(n, L - d)
                    ell = x1 - x0
                    if ell < p["M"] or (ell != n and ell != L):
                        continue
                    m = sum(1 for x in range(x0, x1) if q[x] != text[x + d])
                    if m <= (ell * p["P"]) // 1000:
                        records.append(_record(refs, name_rank, i, (t, strand, d), ell, L, m))
    return _ordered(records)


def placed_text(refs, rec):
    """the container's columns [o, o + length), reverse-complemented when the record says so: what the contained read faces"""
    _, t, length, af, _, o = rec
    piece = refs[t][o:o + length]
    return pc.revcomp(piece) if af & 4 else piece


def check_geometry(refs, rec):
    """what every record holds, whatever found it: the span lies in the container and differs from the contained read in exactly
    num_diff columns"""
    q, t, length, af, m, o = rec
    assert q != t and length == len(refs[q]) and af in (8, 12) and 0 <= o and o + length <= len(refs[t]), rec
    piece = placed_text(refs, rec)
    assert sum(1 for a, b in zip(refs[q], piece) if a != b) == m, rec


def containment_lines(names, records):
    return "".join("%s\t%s\t%d\t%s\t%d\n" % (names[q], names[t], o, "-" if af & 4 else "+", m) for q, t, _, af, m, o in records)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def hand_sets():
    """name -> (refs, names, params, records worked out by hand).  g = mmoverlap_cases.G; the container is g[100:180] or its
    reverse complement, so a piece g[a:b] covers the forward container's columns a - 100 .. b - 100 and the reversed
    container's columns 180 - b .. 180 - a"""
    g = mc.G
    P0 = mc.params(S=12, T=4, M=45, P=0, H=4096, K=4096)
    big, rbig = g[100:180], pc.revcomp(g[100:180])
    sets = {}
    sets["at_offset_0"] = ([g[100:160], big], ["b", "a"], P0, [(0, 1, 60, 8, 0, 0)])
    sets["flush_with_the_end"] = ([big, g[120:180]], ["a", "b"], P0, [(1, 0, 60, 8, 0, 20)])
    sets["reverse_in_forward"] = ([pc.revcomp(g[110:170]), big], ["b", "a"], P0, [(0, 1, 60, 12, 0, 10)])
    sets["forward_in_reverse"] = ([g[105:170], rbig], ["b", "a"], P0, [(0, 1, 65, 12, 0, 10)])  # columns 180 - 170 .. 180 - 105
    sets["reverse_in_reverse"] = ([pc.revcomp(g[105:170]), rbig], ["b", "a"], P0, [(0, 1, 65, 8, 0, 10)])
    # duplicates: the larger name is the contained one, at column 0, whichever read id it has
    sets["dup_forward"] = ([big, big], ["a", "b"], P0, [(1, 0, 80, 8, 0, 0)])
    sets["dup_reverse"] = ([big, rbig], ["b", "a"], P0, [(0, 1, 80, 12, 0, 0)])
    # two mismatches inside the contained read: floor(60 * 40 / 1000) = 2 accepts them and the record carries the count
    sets["two_mismatches"] = ([pc.mutate(g[110:170], [20, 41]), big], ["b", "a"], mc.params(S=12, T=4, M=45, P=40, H=4096, K=4096),
                              [(0, 1, 60, 8, 2, 10)])
    # a piece of a tandem repeat lies in its container on two diagonals: two records of one pair
    unit = pc.random_genome(25, 77)
    sets["two_diagonals"] = ([unit * 2, unit * 3 + "A"], ["b", "a"], P0, [(0, 1, 50, 8, 0, 0), (0, 1, 50, 8, 0, 25)])
    # three nested reads: the innermost lies in both of the others
    sets["nested"] = ([g[100:200], g[110:180], g[120:170]], ["a", "b", "c"], P0, [(1, 0, 70, 8, 0, 10), (2, 0, 50, 8, 0, 20), (2, 1, 50, 8, 0, 10)])
    return sets


def duplicate_chain(n=40, length=100, seed=9):
    """n reads of one length, each differing from the one before in one new column: at P = 10 (one mismatch in 100 columns) only
    neighbours are accepted, and with names ascending by id every read but the first is contained in the one before"""
    base = pc.random_genome(length, seed)
    refs, cur = [base], base
    for k in range(1, n):
        cur = pc.mutate(cur, [2 * k])
        refs.append(cur)
    names = ["d%03d" % k for k in range(n)]
    return refs, names, mc.params(S=12, T=4, M=45, P=10, H=4096, K=4096)


# ---- the placement pass (include/sigax.h, the block of sigax_contained_place_*) ------------------------------------------------------
NOT_CONTAINED, PLACED, NO_RECORD, NO_ROOT, ROOT_REMOVED, INVALID = range(6)
PLACED_CONTAINED = 2
MASK64 = (1 << 64) - 1


def _owner(lay_offs, nu, n, j):
    """the unitig placement j belongs to: the last u with lay_offs[u] <= j (by the bisection the device runs) if it holds j"""
    if nu == 0:
        return None
    lo, hi = 0, nu
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if lay_offs[mid] <= j:
            lo = mid
        else:
            hi = mid
    a, b = lay_offs[lo], lay_offs[lo + 1]
    return lo if a <= b <= n and a <= j < b else None


def expected_placement(res, lengths, contained, records, n_unitigs=None):
    """rules 1-6 with a plain walk along the choices -> dict(lay_offs, layout [(read, flags, offset)], place_class, status).
    res: seq_offs, lay_offs (one entry more than there are unitigs) and layout, padded with (2^32 - 1, 2^32 - 1, 2^64 - 1) to one
    entry a read where it is shorter; n_unitigs: what the device reads as the count, when it is not len(seq_offs) - 1"""
    n = len(lengths)
    so, lo = [int(x) for x in res["seq_offs"]], [int(x) for x in res["lay_offs"]]
    layout = [(int(r), int(f), int(o)) for r, f, o in res["layout"]]
    layout += [(0xFFFFFFFF, 0xFFFFFFFF, MASK64)] * (n - len(layout))
    max_u = min(len(so) - 1, n)
    nu = min(max_u if n_unitigs is None else n_unitigs, max_u)
    owner = [_owner(lo, nu, n, j) for j in range(n)]
    slot = {}
    for j in range(n):
        if owner[j] is not None and layout[j][0] < n:
            slot.setdefault(layout[j][0], j)
    # rules 1-2
    choice, invalid = {}, 0
    for q, t, _, af, m, o in records:
        if not (q < n and t < n and q != t and af & 8 and contained[q] and o + lengths[q] <= lengths[t]):
            invalid += 1
            continue
        key = (1 if contained[t] else 0, m, t, 1 if af & 4 else 0, o)
        if q not in choice or key < choice[q]:
            choice[q] = key
    cls, placed, longest = [NOT_CONTAINED] * n, {}, 0
    for c in range(n):
        if not contained[c]:
            continue
        if c not in choice:
            cls[c] = NO_RECORD
            continue
        # rule 3
        _, _, cur, v, o = choice[c]
        steps = 1
        while contained[cur] and cur in choice and steps <= n:
            _, _, q, v2, o2 = choice[cur]
            o, v = (o2 + lengths[cur] - o - lengths[c], v ^ 1) if v2 else (o2 + o, v)
            cur = q
            steps += 1
        if contained[cur]:
            cls[c] = NO_ROOT
            continue
        longest = max(longest, steps)
        # rule 4
        if cur not in slot:
            cls[c] = ROOT_REMOVED
            continue
        j = slot[cur]
        u, (_, fl, off) = owner[j], layout[j]
        v2 = fl & 1
        o, v = ((off + lengths[cur] - o - lengths[c]) & MASK64, v ^ 1) if v2 else ((off + o) & MASK64, v)
        U = (so[u + 1] - so[u]) & MASK64
        if o <= U and lengths[c] <= U - o:
            cls[c] = PLACED
            placed[c] = (u, o, v | PLACED_CONTAINED)
        else:
            cls[c] = INVALID
    # rule 5
    lay2, lo2 = [], [0]
    for u in range(nu):
        a, b = (lo[u], lo[u + 1]) if lo[u] <= lo[u + 1] <= n else (0, 0)
        rows = [(layout[j][2], 0, layout[j][0], layout[j][1]) for j in range(a, b) if owner[j] == u and not (layout[j][0] < n and cls[layout[j][0]] == PLACED)]
        rows += [(o, 1, c, fl) for c, (pu, o, fl) in placed.items() if pu == u]
        lay2 += [(r, fl, o) for o, _, r, fl in sorted(rows)]
        lo2.append(len(lay2))
    status = [sum(1 for c in contained if c), len(records), invalid, len(placed), sum(1 for k in cls if k in (NO_RECORD, NO_ROOT)),
              sum(1 for k in cls if k == ROOT_REMOVED), longest, len(lay2)]
    return {"lay_offs": lo2, "layout": lay2, "place_class": cls, "status": status}


def placed_bytes(reads, placement):
    """the bytes a placement lays over its unitig's columns [offset, offset + L)"""
    r, fl, _ = placement
    return uc.revcomp(reads[r]) if fl & 1 else bytes(reads[r])


def with_placement(res, exp):
    """the unitig call's dict with the pass's lay_offs and layout in place of its own"""
    out = dict(res)
    out["lay_offs"], out["layout"] = exp["lay_offs"], exp["layout"]
    return out


def single_unitig(root_len, root_rev=False, offset=0, U=None):
    """tables of one unitig that holds read 0 alone, and hidden unitigs of one read each for the n - 1 others"""
    def build(lengths):
        n = len(lengths)
        U0 = U if U is not None else offset + root_len
        so = [0, U0]
        for k in range(1, n):
            so.append(so[-1] + lengths[k])
        return {"seq_offs": so, "lay_offs": list(range(n + 1)), "layout": [(0, 1 if root_rev else 0, offset)] + [(k, 0, 0) for k in range(1, n)]}
    return build


def hand_placements():
    """name -> (lengths, contained, records, tables, want: read -> (unitig, flags, offset)).  Read 0 is the root of 80 bases at
    offset 7 of unitig 0 (of 100 columns); the records are the hand sets' geometry"""
    out = {}
    for name, rev, recs, want in (
            ("at_offset_0", False, [(1, 0, 60, 8, 0, 0)], {1: (0, 2, 7)}),
            ("flush_with_the_end", False, [(1, 0, 60, 8, 0, 20)], {1: (0, 2, 27)}),
            ("reverse_in_forward", False, [(1, 0, 60, 12, 0, 10)], {1: (0, 3, 17)}),
            ("forward_in_reverse", True, [(1, 0, 65, 8, 0, 10)], {1: (0, 3, 7 + 80 - 10 - 65)}),
            ("reverse_in_reverse", True, [(1, 0, 65, 12, 0, 10)], {1: (0, 2, 7 + 80 - 10 - 65)}),
            # read 2 lies in read 1 (reversed there), read 1 in the root: two steps
            ("two_steps", False, [(1, 0, 60, 12, 0, 10), (2, 1, 40, 8, 1, 5)], {1: (0, 3, 17), 2: (0, 3, 17 + 60 - 5 - 40)}),
            # read 2 lies in reads 0 (two mismatches), 3 (one) and 1 (none, but contained itself): a container that is placed
            # directly goes first, then the fewer mismatches win over the smaller id -- read 3, which is unitig 3 on its own
            ("fewest_mismatches", False, [(2, 0, 40, 8, 2, 3), (2, 3, 40, 8, 1, 0), (2, 1, 40, 8, 0, 5), (1, 0, 60, 8, 0, 10)],
             {1: (0, 2, 17), 2: (3, 2, 0)}),
    ):
        lengths = [80, 60 if recs[0][2] == 60 else 65, 40, 90][:max(max(r[0], r[1]) for r in recs) + 1]
        for q, _, ln, _, _, _ in recs:
            lengths[q] = ln
        contained = [0] + [1 if any(r[0] == k for r in recs) else 0 for k in range(1, len(lengths))]
        out[name] = (lengths, contained, recs, single_unitig(80, rev, 7, 100)(lengths), want)
    return out


def crowded_unitig(n_inner=70, seed=4):
    """one unitig of one read of 300 bases, reversed at offset 11 of 400 columns, with n_inner contained reads, more than a wave:
    most lie in the root, every fifth in the contained read before it -> (lengths, contained, records, tables)"""
    import random
    rng = random.Random(seed)
    lengths, recs = [300], []
    for k in range(1, n_inner + 1):
        if k % 5 == 0:  # in read k - 1, which is contained itself
            L = rng.randint(10, lengths[k - 1] - 1)
            recs.append((k, k - 1, L, 8 | (4 if rng.random() < 0.5 else 0), rng.randint(0, 2), rng.randint(0, lengths[k - 1] - L)))
        else:
            L = rng.randint(30, 120)
            recs.append((k, 0, L, 8 | (4 if rng.random() < 0.5 else 0), rng.randint(0, 2), rng.randint(0, 300 - L)))
        lengths.append(L)
    rng.shuffle(recs)
    return lengths, [0] + [1] * n_inner, recs, single_unitig(300, True, 11, 400)(lengths)


def tiled_unitigs(n_units=6, seed=8):
    """several short unitigs of three chain reads each (60 bases, 30 columns apart, alternating strands), every chain read with two
    contained reads and one of those with a read inside it; read ids shuffled; the contained reads are unitigs of their own
    behind the others -> (lengths, contained, records, tables)"""
    import random
    rng = random.Random(seed)
    n_chain = 3 * n_units
    n = n_chain * 4
    ids = list(range(n))
    rng.shuffle(ids)
    lengths, contained, recs = [0] * n, [0] * n, []
    so, lo, layout, nxt = [0], [0], [], n_chain
    for u in range(n_units):
        for k in range(3):
            r = ids[3 * u + k]
            lengths[r] = 60
            layout.append((r, (u + k) & 1, 30 * k))
            inner = []
            for _ in range(2):
                c = ids[nxt]
                nxt += 1
                lengths[c], contained[c] = rng.randint(20, 45), 1
                recs.append((c, r, lengths[c], 8 | (4 if rng.random() < 0.5 else 0), 0, rng.randint(0, 60 - lengths[c])))
                inner.append(c)
            c = ids[nxt]
            nxt += 1
            lengths[c], contained[c] = rng.randint(8, 19), 1
            recs.append((c, inner[0], lengths[c], 8 | (4 if rng.random() < 0.5 else 0), 1, rng.randint(0, lengths[inner[0]] - lengths[c])))
        so.append(so[-1] + 120)
        lo.append(len(layout))
    for c in sorted(ids[n_chain:]):  # the hidden unitigs, by first read
        layout.append((c, 0, 0))
        so.append(so[-1] + lengths[c])
        lo.append(len(layout))
    rng.shuffle(recs)
    return lengths, contained, recs, {"seq_offs": so, "lay_offs": lo, "layout": layout}


def unplaceable():
    """every class but PLACED and INVALID -> (lengths, contained, records, tables)"""
    lengths, contained = [80, 60, 50, 40, 30, 70], [0, 1, 1, 1, 1, 0]
    tables = single_unitig(80, False, 0, 80)(lengths)
    tables["lay_offs"] = tables["lay_offs"][:5] + [5, 5]  # read 5 is unitig 5 without a placement: a trim round took it
    recs = [(1, 0, 60, 8, 0, 30),   # reserved + 60 > 80: not valid, and read 1 has no other record
            (2, 3, 50, 8, 0, 0),    # 50 does not fit 40: not valid
            (3, 2, 40, 8, 0, 5),    # read 3 in read 2, which is contained and has no choice
            (4, 5, 30, 12, 0, 40),  # its root has no placement
            (9, 0, 10, 8, 0, 0), (0, 0, 80, 8, 0, 0), (0, 5, 80, 0, 0, 0)]  # an id too large, a read in itself, no containment
    return lengths, contained, recs, tables


def foreign_tables():
    """name -> (lengths, contained, records, tables): tables no call of this library writes"""
    out = {}
    lengths = [80, 60, 60, 40, 40, 90]
    base = single_unitig(80, False, 0, 80)(lengths)
    # ids beyond n_reads in the records and in the layout
    t = dict(base, layout=[(0, 0, 0), (1000, 0, 0), (2, 0, 0), (0xFFFFFFFF, 1, 5), (4, 0, 0), (5, 0, 0)])
    out["ids_beyond"] = (lengths, [0, 1, 0, 1, 1, 0], [(1, 6, 60, 8, 0, 0), (77, 0, 60, 8, 0, 0), (1, 0, 60, 8, 0, 20), (3, 1, 40, 12, 0, 0),
                                                        (4, 0xFFFFFFFF, 40, 8, 0, 0), (4, 5, 40, 8, 0, 50)], t)
    # reads 1 and 2 contain each other, read 3 hangs on the cycle, read 4 names itself
    out["cycles"] = (lengths, [0, 1, 1, 1, 1, 0], [(1, 2, 60, 8, 0, 0), (2, 1, 60, 12, 0, 0), (3, 1, 40, 8, 0, 7), (4, 4, 40, 8, 0, 0)], base)
    # an offset beyond the container; a root that lies beyond its unitig's columns, and one at 2^64 - 1
    t = dict(base, layout=[(0, 0, 50), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (5, 1, MASK64)])
    out["offsets_beyond"] = (lengths, [0, 1, 0, 1, 1, 0], [(1, 0, 60, 8, 0, 21), (3, 0, 40, 8, 0, 0), (4, 5, 40, 8, 0, 10)], t)
    out["lay_offs_reversed"] = (lengths, [0, 1, 0, 1, 1, 0], [(1, 0, 60, 8, 0, 10), (3, 1, 40, 12, 0, 0), (4, 5, 40, 8, 0, 10)],
                                dict(base, lay_offs=base["lay_offs"][::-1]))
    return out


def long_container_set():
    """a read of 70 000 bases (no query: rule 1) with a read inside it at column 66 000 and a reversed one flush with its end
    -> (refs, names, params, records)"""
    big = pc.random_genome(70000, 31)
    refs = [big, big[66000:66150], pc.revcomp(big[69850:70000])]
    return refs, ["a", "b", "c"], mc.params(S=12, T=4, M=45, P=0, H=4096, K=4096), [(1, 0, 150, 8, 0, 66000), (2, 0, 150, 12, 0, 69850)]


def trimmed_case():
    """consensus_cases.noisy_case(1, True) and, beside it, an island of 100 bases with a read inside it; composed as `siga unitig -e
    40 --reduce -m 30 -x 2` (min branch length 150): the rounds remove every island, the contained reads and that container among
    them -> (case, refs, name ranks, contained, edges, containment records, the unitig call's dict, the placement)"""
    import random
    from tests import consensus_cases as cc
    base = cc.noisy_case(1, True)
    rng = random.Random(77)
    island = bytes(rng.choice(b"ACGT") for _ in range(100))
    reads = list(base["reads"]) + [island, island[20:80]]
    names = list(base["names"]) + ["zz_island", "zz_inside"]
    case = dict(base, reads=reads, names=names)
    refs = [r.decode() for r in reads]
    ranks = mc.name_ranks(names)
    records, contained, _ = mc.expected_mm_overlaps(refs, ranks, base["params"])
    conts, _ = expected_containments(refs, ranks, base["params"])
    edges = [(q, t, ln, af) for q, t, ln, af, _ in records if not contained[q] and not contained[t]]
    red = cc.rc.expected_reduce(reads, edges, 30, 2, 150)
    return case, refs, ranks, contained, edges, conts, red, expected_placement(red, [len(r) for r in reads], contained, conts)
