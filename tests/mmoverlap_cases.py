"""`siga overlap -e`: the rules of include/sigax.h (the block of overlaps with mismatches) restated serially, with Python integers
and strings, on top of the pile-up's restatement (tests/pileup_cases.py), and the cases of tests/test_mmoverlap_cases.py and
tests/test_gpu_mmoverlap.py.  No tests here.

expected_mm_overlaps()  rules 1-8 over the seeds' candidates -> (sorted canonical records, contained, the eight status words)
brute_mm_overlaps()     the same over every read, strand and diagonal, without seeds -> (sorted records, contained)
ed_coords(), ed_line()  the ED coordinates that follow from (length, af, read lengths), and the line `siga overlap -e` writes
completeness_floor()    min over l >= M of ceil((l - m) / (m + 1)): the clean run every accepted alignment holds
case builders           the boundary sets, the noisy genome, the containment-free exact set, the mixed-length set
A record is the tuple (query, target, length, af, num_diff).
"""
import random

from tests import pileup_cases as pc

DEFAULTS = dict(S=24, T=12, H=256, M=45, P=40, K=512, max_len=pc.PILE_MAX_LEN)
FIELDS = dict(S="seed_length", T="seed_stride", H="max_seed_hits", M="min_overlap", P="error_permille", K="max_candidates", max_len="max_read_len")
AF = {("SUFFIX", 0): 0, ("SUFFIX", 1): 6, ("PREFIX", 0): 3, ("PREFIX", 1): 5}


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def name_ranks(names):
    """rank of each name among the distinct names in string order (equal names, equal rank)"""
    order = {n: k for k, n in enumerate(sorted(set(names)))}
    return [order[n] for n in names]


def classify(n, L, d, ell):
    """rule 5"""
    if ell == n == L:
        return "DUP"
    if ell == n:
        return "Q_IN_T"
    if ell == L:
        return "T_IN_Q"
    return "SUFFIX" if d < 0 else "PREFIX"


def _take(refs, ranks, i, cand, p, records, contained, geometry=None):
    """rules 4-7 for one candidate of read i -> 1 if it is accepted; a record goes to `records` (a list), a flag to `contained`.
    geometry: (l, len(text), m) where the caller has them already"""
    t, strand, d = cand
    q = refs[i]
    if geometry is None:
        x0, x1, text, m = pc.overlap_of(refs, q, cand)
        ell, L = x1 - x0, len(text)
    else:
        ell, L, m = geometry
    if ell < p["M"] or m > (ell * p["P"]) // 1000:
        return 0
    cls = classify(len(q), L, d, ell)
    if cls == "DUP":
        contained[i if ranks[i] > ranks[t] else t] = 1
    elif cls == "Q_IN_T":
        contained[i] = 1
    elif cls == "T_IN_Q":
        contained[t] = 1
    else:
        af = AF[(cls, strand)]
        if ranks[i] > ranks[t]:
            records.append((i, t, ell, af, m))
        else:
            records.append((t, i, ell, af if af & 4 else af ^ 3, m))
    return 1


def _ordered(records):
    """rule 8: each (query, target, af, length) once, ascending"""
    return sorted(set(records), key=lambda r: (r[0], r[1], r[3], r[2]))


def expected_mm_overlaps(refs, name_rank, p, first=0, count=None):
    """rules 1-8 with reads first .. first + count as queries (all of them by default) -> (records, contained, status8)"""
    n_reads = len(refs)
    count = n_reads - first if count is None else count
    records, contained, st = [], [0] * n_reads, [0] * 8
    for i in range(first, first + count):
        q = refs[i]
        if len(q) < p["S"] or len(q) > min(p["max_len"], pc.PILE_MAX_LEN):
            st[1] += 1
            continue
        cands, located, repeats, listed = pc.seed_candidates(refs, q, p)
        st[0] += listed
        st[3] += located
        st[4] += repeats
        if len(cands) > p["K"]:
            st[2] += 1
            continue
        mine = []
        for c in sorted(cands):
            if name_rank[c[0]] == name_rank[i]:
                continue
            st[5] += 1
            st[6] += _take(refs, name_rank, i, c, p, mine, contained)
        st[7] += len(mine)
        records += mine
    return _ordered(records), contained, st


def brute_mm_overlaps(refs, name_rank, p):
    """every read against every read, strand and diagonal -> (records, contained).  Rule 4 is restated here once more, so that
    the count can stop at the first mismatch too many"""
    records, contained = [], [0] * len(refs)
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
                    if ell < p["M"]:
                        continue
                    limit, m = (ell * p["P"]) // 1000, 0
                    for x in range(x0, x1):
                        if q[x] != text[x + d]:
                            m += 1
                            if m > limit:
                                break
                    if m <= limit:
                        _take(refs, name_rank, i, (t, strand, d), p, records, contained, (ell, L, m))
    return _ordered(records), contained


def completeness_floor(M, P, longest):
    """the longest clean run every accepted alignment of M .. longest columns is sure to hold: m mismatches cut l columns into
    m + 1 runs with l - m matching columns between them"""
    best = None
    for ell in range(M, longest + 1):
        m = (ell * P) // 1000
        run = -((ell - m) // -(m + 1))
        best = run if best is None else min(best, run)
    return best


def ed_coords(length, af, ql, tl):
    """(s0, e0, ql, s1, e1, tl, rc) as write_edge_line (siga_amd/host/asqg_text.cpp) and OverlapBlock::overlap
    (src/overlap_builder.cpp:158-175) compute them"""
    s0, e0, s1, e1 = ql - length, ql - 1, 0, length - 1
    if af & 1:
        s0, e0 = ql - e0 - 1, ql - s0 - 1
    if af & 2:
        s1, e1 = tl - e1 - 1, tl - s1 - 1
    return s0, e0, ql, s1, e1, tl, 1 if af & 4 else 0


def ed_line(rec, names, refs):
    q, t, length, af, m = rec
    return "ED\t%s %s %d %d %d %d %d %d %d %d" % ((names[q], names[t]) + ed_coords(length, af, len(refs[q]), len(refs[t])) + (m,))


def asqg_text(names, refs, records, contained, min_overlap):
    """the file `siga overlap -e` writes"""
    out = ["HT\tVN:i:1\tOL:i:%d\tCN:i:1" % min_overlap]
    out += ["VT\t%s\t%s\tSS:i:%d" % (n, s, c) for n, s, c in zip(names, refs, contained)]
    out += [ed_line(r, names, refs) for r in records]
    return "\n".join(out) + "\n"


def names_of(n):
    """names whose string order is not the order of the read ids"""
    return ["r%d" % ((i * 7919) % 10007) for i in range(n)]


# ---- case builders --------------------------------------------------------------------------------------------------------------
G = pc.random_genome(1200, 41)


def noisy_case(seed=11):
    """44 reads of 60/75/100/150 bases on both strands of a 700-base genome with 1.5 % substitutions, plus a duplicate, a
    contained piece and a reverse complement"""
    g = pc.random_genome(700, seed)
    rng = random.Random(seed + 1)
    refs = []
    for i in range(44):
        L = (60, 75, 100, 150)[i % 4]
        o = rng.randrange(0, len(g) - L + 1)
        r = pc.mutate(g[o:o + L], [x for x in range(L) if rng.random() < 0.015])
        refs.append(pc.revcomp(r) if rng.random() < 0.5 else r)
    refs.append(refs[5])
    refs.append(refs[7][10:70])
    refs.append(pc.revcomp(refs[11]))
    return refs, names_of(len(refs))


def exact_case(seed=3, n=60, length=70, step=9):
    """error-free reads of one length at distinct places of a random genome, both strands: no read contains another"""
    g = pc.random_genome(step * n + length + 50, seed)
    rng = random.Random(seed + 1)
    refs = []
    for i in range(n):
        r = g[i * step + (i % 3):i * step + (i % 3) + length]
        refs.append(pc.revcomp(r) if rng.random() < 0.5 else r)
    return refs, names_of(n)


def mixed_case(seed=1):
    """some 300 reads of the lengths around the seed and the wave on both strands, a fifth of them with substitutions; reads
    shorter than any seed; one read of 4096 and one of 4097 bases over the same place"""
    case = pc.random_case(seed=seed, n_reads=290, lens=(40, 63, 64, 65, 129, 200), n_queries=0)
    g = case["genome"]
    rng = random.Random(seed + 9)
    refs = [pc.mutate(r, [x for x in range(len(r)) if rng.random() < 0.02]) if k % 5 == 0 else r for k, r in enumerate(case["refs"])]
    refs += [g[100:111], g[300:323]]
    big = pc.random_genome(4097, seed + 5)
    refs += [big[:4096], big, big[4000:4097] + g[:60], pc.revcomp(big[:90])]
    return refs, names_of(len(refs))


def boundary_sets():
    """hand-made sets, one per rule: name -> (refs, names, params, what the restatement must give: records, flagged reads)"""
    g = G
    P0 = params(S=12, T=4, M=45, P=0, H=4096, K=4096)
    sets = {}
    a, b = g[100:180], g[135:215]  # a's suffix of 45 on b's prefix
    # read 0 has the smaller name: its finds are written swapped
    for tag, names in (("q_small", ["a", "b"]), ("q_large", ["b", "a"])):
        swap = tag == "q_small"
        sets["suffix_fwd_" + tag] = ([a, b], names, P0, [(1, 0, 45, 3, 0)] if swap else [(0, 1, 45, 0, 0)], [])
        sets["suffix_rev_" + tag] = ([a, pc.revcomp(b)], names, P0, [(1, 0, 45, 6, 0)] if swap else [(0, 1, 45, 6, 0)], [])
        sets["prefix_fwd_" + tag] = ([b, a], names, P0, [(1, 0, 45, 0, 0)] if swap else [(0, 1, 45, 3, 0)], [])
        sets["prefix_rev_" + tag] = ([b, pc.revcomp(a)], names, P0, [(1, 0, 45, 5, 0)] if swap else [(0, 1, 45, 5, 0)], [])
    sets["l_below_M"] = ([a, g[136:216]], ["b", "a"], P0, [], [])  # 44 columns
    am = pc.mutate(a, [150 - 100, 170 - 100])  # two substitutions inside the overlap of 45
    sets["m_at_floor"] = ([am, b], ["b", "a"], params(S=12, T=4, M=45, P=45, H=4096, K=4096), [(0, 1, 45, 0, 2)], [])  # floor(45 * 45 / 1000) = 2
    sets["m_above_floor"] = ([am, b], ["b", "a"], params(S=12, T=4, M=45, P=44, H=4096, K=4096), [], [])  # floor(45 * 44 / 1000) = 1
    sets["q_in_t"] = ([g[110:170], g[100:180]], ["b", "a"], P0, [], [0])
    sets["t_in_q"] = ([g[100:180], pc.revcomp(g[110:170])], ["a", "b"], P0, [], [1])
    sets["dup_larger_name"] = ([a, a, pc.revcomp(a)], ["m", "k", "z"], P0, [], [0, 2])  # k keeps its place: m and z are flagged
    sets["same_name"] = ([a, b, a], ["x", "x", "y"], P0, [(2, 1, 45, 0, 0)], [2])  # reads 0 and 1 share a name: no record; 2 is a duplicate of 0 with the larger name
    # n + d = L: the query ends where the text ends, a containment; one base further, a prefix overlap of L - d columns
    sets["ends_together"] = ([g[120:180], g[100:180]], ["b", "a"], P0, [], [0])
    sets["one_past_the_end"] = ([g[120:181], g[100:180]], ["b", "a"], P0, [(0, 1, 60, 3, 0)], [])
    return sets
