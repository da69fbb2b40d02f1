"""The consensus pass of `siga unitig -e` (csrc/sigax_consensus.hip): the rules of include/sigax.h restated serially, twice, and the
cases of tests/test_consensus_cases.py and tests/test_gpu_unitig_consensus.py.  No tests here.

expected_consensus()   rules 1-6 placement by placement: every valid placement adds its bytes to the counts of the columns it covers
columnwise_consensus() the same rules column by column: for each column the placements over it are looked up and their bytes read
The two share the letter table and nothing else.  Both take the reads (bytes by read id), the dict of a unitig call (seq_offs,
lay_offs, layout [(read, flags, offset)], useqs) and min_votes, and return dict(useqs bytes, changed [per unitig], support bytes,
status [8]).

A case: dict(name, reads, res) with res the dict above.  Layouts come from the unitig restatement (tests/unitig_cases.py::expected)
over records computed from known genome positions, adjacent reads only, so every record is simple; the vote and robustness cases
write their tables by hand.
"""
import functools
import random

from tests import mmoverlap_cases as mc
from tests import reduce_cases as rc
from tests import unitig_cases as uc

LETTERS = b"ACGT"
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}
REV = uc.PLACED_REV


def _tables(res):
    return [int(x) for x in res["seq_offs"]], [int(x) for x in res["lay_offs"]], [(int(r), int(f), int(o)) for r, f, o in res["layout"]]


def _decide(own, c, min_votes):
    """rules 4-5 for one column -> (byte, changed, support, tie, held)"""
    w = max(range(4), key=lambda k: (c[k], -k))
    c_own = c[LETTERS.index(own)] if own in LETTERS else 0
    more = c[w] > c_own
    replace = more and c[w] >= min_votes
    tie = own in LETTERS and c_own >= 1 and c_own == c[w] and sum(1 for k in range(4) if c[k] == c[w]) >= 2
    byte = LETTERS[w] if replace else own
    return byte, replace, min(255, c[w] if replace else c_own), tie, more and not replace


def expected_consensus(reads, res, min_votes=1):
    """placement by placement"""
    so, lo, layout = _tables(res)
    n, nu = len(reads), len(so) - 1
    own = bytes(res["useqs"])
    out, support, changed = bytearray(own), bytearray(len(own)), [0] * nu
    st = [nu, 0, 0, 0, 0, 0, 0, 0]
    for u in range(nu):
        U = so[u + 1] - so[u]
        counts = [[0, 0, 0, 0] for _ in range(U)]
        for r, fl, o in layout[lo[u]:min(lo[u + 1], len(layout))]:
            if r >= n or o + len(reads[r]) > U:
                st[7] += 1
                continue
            placed = reads[r]
            if fl & REV:
                placed = bytes(_COMP.get(b, b) for b in reversed(placed))
            for k, b in enumerate(placed):
                if b in LETTERS:
                    counts[o + k][LETTERS.index(b)] += 1
        for x in range(U):
            g = so[u] + x
            byte, rep, sup, tie, held = _decide(own[g], counts[x], min_votes)
            out[g], support[g] = byte, sup
            depth = sum(counts[x])
            changed[u] += rep
            st[1] += 1
            st[2] += rep
            st[3] += depth < 2
            st[4] += tie
            st[5] += held
            st[6] = max(st[6], depth)
    return {"useqs": bytes(out), "changed": changed, "support": bytes(support), "status": st}


def columnwise_consensus(reads, res, min_votes=1):
    """column by column"""
    so, lo, layout = _tables(res)
    n, nu = len(reads), len(so) - 1
    own = bytes(res["useqs"])
    cols, changed, status = [], [], [nu] + [0] * 7
    for u in range(nu):
        U = so[u + 1] - so[u]
        mine = layout[lo[u]:lo[u + 1]]
        ok = [p for p in mine if p[0] < n and p[2] + len(reads[p[0]]) <= U]
        status[7] += len(mine) - len(ok)
        n_changed = 0
        for x in range(U):
            c = [0, 0, 0, 0]
            for r, fl, o in ok:
                L = len(reads[r])
                if not o <= x < o + L:
                    continue
                b = reads[r][L - 1 - (x - o)] if fl & REV else reads[r][x - o]
                if fl & REV:
                    b = {65: 84, 84: 65, 67: 71, 71: 67}.get(b, b)
                for k in range(4):
                    c[k] += b == LETTERS[k]
            first = [k for k in range(4) if c[k] == max(c)][0]
            mine_b = own[so[u] + x]
            c_own = c[LETTERS.find(mine_b)] if LETTERS.find(mine_b) >= 0 else 0
            if c[first] > c_own and c[first] >= min_votes:
                cols.append((LETTERS[first], min(c[first], 255)))
                n_changed += 1
            else:
                cols.append((mine_b, min(c_own, 255)))
                status[5] += c[first] > c_own
                status[4] += c_own > 0 and c_own == max(c) and c.count(c_own) > 1
            status[3] += sum(c) <= 1
            status[6] = max(status[6], sum(c))
        changed.append(n_changed)
    status[1], status[2] = len(cols), sum(changed)
    return {"useqs": bytes(b for b, _ in cols), "changed": changed, "support": bytes(s for _, s in cols), "status": status}


# ---- reads on a line ----------------------------------------------------------------------------------------------------------------
def genome(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(LETTERS) for _ in range(n))


def substitute(s, at):
    """s with the next letter of ACGT at every position of `at`"""
    t = bytearray(s)
    for x in at:
        t[x] = LETTERS[(LETTERS.index(t[x]) + 1) % 4]
    return bytes(t)


def adjacent_edges(spans, strands, ids=None, ring=0):
    """the records between neighbours of reads at genome spans [(start, end)] in ascending order (starts and ends both ascend, so
    that no read holds another), stored reverse-complemented where strands[k]; ring = the genome's length when the last read
    overlaps the first across its end"""
    ids = list(range(len(spans))) if ids is None else ids
    out = []
    pairs = [(k, k + 1) for k in range(len(spans) - 1)] + ([(len(spans) - 1, 0)] if ring else [])
    for a, b in pairs:
        ln = spans[a][1] - spans[b][0] - (ring if b < a else 0)
        assert 0 < ln < min(spans[a][1] - spans[a][0], spans[b][1] - spans[b][0])
        af = (1 if strands[a] else 0) | (2 if strands[b] else 0) | (4 if strands[a] != strands[b] else 0)
        out.append((ids[a], ids[b], ln, af))
    return out


def line_reads(g, spans, strands, errors=()):
    """the reads at `spans` of g; errors: (read, genome column) substitutions"""
    reads = []
    for k, (s, e) in enumerate(spans):
        r = substitute(g[s:e], [c - s for i, c in errors if i == k])
        reads.append(uc.revcomp(r) if strands[k] else r)
    return reads


def lines_case(name, lines, m, seed):
    """several genomes side by side, each tiled by a line of reads: lines = [(genome length, spans, errors)] -> a case with the
    layout of the unitig restatement; case["genomes"] the genomes in unitig order"""
    rng = random.Random(seed)
    reads, edges, genomes = [], [], []
    for k, (glen, spans, errors) in enumerate(lines):
        g = genome(glen, seed * 1000 + k)
        strands = [rng.random() < 0.5 for _ in spans]
        ids = list(range(len(reads), len(reads) + len(spans)))
        edges += adjacent_edges(spans, strands, ids)
        reads += line_reads(g, spans, strands, errors)
        genomes.append(g)
    return {"name": name, "reads": reads, "edges": edges, "m": m, "genomes": genomes, "res": uc.expected(reads, edges, m)}


def tiling(total, length, step):
    """spans of `length` every `step` columns, the last one ending at `total`"""
    if total <= length:
        return [(0, total)]
    spans = [(s, s + length) for s in range(0, total - length, step)]
    return spans + [(total - length, total)]


def sizes_case():
    """unitigs of 1, 63, 64, 65, 127, 128 and 129 columns, each once as a single read and once tiled by reads of 30"""
    sizes = (1, 63, 64, 65, 127, 128, 129)
    lines = [(U, [(0, U)], ()) for U in sizes] + [(U, tiling(U, 30, 7), ((1, 20),)) for U in sizes if U > 30]
    return lines_case("sizes", lines, 10, 11)


def short_case():
    """many unitigs shorter than a tile side by side: single reads of 5 to 25 bases and pairs of reads of 20"""
    lines = [(5 + k % 21, [(0, 5 + k % 21)], ()) for k in range(40)] + [(28, [(0, 20), (8, 28)], ()) for _ in range(20)]
    return lines_case("short", lines, 10, 12)


def starts_case():
    """read starts at columns 63, 64 and 65 of a longer unitig; errors at the tile boundaries and, the last two, in bytes the copy takes"""
    starts = (0, 30, 50, 63, 64, 65, 100, 127, 128, 129, 160)
    return lines_case("starts", [(220, [(s, s + 60) for s in starts], ((3, 63), (4, 64), (5, 65), (7, 128), (8, 129), (3, 115), (6, 130)))], 10, 13)


def lengths_case():
    """read lengths from 20 to 300 in one unitig"""
    lens = (20, 35, 80, 150, 300, 290, 280, 200, 120, 60, 30, 20, 45, 300, 100)
    spans, s = [], 0
    for k, L in enumerate(lens):
        spans.append((s, s + L))
        if k + 1 < len(lens):
            s += max(3, L - lens[k + 1] + 2)
    errors = tuple((k, (spans[k][0] + spans[k][1]) // 2) for k in range(2, len(lens) - 1, 3))
    return lines_case("lengths", [(spans[-1][1], spans, errors)], 10, 14)


def deep_case(length, n, name):
    """reads of `length` one column apart: depth up to min(length, n)"""
    spans = [(s, s + length) for s in range(n)]
    errors = tuple((k, spans[k][1] - 1 - (k * 7) % 20) for k in range(0, n, 9))  # (at least 14 reads over each)
    return lines_case(name, [(n - 1 + length, spans, errors)], 10, 15)


def ring_case():
    """a circular genome of 200 tiled by 8 reads of 60: the unitig is circular and is voted on as a line"""
    rng = random.Random(16)
    g = genome(200, 16)
    spans = [(s, s + 60) for s in range(0, 200, 25)]
    strands = [False] + [rng.random() < 0.5 for _ in spans[1:]]
    reads = line_reads(g + g, spans, strands, ((2, 70), (5, 150)))
    edges = adjacent_edges(spans, strands, ring=200)
    res = uc.expected(reads, edges, 10)
    assert res["uflags"] == [uc.CIRCULAR | (35 << 1)]
    return {"name": "ring", "reads": reads, "edges": edges, "m": 10, "res": res}


# ---- votes, by hand -----------------------------------------------------------------------------------------------------------------
# (own byte, the placed bytes of five reads) per column
VOTE_COLUMNS = (
    ("A", "ACNNn"),  # depth 2 disagreeing: own stays on a tie
    ("C", "ACNNN"),  # the same with own the later letter
    ("A", "AACCN"),  # 2 against 2, own among them
    ("C", "AACCN"),
    ("X", "AACCN"),  # own no letter, A x 2 and C x 2: A wins, with 2 votes
    ("G", "AAAGG"),  # 3 against 2
    ("G", "AAGNN"),  # 2 against 1
    ("N", "TNNNN"),  # own N, one vote
    ("a", "aaaaa"),  # nobody votes
    ("T", "tttTN"),  # lower case does not vote: own keeps its one vote
    ("A", "NNNNN"),
    ("g", "GGCNN"),  # lower-case own replaced
    ("T", "ACGTN"),  # four ways, own among them
    ("N", "CGTNN"),  # three ways without own: C, the earliest
)


def votes_case():
    """one unitig whose columns are VOTE_COLUMNS, five reads at offset 0 (the second and the fourth placed reverse), and a second
    unitig of one read that repeats the own bytes"""
    own = bytes(ord(o) for o, _ in VOTE_COLUMNS)
    reads, layout = [], []
    for k in range(5):
        placed = bytes(ord(v[k]) for _, v in VOTE_COLUMNS)
        rev = k in (1, 3)
        reads.append(bytes(_COMP.get(b, b) for b in reversed(placed)) if rev else placed)
        layout.append((k, REV if rev else 0, 0))
    reads.append(own)
    layout.append((5, 0, 0))
    W = len(own)
    res = {"seq_offs": [0, W, 2 * W], "lay_offs": [0, 5, 6], "uflags": [0, 0], "layout": layout, "useqs": own + own}
    return {"name": "votes", "reads": reads, "res": res}


def invalid_case():
    """the starts case and a sizes case side by side with placements made invalid: read ids at and beyond n_reads in the middle of
    a unitig (their offsets kept, so that the offsets still ascend), and the last placement of a unitig moved beyond its end"""
    case = lines_case("invalid", [(220, [(s, s + 60) for s in (0, 30, 50, 63, 64, 65, 100, 127, 128, 129, 160)], ((4, 64),)),
                                  (129, tiling(129, 30, 7), ()), (100, tiling(100, 30, 7), ()), (90, tiling(90, 30, 7), ())], 10, 17)
    res = dict(case["res"])
    lay, lo, n = list(res["layout"]), res["lay_offs"], len(case["reads"])
    lay[lo[0] + 3] = (n, lay[lo[0] + 3][1], lay[lo[0] + 3][2])
    lay[lo[0] + 6] = (0xFFFFFFFF, 1, lay[lo[0] + 6][2])
    r, fl, o = lay[lo[1] - 1]
    lay[lo[1] - 1] = (r, fl, o + 1)  # one column over the end
    r, fl, o = lay[lo[2] - 1]
    lay[lo[2] - 1] = (r, fl, 1 << 40)
    r, fl, o = lay[lo[3] - 1]
    lay[lo[3] - 1] = (r, fl, (1 << 64) - 1)
    res["layout"] = lay
    case["res"] = res
    return case


@functools.lru_cache(maxsize=None)
def planted_cases():
    """cases with planted substitutions whose consensus must be the genome"""
    return (starts_case(), lengths_case(), deep_case(200, 150, "deep150"), deep_case(300, 300, "deep300"))


@functools.lru_cache(maxsize=None)
def all_cases():
    return (sizes_case(), short_case(), ring_case(), votes_case(), invalid_case()) + planted_cases()


def arrays(case, shift=0):
    """-> (lengths u32[n], seqs bytes, offs u64[n+1]) with offs[0] = shift and `shift` bytes of padding before the first read"""
    import numpy as np
    lengths = np.array([len(r) for r in case["reads"]], dtype=np.uint32)
    offs = np.full(len(lengths) + 1, shift, dtype=np.uint64)
    offs[1:] += np.cumsum(lengths, dtype=np.uint64)
    return lengths, b"#" * shift + b"".join(case["reads"]), offs


# ---- noisy reads, end to end ----------------------------------------------------------------------------------------------------------
NOISY = dict(S=12, T=4, M=30, P=40)
# (seed, mixed lengths): seeds 0 to 5, each with equal and with mixed lengths, but for two.  (2, True) has its substitution at
# column 1860 under nine reads of which seven are contained, (3, True) at column 60 under eight of which six are: a contained read
# has no placement and no vote, two placed reads are left, the erroneous one among them, and the tie keeps the copy's byte.  The
# conditions stand; those two variants went.
NOISY_SEEDS = tuple((seed, mixed) for seed in range(6) for mixed in (False, True) if (seed, mixed) not in ((2, True), (3, True)))


@functools.lru_cache(maxsize=None)
def noisy_case(seed, mixed):
    """a random genome of 2 400 bases tiled by reads of 70 (mixed: of 60, 64, 65, 80 and 100) whose starts lie 4 to 10 columns
    apart, the last 100 bases once more as a read of their own, on either strand in shuffled order; 30 to 50 substitutions at
    columns 40 apart, each in one read, where at least three reads cover the column"""
    rng = random.Random(7000 + seed)
    g = genome(2400, 7100 + seed)
    spans, s = [], 0
    while True:
        L = rng.choice((60, 64, 65, 80, 100)) if mixed else 70
        if s + L > len(g):
            break
        spans.append((s, s + L))
        s += rng.randint(4, 10)
    spans.append((len(g) - 100, len(g)))
    rng.shuffle(spans)
    strands = [rng.random() < 0.5 for _ in spans]
    columns = rng.sample(range(20, len(g) - 20, 40), rng.randint(30, 50))
    errors = []
    for c in sorted(columns):
        over = [k for k, (a, b) in enumerate(spans) if a <= c < b]
        if len(over) >= 3:
            errors.append((rng.choice(over), c))
    reads = line_reads(g, spans, strands, errors)
    names = ["n%04d" % ((k * 7919) % 10007) for k in range(len(reads))]
    return {"name": "noisy%d" % seed, "genome": g, "reads": reads, "names": names, "spans": spans, "errors": errors, "params": mc.params(**NOISY)}


@functools.lru_cache(maxsize=None)
def noisy_expected(seed, mixed):
    """the composed expectation of `siga unitig -e 40 --reduce -m 30 --seed-length 12 --seed-stride 4`: the mismatch overlaps, the
    records that touch a contained read dropped, the reduction, and the vote -> dict(records, contained, mm_status, edges, reduced
    (the unitig call's dict, copy bases), consensus (expected_consensus's dict))"""
    case = noisy_case(seed, mixed)
    refs = [r.decode() for r in case["reads"]]
    records, contained, st = mc.expected_mm_overlaps(refs, mc.name_ranks(case["names"]), case["params"])
    edges = [(q, t, ln, af) for q, t, ln, af, _ in records if not contained[q] and not contained[t]]
    red = rc.expected_reduce(case["reads"], edges, NOISY["M"], 0, 0)
    return {"records": records, "contained": contained, "mm_status": st, "edges": edges, "reduced": red,
            "consensus": expected_consensus(case["reads"], red, 1)}


def assembled(case, exp):
    """the unitigs of the composed expectation other than the contained reads on their own -> [(copy bases, consensus bases)],
    brought to the genome's strand where the consensus is its reverse complement"""
    red, out = exp["reduced"], []
    for u in range(len(red["uflags"])):
        a, b = red["lay_offs"][u], red["lay_offs"][u + 1]
        if b - a == 1 and exp["contained"][red["layout"][a][0]]:
            continue
        a, b = red["seq_offs"][u], red["seq_offs"][u + 1]
        copy, cons = bytes(red["useqs"][a:b]), exp["consensus"]["useqs"][a:b]
        if uc.revcomp(cons) == case["genome"]:
            copy, cons = uc.revcomp(copy), uc.revcomp(cons)
        out.append((copy, cons))
    return out
