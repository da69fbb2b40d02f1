"""Read sets whose (read, side) items have a width that is decided by construction, and the CPU-side facts about them.

k_filter_extract_fast (siga_amd/csrc/sigax_kernels.hip) hands an item along the chain of launch_fx_stages by its number of
blocks T = nX + nY and by what happens inside it.  The random fixtures put T wherever coverage puts it; here reads are
placed by genome position, every overlap is exact, and a read at position p of length L sees one block per distinct start
position in (p, p + L - m] on its suffix side (and the mirror image on its prefix side), split between its two lists by the
strand of the reads that start there.

How the kernel counts (GFx::body): side 0 takes finds 0 and 3, side 1 finds 1 and 2; list X = the blocks of the side's first
find (nA) + the containment blocks of finds 0 and 1 (c0, c1), list Y = the second find's (nB) + those of finds 2 and 3
(c2, c3).  A read is its own containment in finds 0 and 2, so c0 = c2 = 1 for every read that is no substring of another:
T = nA + nB + c0 + c1 + c2 + c3 >= 2, and "all of an item's width comes from list Y" means nA == 0.

Generators: `staircase` (one read per position: every width up to S + 1 on both sides), `landings` (a few reads, d positions
without a read start, then W consecutive ones: the single-group extension runs d + 1 rounds with the whole width alive),
landings with a second haplotype (the extension branches inside the landing), with ragged lengths, duplicates and an
opposite-strand twin ('$' below the top level, substring reads, containment blocks at wide items, ranges of two rows) and with
private variants (V reads that each split off into a group of their own).

Facts: `string_facts` computes (nA, nB, c0..c3, top-level blocks, rounds until the top level ends) of every item by string
comparison of the reads themselves -- positions are not used, the generator knows them; `oracle_facts` reads the same numbers
off the oracle's exhaustive block lists grouped by af; `granule_crossers` tells which items hold a block whose capped range
spans two 128-row granules, `late_crossers` which ones meet such a range only in the round that ends their top level.
tests/test_fx_width_cases.py checks that the two agree and that every set holds what it was built
for; tests/test_gpu_fx_widths.py runs the sets on the GPU."""
import os
import random
import re

import numpy as np

from tests.golden.make_reads import revcomp

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the widths at which an item changes launch (16-, 32-, 64-lane groups, GFx::body_big's FX_BIGCAP) and their neighbours
BOUNDARY_WIDTHS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)
BIG_LO, BIG_HI = 65, 256   # GFx::body_big's items
GROUP_SLOTS = 24           # FX_NSLOT


def af_of_finds():
    """(SIGAX_AF_CHAIN0 .. SIGAX_AF_CHAIN3) of siga_amd/csrc/fm_layout.h"""
    text = open(os.path.join(_ROOT, "siga_amd", "csrc", "fm_layout.h")).read()
    return tuple(int(re.search(r"#define\s+SIGAX_AF_CHAIN%d\s+(\d+)u" % k, text).group(1)) for k in range(4))


def _genome(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _other_base(rnd, b):
    return rnd.choice([c for c in "ACGT" if c != b])


class Case:
    """a read set: reads [(name, sequence)], min-overlap m, and what it was built for: `widths` = the widths T that some item
    must have on each side, `notes` = further conditions by name (tests/test_fx_width_cases.py)"""

    def __init__(self, name, m, widths=(), notes=()):
        self.name, self.m, self.widths, self.notes = name, m, tuple(widths), tuple(notes)
        self.reads = []

    def add(self, genome, pos, length, rev=False):
        s = genome[pos:pos + length]
        assert len(s) == length
        self.reads.append(("w%d" % len(self.reads), revcomp(s) if rev else s))
        return len(self.reads) - 1

    @property
    def seqs(self):
        return [s for _, s in self.reads]


# ---- staircases -----------------------------------------------------------------------------------------------------------
def staircase(name, S, L, m, strands, seed, widths=(), notes=(), forward_at=(), twice_every=0):
    """one read per position 0 .. S-1 (two with strands == "both"), L >= S + m: read i sees S-1-i start positions on its
    suffix side and i on its prefix side.  strands: "fwd", "rev" (all reverse-complemented), "coin" (seeded coin) -- in both
    the reads at the positions `forward_at` stay forward --, "both" (one read per strand at every position: two top-level
    blocks of equal length, and every read has a full-length twin on the opposite strand).  twice_every = k: the reads at
    every k-th position twice, so that their blocks' ranges hold two rows (were every read there twice, equal suffixes would
    sit in rows 2j and 2j + 1 and no range could lie across a granule boundary)."""
    assert L >= S + m
    rnd = random.Random(seed)
    g = _genome(rnd, S - 1 + L)
    case = Case(name, m, widths, notes)
    for i in range(S):
        coin = rnd.random() < 0.5
        for _ in range(2 if twice_every and i % twice_every == 0 else 1):
            if strands == "both":
                case.add(g, i, L, False)
                case.add(g, i, L, True)
            else:
                case.add(g, i, L, i not in forward_at and {"fwd": False, "rev": True, "coin": coin}[strands])
    return case


# ---- landings -------------------------------------------------------------------------------------------------------------
def _island_layout(Q, d, W):
    """start positions of an island: Q consecutive reads, d positions without a start, W consecutive reads, d positions
    without a start, Q consecutive reads.  The last read of the first group sees nothing nearer than d + 1 bases on its suffix
    side, the first read of the last group nothing nearer on its prefix side."""
    a = list(range(Q))
    b = [Q - 1 + d + 1 + j for j in range(W)]
    c = [b[-1] + d + 1 + j for j in range(Q)]
    return a, b, c


def _landing_width(Q, d, W, L, m):
    """blocks of the landing item of an island of equal-length, same-strand reads: start positions in (p, p + L - m] for the
    last read of the first group, plus its own two containment blocks"""
    a, b, c = _island_layout(Q, d, W)
    p = a[-1]
    return sum(1 for s in b + c if p < s <= p + L - m) + 2


def _fit_island(T, Q, d, L, m):
    for W in range(1, L):
        if _landing_width(Q, d, W, L, m) == T:
            return W
    raise ValueError("no island of width %d with Q=%d d=%d L=%d m=%d" % (T, Q, d, L, m))


def _add_island(case, rnd, Q, d, W, L, hap_every=None, ragged=False, dup_every=None, twin=False, private=0):
    """one island on a genome stretch of its own (islands share no 40-mer, so they do not see each other)"""
    a, b, c = _island_layout(Q, d, W)
    g = _genome(rnd, c[-1] + L)
    E = a[-1] + L  # first genome coordinate behind the landing read: its extension reads g[E], g[E + 1], ...
    g2 = None
    if hap_every:
        # a second haplotype: a substitution every hap_every bases, one of them ten rounds into the landing
        x = list(g)
        for k in range((E + 10) % hap_every, len(g), hap_every):
            x[k] = _other_base(rnd, g[k])
        g2 = "".join(x)
    ids = []
    for n, p in enumerate(a + b + c):
        src = g2 if (g2 is not None and rnd.random() < 0.5) else g
        length = L
        middle = Q <= n < Q + W
        if ragged and middle and (n - Q) % 4 == 3:
            length = L - rnd.randrange(1, 30)  # shortened at its far end
        ids.append(case.add(src, p, length))
        if dup_every and middle and (n - Q) % dup_every == dup_every - 1:
            case.add(src, p, length)  # an exact duplicate: blocks whose range holds two rows
    if twin:  # the landing read once more, on the opposite strand
        case.add(g, a[-1], L, True)
        case.add(g, c[0], L, True)
    if private:
        # `private` reads of the middle group carry one substitution each, at distinct coordinates inside the landing's
        # extension window: the overlap with the landing read is untouched, and each splits off into a group of its own
        assert private <= W and private + 6 <= d
        pick = rnd.sample(range(W), private)
        for k, j in enumerate(pick):
            i = ids[Q + j]
            coord = E + 3 + k
            nme, s = case.reads[i]
            off = coord - b[j]
            assert 0 <= off < len(s)
            case.reads[i] = (nme, s[:off] + _other_base(rnd, s[off]) + s[off + 1:])
    return ids[Q - 1], ids[Q + W]  # the two landing reads


def landings(name, m, L, islands, seed, notes=(), **kw):
    """islands: [(T or None, Q, d, W or None)]: with T the middle group's size W is fitted so that the landing items have T
    blocks (plain islands only: equal lengths, one strand, one haplotype)"""
    rnd = random.Random(seed)
    widths = [T for T, _, _, _ in islands if T]
    case = Case(name, m, widths, notes)
    case.landing_reads = []
    for T, Q, d, W in islands:
        if T:
            W = _fit_island(T, Q, d, L, m)
        case.landing_reads.extend(_add_island(case, rnd, Q, d, W, L, **kw))
    return case


# ---- the sets -------------------------------------------------------------------------------------------------------------
M, LEN = 40, 340
STAIR_DUP_SEED = 28  # two items meet the late crossing while their reads' other sides finish (exposed_late_crossers)
_BUILDERS = {
    # every width from 2 to 301 on both sides; list Y of side 0 and list X of side 1 hold the read's own copies only
    "stair_fwd": lambda: staircase("stair_fwd", 300, LEN, M, "fwd", 11, BOUNDARY_WIDTHS + (290,), ("nA0",)),
    # no side over FX_BIGCAP, nothing branches, no read is contained: every item finishes on a lane group
    "stair_fwd250": lambda: staircase("stair_fwd250", 250, LEN, M, "fwd", 12, BOUNDARY_WIDTHS[:9]),
    # a forward read among reverse-complemented ones: its suffix side is all list Y, its prefix side all list X
    "stair_rev": lambda: staircase("stair_rev", 260, LEN, M, "rev", 13, BOUNDARY_WIDTHS, ("nA0_big", "nB0_big"), forward_at=(100,)),
    # strands by coin, but the reads whose sides have the widths in question: theirs are split between X and Y as it falls
    "stair_coin": lambda: staircase("stair_coin", 300, LEN, M, "coin", 14, BOUNDARY_WIDTHS + (290,), ("mixed",),
                                    forward_at=_stair_positions(300, BOUNDARY_WIDTHS + (295,))),
    # two reads per position: T = 2 (S-1-i) + 4, two top-level blocks, four containment blocks at every boundary
    "stair_both": lambda: staircase("stair_both", 150, LEN, M, "both", 15, (16, 32, 64, 256, 290), ("ntop2", "twins")),
    # ... and the reads of every third position twice: ranges of two rows, some of them across two 128-row granules -- in
    # the first round (body_big hands the item on) or only in the round in which the top-level blocks end
    "stair_dup": lambda: staircase("stair_dup", 130, LEN, M, "both", STAIR_DUP_SEED, (16, 32, 64, 256),
                                   ("ntop2", "twins", "crosser", "late_crosser"), twice_every=3),
    "landings": lambda: landings("landings", M, LEN, [(64, 2, 30, None), (65, 2, 30, None), (130, 2, 30, None),
                                                      (256, 2, 30, None), (257, 2, 30, None)], 16, ("long_big",)),
    "landings_hap": lambda: landings("landings_hap", M, LEN, [(None, 4, 30, 60), (None, 4, 30, 150), (None, 4, 30, 250)], 17,
                                     ("long_big", "big"), hap_every=91),
    "landings_ragged": lambda: landings("landings_ragged", M, LEN, [(None, 4, 30, 28), (None, 4, 30, 90), (None, 4, 30, 160), (None, 4, 30, 236)],
                                        18, ("big", "twins_big", "crosser", "substrings"), ragged=True, dup_every=9, twin=True),
    "private8": lambda: _private("private8", 8, 19),
    "private40": lambda: _private("private40", 40, 20),
}
NAMES = tuple(_BUILDERS)


def _stair_positions(S, widths):
    """positions of a staircase of S whose read has one of `widths` on a side: T = S-1-i + 2 and i + 2"""
    return tuple(sorted(set([w - 2 for w in widths] + [S - 1 - (w - 2) for w in widths])))
_CASES = {}


def _private(name, V, seed):
    """landing items of at most 64 blocks whose extension splits V times, beside a plain island of 100 blocks"""
    rnd = random.Random(seed)
    case = Case(name, M, (), ("big", "private"))
    case.landing_reads = []
    case.private = V
    for W in ((28, 46) if V <= 8 else (46,)):
        case.landing_reads.extend(_add_island(case, rnd, 4, 60, W, LEN, private=V))
    case.landing_reads.extend(_add_island(case, rnd, 2, 30, _fit_island(100, 2, 30, LEN, M), LEN))
    return case


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


# ---- facts ----------------------------------------------------------------------------------------------------------------
class Facts:
    """per (read, side): nA, nB = blocks of the side's two finds; cont[r] = (c0, c1, c2, c3); ntop = top-level blocks after the
    containment blocks are taken out; rounds = symbols from the longest overlap to the end of the shortest read that has it
    (string facts only)"""

    def __init__(self, n):
        self.nA = np.zeros((n, 2), dtype=np.int64)
        self.nB = np.zeros((n, 2), dtype=np.int64)
        self.cont = np.zeros((n, 4), dtype=np.int64)
        self.ntop = np.zeros((n, 2), dtype=np.int64)
        self.rounds = np.zeros((n, 2), dtype=np.int64)

    @property
    def T(self):
        return self.nA + self.nB + self.cont.sum(axis=1)[:, None]

    def slow_bound(self, irreducible):
        """reads that no lane group can finish: a side over FX_BIGCAP blocks in irreducible mode, over 64 in exhaustive mode"""
        return int((self.T > (BIG_HI if irreducible else 64)).any(axis=1).sum())

    def big_items(self):
        return (self.T >= BIG_LO) & (self.T <= BIG_HI)


def string_facts(seqs, m):
    """the facts from the reads alone: dictionaries of every read's prefixes of m bases and more, on both strands"""
    n = len(seqs)
    rcs = [revcomp(s) for s in seqs]
    pre = [{}, {}]  # prefix -> length of the shortest read (as is / reverse-complemented) that starts with it
    for which, ss in enumerate((seqs, rcs)):
        d = pre[which]
        for s in ss:
            for l in range(m, len(s) + 1):
                k = s[:l]
                if d.get(k, 1 << 30) > len(s):
                    d[k] = len(s)
    f = Facts(n)
    same = [set(seqs), set(rcs)]
    for r in range(n):
        q, qc = seqs[r], rcs[r]
        L = len(q)
        # a read that lies inside a longer one (on that strand) is a substring read: that find makes no containment block
        inside = [any(len(t) > L and q in t for t in ss) for ss in (seqs, rcs)]
        c_same = 1 if (q in same[0] and not inside[0]) else 0
        c_opp = 1 if (q in same[1] and not inside[1]) else 0
        f.cont[r] = (c_same, c_opp, c_same, c_opp)
        # find 0: suffix of q = prefix of a read; find 3: = prefix of a reverse-complemented read
        # find 2: prefix of q = suffix of a read <=> suffix of rc(q) = prefix of a reverse-complemented read; find 1 likewise
        for side, (x, dA, dB) in enumerate(((q, pre[0], pre[1]), (qc, pre[0], pre[1]))):
            lens = [[], []]
            for l in range(m, L):
                k = x[L - l:]
                if k in dA:
                    lens[0].append((l, dA[k]))
                if k in dB:
                    lens[1].append((l, dB[k]))
            # (side 1, seen from rc(q): "a read" is the opposite strand -- find 1, list X -- and "a reverse-complemented read"
            # the same strand -- find 2, list Y)
            f.nA[r, side], f.nB[r, side] = len(lens[0]), len(lens[1])
            both = lens[0] + lens[1]
            if both:
                top = max(l for l, _ in both)
                f.ntop[r, side] = sum(1 for l, _ in both if l == top)
                f.rounds[r, side] = min(tl for l, tl in both if l == top) - top
    return f


def oracle_facts(want, lens):
    """the same numbers from the oracle's exhaustive blocks (pyoracle.overlap_batch(..., irreducible=False)): a block belongs
    to the find whose af it carries, and to the containment blocks when it is as long as its read"""
    af = af_of_finds()
    n = len(lens)
    f = Facts(n)
    offs, b = want["block_offs"].astype(np.int64), want["blocks"]
    side_list = {af[0]: (0, 0), af[3]: (0, 1), af[1]: (1, 0), af[2]: (1, 1)}
    for r in range(n):
        top = [[0, 0], [0, 0]]
        for x in b[offs[r]:offs[r + 1]]:
            length, a = int(x[8]), int(x[9])
            if length == int(lens[r]):
                f.cont[r, af.index(a)] += 1
                continue
            side, lst = side_list[a]
            (f.nA if lst == 0 else f.nB)[r, side] += 1
            if length > top[side][0]:
                top[side] = [length, 1]
            elif length == top[side][0]:
                top[side][1] += 1
        f.ntop[r] = (top[0][1], top[1][1])
    return f


def granule_crossers(want, lens):
    """(read, side) items of 65..256 blocks that hold a block whose second capped range -- the one GFx::body_big walks --
    lies across two 128-row granules, from the oracle's exhaustive blocks"""
    af = af_of_finds()
    f = oracle_facts(want, lens)
    big = f.big_items()
    offs, b = want["block_offs"].astype(np.int64), want["blocks"]
    side_of = {af[0]: 0, af[3]: 0, af[1]: 1, af[2]: 1}
    out = set()
    for r in range(len(lens)):
        if not big[r].any():
            continue
        for x in b[offs[r]:offs[r + 1]]:
            if int(x[8]) == int(lens[r]):
                continue
            side = side_of[int(x[9])]
            if big[r, side] and (int(x[2]) >> 7) != (int(x[3]) >> 7):
                out.add((r, side))
    return out


# ---- the sets as fixtures: reads, the oracle's indexes and answers, cached ------------------------------------------------
class Built:
    """a set in the suite's cache directory: <name>.fa, the oracle-built index files, and the oracle's batch answers (kept as
    .npz beside them, so that the child processes of tests/test_gpu_fx_widths.py do not ask again)"""

    def __init__(self, name):
        from oracle import pyoracle as po
        from tests.fixtures import CACHE, md5_prefix
        from tests.golden.make_reads import fasta_text
        self.case = case(name)
        self.name, self.m, self.reads = name, self.case.m, self.case.reads
        self.seqs = self.case.seqs
        self.lens = np.array([len(s) for s in self.seqs], dtype=np.uint32)
        text = fasta_text(self.reads)
        self.dir = os.path.join(CACHE, "fxw_%s_%s" % (name, md5_prefix(text)))  # another generator, another directory
        os.makedirs(self.dir, exist_ok=True)
        self.prefix = os.path.join(self.dir, name)
        self.fa = self.prefix + ".fa"
        if not all(os.path.exists(self.prefix + e) for e in (".fa", ".bwt", ".rbwt", ".sai", ".rsai")):
            po.Index.build(self.seqs).save(self.prefix + ".bwt", self.prefix + ".sai")
            po.Index.build(self.seqs, reverse=True).save(self.prefix + ".rbwt", self.prefix + ".rsai")
            with open(self.fa + ".tmp", "w") as f:
                f.write(text)
            os.replace(self.fa + ".tmp", self.fa)  # last: the files above are complete when this one exists
        self.fwd = po.Index.load(self.prefix + ".bwt", self.prefix + ".sai")
        self.rev = po.Index.load(self.prefix + ".rbwt", self.prefix + ".rsai")
        self._want, self._facts = {}, None

    def want(self, irreducible):
        """pyoracle.overlap_batch over the whole set"""
        from oracle import pyoracle as po
        if irreducible not in self._want:
            path = self.prefix + (".irr" if irreducible else ".exh") + ".want.npz"
            if os.path.exists(path):
                z = np.load(path)
                w = {k: z[k] for k in ("block_offs", "blocks", "substring")}
                w["n_occ_min"] = int(z["n_occ_min"])
            else:
                w = po.overlap_batch(self.fwd, self.rev, self.seqs, self.m, irreducible=irreducible)
                tmp = self.prefix + ".%d.tmp.npz" % os.getpid()
                np.savez(tmp, block_offs=w["block_offs"], blocks=w["blocks"], substring=w["substring"], n_occ_min=np.uint64(w["n_occ_min"]))
                os.replace(tmp, path)
            self._want[irreducible] = w
        return self._want[irreducible]

    def facts(self):
        if self._facts is None:
            self._facts = string_facts(self.seqs, self.m)
        return self._facts

    def edges(self, irreducible):
        """the edge records that follow from the oracle's blocks (tests.bigcheck.expected_edges), by name rank"""
        from siga_amd.overlap import name_ranks
        from tests.bigcheck import expected_edges
        w = self.want(irreducible)
        if "edges" not in w:
            self.ranks = name_ranks([n for n, _ in self.reads])
            w["edges"] = expected_edges(w["blocks"], w["block_offs"], self.fwd.sai(), self.rev.sai(), self.lens, self.ranks)
        return w["edges"]

    def oracle_text(self, irreducible):
        """(ASQG text, hits text) of pyoracle.build_asqg with rc on"""
        from oracle import pyoracle as po
        tag = "irr" if irreducible else "exh"
        out, hp = self.prefix + "." + tag + ".oracle.asqg", self.prefix + "." + tag + ".oracle.hits"
        if not (os.path.exists(out) and os.path.exists(hp)):
            tmp = "%s.%d.tmp" % (self.prefix, os.getpid())
            po.build_asqg(self.fwd, self.rev, self.fa, self.m, tmp + ".asqg", tmp + ".hits", irreducible, True)
            os.replace(tmp + ".hits", hp)
            os.replace(tmp + ".asqg", out)
        return open(out).read(), open(hp).read()


_BUILT = {}


def built(name):
    if name not in _BUILT:
        _BUILT[name] = Built(name)
    return _BUILT[name]


def late_crossers(b, verbose=False):
    """Items of 65..256 blocks that GFx::body_big carries to the round in which their top-level blocks end, while one of those
    top-level ranges lies across two 128-row granules in that round.  Walks the single-group extension on the oracle's
    indexes (FMIndex::getChar, getOcc, getPC) from the exhaustive blocks, as body_big does from the candidates: a round is
    common when every block's range sits in one granule and all blocks read the same next symbol.
    Returns ({(read, side)}, counters)."""
    af = af_of_finds()
    want = b.want(False)
    big = oracle_facts(want, b.lens).big_items()
    offs, blocks = want["block_offs"].astype(np.int64), want["blocks"]
    side_of = {af[0]: 0, af[3]: 0, af[1]: 1, af[2]: 1}
    rank = {"$": 0, "A": 1, "C": 2, "G": 3, "T": 4}
    index = {a: (b.rev if a in (af[0], af[1]) else b.fwd) for a in af}  # OverlapBlock::index: finds 0 and 1 extend on the reverse index
    pred = {id(ix): ix.pred() for ix in (b.fwd, b.rev)}
    out, count = set(), {"items": 0, "left_before_the_end": 0, "ended": 0}
    count["left"] = set()
    for r in range(len(b.lens)):
        for side in (0, 1):
            if not big[r, side]:
                continue
            mem = [[int(x[2]), int(x[3]), int(x[8]), int(x[9])] for x in blocks[offs[r]:offs[r + 1]]
                   if side_of[int(x[9])] == side and int(x[8]) != int(b.lens[r])]
            top = max(x[2] for x in mem)
            count["items"] += 1
            for _ in range(int(b.lens.max()) + 1):
                cross, syms, ends = [], [], []
                for lo, hi, length, a in mem:
                    ix = index[a]
                    if (lo >> 7) != (hi >> 7):
                        cross.append(length == top)
                        syms.append(None)
                        ends.append(False)
                        continue
                    cs = {rank[ix.getchar(i)] for i in range(lo, hi + 1)}
                    c = min(cs - {0}) if cs - {0} else 0
                    syms.append((5 - c if (a & 4) and c else c) if len(cs) == 1 else None)
                    ends.append(0 in cs)
                if any(e and x[2] == top for e, x in zip(ends, mem)):
                    count["ended"] += 1
                    if any(cross):
                        out.add((r, side))
                    break
                if None in syms or syms[0] == 0 or len(set(syms)) != 1:
                    count["left_before_the_end"] += 1
                    count["left"].add((r, side))
                    break
                for x in mem:
                    ix = index[x[3]]
                    c = rank[ix.getchar(x[0])]
                    before = int(ix.occ(x[0] - 1)[c]) if x[0] > 0 else 0
                    lo = int(pred[id(ix)][c]) + before
                    x[0], x[1] = lo, lo + (x[1] - x[0])
    return out, count


def exposed_late_crossers(b):
    """late_crossers whose read has nothing else that sends it to the general kernel -- which redoes both sides of a read and
    would cover up what the lane group made of the item: the other side has at most FX_BIGCAP blocks, and when it is a
    body_big item itself it runs to its end without such a crossing"""
    hits, st = late_crossers(b)
    T = b.facts().T
    return sorted((r, s) for r, s in hits if T[r, 1 - s] <= BIG_HI and (r, 1 - s) not in st["left"] and (r, 1 - s) not in hits)
