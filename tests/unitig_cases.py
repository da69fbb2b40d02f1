"""Cases and brute force for `siga unitig` (csrc/sigax_unitig.hip); no tests here (tests/test_unitig_cases.py, tests/test_gpu_unitig.py).

expected()   a direct serial restatement of the rules in include/sigax.h: degrees, simple records, walks.
reference()  the reference's own loop (Bigraph::simplify, src/bigraph.cpp:341-414; Vertex::merge, :131-202) written out: a dict of
             vertices, the SENSE pass, then the ANTISENSE pass, pairwise merges until nothing changes.
The two share nothing but revcomp() and the record classifier, and are compared as sets of canonical sequences.

A case: dict(name, reads [bytes by read id], edges [(query, target, length, af)], m).  In every case the SIMPLE records are
real overlaps of the reads' bytes (the others need not be: nothing is merged over them), so a placement's read, as placed,
equals its unitig's bytes at its offset."""
import functools
import random

import numpy as np

B, E = 0, 1
PLACED_REV = 1
CIRCULAR = 1
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
EDGE_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4"), ("length", "<u4"), ("af", "<u4")])  # sigax_edge


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def classify(rec, lens, m):
    """-> "bad" | "low" | (state of query, state of target, containment, self edge); state = 2 * read + end"""
    q, t, ln, af = rec
    n = len(lens)
    if q >= n or t >= n:
        return "bad"
    if af not in (0b000, 0b110, 0b101, 0b011):
        return "bad"
    if ln == 0 or ln > min(lens[q], lens[t]):
        return "bad"
    if ln < m:
        return "low"
    return (2 * q + (B if af & 1 else E), 2 * t + (E if af & 2 else B), ln == lens[q] or ln == lens[t], q == t)


def nbases(read):
    """a read's length: a read is its bytes or, where no step reads them (tables_only), a bare length"""
    return read if isinstance(read, int) else len(read)


def unit_bytes(reads, lay):
    """the bytes of the unitig a layout [(read, flags, offset)] lays out; a read given as a bare length is an assertion failure"""
    seq = bytearray()
    for read, fl, off in lay:
        assert not isinstance(reads[read], int), "the bytes of read %d are needed, and it was given as a length" % read
        placed = revcomp(reads[read]) if fl & PLACED_REV else bytes(reads[read])
        seq += placed[len(seq) - off:]
    return bytes(seq)


# ---- the rules, serially ----
def expected(reads, edges, m, tables_only=False):
    """-> dict(seq_offs, lay_offs, uflags, layout [(read, flags, offset)], useqs bytes, status [6]).  tables_only: no bytes are
    built, a read may be a bare length, useqs is None and everything else is as without it"""
    n = len(reads)
    lens = [nbases(r) for r in reads]
    deg = [0] * (2 * n)
    bad = low = 0
    kept = []
    for rec in edges:
        c = classify(rec, lens, m)
        if c == "bad":
            bad += 1
        elif c == "low":
            low += 1
        else:
            kept.append((c, rec[2]))
            sq, st, contain, _ = c
            if contain:
                for s in (sq & ~1, sq | 1, st & ~1, st | 1):
                    deg[s] += 1
            else:
                deg[sq] += 1
                deg[st] += 1
    link = {}
    simple = 0
    for (sq, st, contain, self_edge), ln in kept:
        if not contain and not self_edge and deg[sq] == 1 and deg[st] == 1:
            link[sq] = (st, ln)
            link[st] = (sq, ln)
            simple += 1
    seen = [False] * n
    unitigs = []  # (start read, [(read, rev, offset)], circular, closing overlap)
    for r in range(n):
        if seen[r]:
            continue
        # r is the smallest id of its component.  Walk from it leaving through E: back at r = a cycle
        comp, s, cyc = [r], 2 * r + E, False
        while s in link:
            nxt = link[s][0]
            if nxt >> 1 == r:
                cyc = True
                break
            comp.append(nxt >> 1)
            s = nxt ^ 1
        if not cyc:
            s = 2 * r + B
            while s in link:
                nxt = link[s][0]
                comp.append(nxt >> 1)
                s = nxt ^ 1
        for x in comp:
            assert not seen[x]
            seen[x] = True
        if cyc:
            start, out = r, E
        else:
            ends = [x for x in comp if (2 * x + B) not in link or (2 * x + E) not in link]
            start = min(ends)
            out = E if (2 * start + E) in link else B
            if len(comp) == 1:
                out = E
        lay, off, cur, left, closing = [(start, 0 if out == E else PLACED_REV, 0)], 0, start, out, 0
        while (2 * cur + left) in link:
            nxt, ln = link[2 * cur + left]
            if nxt >> 1 == start:
                closing = ln
                break
            off += lens[cur] - ln
            cur, left = nxt >> 1, (nxt & 1) ^ 1
            lay.append((cur, 0 if nxt & 1 == B else PLACED_REV, off))
        assert len(lay) == len(comp)
        unitigs.append((start, lay, cyc, closing))
    unitigs.sort(key=lambda u: u[0])
    seq_offs, lay_offs, uflags, layout, useqs = [0], [0], [], [], bytearray()
    for start, lay, cyc, closing in unitigs:
        bases = lay[-1][2] + lens[lay[-1][0]]
        if not tables_only:
            seq = unit_bytes(reads, lay)
            assert len(seq) == bases
            useqs += seq
        layout += lay
        seq_offs.append(seq_offs[-1] + bases)
        lay_offs.append(len(layout))
        uflags.append((CIRCULAR | (closing << 1)) if cyc else 0)
    ncyc = sum(1 for u in unitigs if u[2])
    return {"seq_offs": seq_offs, "lay_offs": lay_offs, "uflags": uflags, "layout": layout, "useqs": None if tables_only else bytes(useqs),
            "status": [len(unitigs), seq_offs[-1], bad, low, simple - ncyc, ncyc]}


NEEDED = None  # a set here collects id() of every read object whose bytes a tables_only run asked for


class LazySeqs:
    """the unitigs' bytes of a tables_only result, each built when a step asks for it: seqs[u] as bytes"""

    def __init__(self, reads, res):
        self.reads, self.res = reads, res

    def __len__(self):
        return len(self.res["uflags"])

    def __getitem__(self, u):
        lay = self.res["layout"][self.res["lay_offs"][u]:self.res["lay_offs"][u + 1]]
        if NEEDED is not None:
            NEEDED.update(id(self.reads[r]) for r, _, _ in lay)
        return unit_bytes(self.reads, lay)


# ---- the reference's loop ----
class _Edge:
    __slots__ = ("start", "dir", "twin", "len", "block")

    def end(self):
        return self.twin.start


def reference(reads, edges, m):
    """-> list of (sequence, circular, overlap of the edge left on a circular vertex)"""
    lens = [len(r) for r in reads]
    verts = {i: {"seq": bytes(r), "edges": []} for i, r in enumerate(reads)}

    def pair(sa, sb, ln, block):
        a, b = _Edge(), _Edge()
        a.start, a.dir, a.twin, a.len, a.block = sa >> 1, sa & 1, b, ln, block
        b.start, b.dir, b.twin, b.len, b.block = sb >> 1, sb & 1, a, ln, block
        verts[a.start]["edges"].append(a)
        verts[b.start]["edges"].append(b)

    for rec in edges:  # Bigraph::load: the minOverlap filter, EdgeCreator::create, containments in both directions
        c = classify(rec, lens, m)
        if c in ("bad", "low"):
            continue
        sq, st, contain, _ = c
        if contain:
            pair(sq, st, rec[2], True)
            pair(sq ^ 1, st ^ 1, rec[2], True)
        else:
            pair(sq, st, rec[2], False)

    def simplify(d):
        changed = True
        while changed:
            changed = False
            for vid in list(verts):
                if vid not in verts:
                    continue
                v = verts[vid]
                es = [e for e in v["edges"] if e.dir == d]
                if len(es) != 1 or es[0].end() == vid:
                    continue
                single, twin = es[0], es[0].twin
                wid = single.end()
                w = verts[wid]
                if sum(1 for e in w["edges"] if e.dir == twin.dir) != 1 or single.block:
                    continue
                # Vertex::merge: the label is what w holds beyond the overlap, as seen from v
                if d == E:
                    o = w["seq"] if twin.dir == B else revcomp(w["seq"])
                    v["seq"] = v["seq"] + o[single.len:]
                else:
                    o = w["seq"] if twin.dir == E else revcomp(w["seq"])
                    v["seq"] = o[:len(o) - single.len] + v["seq"]
                # Bigraph::merge: w's edges of the other direction become v's, in this direction
                for x in [e for e in w["edges"] if e.dir == 1 - twin.dir]:
                    w["edges"].remove(x)
                    x.start, x.dir = vid, d
                    v["edges"].append(x)
                v["edges"].remove(single)
                w["edges"].remove(twin)
                assert not w["edges"]
                del verts[wid]
                changed = True

    simplify(E)
    simplify(B)
    out = []
    for vid, v in verts.items():
        loops = [e for e in v["edges"] if not e.block and e.end() == vid and e.dir == E and e.twin.dir == B and e.twin is not e]
        merged_loop = [e for e in loops if len(v["seq"]) > lens[vid]]  # a self edge that merging made, not one the input gave
        if merged_loop:
            out.append((v["seq"], True, merged_loop[0].len))
        else:
            out.append((v["seq"], False, 0))
    return out


def canonical(seq, circular=False, closing=0):
    """min(s, revcomp(s)); a circular one without the bases its closing overlap repeats, smallest rotation of both strands"""
    seq = bytes(seq)
    if not circular:
        return min(seq, revcomp(seq))
    s = seq[:len(seq) - closing]
    best = None
    for t in (s, revcomp(s)):
        tt = t + t
        for i in range(len(t)):
            c = tt[i:i + len(t)]
            if best is None or c < best:
                best = c
    return b"@" + best


def canonical_set(exp):
    out = []
    for u in range(len(exp["uflags"])):
        seq = exp["useqs"][exp["seq_offs"][u]:exp["seq_offs"][u + 1]]
        out.append(canonical(seq, bool(exp["uflags"][u] & CIRCULAR), exp["uflags"][u] >> 1))
    return sorted(out)


# ---- hand-built graphs ----
class _Build:
    def __init__(self, seed, m=20):
        self.rng = random.Random(seed)
        self.reads, self.edges, self.m = [], [], m

    def genome(self, n):
        return bytes(self.rng.choice(b"ACGT") for _ in range(n))

    def chain(self, n, rc=None, qfirst=None, order=None, lens=None, circular=False, with_n=False):
        """n reads tiling a fresh random genome left to right, each overlapping the next by at least m and containing
        none.  rc[i]: read i is stored reverse-complemented; qfirst[i]: the record of (i, i+1) names i as its query;
        order[i]: read i's id among the chain's n ids.  circular: the genome is a ring and read n-1 overlaps read 0.
        -> the ids by position"""
        rng = self.rng
        rc = rc or [False] * n
        order = order or list(range(n))
        if circular:  # (long reads, short overlaps: the ring is longer than any read, a 2-ring's too)
            lens = lens or [rng.randint(self.m + 35, self.m + 40) for _ in range(n)]
        lens = lens or [rng.randint(self.m + 10, self.m + 40) for _ in range(n)]
        nlinks = n if circular else n - 1
        qfirst = qfirst or [rng.random() < 0.5 for _ in range(nlinks)]
        ov = []
        for i in range(nlinks):
            a, b = lens[i], lens[(i + 1) % n]
            ov.append(rng.randint(self.m, self.m + 2) if circular else rng.randint(min(self.m, min(a, b) - 1), min(a, b) - 1))
        pos = [0]
        for i in range(nlinks):
            pos.append(pos[-1] + lens[i] - ov[i])
        glen = pos[n] if circular else pos[n - 1] + lens[n - 1]
        g = bytearray(self.genome(glen))
        if circular:
            assert all(l <= glen for l in lens), "a read longer than the ring"
        if with_n:
            g[pos[n // 2] + 1] = ord("N")
        gg = bytes(g) + bytes(g)
        base = len(self.reads)
        ids = [base + order[i] for i in range(n)]
        self.reads += [None] * n
        for i in range(n):
            w = gg[pos[i]:pos[i] + lens[i]]
            self.reads[ids[i]] = revcomp(w) if rc[i] else w
        for i in range(nlinks):
            x, y = i, (i + 1) % n
            if qfirst[i]:  # query x (left on the genome), target y
                af = (1 if rc[x] else 0) | (2 if rc[y] else 0)
                q, t = ids[x], ids[y]
            else:  # query y touches its B end when stored forward, target x its E end when stored forward
                af = (0 if rc[y] else 1) | (0 if rc[x] else 2)
                q, t = ids[y], ids[x]
            af |= ((af ^ (af >> 1)) & 1) << 2
            self.edges.append((q, t, ov[i], af))
        return ids

    def read(self, seq):
        self.reads.append(bytes(seq))
        return len(self.reads) - 1

    def case(self, name):
        assert all(r is not None for r in self.reads)
        e = list(self.edges)
        self.rng.shuffle(e)  # records in any order
        return {"name": name, "reads": list(self.reads), "edges": e, "m": self.m}


@functools.lru_cache(maxsize=None)
def hand_built():
    cases = []
    for n in (1, 2, 3, 63, 64, 65, 1000):  # across the jumping rounds and the wave width
        b = _Build(100 + n)
        b.chain(n, rc=[b.rng.random() < 0.5 for _ in range(n)])
        cases.append(b.case("chain%d" % n))
    for k, (rx, ry, qf) in enumerate([(False, False, True), (False, True, True), (True, False, True), (True, True, True)]):
        b = _Build(200 + k)  # each of the four af values, as (left, right) and as (right, left)
        b.chain(2, rc=[rx, ry], qfirst=[qf])
        b.chain(2, rc=[rx, ry], qfirst=[not qf])
        b.chain(3, rc=[rx, ry, rx], qfirst=[qf, not qf])
        assert len({e[3] for e in b.edges}) >= 1
        cases.append(b.case("af%d" % k))
    assert {e[3] for c in cases[-4:] for e in c["edges"]} == {0, 3, 5, 6}
    b = _Build(300)  # the smaller-id terminal at either end, on either strand: the head is left through B or through E
    for rc0 in (False, True):
        b.chain(5, rc=[rc0, False, True, False, rc0], order=[0, 3, 2, 1, 4])
        b.chain(5, rc=[rc0, True, False, True, rc0], order=[4, 1, 2, 3, 0])
        b.chain(2, rc=[rc0, not rc0], order=[1, 0])
    cases.append(b.case("heads"))
    b = _Build(301)  # a Y branch: x's E end meets y and z
    x, y = b.chain(2)
    z = b.read(b.reads[y][:25] + b.genome(20))
    b.edges.append((x, z, 22, 0))
    b.chain(3)
    cases.append(b.case("branch"))
    b = _Build(302)  # a containment blocks both ends of both its reads
    ids = b.chain(4)
    s = b.read(b.reads[ids[1]][5:30])
    b.edges.append((ids[1], s, 25, 0))
    cases.append(b.case("containment"))
    b = _Build(303)  # self edges: E to B, and both touches at E
    ids = b.chain(3, rc=[False, False, False])
    b.edges.append((ids[2], ids[2], 21, 0))
    ids = b.chain(3, rc=[False, False, False])
    b.edges.append((ids[2], ids[2], 21, 6))
    r = b.read(b.genome(40))
    b.edges.append((r, r, 40, 0))
    cases.append(b.case("self"))
    b = _Build(304)  # two records between one pair of ends
    b.chain(2, rc=[False, False])
    b.edges.append(b.edges[0])
    b.chain(2)
    cases.append(b.case("double"))
    for n in (2, 3, 65):
        b = _Build(400 + n)
        b.chain(n, circular=True, rc=[b.rng.random() < 0.5 for _ in range(n)])
        b.chain(2)
        cases.append(b.case("cycle%d" % n))
    b = _Build(410)  # the smallest id mid-list, stored on either strand
    b.chain(7, circular=True, order=[4, 5, 6, 0, 1, 2, 3], rc=[False, True, False, True, True, False, False])
    b.chain(6, circular=True, order=[3, 4, 5, 0, 1, 2], rc=[True] * 6)
    cases.append(b.case("cycle_mid"))
    b = _Build(500, m=1)  # lengths 2 .. 300
    lens = [2, 300, 3, 2, 299, 150, 17, 16, 15, 33, 2, 2, 64, 65, 300, 300, 5]
    b.chain(len(lens), lens=lens, rc=[b.rng.random() < 0.5 for _ in lens])
    b.chain(40, lens=[b.rng.randint(2, 300) for _ in range(40)], rc=[b.rng.random() < 0.5 for _ in range(40)])
    cases.append(b.case("lengths"))
    b = _Build(501)
    b.chain(5, with_n=True, rc=[False, True, True, False, True])
    assert any(b"N" in r for r in b.reads)
    cases.append(b.case("withN"))
    b = _Build(502)  # one malformed record of each kind, and records below m; none of them may count at an end
    ids = b.chain(6)
    n = len(b.reads)
    L = len(b.reads[ids[0]])
    bad = [(n, ids[0], 25, 0), (ids[0], n, 25, 0), (0xFFFFFFFF, 0xFFFFFFFF, 25, 0), (ids[0], ids[1], 25, 1), (ids[0], ids[1], 25, 2),
           (ids[0], ids[1], 25, 4), (ids[0], ids[1], 25, 7), (ids[0], ids[1], 25, 8), (ids[0], ids[1], 25, 16), (ids[2], ids[3], 25, 0x80000000),
           (ids[2], ids[3], 0, 0), (ids[2], ids[3], 1000, 0), (ids[2], ids[3], 0xFFFFFFFF, 3), (ids[1], ids[2], L + 100, 5)]
    low = [(ids[2], ids[3], 19, 0), (ids[4], ids[0], 1, 6), (ids[5], ids[5], 19, 0)]
    b.edges += bad + low
    c = b.case("malformed")
    c["n_bad"], c["n_low"] = len(bad), len(low)
    cases.append(c)
    b = _Build(503)
    for _ in range(5):
        b.read(b.genome(30))
    cases.append(b.case("no_edges"))
    return cases


def arrays(case):
    """-> (edges EDGE_DTYPE[n_edges], lengths u32[n], seqs bytes, offs u64[n+1])"""
    reads = case["reads"]
    lengths = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths, dtype=np.uint64)
    edges = np.ascontiguousarray(np.array(case["edges"], dtype=np.uint64).astype(np.uint32).reshape(-1, 4)).view(EDGE_DTYPE).reshape(-1)
    return edges, lengths, b"".join(reads), offs


# ---- end to end ----
E2E_SEED, E2E_GENOME, E2E_READS, E2E_LEN, E2E_M = 7, 6000, 600, 60, 25


@functools.lru_cache(maxsize=None)
def end_to_end():
    """a 6 000-base random genome without a repeat of E2E_M bases (either strand), 600 error-free reads of 60, both strands"""
    rng = random.Random(E2E_SEED)
    g = bytes(rng.choice(b"ACGT") for _ in range(E2E_GENOME))
    reads = []
    for i in range(E2E_READS):
        p = rng.randrange(E2E_GENOME - E2E_LEN + 1)
        w = g[p:p + E2E_LEN]
        reads.append(("r%d" % i, revcomp(w) if rng.random() < 0.5 else w))
    return {"genome": g, "reads": reads, "m": E2E_M}


def longest_repeat_at_least(g, k):
    """does some k-mer of g occur twice in g, or in g and revcomp(g)?"""
    seen = set()
    for s in (g, revcomp(g)):
        mine = set()
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if w in mine or w in seen:
                return True
            mine.add(w)
        seen |= mine
    return False


def render(names, res):
    """the FASTA and layout texts `siga unitig` writes for a result (expected()'s dict, or the wrapper's with lists)"""
    fa, lay = [], []
    for u in range(len(res["uflags"])):
        a, b = int(res["lay_offs"][u]), int(res["lay_offs"][u + 1])
        head = ">unitig-%d" % u
        if b - a > 1:
            head += " KC:i:%d" % (b - a)
        if int(res["uflags"][u]) & CIRCULAR:
            head += " circular=%d" % (int(res["uflags"][u]) >> 1)
        seq = bytes(res["useqs"][int(res["seq_offs"][u]):int(res["seq_offs"][u + 1])])
        fa.append(head + "\n" + seq.decode() + "\n")
        for read, fl, off in res["layout"][a:b]:
            lay.append("unitig-%d\t%s\t%s\t%d\n" % (u, names[int(read)], "-" if int(fl) & PLACED_REV else "+", int(off)))
    return "".join(fa), "".join(lay)
