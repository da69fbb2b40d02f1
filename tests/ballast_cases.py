"""Ballast in front of a hand-built case of `siga unitig`: reads without records (and one joined pair) that take the read ids
0 .. k-1, so that the case behind them lies at large offsets -- beyond 2^32 in tests/test_gpu_unitig_wide.py -- while its
expected result follows from the small case's by shifting.  No tests here (tests/test_ballast_cases.py holds the shift rule
against the restatements with small ballast; tests/test_gpu_unitig_wide.py uses it where no restatement can run).

A ballast item is a length (a read on its own) or (la, lb, ov): two reads a < b that overlap by ov bases, b stored
reverse-complemented, joined by one record whose flags follow unitig_cases._Build.chain's rule.  A read on its own is one
unitig, forward, at offset 0, its bases its own; the pair is one unitig of the placements (a, forward, 0) and
(b, SIGAX_PLACED_REV, la - ov) with la + lb - ov bases and one merged record.  A longer tuple (l0, .., ln-1, ov0, .., ovn-2) is
the same thing with n reads, every second one stored reverse-complemented: lengths are u32, so only a third read can lie at an
offset beyond 2^32 in its unitig.  By the numbering rule (ascending first read) the ballast unitigs come first, in item
order.  Behind them the case's result is shifted:
  read ids + k (records and layout), unitig numbers + U, lay_offs + k, seq_offs + B, status[0] + U, status[1] + B, merged
  records + the pairs; k = ballast reads, U = ballast unitigs, B = their bases.
Tip trimming sees a ballast unitig as what it is, an island: with max_rounds >= 1 it goes in round 1 iff its bases <= L (and
the coverage test passes), and then has no unitig, no placement, removed[] = 1, and counts as an island; ballast above L stays
and removed[] begins with zeros.  The case's own rounds do not change; the count of removing rounds is at least 1 once ballast
went.  The lifted records are renumbered by the ballast unitigs that stay.
Scaffolds: ballast unitigs in front, a length or (lu, lv, gap): unitigs u < v joined by one link between u's E end and v's E
end, so that v lies reversed lu + gap bases into the scaffold; link keys of the case + 2 k."""
from tests import unitig_cases as uc

U32 = 0xFFFFFFFF


def pair_af(rc_x=False, rc_y=True):
    """_Build.chain's flag rule for x (left, stored reverse-complemented iff rc_x) and y (right), x named as the query"""
    af = (1 if rc_x else 0) | (2 if rc_y else 0)
    return af | (((af ^ (af >> 1)) & 1) << 2)


def item_chain(it):
    """a tuple item -> (lengths, overlaps)"""
    n = (len(it) + 1) // 2
    assert len(it) == 2 * n - 1 and n >= 2
    return list(it[:n]), list(it[n:])


class Ballast:
    """items -> lens [k] by read id, edges (the pairs' records), units [(bases, [(read, flags, offset)])] in unitig order"""

    def __init__(self, items):
        self.items = list(items)
        self.lens, self.edges, self.units = [], [], []
        for it in self.items:
            r = len(self.lens)
            if isinstance(it, int):
                self.lens.append(it)
                self.units.append((it, [(r, 0, 0)]))
            else:
                lens, ovs = item_chain(it)
                lay, off = [(r, 0, 0)], 0
                for i, ov in enumerate(ovs):
                    assert 0 < ov < min(lens[i], lens[i + 1]), "an overlap that contains neither read"
                    assert i == 0 or ovs[i - 1] + ov <= lens[i], "a read's two overlaps overlap"
                    self.edges.append((r + i, r + i + 1, ov, pair_af(i % 2 == 1, i % 2 == 0)))
                    off += lens[i] - ov
                    lay.append((r + i + 1, uc.PLACED_REV if i % 2 == 0 else 0, off))
                self.lens += lens
                self.units.append((off + lens[-1], lay))
        self.k = len(self.lens)
        self.read_bases = sum(self.lens)
        self.read_offs = [0]
        for n in self.lens:
            self.read_offs.append(self.read_offs[-1] + n)

    def unit_seqs(self, reads):
        """the ballast unitigs' bytes from the ballast reads' (small ballast only)"""
        out = []
        for _, lay in self.units:
            seq = bytearray()
            for r, fl, off in lay:
                placed = uc.revcomp(reads[r]) if fl & uc.PLACED_REV else bytes(reads[r])
                assert bytes(seq[off:]) == placed[:len(seq) - off], "the pair's reads do not overlap as its record says"
                seq += placed[len(seq) - off:]
            out.append(bytes(seq))
        return out


def small_reads(bal, rng):
    """random bytes for small ballast, a pair's reads overlapping as their record says -> [bytes] by read id"""
    reads = []
    for it in bal.items:
        if isinstance(it, int):
            reads.append(bytes(rng.choice(b"ACGT") for _ in range(it)))
        else:
            lens, ovs = item_chain(it)
            g = bytes(rng.choice(b"ACGT") for _ in range(sum(lens) - sum(ovs)))
            at = 0
            for i, n in enumerate(lens):
                reads.append(uc.revcomp(g[at:at + n]) if i % 2 else g[at:at + n])
                at += n - (ovs[i] if i < len(ovs) else 0)
    return reads


def shift_id(x, k):
    """a read id of the case behind k ballast reads (an id beyond the reads stays beyond them, within u32)"""
    return min(x + k, U32)


def concat_tables(case, bal):
    """the tables of the case behind the ballast, no bytes -> (edges, lengths, offs [k + n + 1])"""
    assert all(e[2] >= case["m"] for e in bal.edges), "the pair's overlap lies below the case's min_overlap"
    edges = list(bal.edges) + [(shift_id(q, bal.k), shift_id(t, bal.k), ln, af) for q, t, ln, af in case["edges"]]
    lengths = list(bal.lens) + [len(r) for r in case["reads"]]
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + n)
    return edges, lengths, offs


def concat_case(case, bal, ballast_reads):
    """the case with the ballast in front: what the restatement (small ballast) or the device (tables only) is given"""
    assert all(len(r) == n for r, n in zip(ballast_reads, bal.lens)) and len(ballast_reads) == bal.k
    out = dict(case)
    out["reads"] = list(ballast_reads) + list(case["reads"])
    out["edges"] = concat_tables(case, bal)[0]
    return out


def _tables(units, k_placed, exp):
    """ballast units in front of exp's tables -> seq_offs, lay_offs, uflags, layout (the case's read ids not yet shifted)"""
    seq_offs, lay_offs, layout = [0], [0], []
    for bases, lay in units:
        seq_offs.append(seq_offs[-1] + bases)
        lay_offs.append(lay_offs[-1] + len(lay))
        layout += lay
    assert lay_offs[-1] == k_placed
    bu = seq_offs[-1]
    return (seq_offs[:-1] + [x + bu for x in exp["seq_offs"]], lay_offs[:-1] + [x + k_placed for x in exp["lay_offs"]],
            [0] * len(units) + list(exp["uflags"]), layout)


def shifted_unitigs(exp, bal, unit_seqs=None):
    """unitig_cases.expected's dict of the case -> that of the case behind the ballast.  useqs: the whole bytes when the ballast
    unitigs' are given, else None; case_useqs / case_at: the case's bytes and where they begin"""
    seq_offs, lay_offs, uflags, layout = _tables(bal.units, bal.k, exp)
    bu, nu = sum(b for b, _ in bal.units), len(bal.units)
    st = exp["status"]
    return {"seq_offs": seq_offs, "lay_offs": lay_offs, "uflags": uflags,
            "layout": layout + [(r + bal.k, fl, off) for r, fl, off in exp["layout"]],
            "useqs": None if unit_seqs is None else b"".join(unit_seqs) + exp["useqs"], "case_useqs": exp["useqs"], "case_at": bu,
            "status": [st[0] + nu, st[1] + bu, st[2], st[3], st[4] + len(bal.edges), st[5]]}


def ballast_trimmed(bal, max_rounds, L, C=None):
    """which ballast units a trim call removes (all in round 1: each is an island from the start) -> [bool] by unit"""
    gone = []
    for bases, lay in bal.units:
        short = max_rounds >= 1 and bases <= L
        if short and C is not None:
            short = (len(lay) - 1) * max(L, 1) <= (max(C, 1) - 1) * bases
        gone.append(short)
    return gone


def shifted_trim(exp, bal, max_rounds, L, C=None, unit_seqs=None):
    """trim_cases.expected_trim's dict of the case -> that of the case behind the ballast"""
    gone = ballast_trimmed(bal, max_rounds, L, C)
    stay = [u for u, g in zip(bal.units, gone) if not g]
    reads_gone = sum(len(lay) for (_, lay), g in zip(bal.units, gone) if g)
    pairs_gone = sum(len(lay) - 1 for (_, lay), g in zip(bal.units, gone) if g)  # the records inside ballast that went
    seq_offs, lay_offs, uflags, layout = _tables(stay, bal.k - reads_gone, exp)
    bu, nu = sum(b for b, _ in stay), len(stay)
    removed = [0] * bal.k
    for (_, lay), g in zip(bal.units, gone):
        for r, _, _ in lay:
            removed[r] = 1 if g else 0
    st = list(exp["status"])
    st[0] += nu
    st[1] += bu
    st[4] += len(bal.edges) - pairs_gone
    if any(gone):
        st[6] = max(st[6], 1)
    st[7] += sum(gone)
    st[9] += reads_gone
    st[10] += pairs_gone
    seqs = None if unit_seqs is None else b"".join(s for s, g in zip(unit_seqs, gone) if not g) + exp["useqs"]
    return {"seq_offs": seq_offs, "lay_offs": lay_offs, "uflags": uflags, "layout": layout + [(r + bal.k, fl, off) for r, fl, off in exp["layout"]],
            "useqs": seqs, "case_useqs": exp["useqs"], "case_at": bu, "status": st, "removed": removed + list(exp["removed"]),
            "uedges": [(q + nu, t + nu, ln, af) for q, t, ln, af in exp["uedges"]], "ballast_gone": gone}


# ---- scaffolds ----
class ScaffoldBallast:
    """items: a length (a unitig on its own) or (lu, lv, gap) -> lens [k] by unitig, links (insert size `insert_size`), scaffolds
    [(bases, [(unitig, flags, offset)], [gap before each placement])]"""

    def __init__(self, items, insert_size, count=5):
        self.items, self.lens, self.links, self.scaffolds = list(items), [], [], []
        for it in self.items:
            u = len(self.lens)
            if isinstance(it, int):
                self.lens.append(it)
                self.scaffolds.append((it, [(u, 0, 0)], [0]))
            else:
                lu, lv, gap = it
                assert 0 < gap <= insert_size
                self.lens += [lu, lv]
                span = insert_size - gap  # scaffold_cases.gap_of: gap = insert - mean span
                self.links.append((2 * u + 1, 2 * (u + 1) + 1, count, span, span * count))  # E of u, E of v: v lies reversed
                self.scaffolds.append((lu + gap + lv, [(u, 0, 0), (u + 1, uc.PLACED_REV, lu + gap)], [0, gap]))
        self.k = len(self.lens)
        self.bases = sum(self.lens)


def raise_spans(links, d):
    """every link's spans + d: under an insert size raised by d the gaps are what they were"""
    return [(a, b, c, mn + d, sm + d * c) for a, b, c, mn, sm in links]


def concat_scaffold_input(res, links, bal, ballast_useqs=None):
    """(res, links) of a scaffold case behind the ballast unitigs; useqs only when the ballast's bytes are given"""
    offs = [0]
    for n in bal.lens:
        offs.append(offs[-1] + n)
    out = {"seq_offs": offs[:-1] + [int(x) + bal.bases for x in res["seq_offs"]], "uflags": [0] * bal.k + [int(x) for x in res["uflags"]]}
    if ballast_useqs is not None:
        assert len(ballast_useqs) == bal.bases
        out["useqs"] = bytes(ballast_useqs) + bytes(res["useqs"])
    return out, list(bal.links) + [(a + 2 * bal.k, b + 2 * bal.k, c, mn, sm) for a, b, c, mn, sm in links]


def shifted_scaffolds(exp, bal, ballast_seqs=None):
    """scaffold_cases.expected_scaffolds' dict (capacity: exactly enough) of the case -> that of the case behind the ballast.
    ballast_seqs: the ballast scaffolds' bytes, for the whole `seqs`"""
    sc_offs, sc_lay_offs, layout, gaps = [0], [0], [], []
    for bases, lay, g in bal.scaffolds:
        sc_offs.append(sc_offs[-1] + bases)
        sc_lay_offs.append(sc_lay_offs[-1] + len(lay))
        layout += lay
        gaps += g
    total, ns = sc_offs[-1], len(bal.scaffolds)
    st = list(exp["status"])
    st[0] += ns
    st[1] += total
    st[2] += len(bal.links)
    st[10] += len(bal.links)
    st[12] += sum(gaps)
    seqs = None
    if ballast_seqs is not None and exp["seqs"] is not None:
        seqs = b"".join(ballast_seqs) + exp["seqs"]
    return {"sc_offs": sc_offs[:-1] + [x + total for x in exp["sc_offs"]], "sc_lay_offs": sc_lay_offs[:-1] + [x + bal.k for x in exp["sc_lay_offs"]],
            "sc_flags": [0] * ns + list(exp["sc_flags"]), "layout": layout + [(u + bal.k, fl, off) for u, fl, off in exp["layout"]],
            "gaps": gaps + list(exp["gaps"]), "seqs": seqs, "case_seqs": exp["seqs"], "case_at": total, "status": st}
