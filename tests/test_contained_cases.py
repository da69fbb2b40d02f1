"""The serial restatement of the containment records (tests/contained_cases.py) against a search without seeds, against answers
worked out by hand, and against the flags the existing restatement sets.  No GPU."""
import functools

import pytest

from tests import consensus_cases as cc
from tests import contained_cases as kc
from tests import mmoverlap_cases as mc


def _flagged(records, n):
    out = [0] * n
    for r in records:
        out[r[0]] = 1
    return out


def test_seeds_equal_brute_force_on_the_boundary_sets():
    for name, (refs, names, p, _, flagged) in sorted(mc.boundary_sets().items()):
        ranks = mc.name_ranks(names)
        got, written = kc.expected_containments(refs, ranks, p)
        assert got == kc.brute_containments(refs, ranks, p), name
        assert written >= len(got)
        # every flag of the existing restatement has a record and every record a flag
        assert [i for i, c in enumerate(_flagged(got, len(refs))) if c] == flagged, name
        for r in got:
            kc.check_geometry(refs, r)


def test_answers_worked_out_by_hand():
    for name, (refs, names, p, want) in sorted(kc.hand_sets().items()):
        ranks = mc.name_ranks(names)
        got, written = kc.expected_containments(refs, ranks, p)
        assert got == want, name
        assert got == kc.brute_containments(refs, ranks, p), name
        # both reads of a pair find it: the raw stream holds every record twice
        assert written == 2 * len(want), name
        assert _flagged(got, len(refs)) == mc.expected_mm_overlaps(refs, ranks, p)[1], name
        for r in got:
            kc.check_geometry(refs, r)


def test_sides_agree_one_at_a_time():
    """the record found from the contained read alone equals the one found from the container alone"""
    for name, (refs, names, p, want) in sorted(kc.hand_sets().items()):
        ranks = mc.name_ranks(names)
        per_read = [kc.expected_containments(refs, ranks, p, i, 1)[0] for i in range(len(refs))]
        for rec in want:
            assert rec in per_read[rec[0]] and rec in per_read[rec[1]], (name, rec)


def test_duplicate_chain():
    refs, names, p = kc.duplicate_chain()
    ranks = mc.name_ranks(names)
    got, _ = kc.expected_containments(refs, ranks, p)
    assert got == [(k, k - 1, 100, 8, 1, 0) for k in range(1, 40)]
    records, contained, _ = mc.expected_mm_overlaps(refs, ranks, p)
    assert records == [] and contained == [0] + [1] * 39


@functools.lru_cache(maxsize=None)
def _noisy(seed, mixed):
    case = cc.noisy_case(seed, mixed)
    refs = [r.decode() for r in case["reads"]]
    ranks = mc.name_ranks(case["names"])
    return case, refs, ranks, kc.expected_containments(refs, ranks, case["params"])[0]


@pytest.mark.parametrize("seed,mixed", [(0, False), (0, True), (2, True), (3, True)])
def test_noisy_reads_every_flag_has_a_record(seed, mixed):
    case, refs, ranks, got = _noisy(seed, mixed)
    contained = mc.expected_mm_overlaps(refs, ranks, case["params"])[1]
    assert _flagged(got, len(refs)) == contained
    assert sum(contained) >= (150 if mixed else 4)
    for r in got:
        kc.check_geometry(refs, r)
    assert {r[3] for r in got} == {8, 12}


def test_error_free_reads_lie_on_their_containers_columns():
    """reads without errors: the container's bases under every record are the contained read's, column for column"""
    case = cc.noisy_case(1, True)
    g = case["genome"].decode()
    refs = [g[a:b] if not rev else mc.pc.revcomp(g[a:b]) for (a, b), rev in zip(case["spans"], _strands(case))]
    ranks = mc.name_ranks(case["names"])
    got, _ = kc.expected_containments(refs, ranks, mc.params(S=12, T=4, M=30, P=0, H=4096, K=4096))
    assert len(got) > 150 and not any(r[4] for r in got)
    for r in got:
        assert kc.placed_text(refs, r) == refs[r[0]]


def _strands(case):
    """which reads of a noisy case lie on the reverse strand, read off the reads themselves"""
    g = case["genome"].decode()
    out = []
    for (a, b), r in zip(case["spans"], case["reads"]):
        text = r.decode()
        fwd = sum(1 for x, y in zip(text, g[a:b]) if x != y)
        rev = sum(1 for x, y in zip(mc.pc.revcomp(text), g[a:b]) if x != y)
        out.append(rev < fwd)
    return out


# ---- the placement pass ---------------------------------------------------------------------------------------------------------------
def _contained_placements(exp):
    """read -> (unitig, flags, offset) of the placements that carry SIGAX_PLACED_CONTAINED"""
    lo = exp["lay_offs"]
    return {r: (u, fl, o) for u in range(len(lo) - 1) for r, fl, o in exp["layout"][lo[u]:lo[u + 1]] if fl & kc.PLACED_CONTAINED}


def test_placements_worked_out_by_hand():
    for name, (lengths, contained, recs, tables, want) in sorted(kc.hand_placements().items()):
        exp = kc.expected_placement(tables, lengths, contained, recs)
        assert _contained_placements(exp) == want, name
        assert [c for c, k in enumerate(exp["place_class"]) if k == kc.PLACED] == sorted(want), name
        # the hidden unitig of a placed read keeps its number and has no placement; the root keeps its own
        for c, (u, _, _) in want.items():
            assert exp["lay_offs"][c] == exp["lay_offs"][c + 1], name
        assert (0, tables["layout"][0][1], 7) in exp["layout"][:exp["lay_offs"][1]]
        assert exp["status"][7] == len(lengths) and exp["status"][3] == len(want)


def test_duplicate_chain_lands_on_the_first_read():
    refs, names, p = kc.duplicate_chain()
    ranks = mc.name_ranks(names)
    recs, _ = kc.expected_containments(refs, ranks, p)
    lengths = [len(r) for r in refs]
    exp = kc.expected_placement(kc.single_unitig(100)(lengths), lengths, [0] + [1] * 39, recs)
    assert exp["place_class"] == [kc.NOT_CONTAINED] + [kc.PLACED] * 39
    assert exp["status"] == [39, 39, 0, 39, 0, 0, 39, 40]
    assert exp["lay_offs"] == [0] + [40] * 40
    assert exp["layout"] == [(0, 0, 0)] + [(k, 2, 0) for k in range(1, 40)]


def test_classes_of_reads_that_cannot_be_placed():
    lengths, contained, recs, tables = kc.unplaceable()
    exp = kc.expected_placement(tables, lengths, contained, recs)
    assert exp["place_class"] == [kc.NOT_CONTAINED, kc.NO_RECORD, kc.NO_RECORD, kc.NO_ROOT, kc.ROOT_REMOVED, kc.NOT_CONTAINED]
    assert exp["status"] == [4, 7, 5, 0, 3, 1, 1, 5]
    assert exp["layout"] == tables["layout"][:5] and exp["lay_offs"] == tables["lay_offs"]  # an unplaced read keeps what it had


def test_error_free_reads_are_placed_on_their_own_bases():
    case = cc.noisy_case(1, True)
    g = case["genome"].decode()
    refs = [g[a:b] if not rev else mc.pc.revcomp(g[a:b]) for (a, b), rev in zip(case["spans"], _strands(case))]
    reads = [r.encode() for r in refs]
    ranks = mc.name_ranks(case["names"])
    p = mc.params(S=12, T=4, M=30, P=0, H=4096, K=4096)
    records, contained, _ = mc.expected_mm_overlaps(refs, ranks, p)
    conts, _ = kc.expected_containments(refs, ranks, p)
    edges = [(q, t, ln, af) for q, t, ln, af, _ in records if not contained[q] and not contained[t]]
    red = cc.rc.expected_reduce(reads, edges, 30, 0, 0)
    exp = kc.expected_placement(red, [len(r) for r in reads], contained, conts)
    placed = _contained_placements(exp)
    assert len(placed) == sum(contained) > 150 and exp["status"][4:6] == [0, 0]
    so, useqs = red["seq_offs"], bytes(red["useqs"])
    for c, (u, fl, o) in placed.items():
        assert kc.placed_bytes(reads, (c, fl, o)) == useqs[so[u] + o:so[u] + o + len(reads[c])], c
    # ascending in (offset, kind, read id) within every unitig
    for u in range(len(exp["lay_offs"]) - 1):
        rows = [(o, 1 if fl & 2 else 0, r) for r, fl, o in exp["layout"][exp["lay_offs"][u]:exp["lay_offs"][u + 1]]]
        assert rows == sorted(rows)


@functools.lru_cache(maxsize=None)
def noisy_placed(seed, mixed):
    """cc.noisy_expected with the placement pass and the vote over its layout behind it -> (case, exp, placement, consensus)"""
    case, refs, ranks, conts = _noisy(seed, mixed)
    exp = cc.noisy_expected(seed, mixed)
    pl = kc.expected_placement(exp["reduced"], [len(r) for r in refs], exp["contained"], conts)
    cons = cc.expected_consensus(case["reads"], kc.with_placement(exp["reduced"], pl), 1)
    return case, exp, pl, cons


@pytest.mark.parametrize("seed,mixed", [(s, m) for s in range(6) for m in (False, True)])
def test_noisy_variants_assemble_to_the_genome(seed, mixed):
    case, exp, pl, cons = noisy_placed(seed, mixed)
    n_contained = sum(exp["contained"])
    assert pl["status"][0] == pl["status"][3] == n_contained and pl["status"][2] == 0
    assert (172 <= n_contained <= 197) if mixed else (5 <= n_contained <= 6)
    assert all((k == kc.PLACED) == bool(c) for k, c in zip(pl["place_class"], exp["contained"]))
    after = cc.assembled(case, dict(exp, consensus=cons))
    assert [c for _, c in after] == [case["genome"]]
    before = cc.assembled(case, exp)
    assert len(before) == 1 and wrong_bases(before[0][1], case["genome"]) == (1 if (seed, mixed) in ((2, True), (3, True)) else 0)


def wrong_bases(seq, genome):
    """columns in which seq differs from the genome, on the strand on which it differs least"""
    assert len(seq) == len(genome)
    return min(sum(1 for a, b in zip(s, genome) if a != b) for s in (seq, cc.uc.revcomp(seq)))


def test_offsets_beyond_16_bits():
    """a container of 70 000 bases: the offsets are 66 000 and 69 850, and the reads land there"""
    refs, names, p, want = kc.long_container_set()
    got, written = kc.expected_containments(refs, mc.name_ranks(names), p)
    assert got == want and written == 2  # the long read is no query: each record is written once
    for r in got:
        kc.check_geometry(refs, r)
    lengths = [len(r) for r in refs]
    exp = kc.expected_placement(kc.single_unitig(lengths[0], True, 5, lengths[0] + 9)(lengths), lengths, [0, 1, 1], want)
    assert exp["layout"] == [(0, 1, 5), (2, 2, 5), (1, 3, 5 + 70000 - 66000 - 150)]


def test_trim_rounds_take_a_root():
    case, refs, ranks, contained, edges, conts, red, pl = kc.trimmed_case()
    n = len(refs)
    assert pl["place_class"][n - 1] == kc.ROOT_REMOVED and pl["place_class"][n - 2] == kc.NOT_CONTAINED and red["removed"][n - 2]
    assert pl["status"][3] == sum(contained) - 1 and pl["status"][5] == 1 and pl["status"][4] == 0
    # every other contained read was removed as an island and is placed all the same
    assert all(red["removed"][c] for c in range(n) if contained[c]) and len(red["uflags"]) == 1
    assert pl["status"][7] == n - sum(1 for x in red["removed"] if x) + pl["status"][3]
