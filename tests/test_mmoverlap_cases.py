"""The serial restatement of `siga overlap -e` (tests/mmoverlap_cases.py) pinned: answers worked out by hand for every class,
strand and boundary, the seeded search against the search over every read, strand and diagonal, and `-e 0` against the
reference's exhaustive overlap run.  No GPU."""
import collections
import os

import pytest

from oracle import pyoracle as po
from tests import mmoverlap_cases as mc
from tests import pileup_cases as pc
from tests.fixtures import ed_lines
from tests.golden import make_reads as mr


@pytest.mark.parametrize("name", sorted(mc.boundary_sets()))
def test_hand_computed(name):
    refs, names, p, records, flagged = mc.boundary_sets()[name]
    ranks = mc.name_ranks(names)
    got = mc.expected_mm_overlaps(refs, ranks, p)
    assert got[0] == records
    assert [i for i, c in enumerate(got[1]) if c] == flagged
    brute = mc.brute_mm_overlaps(refs, ranks, p)
    assert (brute[0], brute[1]) == (got[0], got[1])


def test_ed_coordinates_of_each_class():
    """two reads of 80 bases, 45 columns: where the overlap lies in each read, by af"""
    assert mc.ed_coords(45, 0, 80, 80) == (35, 79, 80, 0, 44, 80, 0)  # query's suffix on target's prefix
    assert mc.ed_coords(45, 3, 80, 80) == (0, 44, 80, 35, 79, 80, 0)  # query's prefix on target's suffix
    assert mc.ed_coords(45, 6, 80, 80) == (35, 79, 80, 35, 79, 80, 1)  # suffix on suffix, reversed
    assert mc.ed_coords(45, 5, 80, 80) == (0, 44, 80, 0, 44, 80, 1)  # prefix on prefix, reversed
    assert mc.ed_coords(60, 3, 61, 80) == (0, 59, 61, 20, 79, 80, 0)
    refs, names, p, records, _ = mc.boundary_sets()["m_at_floor"]
    assert mc.ed_line(records[0], names, refs) == "ED\tb a 35 79 80 0 44 80 0 2"


def test_canonical_swap():
    """0 <-> 3, 5 and 6 fixed: the same pair from either side is one record"""
    sets = mc.boundary_sets()
    for kind, small, large in (("suffix_fwd", 3, 0), ("prefix_fwd", 0, 3), ("suffix_rev", 6, 6), ("prefix_rev", 5, 5)):
        assert sets[kind + "_q_small"][3][0][3] == small and sets[kind + "_q_large"][3][0][3] == large
    # each side alone finds the record the other finds
    refs, names, p, records, _ = sets["suffix_fwd_q_small"]
    ranks = mc.name_ranks(names)
    assert mc.expected_mm_overlaps(refs, ranks, p, 0, 1)[0] == mc.expected_mm_overlaps(refs, ranks, p, 1, 1)[0] == records


def test_seeded_equals_brute_force():
    S, T, M, P = 12, 4, 45, 40
    assert mc.completeness_floor(M, P, 150) == 16 >= S + T - 1  # at l = 50: 48 matching columns around 2 mismatches
    p = mc.params(S=S, T=T, M=M, P=P, H=4096, K=4096)
    refs, names = mc.noisy_case()
    ranks = mc.name_ranks(names)
    seeded = mc.expected_mm_overlaps(refs, ranks, p)
    brute = mc.brute_mm_overlaps(refs, ranks, p)
    assert seeded[2][2] == seeded[2][4] == 0  # neither K nor H was reached
    assert seeded[0] == brute[0] and seeded[1] == brute[1]
    # what this set holds (its own numbers: the reads are drawn here, from this file's seed)
    records, contained = brute
    assert (len(records), sum(contained)) == (85, 26)
    assert sum(1 for r in records if r[4]) == 70
    assert collections.Counter(r[3] for r in records) == {0: 14, 3: 27, 5: 18, 6: 26}
    # the default seeds are too long for the condition and lose a few
    assert mc.completeness_floor(M, P, 150) < 24 + 12 - 1
    wide = mc.expected_mm_overlaps(refs, ranks, mc.params(H=4096, K=4096))
    assert set(wide[0]) < set(records) and (len(wide[0]), sum(wide[1])) == (78, 24)


def test_e0_equals_the_reference_exhaustive_run(tmp_path):
    refs, names = mc.exact_case()
    S, T, M = 12, 4, 45
    assert M >= S + T - 1
    ranks = mc.name_ranks(names)
    records, contained, status = mc.expected_mm_overlaps(refs, ranks, mc.params(S=S, T=T, M=M, P=0, H=4096, K=4096))
    assert not any(contained) and all(r[4] == 0 for r in records) and len(records) > 100
    fa = str(tmp_path / "reads.fa")
    with open(fa, "w") as f:
        f.write(mr.fasta_text(list(zip(names, refs))))
    fwd, rev = po.Index.build(refs), po.Index.build(refs, reverse=True)
    out = str(tmp_path / "o.asqg")
    po.build_asqg(fwd, rev, fa, M, out, "", irreducible=False)
    text = open(out).read()
    assert "SS:i:1" not in text
    want = {tuple(l.split()[:9]) for l in ed_lines(text)}
    got = {tuple(mc.ed_line(r, names, refs)[3:].split()[:9]) for r in records}
    assert len(got) == len(records) and got == want
    assert {l.split()[9] for l in ed_lines(text)} == {"0"}
