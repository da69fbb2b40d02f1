"""The conditions that keep tests/test_gpu_fx_widths.py from being hollow, checked against the oracle alone (no GPU): the sets
of tests/fx_width_cases.py hold items at the widths and with the events they were built for, the widths computed from the
reads by string comparison are the ones the oracle's block lists show, and the oracle handles every set in both modes."""
import numpy as np
import pytest

from tests import fx_width_cases as fw


@pytest.fixture(scope="module", params=fw.NAMES)
def built(request):
    return fw.built(request.param)


def test_af_values_are_those_of_the_layout_header():
    assert fw.af_of_finds() == (0, 5, 3, 6)


def test_width_computations_agree(built):
    """(nA, nB, c0..c3, top-level blocks) of every item: from the reads' strings and from the oracle's exhaustive blocks"""
    f, o = built.facts(), fw.oracle_facts(built.want(False), built.lens)
    for k in ("nA", "nB", "cont", "ntop"):
        a, b = getattr(f, k), getattr(o, k)
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert len(bad) == 0, "%s %s: %d reads differ; first: read %d, strings %s, oracle %s" % (built.name, k, len(bad), bad[0], a[bad[0]], b[bad[0]])
    assert (f.T >= 2).all() or built.want(False)["substring"].any()  # a read is its own containment in finds 0 and 2


def test_set_holds_what_it_was_built_for(built):
    f = built.facts()
    T, big = f.T, f.big_items()
    for side in (0, 1):
        for w in built.case.widths:
            hit = (T[:, side] >= w) if w >= 290 else (T[:, side] == w)
            assert hit.any(), "%s: no item of %s%d blocks on side %d" % (built.name, ">= " if w >= 290 else "", w, side)
    notes = built.case.notes
    at = np.isin(T, fw.BOUNDARY_WIDTHS)
    if "nA0" in notes:  # at every boundary width an item whose width is all list Y's, and one whose width is all list X's
        for w in fw.BOUNDARY_WIDTHS:
            assert ((T == w) & (f.nA == 0)).any() and ((T == w) & (f.nB == 0)).any(), w
    if "nA0_big" in notes:  # ... and on either side among GFx::body_big's items
        for side in (0, 1):
            assert (big[:, side] & (f.nA[:, side] == 0)).any() and (big[:, side] & (f.nB[:, side] == 0)).any(), side
    if "mixed" in notes:  # boundary items with blocks in both lists, neither list a mere remainder
        assert (at & (f.nA >= 4) & (f.nB >= 4)).sum() >= len(fw.BOUNDARY_WIDTHS)
    if "ntop2" in notes:
        for w in built.case.widths:
            assert (((T >= w) if w >= 290 else (T == w)) & (f.ntop == 2)).any(), w
        assert (big & (f.ntop == 2)).any()
    if "twins" in notes:  # all four containment blocks count into the width at the boundaries
        rows = np.nonzero((f.cont.sum(axis=1) == 4))[0]
        assert len(rows) and np.isin(T[rows], built.case.widths[:4]).any()
    if "twins_big" in notes:
        rows = np.nonzero((f.cont.sum(axis=1) == 4))[0]
        assert len(rows) and big[rows].any()
    if "big" in notes or "long_big" in notes:
        assert big.any()
    if "long_big" in notes:  # a body_big item whose single-group extension runs more than 20 rounds
        lr = np.array(built.case.landing_reads)
        assert (big[lr] & (f.rounds[lr] > 20)).any(), (T[lr], f.rounds[lr])
    if "two_rows" in notes:
        b = built.want(False)["blocks"]
        assert (b[:, 3] > b[:, 2]).all()
    if "substrings" in notes:
        sub = built.want(False)["substring"].astype(bool)
        assert sub.any() and not sub.all()
        assert (f.cont[sub] == 0).all()
    if "private" in notes:
        V = built.case.private
        assert (V + 1 <= fw.GROUP_SLOTS) == (V <= 8) and (f.rounds[built.case.landing_reads] > V + 3).any()
    if "crosser" in notes:
        assert len(fw.granule_crossers(built.want(False), built.lens)) > 0
    if "late_crosser" in notes:
        # a top-level range across two granules in the very round in which the top level ends, in a read that the general
        # kernel has no other reason to redo
        assert len(fw.exposed_late_crossers(built)) >= 1


def test_landing_widths_are_the_fitted_ones():
    b = fw.built("landings")
    f = b.facts()
    lr = b.case.landing_reads
    got = sorted(int(f.T[r].max()) for r in lr)
    assert got == sorted(2 * list(b.case.widths))
    assert all(int(f.rounds[r].max()) == 31 for r in lr)  # d + 1


def test_some_set_holds_a_granule_crossing_range():
    assert any(len(fw.granule_crossers(fw.built(n).want(False), fw.built(n).lens)) for n in fw.NAMES if "crosser" in fw.case(n).notes)


def test_path_bounds_of_the_staircases():
    """what tests/test_gpu_fx_widths.py asserts of n_slow_reads, from the reads"""
    f = fw.built("stair_fwd").facts()
    assert f.slow_bound(True) == 2 * (301 - 256) and f.slow_bound(False) == 300  # T = S-1-i + 2 and i + 2
    f = fw.built("stair_fwd250").facts()
    assert f.slow_bound(True) == 0 and f.T.max() == 251
    assert not fw.built("stair_fwd250").want(False)["substring"].any()
    for name in ("private8", "private40"):
        assert fw.built(name).facts().slow_bound(True) == 0


def test_oracle_handles_every_set_in_both_modes(built):
    """the pin the GPU test compares with: block lists in both modes, edge records from the irreducible ones"""
    from tests.bigcheck import expected_edges
    from siga_amd.overlap import name_ranks
    ranks = name_ranks([n for n, _ in built.reads])
    for irr in (True, False):
        w = built.want(irr)
        n = len(built.seqs)
        assert len(w["block_offs"]) == n + 1 and int(w["block_offs"][-1]) == len(w["blocks"]) > 0
        assert w["n_occ_min"] > 0
        e = expected_edges(w["blocks"], w["block_offs"], built.fwd.sai(), built.rev.sai(), built.lens, ranks)
        assert len(e) > 0
    # irreducible mode keeps fewer blocks than exhaustive mode wherever an item is wide
    assert len(built.want(True)["blocks"]) < len(built.want(False)["blocks"])
