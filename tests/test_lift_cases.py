"""The shift rule of tests/lift_cases.py against the restatements themselves, with small ballast of explicit bytes: a small case
of `--join-overlaps` or `--gapfill` lifted behind ballast must give, under join_cases.expected_join and
gapfill_cases.expected_gapfill, exactly the small case's own result shifted -- every table, record, status entry and output
byte.  Only then may tests/test_gpu_gapfill_join_wide.py use the rule where the ballast has 2^32 bases and no restatement can run.
The small cases, their options and the ballast forms are that test's, the lengths scaled down.  No GPU."""
import random

import pytest

from tests import gapfill_cases as gc
from tests import join_cases as jc
from tests import lift_cases as lc

# the forms of tests/test_gpu_gapfill_join_wide.py, small
JOIN_SHAPES = {"a": dict(front=[4099]), "b": dict(front=[1000, 37, 4099]), "c": dict(front=[(1100, 1200, 1000, 5)]), "d": dict(grow=4099),
               "c_then_single": dict(front=[(1100, 4099, 1000, 5), 37]), "front_and_grow": dict(front=[37, (1003, 1001, 1000, 1)], grow=1000)}
GAPFILL_SHAPES = {"a": dict(front=[4099]), "b": dict(front=[1000, 37, 4099]), "c_rev": dict(front=[(1000, 4099, 40, True)]),
                  "c_fwd": dict(front=[37, (1000, 4099, 40, False)]), "d": dict(grow=4099), "d_rev": dict(grow_rev=4099),
                  "front_and_grow_rev": dict(front=[(37, 1000, 7, True), 37], grow_rev=1000)}
FILLED, DEAD_END = gc.C["FILLED"], gc.C["DEAD_END"]
JOIN_KEYS = ("status", "sc_offs", "sc_lay_offs", "sc_flags", "layout", "joins")
GAPFILL_KEYS = ("status", "sc_offs", "sc_lay_offs", "sc_flags", "layout", "gaps", "fills")


def _lifted_join(c, shape, seed):
    lf = lc.lift_join(c["res"], c["scaf"], c["opts"], **JOIN_SHAPES[shape])
    seqs = lc.materialise(lf["scaf"]["seqs_plan"], random.Random(seed))
    return lf, seqs, dict(lf["scaf"], seqs=seqs)


@pytest.mark.parametrize("shape", list(JOIN_SHAPES))
@pytest.mark.parametrize("which", ["three", "random"])
def test_join_behind_ballast_is_the_shifted_one(which, shape):
    c = lc.join_small(which)
    small = jc.case_expected(c)
    lf, seqs, scaf = _lifted_join(c, shape, 11)
    got = jc.expected_join(c["reads"], lf["res"], scaf, lf["opts"])
    want = lc.shifted_join(small, lf)
    for key in JOIN_KEYS:
        assert got[key] == want[key], key
    assert got["seqs"] == lc.expected_bytes(want["seqs_plan"], seqs) and got["seqs"][want["case_at"]:] == small["seqs"]
    # one byte short: the status says so and there are no bases
    total = want["status"][11]
    short = jc.expected_join(c["reads"], lf["res"], scaf, lf["opts"], sseqs_capacity=total - 1)
    assert short["status"] == lc.shifted_join(small, lf, capacity=total - 1)["status"] and short["status"][14] == 1 and short["seqs"] is None
    # what the ballast is for: its gaps are JOINED on their overlap alone, and v is the only match
    for g in lf["gaps"]:
        L, R = seqs[g["at"]:g["at"] + g["lu"]], seqs[g["at"] + g["lu"] + g["G"]:g["at"] + g["lu"] + g["G"] + g["lv"]]
        o = lf["opts"]
        assert jc.matches_of(L, R, o["min_overlap"], min(o["max_overlap"], len(L) - 1, len(R) - 1)) == [g["v"]]


def test_the_small_join_cases_are_what_the_wide_test_needs():
    three, rnd = lc.join_small("three"), lc.join_small("random")
    assert three["k"] == 31 and [j[5] for j in jc.case_expected(three)["joins"]] == [jc.C["JOINED"]] * 3
    exp = jc.case_expected(rnd)
    assert exp["status"][1 + jc.C["UNSUPPORTED"]] >= 1 and exp["status"][1] >= 1 and rnd["opts"]["max_overlap"] >= 1000
    fills = [j for j in exp["joins"] if j[5] == jc.C["CLOSED"] and 0 < j[3] <= rnd["opts"]["slack"]]
    assert fills  # a gap whose bytes are not N: what gapfill leaves behind


def test_grow_that_raises_hi_to_max_overlap():
    """hi_by_left: |L| = 30, |R| = 80, v = 29 = |L| - 1.  With L grown hi is |R| - 1 = 79, and with max_overlap 50 it is
    max_overlap: status 12 rises by as much, the v stays, since L is not in R a second time"""
    c = next(x for x in jc.hand_built(31) if x["kind"] == "hi_by_left")
    for mx, hi in ((1000, 79), (50, 50)):
        opts = dict(c["opts"], max_overlap=mx)
        small = jc.expected_join(c["reads"], c["res"], c["scaf"], opts)
        assert small["status"][12] == 29 - 16 + 1
        lf = lc.lift_join(c["res"], c["scaf"], opts, grow=4099)
        assert lf["dhi"] == hi - 29
        seqs = lc.materialise(lf["scaf"]["seqs_plan"], random.Random(12))
        got = jc.expected_join(c["reads"], lf["res"], dict(lf["scaf"], seqs=seqs), opts)
        want = lc.shifted_join(small, lf)
        for key in JOIN_KEYS:
            assert got[key] == want[key], (mx, key)
        assert got["status"][12] == hi - 16 + 1 and got["joins"][0][4:6] == (29, jc.C["JOINED"])
        assert got["seqs"] == lc.expected_bytes(want["seqs_plan"], seqs)
    # the cases the wide test grows do not depend on it: their first gap's hi is R's or max_overlap's
    for which in ("three", "random"):
        c = lc.join_small(which)
        assert lc.lift_join(c["res"], c["scaf"], c["opts"], grow=(1 << 32) + 31)["dhi"] == 0, which


def test_lift_join_refuses_what_the_rule_does_not_cover():
    c = next(x for x in jc.hand_built(31) if x["kind"] == "left_within_right")  # L lies in R a second time, at v = |L|
    with pytest.raises(AssertionError, match="could match"):
        lc.lift_join(c["res"], c["scaf"], c["opts"], grow=100)
    c = lc.join_small("three")
    with pytest.raises(AssertionError, match="JOINED without read support"):
        lc.lift_join(c["res"], c["scaf"], c["opts"], front=[(100, 100, 20, 5)])  # v < k - 1


def _gapfill_small(shape):
    return lc.gapfill_small(shape in ("d_rev", "front_and_grow_rev"))


@pytest.mark.parametrize("shape", list(GAPFILL_SHAPES))
def test_gapfill_behind_ballast_is_the_shifted_one(shape):
    c = _gapfill_small(shape)
    mw = gc.scratch_needed(c)
    small = gc.expected_gapfill(c["reads"], c["res"], c["scaf"], c["opts"], max_walk_bases=mw)
    lf = lc.lift_gapfill(c["res"], c["scaf"], c["opts"], max_walk_bases=mw, **GAPFILL_SHAPES[shape])
    useqs = lc.materialise(lf["res"]["useqs_plan"], random.Random(13))
    res = {"seq_offs": lf["res"]["seq_offs"], "useqs": useqs}
    got = gc.expected_gapfill(c["reads"], res, lf["scaf"], lf["opts"], max_walk_bases=lf["max_walk_bases"])
    want = lc.shifted_gapfill(small, lf)
    for key in GAPFILL_KEYS:
        assert got[key] == want[key], key
    assert got["seqs"] == lc.expected_bytes(want["seqs_plan"], useqs) and got["seqs"][want["case_at"]:] == small["seqs"]
    assert got["status"][21] == 0 and [g[5:9] for g in small["gaps"]] == [(FILLED, FILLED, gc.NOT_RUN, 0)] * 3 + [
        (FILLED, gc.C["BRANCH"], FILLED, 1), (DEAD_END, DEAD_END, DEAD_END, 0)]  # no NO_ROOM; forward and reverse fills, a gap left as laid
    total = want["status"][16]
    short = gc.expected_gapfill(c["reads"], res, lf["scaf"], lf["opts"], max_walk_bases=lf["max_walk_bases"], sseqs_capacity=total - 1)
    assert short["status"] == lc.shifted_gapfill(small, lf, capacity=total - 1)["status"] and short["status"][20] == 1 and short["seqs"] is None
    # one byte of scratch less and the case's last walked gap is NO_ROOM: the ballast gaps' scratch is counted
    less = gc.expected_gapfill(c["reads"], res, lf["scaf"], lf["opts"], max_walk_bases=lf["max_walk_bases"] - 1)
    assert less["status"][21] == 1 and less["status"][1 + gc.C["NO_ROOM"]] == 1


def test_flip_first_changes_only_how_the_first_unitig_is_stored():
    c = lc.gapfill_small()
    res, scaf = lc.flip_first(c["res"], c["scaf"])
    a, b = gc.case_expected(c), gc.expected_gapfill(c["reads"], res, scaf, c["opts"])
    assert scaf["layout"][0][1] == c["scaf"]["layout"][0][1] ^ gc.REV and res["useqs"] != c["res"]["useqs"]
    assert a["layout"][1:] == b["layout"][1:] and b["layout"][0] == scaf["layout"][0]
    for key in ("status", "sc_offs", "gaps", "seqs", "fills"):
        assert a[key] == b[key], key
    assert c["scaf"]["layout"][0][1] == 0 and lc.gapfill_small(True)["scaf"]["layout"][0][1] == gc.REV
    assert lc.gapfill_small(True)["res"]["useqs"] == res["useqs"]
