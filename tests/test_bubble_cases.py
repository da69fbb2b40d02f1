"""The two brute forces of tests/bubble_cases.py against each other, against chimeric_cases.expected_chimeric where there is no
bubble step, and against what every hand-built case was built to show.  No GPU."""
import random

import pytest

from tests import bubble_cases as bc
from tests import chimeric_cases as cc

CASES = bc.hand_built()
IDS = [c["name"] for c in CASES]
KEYS = ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "status", "removed", "cut", "uedges")


def _equal(a, b, what):
    for k in KEYS:
        assert a[k] == b[k], "%s: %s" % (what, k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_brute_forces_agree(case):
    _equal(bc.expected_of(case["name"]), bc.run(bc.independent_bubble, case), case["name"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_claims(case):
    exp, claims = bc.expected_of(case["name"]), case["claims"]
    st = exp["status"]
    print(case["name"], st, exp["bubble_log"][:3])
    for key, at in (("unitigs", 0), ("rounds", 6), ("chim", 16), ("popped", 20), ("bub_reads", 21), ("bub_rounds", 22), ("kept_div", 23)):
        if key in claims:
            assert st[at] == claims[key], key
    for r, rnd in claims.get("flagged", {}).items():
        assert exp["removed"][r] == rnd | bc.BUBBLE, r
    for r in claims.get("kept_ids", []):
        assert exp["removed"][r] == 0, r
    if "log" in claims:
        assert claims["log"](exp["bubble_log"])
    assert st[21] == sum(1 for x in exp["removed"] if x & bc.BUBBLE) and st[9] == sum(1 for x in exp["removed"] if x)
    assert not any(x & bc.BUBBLE and x & cc.CHIMERIC for x in exp["removed"])
    assert all(e["winner"] != e["loser"] and exp["removed"][e["winner"]] & bc.BUBBLE == 0 for e in exp["bubble_log"])


def test_what_the_cases_cover():
    logs = {c["name"]: bc.expected_of(c["name"])["bubble_log"] for c in CASES}
    assert any(e["reversed"] != e["winner_reversed"] for e in logs["entered_right"]) and any(e["reads"] == 3 for e in logs["chains_flipped"])
    # a winner with more reads and a larger first read id than the loser it beats; a tie decided by the id
    assert any(e["winner"] > e["loser"] for e in logs["chains"]) and all(e["winner"] < e["loser"] for e in logs["two_arms"])
    assert logs["at_divergence"][0]["mism"] * 1000 == 50 * logs["at_divergence"][0]["span"]
    assert logs["above_divergence"][0]["mism"] * 1000 > 50 * logs["above_divergence"][0]["span"]
    assert {e["span"] for e in logs["two_spans"]} == {20, 30} and logs["span_1"][0]["span"] == 1
    assert logs["second_round"][0]["round"] == 2 and len({(e["lo"], e["hi"]) for e in logs["series"]}) == 2
    assert len({(e["lo"], e["hi"]) for e in logs["arms130"]}) == 1 and len(logs["arms130"]) >= 129
    # without the bubble step the winner of chimeric_winner goes as chimeric
    c = bc.case_named("chimeric_winner")
    plain = bc.run(bc.expected_bubble, c, Lb=0)
    w = [r for r in c["claims"]["kept_ids"]]
    assert all(plain["removed"][r] == 1 | cc.CHIMERIC for r in w) and all(bc.expected_of("chimeric_winner")["removed"][r] == 0 for r in w)


@pytest.mark.parametrize("rounds", [0, 1, 2, 3])
def test_second_round_round_by_round(rounds):
    exp = bc.expected_of("second_round", rounds)
    assert exp["status"][6] == min(rounds, 2) and exp["status"][20] == (rounds >= 2)


def test_random_graphs():
    popped = kept = 0
    for seed in range(300):
        case = bc.random_case(seed)
        exp = bc.run(bc.expected_bubble, case)
        _equal(exp, bc.run(bc.independent_bubble, case), case["name"])
        popped += exp["status"][20] > 0
        kept += exp["status"][23] > 0
    print("graphs that pop an arm", popped, "that keep a loser on divergence", kept)
    assert popped >= 150 and kept >= 75


@pytest.mark.parametrize("case", cc.hand_built(), ids=[c["name"] for c in cc.hand_built()])
def test_lb_0_is_expected_chimeric(case):
    want = cc.expected_of(case["name"])
    got = bc.run(bc.expected_bubble, bc.with_bubble_keys(case, Lb=0, D=7))
    for k in KEYS:
        if k != "status":
            assert got[k] == want[k], k
    assert got["status"][:20] == want["status"] and got["status"][20:] == [0] * 4
    for d in (10,):
        with_d = dict(case, delta=d)
        assert bc.run(bc.expected_bubble, bc.with_bubble_keys(with_d))["status"][:20] == cc.run(cc.expected_chimeric, with_d)["status"]


def _shuffled(case, seed):
    """the same graph with its reads relabelled and its records in another order -> (case, old read id -> new)"""
    rng = random.Random(seed)
    n = len(case["reads"])
    new = list(range(n))
    rng.shuffle(new)
    reads = [None] * n
    for r in range(n):
        reads[new[r]] = case["reads"][r]
    edges = [(new[q], new[t], ln, af) if q < n and t < n else (q, t, ln, af) for q, t, ln, af in case["edges"]]
    rng.shuffle(edges)
    return dict(case, reads=reads, edges=edges), new


@pytest.mark.parametrize("name", ["three_arms", "arms65", "chains_flipped", "entered_right", "two_spans", "series", "second_round", "same_unitig"])
def test_order_of_records_and_reads(name):
    case, exp = bc.case_named(name), bc.expected_of(name)
    # records in another order: the very same result but for the order of the lifted records
    only_edges = dict(case, edges=random.Random(5).sample(case["edges"], len(case["edges"])))
    got = bc.run(bc.expected_bubble, only_edges)
    assert got["removed"] == exp["removed"] and got["status"] == exp["status"] and got["useqs"] == exp["useqs"]
    # reads relabelled: the winner of a K tie follows the ids by rule, so in a group of three or more tied arms the mismatches of
    # the others may change with it; everywhere else the same groups lose the same number of arms in the same rounds
    if name in ("three_arms", "arms65"):
        return
    other, new = _shuffled(case, 6)
    got = bc.run(bc.expected_bubble, other)
    assert got["status"][:2] + got["status"][6:] == exp["status"][:2] + exp["status"][6:]
    by_group = lambda res: sorted((e["round"], e["span"], e["mism"], e["reads"]) for e in res["bubble_log"])  # noqa: E731
    assert by_group(got) == by_group(exp)
    if not all(e["reads"] == 1 for e in exp["bubble_log"]):  # K decides: the same reads go
        assert [got["removed"][new[r]] for r in range(len(new))] == exp["removed"]
