"""The two restatements of the indel step (tests/indel_cases.py) against each other, against the hand-built cases' claims and, with
E = 0, against bubble_cases.expected_bubble: no GPU."""
import random

import pytest

from tests import bubble_cases as bc
from tests import indel_cases as ic

CASES = ic.hand_built()
IDS = [c["name"] for c in CASES]
SAME = ("status", "removed", "cut", "uedges", "seq_offs", "lay_offs", "uflags", "layout", "useqs")


def _agree(a, b, what):
    for k in SAME:
        assert a[k] == b[k], "%s: %s" % (what, k)


def test_the_two_distances_agree():
    rng = random.Random(5)
    for _ in range(300):
        x = ic.bases(rng, rng.randint(0, 70))
        y = x if rng.random() < 0.2 else ic.bases(rng, rng.randint(0, 70))
        for _e in range(rng.randint(0, 5)):
            if y:
                at = rng.randrange(len(y))
                y = rng.choice((ic.delete(y, at), ic.insert(rng, y, at), ic.mutate(rng, y, (at,))))
        assert ic.lev(x, y) == ic.lev_bits(x, y) == ic.lev(y, x)
    assert ic.lev(b"", b"ACG") == 3 and ic.lev_bits(b"ACG", b"") == 3 and ic.lev(b"kitten", b"sitting") == 3 and ic.lev_bits(b"Na", b"NA") == 1
    # a common prefix and suffix change nothing
    assert ic.lev_bits(b"TTTT" + b"ACGGT" + b"CCA", b"TTTT" + b"AGGTA" + b"CCA") == ic.lev(b"ACGGT", b"AGGTA")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_built(case):
    exp = ic.expected_of(case["name"])
    _agree(exp, ic.run(ic.independent_indel, case), case["name"])
    st, cl = exp["status"], case["claims"]
    print(case["name"], st, [(e["cls"], e["ed"], e["round"]) for e in exp["indel_log"]][:12])
    for key, at in (("popped", 24), ("ind_reads", 25), ("ind_rounds", 26), ("kept", 27), ("skipped", 28), ("bub", 20), ("chim", 16), ("rounds", 6),
                    ("unitigs", 0)):
        if key in cl:
            assert st[at] == cl[key], (key, st[at], cl[key])
    assert st[29:] == [0, 0, 0] and len(st) == 32
    for r, rnd in cl.get("flagged", {}).items():
        assert exp["removed"][r] == rnd | ic.INDEL, r
    for r in cl.get("kept_ids", []):
        assert exp["removed"][r] == 0, r
    first = [e for e in exp["indel_log"] if e["round"] == 1]
    if "eds" in cl:
        assert sorted(e["ed"] for e in first if e["ed"] is not None) == cl["eds"]
    if "classes" in cl:
        assert sorted(e["cls"] for e in first) == cl["classes"]
    assert st[9] == sum(1 for x in exp["removed"] if x) and st[25] == sum(1 for x in exp["removed"] if x & ic.INDEL)


def test_orientations_and_sizes_are_reached():
    """what the cases are there for, read from the restatement's log"""
    log = {c["name"]: ic.expected_of(c["name"])["indel_log"] for c in CASES}
    ways = {(e["reversed"], e["winner_reversed"]) for k, lg in log.items() if k.startswith("entered_") for e in lg}
    assert ways == {(False, False), (False, True), (True, False), (True, True)}
    assert {(e["span"], e["winner_span"]) for e in log["span_4096_winner"]} == {(4095, 4096)}
    assert {(e["span"], e["winner_span"]) for e in log["span_4096_loser"]} == {(4096, 4095)}
    assert all(e["reads"] == 39 for e in log["span_4096_winner"] + log["span_4096_loser"])
    assert {(e["span"], e["winner_span"]) for e in log["span_1_2"] + log["span_2_1"] + log["span_1_4"]} == {(2, 1), (1, 2), (4, 1)}
    assert len({e["cls"] for e in log["arms130"]}) == 4 and len([e for e in log["arms130"] if e["round"] == 1]) == 129


def test_chimeric_winner_without_the_step():
    case = ic.case_named("chimeric_winner")
    assert ic.run(ic.expected_indel, case, Ed=0)["status"][16] >= 1 and ic.expected_of("chimeric_winner")["status"][16] == 0


@pytest.mark.parametrize("name", ["three_bubble_keeps", "arms130", "entered_111", "span_4096_loser", "second_round"])
@pytest.mark.parametrize("seed", [11, 12])
def test_order_does_not_matter(name, seed):
    case, exp = ic.case_named(name), ic.expected_of(name)
    other, new = ic.shuffled(case, seed, 6)  # (reads 0-5 are the two chains the arms hang between)
    got = ic.run(ic.expected_indel, other)
    assert got["status"] == exp["status"]
    assert [got["removed"][new[r]] for r in range(len(new))] == exp["removed"]
    _agree(got, ic.run(ic.independent_indel, other), name + ", shuffled")


def test_random_graphs():
    seen = {}
    for seed in range(300):
        case = ic.random_case(seed)
        exp = ic.run(ic.expected_indel, case)
        _agree(exp, ic.run(ic.independent_indel, case), case["name"])
        for e in exp["indel_log"]:
            seen[e["cls"]] = seen.get(e["cls"], 0) + 1
    print(seen)
    assert all(seen.get(k, 0) >= 10 for k in ("POPPED", "KEPT_EDITS", "KEPT_PERMILLE", "SAME_SPAN", "FAR")), seen


def test_e_0_is_expected_bubble():
    for case in [c for c in bc.hand_built() if len(c["reads"]) <= 200] + [bc.random_case(s) for s in range(0, 300, 7)]:
        want = bc.run(bc.expected_bubble, case)
        got = ic.run(ic.expected_indel, ic.with_indel_keys(case, Ed=0, De=7))
        assert got["status"][:24] == want["status"] and got["status"][24:] == [0] * 8
        for k in SAME[1:]:
            assert got[k] == want[k], k
        assert not any(x & ic.INDEL for x in got["removed"])


def test_end_to_end_reads():
    names, reads = ic.end_to_end()
    assert len(reads) == ic.E2E_READS == len(set(reads)) and all(len(r) == ic.E2E_LEN for r in reads)
