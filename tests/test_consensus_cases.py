"""The serial restatement of the consensus pass (tests/consensus_cases.py) pinned: its two statements against each other, answers
worked out by hand for every vote, exact overlaps left as they are, planted errors voted out, and the noisy sets composed from the
restatements of `siga overlap -e`, `--reduce` and the vote.  No GPU."""
import pytest

from tests import consensus_cases as cc
from tests import mmoverlap_cases as mc
from tests import unitig_cases as uc

CASES = {c["name"]: c for c in cc.all_cases()}


@pytest.mark.parametrize("min_votes", (1, 2, 3))
@pytest.mark.parametrize("name", sorted(CASES))
def test_two_statements_agree(name, min_votes):
    case = CASES[name]
    assert cc.expected_consensus(case["reads"], case["res"], min_votes) == cc.columnwise_consensus(case["reads"], case["res"], min_votes)


def test_votes_by_hand():
    """VOTE_COLUMNS, worked out on paper: the byte, its support, and the status words under min_votes 1, 2 and 3"""
    case = CASES["votes"]
    W = len(cc.VOTE_COLUMNS)
    one = cc.expected_consensus(case["reads"], case["res"], 1)
    assert one["useqs"][:W] == b"ACACAAATaTAGTC"
    assert list(one["support"][:W]) == [1, 1, 2, 2, 2, 3, 2, 1, 0, 1, 0, 2, 1, 1]
    assert one["changed"] == [6, 0]
    # the second unitig: one read over its own copy, where N, X and lower case have no vote and the letters one
    assert one["useqs"][W:] == case["res"]["useqs"][W:] and list(one["support"][W:]) == [1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0]
    # unitigs, columns, changed, depth < 2, ties, held back, largest depth, invalid
    assert one["status"] == [2, 2 * W, 6, 4 + W, 5, 0, 5, 0]
    two = cc.expected_consensus(case["reads"], case["res"], 2)
    assert two["useqs"][:W] == b"ACACAAANaTAGTN" and two["status"] == [2, 2 * W, 4, 4 + W, 5, 2, 5, 0]
    three = cc.expected_consensus(case["reads"], case["res"], 3)
    assert three["useqs"][:W] == b"ACACXAGNaTAgTN" and three["status"] == [2, 2 * W, 1, 4 + W, 5, 5, 5, 0]
    assert list(three["support"][:W]) == [1, 1, 2, 2, 0, 3, 1, 0, 0, 1, 0, 0, 1, 0]


def test_invalid_placements_are_counted_and_skipped():
    case = CASES["invalid"]
    got = cc.expected_consensus(case["reads"], case["res"], 1)
    assert got["status"][7] == 5 and got["status"][0] == 4
    # the end of each of the first three unitigs lost its only read: depth 0 there, the copy stays
    so = case["res"]["seq_offs"]
    assert [got["support"][so[u + 1] - 1] for u in range(4)] == [0, 0, 0, 1]
    assert got["useqs"][so[1]:] == case["res"]["useqs"][so[1]:]


@pytest.mark.parametrize("min_votes", (1, 2))
def test_exact_overlaps_change_nothing(min_votes):
    """every case of unitig_cases: a placement's read, as placed, equals its unitig's bytes at its offset, so no letter outvotes
    the own one"""
    for c in uc.hand_built():
        res = uc.expected(c["reads"], c["edges"], c["m"])
        got = cc.expected_consensus(c["reads"], res, min_votes)
        assert got["useqs"] == res["useqs"], c["name"]
        assert got["changed"] == [0] * len(res["uflags"]) and got["status"][2] == 0 and got["status"][5] == 0, c["name"]
        assert got["status"][:2] == [len(res["uflags"]), len(res["useqs"])] and got["status"][7] == 0, c["name"]


@pytest.mark.parametrize("case", cc.planted_cases(), ids=lambda c: c["name"])
def test_planted_errors_are_voted_out(case):
    """the consensus is the genome and the copy is not: no later test can pass with the vote switched off"""
    res, g = case["res"], case["genomes"][0]
    assert len(res["uflags"]) == 1 and len(res["useqs"]) == len(g)
    got = cc.expected_consensus(case["reads"], res, 1)
    assert got["useqs"] == g
    wrong = sum(1 for a, b in zip(res["useqs"], g) if a != b)
    assert wrong >= 1 and got["changed"] == [wrong] and got["status"][2] == wrong


def test_deep_cases_saturate_support():
    deep = {c["name"]: cc.expected_consensus(c["reads"], c["res"], 1) for c in cc.planted_cases() if c["name"].startswith("deep")}
    assert deep["deep150"]["status"][6] == 150 and max(deep["deep150"]["support"]) == 150
    assert deep["deep300"]["status"][6] == 300 and max(deep["deep300"]["support"]) == 255
    assert deep["deep300"]["support"][0] == deep["deep300"]["support"][-1] == 1  # depth 1 at both ends
    assert deep["deep300"]["status"][3] == 2


def test_ring_is_voted_on_as_a_line():
    case = CASES["ring"]
    got = cc.expected_consensus(case["reads"], case["res"], 1)
    assert len(case["res"]["useqs"]) == 235 and got["status"][6] == 3
    assert got["support"][0] == 1  # the closing overlap is not wrapped round: the last read does not vote on column 0


@pytest.mark.parametrize("seed,mixed", cc.NOISY_SEEDS)
def test_noisy_sets_compose_to_the_genome(seed, mixed):
    case, P = cc.noisy_case(seed, mixed), cc.NOISY
    longest = max(len(r) for r in case["reads"])
    assert mc.completeness_floor(P["M"], P["P"], longest) >= P["S"] + P["T"] - 1
    exp = cc.noisy_expected(seed, mixed)
    assert exp["mm_status"][2] == 0 and exp["mm_status"][4] == 0  # no read over K, no seed skipped
    assert 30 <= len(case["errors"]) <= 50 and sum(exp["contained"]) >= 1
    units = cc.assembled(case, exp)
    assert len(units) == 1
    copy, cons = units[0]
    assert cons == case["genome"]
    assert len(copy) == len(cons) and 1 <= sum(1 for a, b in zip(copy, cons) if a != b) <= len(case["errors"])


def test_min_votes_without_the_pass_is_refused_by_the_wrapper():
    """unitig_file(min_votes=...) with nothing that turns the consensus pass on: refused before any file or library is touched"""
    from siga_amd import host
    for kw in ({}, {"consensus": False, "error_permille": 40}, {"reduce": True}):
        with pytest.raises(ValueError, match="min_votes"):
            host.unitig_file("absent.fa", "absent", 45, min_votes=2, **kw)
