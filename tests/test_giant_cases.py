"""The tables-only mode of the round restatements, and what tests/giant_cases.py claims of its cases.  No GPU.

Tables only: every hand-built case of trim_cases, prune_cases, chimeric_cases, bubble_cases, indel_cases and reduce_cases runs through
its restatement in tables-only mode twice -- over its own reads, and over its reads with every read whose bytes the first run never
asked for (no arm of a compared bubble or indel group) replaced by its length -- and both give the normal run's tables, key by key.

The claims: every case of giant_cases (b) and (c) has the decision it names; the cases of LOW_WORD_DIFFERS have the other one when
the giant's bases are cut to their low word; every case of (c) falls on the other side when its expression wraps at 32 bits."""
import pytest

from tests import giant_cases as gc
from tests import unitig_cases as uc

EVERY = [(step, c["name"]) for step in ("trim", "cut", "chimeric", "bubble", "indel", "reduce") for c in gc.STEPS[step][0].hand_built()]


@pytest.mark.parametrize("step,name", EVERY, ids=["%s-%s" % e for e in EVERY])
def test_tables_only_gives_the_same_tables(step, name):
    mod = gc.STEPS[step][0]
    case, want = gc.full(mod.case_named(name)), mod.expected_of(name)
    uc.NEEDED = set()
    try:
        own = gc.restate(step, case)
        needed = set(uc.NEEDED)
    finally:
        uc.NEEDED = None
    lengths = dict(case, reads=[r if id(r) in needed else len(r) for r in case["reads"]])
    assert step in ("bubble", "indel") or not needed
    assert any(isinstance(r, int) for r in lengths["reads"])
    bare = gc.restate(step, lengths)
    for k in gc.TABLES:
        if k in want:
            assert own[k] == want[k] and bare[k] == want[k], k
    assert own["useqs"] is None and bare["useqs"] is None and set(own) == set(want)


def test_an_arm_given_as_a_length_is_refused():
    case = gc.full(gc.STEPS["bubble"][0].case_named("two_arms"))
    with pytest.raises(AssertionError, match="given as a length"):
        gc.restate("bubble", dict(case, reads=[len(r) for r in case["reads"]]))
    case = gc.full(gc.STEPS["indel"][0].case_named("deleted_first"))
    with pytest.raises(AssertionError, match="given as a length"):
        gc.restate("indel", dict(case, reads=[len(r) for r in case["reads"]]))


# ---- (a) ----
def test_the_table_of_cases_behind_ballast():
    assert len(gc.BEHIND) == 29 + 10 and {s for _, _, s in gc.BEHIND} == {"a", "c"}
    assert sum(gc.SHAPES["a"]) == gc.G32 - 37 and sum(gc.SHAPES["c"]) == gc.G32 + gc.G31 + 1


@pytest.mark.parametrize("step,name,shape", [b for b in gc.BEHIND if b[1] in ("two_arms", "e31_ed32", "fork", "bridge_flipped", "revive")],
                         ids=lambda v: str(v))
def test_behind_ballast_the_case_is_the_small_one_further_on(step, name, shape):
    """(the GPU tests take the restatement's tables as they are; this is what they must look like)"""
    big, bal, exp, small = gc.behind(step, name, shape)
    nu, at = len(bal.units), sum(b for b, _ in bal.units)
    assert exp["seq_offs"][:nu + 1] == [sum(bal.lens[:i]) for i in range(nu + 1)] and exp["seq_offs"][nu] == at
    assert [x - at for x in exp["seq_offs"][nu:]] == small["seq_offs"]
    assert exp["removed"] == [0] * bal.k + small["removed"] and exp["cut"] == small["cut"]
    assert exp["status"][2:] == small["status"][2:] and exp["status"][1] == small["status"][1] + at
    assert exp["layout"][bal.k:] == [(r + bal.k, fl, off) for r, fl, off in small["layout"]]


# ---- (b) ----
GIANTS = [c["name"] for c in gc.giants()]


@pytest.mark.parametrize("name", GIANTS)
def test_a_giant_case_has_its_decision(name):
    case = gc.giant_named(name)
    exp = gc.giant_expected(name)
    assert gc.decision(case, exp) == case["want"]
    assert exp["status"][1] > gc.G32 and case["third"] in exp["layout"] and max(off for _, _, off in exp["layout"]) > gc.G32
    if name in gc.LOW_WORD_DIFFERS:
        low = gc.restate(case["step"], gc.truncated(case))  # (never run on the device: the restatement's own margin)
        assert gc.decision(case, low) != case["want"], "the low word alone decides the same"
    if case["step"] == "reduce":  # through the reduce entry with reduce = 1: no record is transitive, and nothing else changes
        red = gc.giant_expected(name, 1)
        assert red["first_flags"] == set() and not any(x & gc.rc.TRANSITIVE for x in red["cut"])
        assert red["status"][32:34] == [0, 0] and red["status"][34] >= 1 and red["status"][35] > 0
        assert gc.giant_expected(name, 0)["status"] == exp["status"] and exp["status"][32:] == [0] * 8
        for k in gc.TABLES:
            assert k == "status" or red[k] == exp[k], k
        assert red["status"][:32] == exp["status"][:32]


def test_what_the_giant_cases_were_built_to_show():
    fork = gc.giant_expected("giant_fork_third_of_genome")
    case = gc.giant_named("giant_fork_third_of_genome")
    assert fork["status"][12] == 1 and fork["status"][14] == 1  # one record cut; in round 1 the giant alone is unique
    assert fork["removed"].count(1) == 2  # the loser, a dead end of 78 bases, goes in the same round
    assert max(off for _, _, off in fork["layout"]) > gc.G32 + 31  # the winner's reads are placed behind the giant's
    assert gc.giant_expected("giant_fork_beyond_genome")["status"][12] == 0
    assert gc.giant_expected("giant_fork_over_half_genome")["status"][14] == 1
    assert gc.giant_expected("giant_fork_careful")["status"][12] == 1
    other = gc.giant_expected("giant_other")
    assert other["status"][16:19] == [1, 1, 1] and other["status"][0] == 1  # the bridge gone, a + giant + c are one unitig
    assert gc.giant_expected("giant_other_saturated")["status"][16] == 0
    assert gc.giant_named("giant_other_saturated")["delta_c"] + 60 == gc.U32
    assert gc.giant_expected("giant_other_below_saturation")["status"][16] == 1
    assert gc.giant_expected("giant_neighbour_unique")["status"][16] == 1
    assert gc.giant_expected("giant_neighbour_not_unique")["status"][16] == 0
    assert gc.giant_named("giant_neighbour_not_unique")["Tc"] > gc.GIANT_SCORE + 1.0
    tip = gc.giant_expected("giant_tip")
    assert tip["removed"][gc.giant_named("giant_tip")["tip"]] == 1 and tip["removed"][:3] == [0, 0, 0] and tip["status"][6:10] == [1, 0, 1, 1]
    indel = gc.giant_expected("giant_indel_permille")
    small = gc.ic.expected_of("at_permille")
    assert indel["status"][24:29] == small["status"][24:29] == [1, 1, 1, 0, 0]
    assert indel["status"][0] == 1 and indel["status"][1] > 2 * gc.G32  # both giants and the winner are one unitig
    assert case["giants"] == 1 and gc.giant_named("giant_indel_permille")["giants"] == 2


# ---- (c) ----
NO_WRAP = [c["name"] for c in gc.no_wrap()]


@pytest.mark.parametrize("name", NO_WRAP)
def test_a_no_wrap_case_has_its_decision_and_the_other_one_wrapped(name):
    case = gc.no_wrap_named(name)
    exp = gc.no_wrap_expected(name)
    assert gc.decision(case, exp) == case["want"] == case["expr"](False) != case["expr"](True)
    tables = gc.no_wrap_expected(name, True)
    for k in gc.TABLES:
        assert k not in exp or tables[k] == exp[k], k
