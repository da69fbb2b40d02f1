"""The two brute forces of tests/prune_cases.py agree on every hand-built case and on 300 seeded random graphs, delta = 0 is the
trim restatement, and the cases show what they claim.  No GPU."""
import pytest

from tests import prune_cases as pc
from tests import trim_cases as tc
from tests import unitig_cases as uc

CASES = pc.hand_built()
IDS = [c["name"] for c in CASES]


def _both(case, max_rounds=None, **over):
    exp = pc.run(pc.expected_prune, case, max_rounds, **over)
    ref, gone, cuts, rounds = pc.run(pc.reference_prune, case, max_rounds, **over)
    what = (case["name"], max_rounds, over)
    assert uc.canonical_set(exp) == tc.canonical_reference(ref), what
    assert {r: x for r, x in enumerate(exp["removed"]) if x} == gone, what
    assert {i: x for i, x in enumerate(exp["cut"]) if x} == cuts, what
    assert exp["status"][6] == rounds, what
    return exp


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rules_equal_the_reference_loop(case):
    if len(case["reads"]) > 40:
        _both(case)
        return
    for x in sorted({0, 1, 2, case["x"]}):  # and in either mode, and with delta = 1
        _both(case, x)
    _both(case, careful=not case["careful"])
    _both(case, delta=1)


@pytest.mark.parametrize("block", range(10))
def test_random_graphs(block):
    cut = gone = 0
    for seed in range(30 * block, 30 * block + 30):
        case = pc.random_case(seed)
        assert len(case["reads"]) <= 12 and 1 <= case["delta"] <= 30
        exp = _both(case)
        _both(case, careful=not case["careful"])
        cut += exp["status"][12]
        gone += exp["status"][9]
    print("block", block, "records cut", cut, "reads removed", gone)


def test_random_graphs_cut_and_trim():
    """the random graphs are no idle exercise: records are cut in both modes, and reads go after a cut"""
    st = [pc.run(pc.expected_prune, pc.random_case(s))["status"] + [pc.random_case(s)["careful"]] for s in range(300)]
    assert sum(1 for s in st if s[12] and s[16]) >= 5 and sum(1 for s in st if s[12] and not s[16]) >= 10
    assert sum(1 for s in st if s[12] and s[9]) >= 10


@pytest.mark.parametrize("case", tc.hand_built(), ids=[c["name"] for c in tc.hand_built()])
def test_delta_0_is_the_trim_result(case):
    want = tc.expected_of(case["name"])
    for careful in (False, True):
        exp = pc.expected_prune(case["reads"], case["edges"], case["m"], case["x"], case["L"], case["C"], 0, careful, None, 5000, 13.0)
        for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "removed", "uedges"):
            assert exp[k] == want[k], k
        assert exp["status"][:12] == want["status"] and exp["status"][12:] == [0] * 4 and not any(exp["cut"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_shows_what_it_claims(case):
    exp = pc.expected_of(case["name"])
    st, cl = exp["status"], case["claims"]
    for key, at in (("unitigs", 0), ("cycles", 5), ("rounds", 6), ("islands", 7), ("dead_ends", 8), ("gone", 9), ("cut", 12), ("cut_rounds", 13),
                    ("unique", 14)):
        if key in cl:
            assert st[at] == cl[key], "%s: %s = %d, built for %d" % (case["name"], key, st[at], cl[key])
    assert all(exp["removed"][r] for r in cl.get("removed_ids", []))
    assert not any(exp["removed"][r] for r in cl.get("kept_ids", []))
    for rnd, ids in cl.get("by_round", {}).items():
        assert all(exp["removed"][r] == rnd for r in ids)
    for (a, b), rnd in cl.get("cut_recs", {}).items():
        assert exp["cut"][pc.rec_between(case, a, b)] == rnd, (case["name"], a, b)
    for a, b in cl.get("kept_recs", []):
        assert exp["cut"][pc.rec_between(case, a, b)] == 0, (case["name"], a, b)
    assert st[12] == sum(1 for x in exp["cut"] if x) and st[15] == 0
    assert len(case["reads"]) <= 40 or case["name"].startswith("hub300")
    assert all(40 <= len(r) <= 150 for r in case["reads"])


def test_every_kept_record_is_a_real_overlap():
    for case in CASES + [pc.random_case(s) for s in range(0, 300, 7)] + [pc.large_case(600)]:
        lens = [len(r) for r in case["reads"]]
        for rec in case["edges"]:
            c = uc.classify(rec, lens, case["m"])
            if c in ("bad", "low") or c[3]:  # (a read-level self record is never merged)
                continue
            q, t, ln, af = rec
            a = case["reads"][q][:ln] if af & 1 else case["reads"][q][lens[q] - ln:]
            b = case["reads"][t][lens[t] - ln:] if af & 2 else case["reads"][t][:ln]
            assert a == (uc.revcomp(b) if af & 4 else b), (case["name"], rec)


def test_hub_has_300_records_at_one_end_and_states_across_blocks():
    case = pc.case_named("hub300")
    exp = pc.expected_of("hub300")
    assert sum(1 for q, t, _, _ in case["edges"] if 0 in (q, t)) == 300 and len(case["reads"]) == 3301
    assert exp["status"][12] > 200 and pc.expected_of("hub300_careful")["status"][12] == 0


def test_careful_differs_where_built_to():
    for plain, careful in (("fork", "fork_careful"), ("parallel", "parallel_careful"), ("self_self", "self_self_careful")):
        assert pc.expected_of(plain)["status"][12] == 1 and pc.expected_of(careful)["status"][12] == 0
    for same in ("one_side", "self_tip"):
        assert pc.expected_of(same)["cut"] == pc.expected_of(same + "_careful")["cut"] and any(pc.expected_of(same)["cut"])


def test_large_case_shape():
    case = pc.large_case()
    assert 19000 <= len(case["reads"]) <= 21000 and 50000 <= len(case["edges"]) <= 70000, (len(case["reads"]), len(case["edges"]))
