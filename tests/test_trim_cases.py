"""The two brute forces of tests/trim_cases.py agree on every hand-built case, and the cases show what they claim.  No GPU."""
import pytest

from tests import trim_cases as tc
from tests import unitig_cases as uc

CASES = tc.hand_built()
IDS = [c["name"] for c in CASES]


def _both(case, max_rounds):
    exp = tc.expected_trim(case["reads"], case["edges"], case["m"], max_rounds, case["L"], case["C"])
    ref, gone, rounds = tc.reference_trim(case["reads"], case["edges"], case["m"], max_rounds, case["L"], case["C"])
    assert uc.canonical_set(exp) == tc.canonical_reference(ref), case["name"]
    assert {r: x for r, x in enumerate(exp["removed"]) if x} == gone, case["name"]
    assert exp["status"][6] == rounds
    return exp


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rules_equal_the_reference_loop(case):
    for x in sorted({0, 1, 2, case["x"]}):
        _both(case, x)


@pytest.mark.parametrize("case", uc.hand_built(), ids=[c["name"] for c in uc.hand_built()])
def test_no_rounds_is_the_unitig_result(case):
    exp = tc.expected_trim(case["reads"], case["edges"], case["m"], 0, 100, None)
    want = uc.expected(case["reads"], case["edges"], case["m"])
    for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs"):
        assert exp[k] == want[k], k
    assert exp["status"][:6] == want["status"] and exp["status"][6:11] == [0] * 5 and not any(exp["removed"])
    # every kept record is merged or lifted
    assert exp["status"][11] == len(case["edges"]) - want["status"][2] - want["status"][3] - want["status"][4]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_shows_what_it_claims(case):
    exp = tc.expected_of(case["name"])
    st, cl = exp["status"], case["claims"]
    for key, at in (("unitigs", 0), ("cycles", 5), ("rounds", 6), ("islands", 7), ("dead_ends", 8), ("gone", 9)):
        if key in cl:
            assert st[at] == cl[key], "%s: %s = %d, built for %d" % (case["name"], key, st[at], cl[key])
    assert all(exp["removed"][r] for r in cl.get("removed_ids", []))
    assert not any(exp["removed"][r] for r in cl.get("kept_ids", []))
    for rnd, ids in cl.get("by_round", {}).items():
        assert all(exp["removed"][r] == rnd for r in ids)
    if "afs" in cl:
        assert {e[3] for e in exp["uedges"]} == cl["afs"]
    assert sum(exp["lay_offs"][-1:]) == len(case["reads"]) - st[9]
    assert st[11] == len(exp["uedges"]) and all(q < st[0] and t < st[0] for q, t, _, _ in exp["uedges"])


def test_cascade_round_by_round():
    case = tc.case_named("cascade")
    gone = [tc.expected_of("cascade", x)["status"][9] for x in (0, 1, 2, 3, 10)]
    assert gone == [0, 4, 6, 7, 7]
    assert [tc.expected_of("cascade", x)["status"][6] for x in (1, 2, 3, 10)] == [1, 2, 3, 3]
    assert tc.expected_of("cascade", 3)["status"][0] == 1 and tc.expected_of("cascade", 2)["status"][0] > 1
    assert len(case["reads"]) == 13


def test_graph_case_joins_reversed_multi_read_unitigs():
    exp = tc.expected_of("graph")
    sizes = [exp["lay_offs"][u + 1] - exp["lay_offs"][u] for u in range(exp["status"][0])]
    starts_reversed = [exp["layout"][exp["lay_offs"][u]][1] & uc.PLACED_REV for u in range(exp["status"][0])]
    between = [(q, t, af) for q, t, _, af in exp["uedges"] if sizes[q] > 1 and sizes[t] > 1 and (starts_reversed[q] or starts_reversed[t])]
    assert {af for _, _, af in between} == {0, 3, 5, 6}


def test_lifted_records_are_real_overlaps_of_the_unitigs():
    """a lifted record over unitig bytes, by the coordinates the ED formatter derives from (length, af, lengths)"""
    for name in ("graph", "y", "ring_tip", "coverage"):
        exp = tc.expected_of(name)
        seqs = [exp["useqs"][exp["seq_offs"][u]:exp["seq_offs"][u + 1]] for u in range(exp["status"][0])]
        for q, t, ln, af in exp["uedges"]:
            a = seqs[q][:ln] if af & 1 else seqs[q][len(seqs[q]) - ln:]
            b = seqs[t][len(seqs[t]) - ln:] if af & 2 else seqs[t][:ln]
            assert a == (uc.revcomp(b) if af & 4 else b), (name, q, t, ln, af)


def test_end_to_end_error_reads_are_no_pieces_of_the_genome():
    """the 80 added reads of the end-to-end set each carry a substitution: none is a window of the genome on either strand (that
    trimming them takes two rounds is asserted where their records are made, in tests/test_gpu_unitig_trim.py)"""
    case = tc.end_to_end()
    assert len(case["reads"]) == uc.E2E_READS + tc.E2E_ERR_READS
    g, rg = case["genome"], uc.revcomp(case["genome"])
    for _, s in case["reads"][uc.E2E_READS:]:
        assert s not in g and s not in rg
