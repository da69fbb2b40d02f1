"""The serial restatement of the transitive reduction (tests/reduce_cases.py) against the claims written into its cases and, on five
read sets, against the irreducible overlap run of the CPU oracle: exhaustive records, reduced, are that run's records."""
import pytest

from tests import indel_cases as ic
from tests import reduce_cases as rc
from tests import unitig_cases as uc

CASES = rc.hand_built()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_claims(case):
    exp = rc.expected_of(case["name"])
    cl, st = case["claims"], exp["status"]
    flagged = [i for i, x in enumerate(exp["cut"]) if x & rc.TRANSITIVE]
    print(case["name"], "status", st, "flagged", flagged, "first", sorted(exp["first_flags"]))
    assert len(st) == 40 and st[36:] == [0] * 4 and st[33] == len(flagged) and st[32] == len(exp["first_flags"])
    if "flagged" in cl:
        assert flagged == cl["flagged"]
        assert sorted(exp["first_flags"]) == cl.get("first", cl["flagged"])
    for key, at in (("unitigs", 0), ("rounds", 6), ("passes", 34)):
        if key in cl:
            assert st[at] == cl[key], key
    where = rc.unit_of(exp)
    if "together" in cl:
        assert len({where[r] for r in cl["together"]}) == 1
    if "apart" in cl:
        assert len({where[r] for r in cl["apart"]}) == len(cl["apart"])
    for i in cl.get("cut_in_1", []):
        assert exp["cut"][i] == 1
    for r, rnd in cl.get("chimeric", {}).items():
        assert exp["removed"][r] == rnd | ic.CHIMERIC
    # no record is both flagged and lifted, and a containment or a self edge is never flagged
    lens = [len(r) for r in case["reads"]]
    for i in flagged:
        sq, st_, contain, self_edge = uc.classify(case["edges"][i], lens, case["m"])
        assert not contain and not self_edge


def test_triple_strands_cover_every_af_and_agree():
    base = rc.expected_of("triple")
    afs = {0: set(), 1: set(), 2: set()}
    for k in range(16):
        case = rc.case_named("triple_strands_%d" % k)
        exp = rc.expected_of(case["name"])
        assert uc.canonical_set(exp) == uc.canonical_set(base)
        assert [i for i, x in enumerate(exp["cut"]) if x] == [2]
        for i in range(3):
            afs[i].add(case["edges"][i][3])
    assert all(v == {0, 3, 5, 6} for v in afs.values()), afs


def test_chain5_needs_flagged_witnesses():
    """the record between the first and the last read has no pair of witnesses that are both unflagged"""
    case, exp = rc.case_named("chain5"), rc.expected_of("chain5")
    lens = [len(r) for r in case["reads"]]
    kept = [e for i, e in enumerate(case["edges"]) if not exp["cut"][i]]
    again, _ = rc.reduce_pass(lens, kept, case["m"], [0] * 5, [0] * len(kept))
    assert len(kept) == 4 and not again
    full = [i for i, e in enumerate(case["edges"]) if e[2] == 20]
    assert len(full) == 1 and exp["cut"][full[0]] == rc.TRANSITIVE


def test_revive_is_what_the_feature_is_for():
    case, exp = rc.case_named("revive"), rc.expected_of("revive")
    a, b, c = case["claims"]["abc"]
    ac = case["claims"]["ac"]
    assert exp["pass_flags"] == [(1, {ac}), (2, set())] and exp["cut"][ac] == 0 and exp["status"][32:36] == [1, 0, 2, exp["status"][35]]
    assert exp["removed"][b] == 1 | ic.CHIMERIC
    where = rc.unit_of(exp)
    assert where[a] == where[c]
    irr = rc.case_named("revive_irreducible")
    assert irr["edges"] == [e for i, e in enumerate(case["edges"]) if i != ac] and irr["reads"] == case["reads"]
    plain = ic.run(ic.expected_indel, irr)
    where = rc.unit_of(plain)
    assert where[a] != where[c] and plain["removed"][b] == 1 | ic.CHIMERIC
    # one round only: the pass of round 1 alone would leave A-C flagged and the chain broken
    one = rc.expected_of("revive", 1)
    assert one["cut"][ac] == 0 and one["status"][34] == 2  # (the final pass runs behind a round that changed something)


def test_wide_end_and_sizes():
    case = rc.case_named("wide_end")
    lens = [len(r) for r in case["reads"]]
    part = rc.participants(lens, case["edges"], case["m"], [0] * len(lens), [0] * len(case["edges"]))
    assert sum(1 for _, a, b, _ in part if 1 in (a, b)) == 300
    exp = rc.expected_of("wide_end")
    assert 50 <= exp["status"][33] < len(part)
    for want in (0, 1, 63, 64, 65, 255, 256, 257):
        exp = rc.expected_of("participants_%d" % want)
        assert exp["status"][35] == want == len(rc.case_named("participants_%d" % want)["edges"])


def test_reduce_off_is_the_indel_restatement():
    for name in ("triple", "revive", "chain5"):
        case = rc.case_named(name)
        off = rc.run(rc.expected_reduce, case, reduce=False)
        plain = ic.run(ic.expected_indel, case)
        assert off["status"] == plain["status"] + [0] * 8 and off["cut"] == plain["cut"] and off["layout"] == plain["layout"]


def test_a_graph_without_transitive_records_goes_through_the_rounds_as_before():
    """a case of the indel cases: the passes flag nothing, and round by round the result is expected_indel's"""
    case = ic.case_named("deleted_middle")
    exp = ic.run(rc.expected_reduce, case)
    plain = ic.run(ic.expected_indel, case)
    assert exp["status"][32:34] == [0, 0] and exp["status"][34] >= 2
    for key in ("removed", "cut", "seq_offs", "lay_offs", "uflags", "layout", "useqs", "uedges"):
        assert exp[key] == plain[key], key
    assert exp["status"][:32] == plain["status"]


# ---- the yardstick from the reference: its own irreducible overlap run ----
@pytest.mark.parametrize("k", range(len(rc.ORACLE_SETS)), ids=[s[0] for s in rc.ORACLE_SETS])
def test_exhaustive_reduced_is_the_oracles_irreducible_run(k):
    s = rc.oracle_sets()[k]
    reads, m, exh, irr = s["reads"], s["m"], s["exhaustive"], s["irreducible"]
    lens = [len(r) for r in reads]
    classes = [uc.classify(e, lens, m) for e in exh]
    # a condition, not a measurement: no containment and no self record, so the test cannot pass by leaving records out
    assert all(c not in ("bad", "low") for c in classes)
    assert sum(1 for c in classes if c[2]) == 0 and sum(1 for c in classes if c[3]) == 0
    exp = rc.expected_reduce(reads, exh, m, 0, 0)
    left = [e for i, e in enumerate(exh) if not exp["cut"][i] & rc.TRANSITIVE]
    print(s["name"], "reads", len(reads), "exhaustive", len(exh), "irreducible", len(irr), "reduced", len(left))
    assert len(set(exh)) == len(exh) and len(irr) < len(exh)
    assert set(left) == set(irr) and len(left) == len(irr)
    assert exp["status"][32] == exp["status"][33] == len(exh) - len(irr) and exp["status"][34] == 1 and exp["status"][35] == len(exh)
    want = uc.expected(reads, irr, m)
    for key in ("seq_offs", "lay_offs", "uflags", "layout", "useqs"):
        assert exp[key] == want[key], key
