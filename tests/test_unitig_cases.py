"""The two brute-force restatements of `siga unitig` (tests/unitig_cases.py) against each other, and what every layout must
hold, on the hand-built graphs.  No GPU."""
import pytest

from tests import unitig_cases as uc

CASES = uc.hand_built()


@pytest.fixture(scope="module")
def exp():
    return {c["name"]: uc.expected(c["reads"], c["edges"], c["m"]) for c in CASES}


def test_the_cases_cover_what_they_claim(exp):
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    for n in (1, 2, 3, 63, 64, 65, 1000):
        e = exp["chain%d" % n]
        assert e["status"][0] == 1 and e["status"][4] == n - 1 and e["lay_offs"] == [0, n]
    for n in (2, 3, 65):
        e = exp["cycle%d" % n]
        assert e["status"][5] == 1 and e["status"][4] == n - 1 + 1 and e["uflags"][0] & uc.CIRCULAR and e["uflags"][0] >> 1 >= 20
    assert exp["cycle_mid"]["status"][5] == 2
    heads = exp["heads"]
    first = [heads["layout"][a] for a in heads["lay_offs"][:-1]]
    assert {fl for _, fl, _ in first} == {0, uc.PLACED_REV}  # heads left through E and through B
    assert exp["branch"]["status"][0] == 3 + 1 and exp["branch"]["status"][4] == 2
    assert exp["containment"]["status"][4] == 1  # 4 reads in a chain, the second blocked at both ends: only (2, 3) is left
    assert exp["self"]["status"][4] == 3  # the self edge at E alone leaves the B end simple
    assert exp["double"]["status"][4] == 1
    mal = next(c for c in CASES if c["name"] == "malformed")
    assert exp["malformed"]["status"][2:5] == [mal["n_bad"], mal["n_low"], 5]
    assert exp["no_edges"]["status"] == [5, 150, 0, 0, 0, 0]
    lens = sorted({len(r) for r in next(c for c in CASES if c["name"] == "lengths")["reads"]})
    assert lens[0] == 2 and lens[-1] == 300
    assert any(any(fl for _, fl, _ in e["layout"]) and not all(fl for _, fl, _ in e["layout"]) for e in exp.values())


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_two_brute_forces_agree(case, exp):
    ref = uc.reference(case["reads"], case["edges"], case["m"])
    assert sorted(uc.canonical(s, c, k) for s, c, k in ref) == uc.canonical_set(exp[case["name"]])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_placements(case, exp):
    e = exp[case["name"]]
    reads = case["reads"]
    assert sorted(r for r, _, _ in e["layout"]) == list(range(len(reads)))  # placements partition the reads
    assert e["lay_offs"][0] == 0 and e["lay_offs"][-1] == len(reads) and e["seq_offs"][-1] == len(e["useqs"])
    starts = []
    for u in range(len(e["uflags"])):
        seq = e["useqs"][e["seq_offs"][u]:e["seq_offs"][u + 1]]
        lay = e["layout"][e["lay_offs"][u]:e["lay_offs"][u + 1]]
        starts.append(lay[0][0])
        assert lay[0][2] == 0
        for read, fl, off in lay:
            placed = uc.revcomp(reads[read]) if fl & uc.PLACED_REV else reads[read]
            assert seq[off:off + len(placed)] == placed
        if e["uflags"][u] & uc.CIRCULAR:
            k = e["uflags"][u] >> 1
            assert lay[0][0] == min(r for r, _, _ in lay) and lay[0][1] == 0 and seq[-k:] == seq[:k]
    assert starts == sorted(starts)  # numbered by ascending start read


def test_end_to_end_genome_has_no_long_repeat():
    c = uc.end_to_end()
    assert len(c["genome"]) == 6000 and len(c["reads"]) == 600 and all(len(s) == 60 for _, s in c["reads"])
    assert not uc.longest_repeat_at_least(c["genome"], c["m"])
    assert uc.longest_repeat_at_least(c["genome"] + c["genome"][100:130], 25)  # (the check sees one when there is one)
    strands = [s in c["genome"] for _, s in c["reads"]]
    assert any(strands) and not all(strands)
