"""The shift rule of tests/ballast_cases.py against the restatements themselves, with small ballast of real bytes: a hand-built
case behind ballast reads (or unitigs) must give, under unitig_cases.expected, trim_cases.expected_trim and
scaffold_cases.expected_scaffolds, exactly the case's own result shifted.  Only then may tests/test_gpu_unitig_wide.py use the
rule where the ballast has 2^32 bases and no restatement can run.  No GPU."""
import random

import pytest

from tests import ballast_cases as bc
from tests import scaffold_cases as sc
from tests import trim_cases as tc
from tests import unitig_cases as uc

# reads on their own; the joined pair; both, with lengths either side of the trim cases' L = 60; a joined chain of three
VARIANTS = {"singles": [40, 17, 1], "pair": [(60, 55, 25)], "mixed": [61, (60, 55, 25), 60, 1], "triple": [17, (60, 55, 50, 25, 21), 1]}
UC_CASES = uc.hand_built()
TC_CASES = tc.hand_built()
SC_CASES = sc.hand_built()
KEYS = ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "status")


def _ballast(variant, seed):
    bal = bc.Ballast(VARIANTS[variant])
    return bal, bc.small_reads(bal, random.Random(seed))


def test_the_ballast_is_what_it_says():
    assert bc.pair_af() == 6  # a touched at E, b touched at E: b lies reverse-complemented behind a
    bal, reads = _ballast("mixed", 1)
    assert bal.k == 5 and bal.lens == [61, 60, 55, 60, 1] and bal.edges == [(1, 2, 25, 6)]
    assert [b for b, _ in bal.units] == [61, 90, 60, 1] and bal.units[1][1] == [(1, 0, 0), (2, uc.PLACED_REV, 35)]
    # the ballast alone, through the restatement: the units, in item order, and one merged record
    exp = uc.expected(reads, bal.edges, 20)
    seqs = bal.unit_seqs(reads)
    assert exp["layout"] == [p for _, lay in bal.units for p in lay] and exp["useqs"] == b"".join(seqs)
    assert exp["status"] == [4, 212, 0, 0, 1, 0]
    assert seqs[1][:60] == reads[1] and seqs[1][35:] == uc.revcomp(reads[2])
    assert bc.shift_id(7, 5) == 12 and bc.shift_id(0xFFFFFFFF, 5) == 0xFFFFFFFF


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", UC_CASES, ids=[c["name"] for c in UC_CASES])
def test_unitigs_behind_ballast_are_the_shifted_ones(case, variant):
    bal, reads = _ballast(variant, 7)
    big = bc.concat_case(case, bal, reads)
    want = bc.shifted_unitigs(uc.expected(case["reads"], case["edges"], case["m"]), bal, bal.unit_seqs(reads))
    got = uc.expected(big["reads"], big["edges"], big["m"])
    for k in KEYS:
        assert got[k] == want[k], k
    assert want["useqs"][want["case_at"]:] == want["case_useqs"]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", TC_CASES, ids=[c["name"] for c in TC_CASES])
def test_trimmed_unitigs_behind_ballast_are_the_shifted_ones(case, variant):
    bal, reads = _ballast(variant, 8)
    big = bc.concat_case(case, bal, reads)
    want = bc.shifted_trim(tc.expected_of(case["name"]), bal, case["x"], case["L"], case["C"], bal.unit_seqs(reads))
    got = tc.expected_trim(big["reads"], big["edges"], big["m"], big["x"], big["L"], big["C"])
    for k in KEYS + ("removed", "uedges"):
        assert got[k] == want[k], k
    # ballast of at most L bases goes as an island in round 1, ballast above L stays
    for (bases, lay), gone in zip(bal.units, want["ballast_gone"]):
        assert gone == (bases <= case["L"])
        assert all(want["removed"][r] == int(gone) for r, _, _ in lay)


def test_trim_without_rounds_leaves_the_ballast():
    case = tc.case_named("all_removed")
    bal, reads = _ballast("mixed", 9)
    big = bc.concat_case(case, bal, reads)
    want = bc.shifted_trim(tc.expected_of("all_removed", 0), bal, 0, case["L"], case["C"], bal.unit_seqs(reads))
    got = tc.expected_trim(big["reads"], big["edges"], big["m"], 0, big["L"], big["C"])
    for k in KEYS + ("removed", "uedges"):
        assert got[k] == want[k], k
    assert not any(want["ballast_gone"])


def _scaffold_ballast(variant, insert_size, seed):
    items = {"singles": [40, 17, 1], "pair": [(60, 55, 7)], "mixed": [61, (60, 55, 7), 60, 1], "triple": [5, (33, 16, 119)]}[variant]
    bal = bc.ScaffoldBallast(items, insert_size)
    rng = random.Random(seed)
    useqs = bytes(rng.choice(b"ACGT") for _ in range(bal.bases))
    seqs, at = [], 0
    for it in items:
        if isinstance(it, int):
            seqs.append(useqs[at:at + it])
            at += it
        else:
            lu, lv, gap = it
            seqs.append(useqs[at:at + lu] + b"N" * gap + uc.revcomp(useqs[at + lu:at + lu + lv]))
            at += lu + lv
    return bal, useqs, seqs


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", [c[0] for c in SC_CASES])
def test_scaffolds_behind_ballast_are_the_shifted_ones(name, variant):
    _, res, links, o = sc.case_named(name)
    bal, useqs, seqs = _scaffold_ballast(variant, o["insert_size"], 10)
    exp = sc.expected_scaffolds(res, links, [0] * 24, o)
    big_res, big_links = bc.concat_scaffold_input(res, links, bal, useqs)
    want = bc.shifted_scaffolds(exp, bal, seqs)
    got = sc.expected_scaffolds(big_res, big_links, [0] * 24, o)
    for k in ("sc_offs", "sc_lay_offs", "sc_flags", "layout", "gaps", "seqs", "status"):
        assert got[k] == want[k], k
    # a larger insert size with every span of the case raised as much: the same scaffolds, so the ballast's gap is free
    bal2 = bc.ScaffoldBallast([(60, 55, 1000)], o["insert_size"] + 1000)
    raised = bc.raise_spans(links, 1000)
    assert sc.expected_scaffolds(res, raised, [0] * 24, dict(o, insert_size=o["insert_size"] + 1000)) == exp
    plain = {k: v for k, v in res.items() if k != "useqs"}
    big_res, big_links = bc.concat_scaffold_input(plain, raised, bal2)
    got = sc.expected_scaffolds(big_res, big_links, [0] * 24, dict(o, insert_size=o["insert_size"] + 1000))
    want = bc.shifted_scaffolds(sc.expected_scaffolds(plain, links, [0] * 24, o), bal2)
    for k in ("sc_offs", "sc_lay_offs", "sc_flags", "layout", "gaps", "status"):
        assert got[k] == want[k], k
    assert want["layout"][:2] == [(0, 0, 0), (1, uc.PLACED_REV, 1060)] and want["sc_offs"][1] == 1115
