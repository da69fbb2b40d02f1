"""The two brute forces of tests/chimeric_cases.py agree on every hand-built case and on 300 seeded random graphs, Lc = 0 is the
prune restatement, the cases show what they claim, and on reads tiling a genome with reads made of two distant halves among them
the chimeric step takes planted reads and nothing else.  No GPU."""
import functools

import numpy as np
import pytest

from tests import chimeric_cases as cc
from tests import prune_cases as pc
from tests import trim_cases as tc
from tests import unitig_cases as uc

CASES = cc.hand_built()
IDS = [c["name"] for c in CASES]


def _both(case, max_rounds=None, **over):
    exp = cc.run(cc.expected_chimeric, case, max_rounds, **over)
    ref, gone, cuts, rounds = cc.run(cc.reference_chimeric, case, max_rounds, **over)
    what = (case["name"], max_rounds, over)
    assert uc.canonical_set(exp) == tc.canonical_reference(ref), what
    assert {r: x for r, x in enumerate(exp["removed"]) if x} == gone, what  # (the round and, by the flag bit, the step)
    assert {i: x for i, x in enumerate(exp["cut"]) if x} == cuts, what
    assert exp["status"][6] == rounds, what
    return exp


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rules_equal_the_reference_loop(case):
    for x in sorted({0, 1, 2, case["x"]}):
        for delta in (0, 10):  # without and with -d
            _both(case, x, delta=delta)
    _both(case, delta=10, careful=True)


@pytest.mark.parametrize("block", range(10))
def test_random_graphs(block):
    chim = 0
    for seed in range(30 * block, 30 * block + 30):
        case = cc.random_case(seed)
        assert len(case["reads"]) <= 15
        exp = _both(case)
        _both(case, delta=0)
        _both(case, careful=not case["careful"])
        chim += exp["status"][16]
    print("block", block, "chimeric unitigs", chim)


def test_random_graphs_remove_chimeric_unitigs():
    """the random graphs are no idle exercise"""
    st = [cc.run(cc.expected_chimeric, cc.random_case(s))["status"] for s in range(300)]
    assert sum(1 for s in st if s[16]) >= 30 and sum(1 for s in st if s[16] and s[12]) >= 5 and sum(1 for s in st if s[16] and s[7] + s[8]) >= 5


PC_SMALL = [c for c in pc.hand_built() if len(c["reads"]) <= 40]  # (not the two of 3 301 reads: the serial rules take seconds there)


@pytest.mark.parametrize("case", PC_SMALL, ids=[c["name"] for c in PC_SMALL])
def test_lc_0_is_the_prune_result(case):
    want = pc.expected_of(case["name"])
    exp = cc.expected_chimeric(case["reads"], case["edges"], case["m"], case["x"], case["L"], case["C"], case["delta"], case["careful"], case["N"],
                               case["G"], case["T"], Lc=0, Ac=2, delta_c=5, Tc=1.0)
    for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "removed", "cut", "uedges"):
        assert exp[k] == want[k], k
    assert exp["status"][:16] == want["status"] and exp["status"][16:] == [0] * 4


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_shows_what_it_claims(case):
    exp = cc.expected_of(case["name"])
    st, cl = exp["status"], case["claims"]
    for key, at in (("unitigs", 0), ("cycles", 5), ("rounds", 6), ("islands", 7), ("dead_ends", 8), ("chim", 16), ("chim_reads", 17),
                    ("chim_rounds", 18)):
        if key in cl:
            assert st[at] == cl[key], "%s: %s = %d, built for %d" % (case["name"], key, st[at], cl[key])
    assert "chim" in cl
    assert all(exp["removed"][r] for r in cl.get("removed_ids", []))
    assert not any(exp["removed"][r] for r in cl.get("kept_ids", []))
    for r, rnd in cl.get("flagged", {}).items():
        assert exp["removed"][r] == rnd | cc.CHIMERIC, (case["name"], r)
    assert st[17] == sum(1 for x in exp["removed"] if x & cc.CHIMERIC) and st[9] == sum(1 for x in exp["removed"] if x) and st[19] == 0
    assert len(case["reads"]) <= 12 and all(40 <= len(r) <= 150 for r in case["reads"])


def test_every_kept_record_is_a_real_overlap():
    for case in CASES + [cc.random_case(s) for s in range(0, 300, 7)] + [cc.large_case(600, bridges=20)]:
        lens = [len(r) for r in case["reads"]]
        for rec in case["edges"]:
            c = uc.classify(rec, lens, case["m"])
            if c in ("bad", "low") or c[3]:  # (a read-level self record is never merged)
                continue
            q, t, ln, af = rec
            a = case["reads"][q][:ln] if af & 1 else case["reads"][q][lens[q] - ln:]
            b = case["reads"][t][lens[t] - ln:] if af & 2 else case["reads"][t][:ln]
            assert a == (uc.revcomp(b) if af & 4 else b), (case["name"], rec)


def test_pairs_differ_where_built_to():
    for gone, stays in (("bridge2_within", "bridge2_beyond"), ("others_above_bases", "others_at_bases"), ("others_above_reads", "others_at_reads"),
                        ("good_by_reads", "good_by_neither"), ("coverage_low_enough", "coverage_too_high"), ("bridge", "not_unique"),
                        ("bridge", "beyond_genome"), ("bridge", "no_step"), ("second_round", "second_round_1round")):
        assert cc.expected_of(gone)["status"][16] == 1 and cc.expected_of(stays)["status"][16] == 0, (gone, stays)
    # the bridge of "after_trim" is one only because the step reads what the trim step of the same round left
    case = cc.case_named("after_trim")
    assert cc.run(cc.expected_chimeric, dict(case, L=30))["status"][16] == 0


def test_large_case_shape():
    case = cc.large_case()
    assert 20000 <= len(case["reads"]) <= 20200 and 60000 <= len(case["edges"]) <= 70400


# ---- end to end over the CPU oracle's overlap records ----
@functools.lru_cache(maxsize=None)
def _oracle_edges():
    from oracle import pyoracle as po
    from siga_amd.overlap import name_ranks
    from tests.bigcheck import expected_edges
    names, reads, _ = cc.end_to_end()
    seqs = [r.decode() for r in reads]
    fwd, rev = po.Index.build(seqs), po.Index.build(seqs, reverse=True)
    want = po.overlap_batch(fwd, rev, seqs, cc.E2E_M)
    lengths = np.array([len(r) for r in reads], dtype=np.uint32)
    e = expected_edges(want["blocks"], want["block_offs"], fwd.sai(), rev.sai(), lengths, np.asarray(name_ranks(names)))
    return [tuple(int(x) for x in rec) for rec in e.tolist()]


def test_end_to_end_takes_planted_reads_only():
    _, reads, planted = cc.end_to_end()
    edges = _oracle_edges()
    assert len(edges) > len(reads) // 2
    kw = dict(delta=cc.E2E_DELTA, N=None, G=cc.E2E_GENOME, T=cc.E2E_T, Lc=cc.E2E_LC, Ac=None, delta_c=0, Tc=cc.E2E_TC)
    exp = cc.expected_chimeric(reads, edges, cc.E2E_M, cc.E2E_X, cc.E2E_L, None, **kw)
    ref, gone, cuts, rounds = cc.reference_chimeric(reads, edges, cc.E2E_M, cc.E2E_X, cc.E2E_L, None, **kw)
    assert uc.canonical_set(exp) == tc.canonical_reference(ref)
    assert {r: x for r, x in enumerate(exp["removed"]) if x} == gone and exp["status"][6] == rounds
    taken = [r for r, x in enumerate(exp["removed"]) if x & cc.CHIMERIC]
    print("status", exp["status"], "taken as chimeric", taken, "planted", planted)
    assert any(r in planted for r in taken)
    assert all(r in planted for r in taken)
