"""The brute-force expectation of tests/locate_cases.py against itself and against the oracle's counts, on the CPU: what
tests/test_gpu_locate.py compares the device's hits with is right before any kernel runs."""
import numpy as np
import pytest

from tests import locate_cases as lc
from tests import match_cases as mc


def test_small_case_holds_every_class():
    case = lc.small()
    seqs = [s for _, s in case["reads"]]
    assert all(set(s) <= set("ACGT") for s in seqs)
    assert sorted({len(s) for s in seqs}) == [1, 2, 13, lc.SMALL_LEN, 300]
    assert seqs.count(seqs[3]) == lc.N_DUP + 1
    assert any(s == mc.revcomp(s) for s in seqs)
    q = case["queries"]
    assert len({n for n, _, _ in q}) == len(q)
    lens = {len(s) for _, s, _ in q}
    assert {0, 1, 2, 12, 13, 14, 31, lc.SMALL_LEN, 300, 400} <= lens
    ns = [s for _, s, c in q if c.startswith("n_")]
    assert any(s[0] == "N" and len(s) > 1 for s in ns) and any(s[-1] == "N" and len(s) > 1 for s in ns)
    assert any("N" in s[1:-1] for s in ns)


@pytest.mark.parametrize("rc", (True, False))
def test_brute_force_is_self_consistent(rc):
    case = lc.small()
    seqs = [s for _, s in case["reads"]]
    q = case["queries"]
    exp = lc.expected(seqs, [s for _, s, _ in q], rc)
    by_class = {}
    for (name, w, cls), hits in zip(q, exp):
        if hits is None:
            assert not lc.is_acgt(w), name
            continue
        assert len(set(hits)) == len(hits), name
        for r, o, strand in hits:
            assert seqs[r][o:o + len(w)] == (mc.revcomp(w) if strand else w), (name, r, o, strand)
        if not rc:
            assert all(s == 0 for _, _, s in hits)
        by_class.setdefault(cls, []).append((w, hits))
    assert [h for _, h in by_class["absent"]] == [[]] and [h for _, h in by_class["absent_subst"]] == [[]]
    assert [h for _, h in by_class["longer_than_reads"]] == [[]]
    (w, hits), = by_class["duplicate"]
    assert len({r for r, o, s in hits if o == 0 and s == 0}) >= lc.N_DUP + 1  # several reads, same offset
    (w, hits), = by_class["palindrome"]
    pal_read = [n for n, _ in case["reads"]].index("pal")
    assert [h for h in hits if h[0] == pal_read] == ([(pal_read, 0, 0), (pal_read, 0, 1)] if rc else [(pal_read, 0, 0)])
    w, hits = by_class["periodic"][0]
    per = [n for n, _ in case["reads"]].index("periodic")
    assert [o for r, o, s in hits if r == per and s == 0] == list(range(0, lc.SMALL_LEN, 2))  # overlapping offsets in one read
    (w, hits), = by_class["at_start"]
    assert any(o == 0 for _, o, _ in hits)
    (w, hits), = by_class["at_end"]
    assert any(o + len(w) == len(seqs[r]) for r, o, _ in hits)


@pytest.mark.parametrize("rc", (True, False))
def test_totals_equal_the_oracles_counts(rc):
    case = lc.small()
    seqs = [s for _, s in case["reads"]]
    fwd = lc.oracle_index("small")
    q = case["queries"]
    exp = lc.expected(seqs, [s for _, s, _ in q], rc)
    for (name, w, _), hits in zip(q, exp):
        if hits is not None:
            assert len(hits) == mc.count(fwd, w, rc), name


def test_many_case_one_base_counts():
    case = lc.many()
    fwd = lc.oracle_index("many")
    assert case["reads"].shape == (lc.MANY_READS, lc.MANY_LEN)
    for name, w, _ in case["queries"]:
        for rc in (False, True):
            hits = lc.expected_one_base(case["reads"], w, rc)
            assert len(hits) == mc.count(fwd, w, rc)
            assert len(hits) > (250000 if not rc else 500000)
            assert len(np.unique(hits, axis=0)) == len(hits)
