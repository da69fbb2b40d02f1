"""The cases of tests/test_gpu_correct_matrix.py (tests/golden/make_reads.py: correct_case) hold what they claim, judged by
the oracle alone: every k and every option set of the lists, every planted class, and enough reads that the oracle corrects,
leaves alone and refuses -- among them planted reads whose winning candidate lies beyond the first eight unsolid bases and
beyond the first 64-base chunk.  CPU only."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests.bigcheck import correct_oracle, pack_case
from tests.golden import make_reads as mr


@pytest.fixture(scope="module")
def cases():
    out = {}
    for seed in mr.CORRECT_SEEDS:
        case = mr.correct_case(seed)
        seqs, quals, offs = pack_case(case)
        got, valid = correct_oracle(case)
        o = offs.astype(np.int64)
        changed = np.array([not np.array_equal(got[o[i]:o[i + 1]], seqs[o[i]:o[i + 1]]) for i in range(len(valid))])
        out[seed] = dict(case=case, seqs=seqs, offs=o, out=got, valid=valid.astype(bool), changed=changed)
    return out


def test_cases_cover_the_lists(cases):
    ks = {c["case"]["k"] for c in cases.values()}
    assert ks >= {7, 8, 12, 13, 14, 31, 32, 33, 55, 56, 57, 65, 100} and ks >= set(mr.CORRECT_KS)
    opts = {(c["case"]["threshold"], c["case"]["rounds"], c["case"]["offset"]) for c in cases.values()}
    assert opts >= {(3, 10, 1), (-1, 10, 1), (-2, 10, 1), (0, 10, 0), (5, 1, 4), (3, 0, 1), (2, 3, 0)}
    assert all(c["case"]["quals"] is not None for c in cases.values() if c["case"]["threshold"] == 0)
    assert {c["case"]["quals"] is None for c in cases.values()} == {True, False}
    # a negative threshold with and without qualities: -1 leaves `high` at 0, which only a phred of 20 and more selects
    assert {c["case"]["quals"] is None for c in cases.values() if c["case"]["threshold"] == -1} == {True, False}
    # k-mer lookups by every route have cases that correct (threshold >= 1, rounds >= 1): the table with one- and two-word
    # keys, the prefix table at k > 56 and at k = 13, the plain walk at k < 13 and k < 8
    active = {c["case"]["k"] for c in cases.values() if c["case"]["threshold"] >= 1 and c["case"]["rounds"] >= 1}
    assert active >= {7, 8, 12, 13, 31, 32, 33, 56, 57, 65, 100}


def test_each_case_holds_its_planted_classes(cases):
    for seed, c in cases.items():
        case = c["case"]
        k, reads, planted = case["k"], case["reads"], case["planted"]
        what = "seed %d (k=%d)" % (seed, k)
        assert len(reads) <= 3000, what
        assert (case["quals"] is None) or all(len(q) == len(s) for q, (_, s) in zip(case["quals"], reads)), what
        by = {}
        for p in planted:
            by.setdefault(p["cls"], []).append(p)
        L = lambda p: len(reads[p["i"]][1])
        # single substitutions at every offset of the list from both ends
        assert {p["errs"][0] for p in by["sub_start"]} >= set(mr.correct_offsets(k)), what
        assert {L(p) - 1 - p["errs"][0] for p in by["sub_end"]} >= set(mr.correct_offsets(k)), what
        assert {0, 1, 7, 8, 9, 31, 32, 33, k - 2, k - 1, k} == set(mr.correct_offsets(k))
        assert by["two_subs"] and all(0 < p["errs"][1] - p["errs"][0] < k for p in by["two_subs"]), what
        for cls, want in (("len_k", k), ("len_k1", k + 1), ("len_km1", k - 1), ("len_1", 1)):
            assert by[cls] and all(L(p) == want for p in by[cls]), (what, cls)
        lens = {L(p) for p in by["sh0_length"]}
        assert lens == set(mr.correct_sh0_lengths(k)) and any((l - k) % 32 == 0 for l in lens), what
        assert all(L(p) in (k + 32 * j + d for j in range(1, 8) for d in (-1, 0, 1)) for p in by["sh0_length"]), what
        for cls in ("n_window_tail", "n_window_head", "n_far", "n_alone"):
            assert by[cls] and all(reads[p["i"]][1].count("N") == 1 for p in by[cls]), (what, cls)
        for p in by["n_window_tail"]:  # the N lies in the last 13 bases of some window that holds the substitution
            s, e = reads[p["i"]][1], p["errs"][0]
            n = s.index("N")
            assert any(w <= e < w + k and w + k - 13 <= n < w + k for w in range(max(0, len(s) - k + 1))), what
        for p in by["n_window_head"]:
            s, e = reads[p["i"]][1], p["errs"][0]
            n = s.index("N")
            assert any(w <= e < w + k and w <= n < w + 4 for w in range(max(0, len(s) - k + 1))), what
        for p in by["n_far"]:
            assert abs(reads[p["i"]][1].index("N") - p["errs"][0]) >= k, what
        assert by["all_n"] and all(set(reads[p["i"]][1]) == {"N"} and L(p) > 1 for p in by["all_n"]), what
        assert by["duplicate"] and len({s for _, s in reads}) < len(reads), what
        if case["quals"] is not None:
            for trio in ((19, 19, 19), (20, 20, 20), (21, 21, 21), (19, 20, 21), (21, 19, 21), (19, 21, 19)):
                ps = by["qual_%d_%d_%d" % trio]
                for p in ps:
                    q, e = case["quals"][p["i"]], p["errs"][0]
                    assert tuple(ord(ch) - 33 for ch in q[e - 1:e + 2]) == trio, what
        # the planted substitutions are substitutions: the read differs from the genome piece exactly there is the
        # generator's business; here: the base set carries reads with an N as well
        plain = set(range(len(reads))) - {p["i"] for p in planted}
        assert sum("N" in reads[i][1] for i in plain) >= 5, what


def test_oracle_corrects_leaves_and_refuses_in_every_case(cases):
    """The conditions of the matrix.  An offset of 8 and more inside the first k bases exists from k = 9 on (the generator
    plants that class from k = 10), so the candidate condition is asked of the cases with k >= 10; k = 7 and k = 8 keep the
    first three conditions."""
    for seed, c in cases.items():
        case = c["case"]
        k = case["k"]
        what = "seed %d (k=%d, -x %d -i %d -O %d)" % (seed, k, case["threshold"], case["rounds"], case["offset"])
        valid, changed = c["valid"], c["changed"]
        assert not np.any(changed & ~valid), what  # a read that is not valid comes back as it went in
        lens = np.diff(c["offs"])
        assert not np.any(valid[lens < k]), what
        if case["rounds"] == 0:
            assert not changed.any(), what
        if case["threshold"] <= -2 or (case["threshold"] == -1 and case["quals"] is None):
            assert not valid.any(), what  # a support no count reaches
        if case["threshold"] == -1 and case["quals"] is not None:
            assert valid.any() and (~valid[lens >= k]).any(), what  # `high` is 0, `low` out of reach
        if not (case["threshold"] >= 1 and case["rounds"] >= 1):
            continue
        n_corr, n_same, n_bad = int((valid & changed).sum()), int((valid & ~changed).sum()), int((~valid).sum())
        print(what, "corrected %d, unchanged %d, not valid %d" % (n_corr, n_same, n_bad))
        assert n_corr >= 50 and n_same >= 20 and n_bad >= 20, (what, n_corr, n_same, n_bad)
        fixed = [p for p in case["planted"] if valid[p["i"]] and changed[p["i"]] and p["errs"]]
        if k >= 10:
            deep = [p for p in fixed if len(p["errs"]) == 1 and 8 <= p["errs"][0] < k]
            assert len(deep) >= 10, (what, len(deep))
        if k > 64:
            far = [p for p in fixed if len(p["errs"]) == 1 and 64 <= p["errs"][0] < k]
            assert len(far) >= 5, (what, len(far))


def test_oracle_restores_the_planted_base(cases):
    """A planted read that the oracle corrects and calls valid has its substituted bases changed (the genome's base back, as
    far as the oracle alone can tell: the base differs from the planted one)."""
    for seed, c in cases.items():
        case = c["case"]
        if not (case["threshold"] >= 1 and case["rounds"] >= 1 and case["k"] >= 12):
            continue
        n = 0
        for p in case["planted"]:
            i = p["i"]
            if p["cls"].startswith("sub_") and c["valid"][i] and c["changed"][i]:
                a = int(c["offs"][i])
                e = p["errs"][0]
                assert c["out"][a + e] != c["seqs"][a + e], (seed, p)
                n += 1
        assert n >= 20, (seed, n)
