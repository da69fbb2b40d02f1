"""The two restatements behind `siga unitig --pairs` against each other, without a GPU (tests/pair_cases.py): the serial rules
over the serial unitigs give the samples the reference's walk collects, on every graph where the reference's chains are the
unitigs; where reads differ in length and the walk flips strand they differ as documented; and the estimate's arithmetic."""
import ctypes as C
import math
from collections import Counter

import pytest

from tests import pair_cases as pp
from tests import unitig_cases as uc

CASES = pp.hand_built()
# at most this share of the seeded random graphs may be turned away by comparable(): the generator gives one in five a record
# twice and one in ten a containment (some 28 % together), far below the cap
MAX_FILTERED = 0.5
N_RANDOM = 300


def _samples(case):
    reads = case["reads"]
    exp = uc.expected(reads, case["edges"], case["m"])
    got = pp.expected_pairs(exp, [len(r) for r in reads], case["mate"])
    return got, pp.reference_insert_size(reads, case["edges"], case["m"], case["mate"])


@pytest.mark.parametrize("case", [c for c in CASES if pp.comparable(c)], ids=lambda c: c["name"])
def test_hand_built_samples_equal_the_reference_walk(case):
    got, ref = _samples(case)
    assert Counter(got["samples"]) == Counter(ref), case["name"]
    assert got["status"][10] == len(ref) and got["status"][11] == sum(ref)
    assert got["status"][12] + (got["status"][13] << 64) == sum(d * d for d in ref)


def test_hand_built_cases_cover_the_classes():
    names = {c["name"] for c in CASES if pp.comparable(c)}
    assert {"chain_forward", "chain_mixed", "chain_reversed", "two_chains", "branch", "singles"} <= names
    assert not {"ring", "containment", "unequal_flip"} & names
    total = [0] * 24
    for c in CASES:
        got, _ = _samples(c)
        total = [a + b for a, b in zip(total, got["status"])]
    # every class occurs somewhere: malformed, same in its three orientations, ring, across, a dropped ring link, links
    assert all(total[k] > 0 for k in (0, 1, 2, 4, 5, 6, 7, 8, 10, 14, 18, 19, 21, 22)), total


def test_random_graphs_samples_equal_the_reference_walk():
    kept = sampled = 0
    for seed in range(N_RANDOM):
        case = pp.random_uniform_case(seed)
        if not pp.comparable(case):
            continue
        kept += 1
        got, ref = _samples(case)
        assert Counter(got["samples"]) == Counter(ref), case["name"]
        sampled += len(ref)
    print("kept", kept, "of", N_RANDOM, "samples", sampled)
    assert kept >= N_RANDOM * (1 - MAX_FILTERED)
    assert sampled > 0


def test_unequal_lengths_and_a_strand_flip_differ_as_documented():
    """lengths 40, 70, 50, 90 stored + - + -, overlaps o0 o1 o2.  Left ends: 0, 40 - o0, 110 - o0 - o1, 160 - o0 - o1 - o2.
    The reference starts at read 0 walking forward and adds the overhang of the read it leaves (40 - o0), then flips and adds
    the overhang of the read it enters: 50 - o1 instead of 70 - o1, then flips back and adds that of the one it leaves."""
    case = pp.case_named("unequal_flip")
    assert not pp.comparable(case)
    got, ref = _samples(case)
    ov = {}
    for q, t, ln, _ in case["edges"]:
        ov[frozenset((q, t))] = ln
    o0, o1, o2 = (ov[frozenset((k, k + 1))] for k in range(3))
    left = [0, 40 - o0, 110 - o0 - o1, 160 - o0 - o1 - o2]
    assert sorted(got["samples"]) == sorted([left[3] - left[0], left[2] - left[1]])
    walk = [0, 40 - o0, 40 - o0 + 50 - o1, 40 - o0 + 50 - o1 + 50 - o2]
    assert sorted(ref) == sorted([walk[3] - walk[0], walk[2] - walk[1]])
    assert sorted(ref) != sorted(got["samples"])


def test_estimate_by_hand():
    st = [0] * 24
    st[10:14] = [4, 10 + 20 + 30 + 41, 100 + 400 + 900 + 1681, 0]  # mean 25.25, second moment 770.25, variance 132.6875
    st[14:18] = [2, 300, 50000, 0]  # 100 and 200: mean 150, sd 50
    assert pp.estimate(st) == (25, 11, 150.0, 50.0)
    assert pp.estimate([0] * 24) == (0, 0, 0.0, 0.0)
    big = [0] * 24
    d = (1 << 32) - 200
    big[10:14] = [2, 2 * d, (2 * d * d) & pp.M64, (2 * d * d) >> 64]  # the squares carry into the high word; no spread
    assert big[13] == 1 and pp.estimate(big)[:2] == (d, 0)
    one = [0] * 24
    one[10:14] = [3, 7, 17, 0]  # 1, 2, 4... mean 2.33 truncated to 2; variance 17/3 - 49/9 = 0.22 -> 0
    assert pp.estimate(one)[:2] == (2, 0)


def test_library_estimate_equals_the_formula():
    """sigax_pairs_estimate is host arithmetic: it runs without a device"""
    import siga_amd
    for st in ([0] * 24, [0] * 10 + [4, 101, 3081, 0, 2, 300, 50000, 0] + [0] * 6,
               [0] * 10 + [2, 2 * ((1 << 32) - 200), (2 * ((1 << 32) - 200) ** 2) & pp.M64, 1, 5, 12345, 99999999, 0] + [0] * 6):
        got = siga_amd.pairs_estimate(st)
        want = pp.estimate(st)
        assert got[:2] == want[:2] and math.isclose(got[2], want[2], rel_tol=0, abs_tol=0) and got[3] == want[3], (got, want)
    from siga_amd import _lib
    assert _lib.lib().sigax_pairs_estimate(None, None, None, None, None) == _lib.SIGAX_E_ARG


def test_mates_by_name():
    import siga_amd
    from siga_amd import _lib
    N = _lib.SIGAX_NO_MATE
    names = ["a/1", "a/2", "b/1", "c/2", "c/1", "dA", "dB", "ef", "er", "x", "g/1", "g/1", "g/2", "h/3"]
    assert siga_amd.mates_by_name(names).tolist() == [1, 0, N, 4, 3, 6, 5, 8, 7, N, N, N, N, N]
    assert siga_amd.mates_by_name([]).tolist() == []
