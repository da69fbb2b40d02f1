"""The cases of tests/gapfill_cases.py show what they claim, from the serial restatement alone: every class of a gap, both
directions of a fill, fills that are the genome's, the outcomes the named cases were built for -- and the restatement's count()
is the oracle's occurrences on both strands.  No GPU."""
import collections
import random

import pytest

from oracle import pyoracle as po
from tests import gapfill_cases as gc

ISSUE_CLASSES = ("FILLED", "SHORT", "NON_ACGT", "FAR", "NO_ROOM", "DEAD_END", "BRANCH", "TOO_LONG", "OVERLAP", "OFF_ESTIMATE")
FILLED, BRANCH, DEAD_END, TOO_LONG = (gc.C[c] for c in ("FILLED", "BRANCH", "DEAD_END", "TOO_LONG"))


@pytest.fixture(scope="module")
def expected():
    return [(c, gc.case_expected(c)) for c in gc.all_cases()]


def test_every_class_and_both_directions(expected):
    cases_with = collections.Counter()
    directions = collections.Counter()
    for c, exp in expected:
        for cls in {g[5] for g in exp["gaps"]}:
            cases_with[gc.CLASSES[cls]] += 1
        for d in {g[8] for g in exp["gaps"] if g[5] == FILLED}:
            directions[d] += 1
    print(dict(cases_with), dict(directions))
    assert all(cases_with[c] >= 5 for c in ISSUE_CLASSES), cases_with
    assert directions[0] >= 20 and directions[1] >= 20, directions


def test_every_fill_is_the_genomes(expected):
    fills = 0
    for c, exp in expected:
        assert len(exp["gaps"]) == len(c["truth"]) and exp["status"][0] == len(c["truth"])
        for i, g in enumerate(exp["gaps"]):
            if g[5] == FILLED:
                assert exp["fills"][i] == c["truth"][i] and g[4] == len(c["truth"][i]), (c["name"], i)
                fills += 1
        if exp["seqs"] is not None:  # and the bases are the genome's wherever no N was left
            total = 0
            for s in range(exp["status"][22]):
                b = exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]]
                total += len(b)
                assert b.count(b"N") <= exp["status"][15] + c["res"]["useqs"].count(b"N")
            assert total == exp["status"][16] == len(exp["seqs"])
    assert fills > 1000


@pytest.mark.parametrize("k", gc.KS)
def test_named_cases_show_what_they_were_built_for(k):
    by = {c["kind"]: gc.case_expected(c)["gaps"] for c in gc.hand_built(k)}
    one = lambda kind: by[kind][0]
    for kind in ("plain", "right_reversed", "left_reversed", "both_reversed", "minus_strand_only", "fork_below_min_count", "far_not",
                 "g_at_fill_minus_slack", "g_at_fill_plus_slack"):
        assert one(kind)[5:9] == (FILLED, FILLED, gc.NOT_RUN, 0), kind
    assert [g[4] for g in by["three_gaps"]] == [25, 11, 44] and [g[0] for g in by["circular_and_single"]] == [1]
    for fill, kind in ((0, "fill_0"), (1, "fill_1"), (k - 1, "fill_k_minus_1"), (k, "fill_k"), (k + 1, "fill_k_plus_1")):
        assert one(kind)[4:6] == (fill, FILLED), kind
    assert one("g_at_fill_minus_slack_minus_1")[5:8] == (TOO_LONG, TOO_LONG, TOO_LONG)
    assert one("g_at_fill_plus_slack_plus_1")[5] == gc.C["OFF_ESTIMATE"]
    assert one("overlap_1")[5] == one("overlap_k_minus_1")[5] == gc.C["OVERLAP"]
    assert [g[5] for g in by["unitig_of_k"]] == [FILLED, FILLED] and [g[5] for g in by["unitig_of_k_minus_1"]] == [gc.C["SHORT"]] * 2
    assert one("far")[5] == gc.C["FAR"] and one("n_in_anchor")[5] == one("lower_case_in_anchor")[5] == gc.C["NON_ACGT"]
    assert one("n_in_reads")[5:8] == (DEAD_END, DEAD_END, DEAD_END) and one("coverage_hole")[5:8] == (DEAD_END, DEAD_END, DEAD_END)
    for kind in ("fork_at_min_count", "fork_at_min_count_left_reversed", "fork_at_min_count_both_reversed"):
        assert one(kind)[5:9] == (FILLED, BRANCH, FILLED, 1), kind
    assert one("forks_at_both_ends")[5:8] == (BRANCH, BRANCH, BRANCH)
    if k % 2 == 0:
        assert one("palindrome_doubled_crosses")[5:9] == (FILLED, BRANCH, FILLED, 1)
        assert one("palindrome_doubled_below")[5:9] == (FILLED, FILLED, gc.NOT_RUN, 0)
    assert [g[5] for g in by["scratch_one_byte_short"]] == [FILLED, FILLED, gc.C["NO_ROOM"]]
    assert [g[5] for g in by["scratch_exact"]] == [FILLED] * 3


def test_many_gaps_cross_a_wave_and_a_workgroup():
    for count in (70, 300):
        exp = gc.case_expected(gc.many_gaps(count))
        assert exp["status"][0] == count + 1 and exp["status"][22] == 2


def test_count_is_the_oracles_occurrences_on_both_strands():
    rng = random.Random(5)
    for k in (15, 32, 128):
        case = next(c for c in gc.hand_built(k) if c["kind"] == ("palindrome_doubled_crosses" if k % 2 == 0 else "fork_at_min_count"))
        reads, g = case["reads"], case["genome"]
        idx = po.Index.build([r.decode() for r in reads])
        sample = [g[p:p + k] for p in rng.sample(range(len(g) - k), 40)] + [bytes(rng.choice(b"ACGT") for _ in range(k)) for _ in range(5)]
        sample += [r[p:p + k] for r in reads[-3:] for p in range(len(r) - k + 1)]  # the odd reads' windows, the palindrome among them
        pal = 0
        for w in sample:
            assert gc.kmer_count(reads, k, w) == idx.occurrences(w) + idx.occurrences(gc.revcomp(w)), (k, w)
            pal += w == gc.revcomp(w)
        assert pal or k % 2


@pytest.mark.parametrize("k", [31, 128])
def test_long_fill(k):
    c = gc.long_fill(k)
    exp = gc.case_expected(c)
    assert c["opts"]["max_fill"] == 10000 and c["opts"]["slack"] == 100
    assert [g[3:9] for g in exp["gaps"]] == [(4950, 5000, FILLED, FILLED, gc.NOT_RUN, 0), (4950, 5000, FILLED, BRANCH, FILLED, 1)]
    assert [exp["fills"][i] for i in (0, 1)] == c["truth"] and all(len(t) == 5000 for t in c["truth"])
    assert c["scaf"]["layout"][1][1] & gc.REV  # the piece between the two fills lies reversed
