"""The cases of tests/join_cases.py against themselves, without a GPU: what the restatement of `siga unitig --scaffold
--join-overlaps` gives on the hand-built and the random cases is what the cases were built to show."""
import collections

import pytest

from tests import gapfill_cases as gc
from tests import join_cases as jc


def _classes(cases):
    seen = collections.Counter()
    for c in cases:
        for j in jc.case_expected(c)["joins"]:
            seen[jc.CLASSES[j[5]]] += 1
    return seen


@pytest.mark.parametrize("k", jc.KS)
def test_hand_built_cases_show_what_they_are_named_for(k):
    by = {c["kind"]: jc.case_expected(c) for c in jc.hand_built(k)}
    cls = lambda kind, g=0: jc.CLASSES[by[kind]["joins"][g][5]]
    for v in sorted({16, 31, 32, 33, 63, 64, 65, k - 2, k - 1, k}):
        j = by["v_%d" % v]["joins"][0]
        assert (jc.CLASSES[j[5]], j[4], j[6], j[7]) == ("JOINED", v, 1, max(0, k - v - 1)), (k, v, j)
    assert cls("v_at_lo") == "JOINED" and cls("v_below_lo") == "NONE" and cls("v_at_hi") == "JOINED" and cls("v_above_hi") == "NONE"
    assert by["range_over_64"]["status"][12] > 64 and by["range_over_64"]["joins"][0][4] == 90
    assert by["range_over_128"]["status"][12] > 128 and by["range_over_128"]["joins"][0][4] == 150
    assert by["range_over_128_at_the_top"]["joins"][0][4:6] == (219, jc.C["JOINED"])
    assert by["hi_by_left"]["joins"][0][4] == 29 and by["hi_by_right"]["joins"][0][4] == 29 and cls("left_within_right") == "NONE"
    assert by["hi_by_left"]["status"][12] == 29 - 16 + 1 and by["v_at_hi"]["status"][12] == 40 - 16 + 1
    assert [cls("piece_of_min_overlap", g) for g in (0, 1)] == ["SHORT", "SHORT"]
    assert [cls("piece_of_min_overlap_plus_1", g) for g in (0, 1)] == ["JOINED", "JOINED"]
    for kind in ("forward_reverse", "reverse_forward", "reverse_reverse", "g_1", "g_at_slack", "minus_strand_only", "windows_at_min_count",
                 "hole_behind_the_junction_windows"):
        assert cls(kind) == "JOINED", (k, kind)
    assert all(j[5] == jc.C["JOINED"] for j in by["residues"]["joins"]) and len(by["residues"]["joins"]) == 16
    assert cls("g_above_slack") == "FAR" and cls("filled_by_gapfill") == "CLOSED" and cls("one_base_in_the_gap") == "CLOSED" and cls("g_0") == "CLOSED"
    assert cls("no_overlap") == "NONE"
    for nm in ("n", "lower_case"):
        assert cls(nm + "_inside_overlap_first") == "NONE" and cls(nm + "_inside_overlap_last") == "NONE"
        # v = 22: windows across the junction there are for k > 23, and each holds the byte on either side of the overlap
        want = "UNSUPPORTED" if k > 23 else "JOINED"
        assert cls(nm + "_before_overlap") == want and cls(nm + "_behind_overlap") == want
    for kind in ("tandem_repeat", "homopolymer"):
        c = next(x for x in jc.hand_built(k) if x["kind"] == kind)
        assert cls(kind) == "AMBIGUOUS" and by[kind]["joins"][0][6] == c["matches"] and by[kind]["joins"][0][4] == 0
    assert (cls("one_window_in_a_hole"), by["one_window_in_a_hole"]["joins"][0][7]) == ("UNSUPPORTED", 1)
    assert (cls("four_windows_in_a_hole"), by["four_windows_in_a_hole"]["joins"][0][7]) == ("UNSUPPORTED", 4)
    assert (cls("windows_below_min_count"), by["windows_below_min_count"]["joins"][0][7]) == ("UNSUPPORTED", 2)
    three = by["three_joins_in_a_row"]
    assert [j[5] for j in three["joins"]] == [jc.C["JOINED"]] * 3 and three["joins"][0][4] + three["joins"][1][4] > 40
    ring = by["ring_and_single"]
    assert ring["status"][0] == 1 and ring["status"][15] == 3 and ring["sc_flags"][1] == 1 | (17 << 1)
    assert [jc.CLASSES[j[5]] for j in by["bad_placement"]["joins"]] == ["MALFORMED", "MALFORMED"]
    seen = _classes(jc.hand_built(k))
    assert all(seen[c] for c in jc.CLASSES), (k, seen)


def test_joined_scaffolds_of_clean_cases_are_the_genome():
    n = 0
    for c in jc.all_cases():
        exp = jc.case_expected(c)
        per = collections.defaultdict(list)
        for j in exp["joins"]:
            per[j[0]].append(j[5])
        for s, classes in per.items():
            if all(x == jc.C["JOINED"] for x in classes) and (c["clean"] or c["kind"].startswith("random")):
                seq = exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]]
                if c["clean"] or (b"N" not in seq and seq.isupper()):
                    assert seq in c["genome"], (c["name"], s)
                    n += 1
    assert n > 100


def test_random_cases_reach_every_class_but_malformed():
    seen = _classes([jc.random_case(s) for s in range(100)])
    print(seen)
    assert all(seen[c] for c in jc.CLASSES if c != "MALFORMED"), seen
    assert seen["MALFORMED"] == 0


def test_many_gaps():
    for count in (70, 300):
        exp = jc.case_expected(jc.many_gaps(count))
        assert exp["status"][0] == count + 1 and exp["status"][1] > count // 2


def test_a_second_join_changes_nothing():
    for c in jc.all_cases():
        exp = jc.case_expected(c)
        again = jc.case_expected(jc.joined_again(c, exp))
        for key in ("sc_offs", "sc_lay_offs", "sc_flags", "layout", "seqs"):
            assert again[key] == exp[key], (c["name"], key)
        assert again["status"][1] == 0 and again["status"][9] == again["status"][10] == 0, c["name"]
        assert again["status"][1 + jc.C["FAR"]] == exp["status"][1 + jc.C["FAR"]] + exp["status"][1], c["name"]


def test_matches_and_windows_against_a_brute_force_count():
    """|M| by comparing byte by byte, the windows by enumerating every k-mer of the joined sequence and keeping those that are
    in neither neighbour's own span"""
    checked = 0
    for c in jc.all_cases():
        exp = jc.case_expected(c)
        o, scaf, so = c["opts"], c["scaf"], c["res"]["seq_offs"]
        lay, seqs = scaf["layout"], scaf["seqs"]
        pos = {}
        for s in range(len(scaf["sc_lay_offs"]) - 1):
            for p in range(scaf["sc_lay_offs"][s], scaf["sc_lay_offs"][s + 1]):
                pos[(s, lay[p][0])] = (scaf["sc_offs"][s] + lay[p][2], p)
        for j in exp["joins"]:
            if jc.CLASSES[j[5]] not in ("JOINED", "UNSUPPORTED", "NONE", "AMBIGUOUS"):
                continue
            (al, _), (ar, _) = pos[(j[0], j[1])], pos[(j[0], j[2])]
            L, R = seqs[al:al + so[j[1] + 1] - so[j[1]]], seqs[ar:ar + so[j[2] + 1] - so[j[2]]]
            hi = min(o["max_overlap"], len(L) - 1, len(R) - 1)
            m = 0
            for v in range(o["min_overlap"], hi + 1):
                m += all(L[len(L) - v + i] == R[i] and R[i] in b"ACGT" for i in range(v))
            assert min(m, 255) == j[6], (c["name"], j)
            if j[4]:
                v, k = j[4], o["k"]
                J = L + R[v:]
                w = sum(1 for s in range(len(J) - k + 1) if not (s + k <= len(L)) and not (s >= len(L) - v))
                assert w == j[7], (c["name"], j, w)
                if jc.CLASSES[j[5]] == "JOINED":
                    assert all(gc.kmer_count(c["reads"], k, J[s:s + k]) >= o["min_count"] for s in range(len(J) - k + 1)
                               if not (s + k <= len(L)) and not (s >= len(L) - v))
            checked += 1
    assert checked > 300
