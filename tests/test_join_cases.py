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


def test_long_overlaps_show_what_they_are_named_for():
    cases = jc.long_overlaps(31)
    by = {c["kind"]: (c, jc.case_expected(c)) for c in cases}
    for c, exp in by.values():
        (j,) = exp["joins"]
        if c["v"] is not None:
            assert (jc.CLASSES[j[5]], j[4], j[6], j[7]) == ("JOINED", c["v"], 1, 0), (c["name"], j)
    hi = lambda kind: by[kind][1]["status"][12] + by[kind][0]["opts"]["min_overlap"] - 1
    assert hi("hi_4096_by_both_lengths") == hi("hi_by_max_overlap") == hi("last_word_partly_filled") == 4096
    assert hi("hi_66_words") == 2112 and (2112 + 31) // 32 == 66
    for kind in ("v_just_above_hi", "n_far_in_the_tail", "lower_case_far_in_the_head"):
        assert (jc.CLASSES[by[kind][1]["joins"][0][5]], hi(kind)) == ("NONE", 4096), kind
    # without the odd byte, in both copies of the overlap, the two patched cases are the first one; with it the two ends still
    # agree byte for byte at v = 4096 -- and a packing that gives the odd byte T's code sees T there in both -- so that nothing
    # but the run of ACGT makes the class NONE
    first = by["hi_4096_by_both_lengths"][0]["scaf"]["seqs"]
    for kind, i, what in (("n_far_in_the_tail", 4096 - 3000, b"N"), ("lower_case_far_in_the_head", 3000, None)):
        s = by[kind][0]["scaf"]["seqs"]
        L, R = s[:4097], s[4102:4102 + 4097]
        odd = what or first[4102 + i:4103 + i].lower()
        assert L[1 + i:2 + i] == R[i:i + 1] == odd and not jc.ACGT.issuperset(odd)
        assert L[1:] == R[:4096] and L[1:].replace(odd, b"T") == R[:4096].replace(odd, b"T")
        assert s[:1 + i] + first[1 + i:2 + i] + s[2 + i:4102 + i] + first[4102 + i:4103 + i] + s[4103 + i:] == first
        assert jc.matches_of(L.replace(odd, b"T"), R.replace(odd, b"T"), 16, 4096) == [4096]
    # the saturation: more than 255 lengths match, the record says 255
    for kind, want in (("matches_saturate", list(range(16, 601))), ("long_tandem_repeat", list(range(18, 601, 3)))):
        c, exp = by[kind]
        sc, so, lay = c["scaf"], c["res"]["seq_offs"], c["scaf"]["layout"]
        L, R = (sc["seqs"][p[2]:p[2] + so[p[0] + 1] - so[p[0]]] for p in lay)
        assert jc.matches_of(L, R, 16, min(4096, len(L) - 1, len(R) - 1)) == want
        assert exp["joins"][0][5:7] == (jc.C["AMBIGUOUS"], min(len(want), 255)) and exp["joins"][0][6] == c["matches"]
    assert by["matches_saturate"][1]["joins"][0][6] == 255


def test_many_gaps_options_leave_the_pieces_alone():
    a, b = jc.many_gaps(300), jc.many_gaps(300, 15, step=30, depth=1, min_count=1, hole_under=200)
    assert a["res"] == b["res"] and a["scaf"] == b["scaf"] and a["genome"] == b["genome"]
    assert a["opts"]["min_count"] == 3 and b["opts"]["min_count"] == 1 and len(b["reads"]) < len(a["reads"]) // 10


def test_more_open_gaps_than_the_match_grid():
    """16 workgroups a compute unit, 256 compute units on an MI355X (tests/test_gpu_join.py takes the device's own count)"""
    n_cu = 256
    c, exp, hole = jc.beyond_the_grid(n_cu)
    opened = jc.came_to_the_match(exp)
    print(exp["status"], len(opened), hole)
    assert exp["status"][0] == 16 * n_cu + 301 and len(opened) > 16 * n_cu
    assert exp["status"][13] > 0 and sum(1 for i in opened[16 * n_cu:] if exp["joins"][i][7]) > 0  # windows beyond the grid, too
    assert exp["joins"][hole][5] == jc.C["UNSUPPORTED"] and opened.index(hole) >= 16 * n_cu
