"""The restatement of `--join-mismatches` (tests/join_approx_cases.py) against the one of `--join-overlaps` and against the genomes its
cases are cut from; no GPU."""
from tests import join_approx_cases as ja
from tests import join_cases as jc


def test_without_mismatches_it_is_the_exact_restatement():
    for c in jc.all_cases():
        exp = jc.case_expected(c)
        got = ja.expected_join_approx(c["reads"], c["res"], c["scaf"], dict(c["opts"], max_mismatches=0))
        assert got["status"][:16] == exp["status"] and got["status"][16:] == [0] * 8 and got["mm"] == [0] * len(exp["joins"]), c["name"]
        for key in ("sc_offs", "sc_lay_offs", "sc_flags", "layout", "seqs", "joins"):
            assert got[key] == exp[key], (c["name"], key)


def _planted():
    return [c for k in ja.KS for c in ja.planted(k)] + [ja.long_overlap(31)]


def test_planted_cases_give_the_classes_they_were_built_for():
    kinds = set()
    for c in _planted():
        exp = ja.case_expected(c)
        got = [ja.CLASSES[j[5]] for j in exp["joins"]]
        print(c["name"], got, exp["mm"], exp["status"][16:21])
        for cls, want in zip(got, c["want"]):
            assert want is None or cls == want, c["name"]
        kinds.add(c["kind"])
        if c["kind"] == "tandem_repeat_one_substitution":
            assert exp["joins"][0][6] == 2
        if c["kind"] == "exact_and_approximate":
            assert exp["mm"] == [0] and exp["joins"][0][4] == c["exact_v"] and exp["joins"] == jc.case_expected(c)["joins"]
        if c["kind"] == "j_shorter_than_k":
            assert exp["joins"][0][7] == 0 and exp["mm"] == [1 | ja.APPROX]
        if c["kind"] == "sixteen_columns":
            assert exp["mm"] == [16 | 16 << 8 | ja.APPROX]
        if c["kind"] == "one_in_left":
            assert exp["mm"] == [1 | 1 << 8 | ja.APPROX] and exp["status"][16:19] == [1, 1, 1] and exp["status"][20] == 2
        if c["kind"] == "one_in_right":
            assert exp["mm"] == [1 | ja.APPROX]
    assert {"j_shorter_than_k", "middle_joined_on_both_sides", "minus_strand_only"} <= kinds


def test_joined_planted_cases_read_like_the_genome():
    n = 0
    for c in _planted():
        if not c["genome_out"]:
            continue
        exp = ja.case_expected(c)
        a, b = c["span"]
        assert exp["seqs"] == c["genome"][a:b], c["name"]
        assert all(j[5] == ja.C["JOINED"] for j in exp["joins"]) and all(m & ja.APPROX for m in exp["mm"]), c["name"]
        n += 1
    assert n >= 60


def test_exact_call_joins_none_of_the_planted_cases():
    """what the feature is for: without it every planted gap but the exact-first one stays open"""
    for c in _planted():
        exp = jc.expected_join(c["reads"], c["res"], c["scaf"], {x: y for x, y in c["opts"].items() if x in jc.DEFAULT_OPTS})
        if c["kind"] != "exact_and_approximate":
            assert all(j[5] == jc.C["NONE"] for j in exp["joins"]), c["name"]


def test_random_cases_are_restated_and_mixed():
    seen = set()
    for s in ja.RANDOM_SEEDS:
        exp = ja.case_expected(ja.random_case(s))
        seen |= {(ja.CLASSES[j[5]], bool(m)) for j, m in zip(exp["joins"], exp["mm"])}
    assert {("JOINED", True), ("JOINED", False), ("NONE", False)} <= seen, seen
