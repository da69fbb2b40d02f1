"""The cases of tests/match_cases.py are what they claim (CPU, oracle only), and the command line knows `match`."""
import subprocess

import pytest

from siga_amd import host
from tests import match_cases as mc
from tests.golden import make_reads as mr


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_case_has_every_class(seed):
    case = mc.match_case(seed)
    classes = [c for _, _, c in case["queries"]]
    for c in mc.CLASSES:
        assert classes.count(c) >= 1, c
    for cls in ("non_acgt_first", "non_acgt_last", "non_acgt_inner"):
        got = set()
        for _, s, c in case["queries"]:
            if c == cls:
                got |= set(s) - set("ACGT")
        assert got == set(mr.NON_ACGT_BYTES), cls
    lens = {len(s) for _, s, c in case["queries"] if c == "length"}
    assert lens == set(mc.lengths_for(case["L"]))
    assert max(len(s) for _, s, c in case["queries"] if c == "long") >= 20000
    reads = {s for _, s in case["reads"]}
    assert all(s in reads for _, s, c in case["queries"] if c == "verbatim")
    assert all(mc.revcomp(s) in reads for _, s, c in case["queries"] if c == "revcomp")
    assert all(s not in reads and any(s in r for r in reads) for _, s, c in case["queries"] if c == "substring")


def test_seeds_cover_the_parameters():
    got = {mc.params(s) for s in mc.SEEDS}
    assert got == {(L, rc) for L in (None, 0, 1, 13, 40, mc.READ_LEN) for rc in (True, False)}


@pytest.mark.parametrize("seed", (1, 8))
def test_substitutions_die_at_many_depths(seed):
    case, fwd = mc.match_case(seed), mc.oracle_index(seed)
    depths = {mc.stop_depth(fwd, s) for _, s, c in case["queries"] if c == "subst"}
    assert len(depths) >= 20
    assert any(d % 2 for d in depths) and any(d % 2 == 0 for d in depths)
    # stop_depth is the reference's loop: one step further the suffix has no occurrence, one step before it has
    for _, s, c in case["queries"]:
        if c == "subst":
            d = mc.stop_depth(fwd, s)
            assert d == len(s) or fwd.occurrences(s[len(s) - d:]) == 0
            assert fwd.occurrences(s[len(s) - d + 1:]) > 0


@pytest.mark.parametrize("seed", (1, 2, 9))
def test_palindrome_counts_twice(seed):
    case, fwd = mc.match_case(seed), mc.oracle_index(seed)
    pals = [s for _, s, c in case["queries"] if c == "palindrome"]
    assert all(mc.revcomp(s) == s for s in pals)
    for s in pals:
        n = mc.count(fwd, s, True)
        assert n % 2 == 0 and n >= 2
    head, tail, text = mc.expected(fwd, case["queries"], case["L"], case["rc"])
    assert len(head) == len(case["queries"]) and text.count("\n") == len(head) + sum(t is not None for t in tail)


def test_half_substituted_set_stops_early():
    """the oracle's own bound: with every second query substituted the reference's loop consumes less than 3/4 of the symbols"""
    fwd = mc.oracle_index(1)
    pats = mc.patterns(mc.half_substituted(1), None, True)
    assert sum(mc.stop_depth(fwd, w) for w in pats) < 0.75 * sum(len(w) for w in pats)


def test_usage_lists_match():
    r = subprocess.run([host.CLI_PATH], capture_output=True, text=True)
    assert r.returncode == 0  # usage returns 256: exit status 0 (src/main.cpp)
    assert "match" in r.stdout and "|match]" in r.stdout.splitlines()[0]


def test_match_help():
    r = subprocess.run([host.CLI_PATH, "match"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--max-length" in r.stdout and "--no-opposite-strand" in r.stdout and "--prefix" in r.stdout
