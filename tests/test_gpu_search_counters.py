"""The backward-search kernels (csrc/sigax_match.hip, sigax_spectrum.hip, sigax_locate.hip) against the record of themselves in
tests/golden/search_counters.json: the cases of tools/record_search_counters.py, in every form of the index, give the same
results AND the same status words -- chains run, symbols consumed, rank-table sectors asked for, walks cut -- word for word.
The other GPU tests compare results with the oracle or with brute force and only bound the work counters; a change to the
shared search step can keep every count right and still do other work for it.  The file was recorded with the library as it was
before the step, the constants, the table lookup and the chain reservation moved into csrc/sigax_rank.h."""
import json

import pytest

from tools import record_search_counters as rsc

pytestmark = pytest.mark.gpu
RECORD = json.load(open(rsc.GOLDEN))


def test_the_record_is_of_these_cases():
    assert RECORD["input"] == rsc.describe_input()
    assert sorted(RECORD["forms"]) == sorted(rsc.FORMS)


@pytest.mark.parametrize("form", sorted(rsc.FORMS))
def test_results_and_counters_equal_the_record(form):
    got, want = rsc.run_form(form), RECORD["forms"][form]
    assert sorted(got) == sorted(want)
    for case in want:
        print(form, case, got[case])
        assert got[case] == want[case], "%s, %s" % (form, case)
    # the record covers what it is meant to: queries over max_hits, cut walks on both strands and in locate, symbols and sectors counted
    assert want["locate rc=1 max_hits=5 max_len=10"]["over"] > 0 and want["locate rc=1 max_hits=5 max_len=10"]["cut"] > 0
    assert all(want["walk strand=%d max_len=10" % s]["status2"][1] > 0 for s in (0, 1))
    assert all(want[c]["stat3"][1] > 0 and want[c]["stat3"][2] > 0 for c in want if c.startswith("match"))
