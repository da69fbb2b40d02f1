"""The cases of tests/spectrum_cases.py are well formed: walks give back the read set, the stretch index names the read through
the .sai table, and the spectrum's bins add up.  CPU only."""
import collections
import re

import pytest

from tests import match_cases as mc
from tests import spectrum_cases as sc
from tests.fixtures import fixture


@pytest.mark.parametrize("name", ("corner", "tiny", "dup"))
def test_rows_below_n_strings_walk_to_whole_reads(name):
    fx = fixture(name)
    seqs = fx.seqs
    for ix, rev in ((fx.fwd, False), (fx.rev, True)):
        sai = ix.sai()
        assert ix.nstrings == len(seqs) == len(sai)
        texts = []
        for row in range(len(seqs)):
            text, stretch = sc.walk(ix, row)
            want = seqs[int(sai[stretch])]
            assert text == (want[::-1] if rev else want), "%s %s row %d" % (name, "rev" if rev else "fwd", row)
            texts.append(text[::-1] if rev else text)
        assert collections.Counter(texts) == collections.Counter(seqs)


def test_lf_table_agrees_with_the_oracle_occ():
    """the walk's LF comes from getchar and pred; Occ as the oracle computes it says the same"""
    fx = fixture("ragged_n")
    codes, lf, dollars = sc.lf_table(fx.fwd)
    pred = fx.fwd.pred()
    n = len(fx.fwd)
    for p in list(range(1, n, 97)) + [n - 1]:
        occ = fx.fwd.occ(p - 1)
        assert int(dollars[p]) == int(occ[0])
        r = int(codes[p])
        if r:
            assert int(lf[p]) == int(pred[r]) + int(occ[r])


def test_ragged_n_rank0_rows_walk_to_the_acgt_pieces():
    fx = fixture("ragged_n")
    pieces = [p for s in fx.seqs for p in re.split("[^ACGT]", s)]
    assert len(fx.seqs) == 203 and len(pieces) == 210
    n0 = int(fx.fwd.pred()[1])
    assert n0 == 210
    assert collections.Counter(sc.walk(fx.fwd, row)[0] for row in range(n0)) == collections.Counter(pieces)
    assert collections.Counter(sc.walk(fx.rev, row)[0][::-1] for row in range(n0)) == collections.Counter(pieces)
    assert sorted(sc.walk(fx.fwd, row)[1] for row in range(n0)) == list(range(n0))


def test_cut_walk_keeps_the_symbols_nearest_the_row():
    fx = fixture("tiny")
    for row in (0, 5, 4000, 20000):
        full, _ = sc.walk(fx.fwd, row)
        got, stretch = sc.walk(fx.fwd, row, max_len=10)
        if len(full) > 10:
            assert got == full[-10:] and stretch is None
        else:
            assert got == full and stretch is not None


@pytest.mark.parametrize("k", (1, 13, 31, 60, 61))
def test_spectrum_adds_up(k):
    fx = fixture("tiny")
    strings = [s for _, s in sc.spectrum_strings(fx.seqs, k, 0)]
    for n_bins in sc.BINS:
        hist, n, L, windows = sc.spectrum(fx.fwd, strings, k, n_bins)
        assert sum(hist) == windows == sum(max(len(s) - k, 0) for s in strings if len(s) >= k)
        assert n == sum(1 for s in strings if len(s) >= k) and L == sum(len(s) for s in strings if len(s) >= k)
    reads = set(fx.seqs) | set(mc.revcomp(s) for s in fx.seqs)
    for s in strings:
        if len(s) >= k and any(c == 0 for cs in sc.window_counts(fx.fwd, [s], k) for c in cs):
            assert s not in reads


def test_spectrum_of_the_read_set():
    """every read once at k = 31: the numbers `siga preqc --all` must print for `tiny`"""
    fx = fixture("tiny")
    hist, n, L, windows = sc.spectrum(fx.fwd, fx.seqs, 31, 1025)
    assert (n, L, windows) == (400, 24000, 11600)
    assert hist[0] == 0 and sum(hist) == windows
