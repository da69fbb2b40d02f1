"""The read sets of tests/test_gpu_non_acgt.py (tests/golden/make_reads.py: non_acgt_case) hold what they are meant to:
every non-ACGT byte, at every offset class from both read ends, runs, pieces of the table-edge lengths, degenerate reads.
And the oracle gives block lists for all of them, the same ones whichever non-ACGT byte stands where.  CPU only."""
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.golden import make_reads as mr

_NON = re.compile("[^ACGT]+")


def census(reads):
    """what a read set holds, measured on the reads themselves"""
    c = {"bytes": set(), "from_start": set(), "from_end": set(), "runs": set(), "pieces": set(), "with": 0, "plain": 0,
         "all_non": False, "lengths": set(), "window_multi": False, "dups": len({s for _, s in reads}) < len(reads)}
    for _, s in reads:
        L = len(s)
        c["lengths"].add(L)
        idx = [i for i, ch in enumerate(s) if ch not in "ACGT"]
        if not idx:
            c["plain"] += 1
            continue
        c["with"] += 1
        c["all_non"] |= len(idx) == L
        for i in idx:
            c["bytes"].add(s[i])
            c["from_start"].add(i)
            c["from_end"].add(L - 1 - i)
        c["window_multi"] |= sum(i < 12 for i in idx) >= 2 or sum(i >= L - 12 for i in idx) >= 2
        for mt in _NON.finditer(s):
            c["runs"].add(mt.end() - mt.start())
        for a, b in zip(idx, idx[1:]):
            if b - a > 1:
                c["pieces"].add(b - a - 1)
    return c


@pytest.fixture(scope="module")
def cases():
    return {seed: mr.non_acgt_case(seed) for seed in mr.NON_ACGT_SEEDS}


def test_each_case_covers_its_classes(cases):
    for seed, case in cases.items():
        m = case["m"]
        c = census(case["reads"])
        what = "seed %d (m=%d)" % (seed, m)
        assert c["bytes"] == set(mr.NON_ACGT_BYTES), what
        assert all(ord(b) < 0x80 for b in c["bytes"])
        for o in mr.non_acgt_offsets(m):
            assert o in c["from_start"] and o in c["from_end"], (what, o)
        for side in ("from_start", "from_end"):
            assert {o & 1 for o in c[side] if 0 < o < 40} == {0, 1}, (what, side)
        assert set(mr.non_acgt_pieces(m)) <= c["pieces"], what
        assert set(mr.non_acgt_runs(seed)) <= c["runs"], what
        assert c["all_non"] and c["window_multi"] and c["dups"], what
        assert 1 in c["lengths"] and min(L for L in c["lengths"] if L > 1) < 12, what
        assert m - 1 in c["lengths"], what
        assert c["plain"] > 0 and c["with"] > 0, what
        frac = c["with"] / (c["with"] + c["plain"])
        assert (frac > 0.95) if case["dense"] else (frac < 0.4), (what, frac)
        assert len(case["reads"]) <= 4000


def test_cases_cover_the_parameters(cases):
    assert {c["m"] for c in cases.values()} == set(mr.NON_ACGT_MS)
    assert {c["irreducible"] for c in cases.values()} == {True, False}
    assert {c["rc"] for c in cases.values()} == {True, False}
    assert any(c["dense"] for c in cases.values()) and not all(c["dense"] for c in cases.values())
    runs = set()
    longest = set()
    for seed, c in cases.items():
        runs |= census(c["reads"])["runs"]
        longest.add(max(len(s) for _, s in c["reads"]))
    assert set(range(2, 31)) <= runs
    assert {250, 700} <= longest and min(longest) <= 150
    # sparse cases: besides the planted reads, about one read in 30 of the base set carries an N
    sparse = [c for c in cases.values() if not c["dense"]]
    assert all(0.02 < census(c["reads"])["with"] / len(c["reads"]) for c in sparse)


def _normalised(seqs):
    return [_NON.sub(lambda mt: "N" * len(mt.group()), s) for s in seqs]


@pytest.mark.parametrize("seed", mr.NON_ACGT_SEEDS)
def test_oracle_blocks_for_every_case(cases, seed, tmp_path):
    """The oracle indexes every case and returns block lists for every read; lowercase, IUPAC codes and '.' give the
    same index and the same blocks as N in their place (all rank as '$').  `siga index` on the host writes the oracle
    builder's files."""
    from siga_amd import host
    case = cases[seed]
    seqs = [s for _, s in case["reads"]]
    m, irr, rc = case["m"], case["irreducible"], case["rc"]
    fwd, rev = po.Index.build(seqs), po.Index.build(seqs, reverse=True)
    fa, got_p, want_p = str(tmp_path / "r.fa"), str(tmp_path / "r"), str(tmp_path / "o")
    with open(fa, "w") as f:
        f.write(mr.fasta_text(case["reads"]))
    host.index_file(fa, got_p, threads=2)
    fwd.save(want_p + ".bwt", want_p + ".sai")
    rev.save(want_p + ".rbwt", want_p + ".rsai")
    for ext in (".bwt", ".rbwt", ".sai", ".rsai"):
        assert open(got_p + ext, "rb").read() == open(want_p + ext, "rb").read(), ext
    got = po.overlap_batch(fwd, rev, seqs, m, irr, rc)
    assert len(got["block_offs"]) == len(seqs) + 1
    assert int(got["block_offs"][-1]) == len(got["blocks"]) > 0
    with_n = [k for k, s in enumerate(seqs) if any(ch not in "ACGT" for ch in s)]
    assert any(got["block_offs"][k + 1] > got["block_offs"][k] for k in with_n)  # reads with N find overlaps too
    norm = _normalised(seqs)
    nf, nr = po.Index.build(norm), po.Index.build(norm, reverse=True)
    assert len(nf) == len(fwd) and np.array_equal(nf.runs(), fwd.runs()) and np.array_equal(nr.runs(), rev.runs())
    want = po.overlap_batch(nf, nr, norm, m, irr, rc)
    assert np.array_equal(got["block_offs"], want["block_offs"])
    assert np.array_equal(got["blocks"], want["blocks"])
    assert np.array_equal(got["substring"], want["substring"])
    assert got["n_occ_min"] == want["n_occ_min"]
    dup = po.overlap_batch(fwd, rev, seqs, 0, duplicate=True)
    assert np.array_equal(dup["blocks"], po.overlap_batch(nf, nr, norm, 0, duplicate=True)["blocks"])
