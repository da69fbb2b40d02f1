"""Reads with non-ACGT bytes (N, lowercase, IUPAC codes, '.': all rank as '$', alphabet.h:19-39) through the GPU index
builder, the block finder and the extractor in both index states, rmdup's duplicate blocks, Occ and the CLI -- against the
oracle.  The cases (tests/golden/make_reads.py: non_acgt_case) put such bytes where the finder's start tables, its double
step and the extractor's row tables and text windows change form; tests/test_non_acgt_cases.py checks that they do.
tests/test_gpu_wide.py runs test_non_acgt_case under the other kernel forms."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.bigcheck import blocks_matrix
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu

EXTS = (".bwt", ".rbwt", ".sai", ".rsai")


def _write_case(case, d):
    fa = os.path.join(d, "r.fa")
    with open(fa, "w") as f:
        f.write(mr.fasta_text(case["reads"]))
    return fa, os.path.join(d, "r")


def _run_batch(pair, seqs, m, flags):
    from tests.test_gpu_parity import _run_batch as run
    from siga_amd import _lib
    return run(None, _lib.lib(), pair, seqs, m, flags)


def _expected_deep_k(m):
    """what sigax_index_prepare_overlap builds for min-overlap m (sigax_tables.cpp: deep_k_for)"""
    if os.environ.get("SIGAX_FIND_DEEP") == "0":
        return 0
    env = os.environ.get("SIGAX_DEEP_K")
    k = int(env) if env else min(m, 56)
    if k > m or k > 56:
        k = min(m, 56)
    return k if k >= (2 if env else 16) else 0


def _same_blocks(got, want, seqs, what):
    offs, blocks, sub, edges, stats, info = got
    gm = blocks_matrix(blocks)
    if not (np.array_equal(offs, want["block_offs"]) and np.array_equal(gm, want["blocks"])):
        wo = want["block_offs"]
        for r in range(len(seqs)):
            a = gm[int(offs[r]):int(offs[r + 1])] if r + 1 < len(offs) else None
            b = want["blocks"][int(wo[r]):int(wo[r + 1])]
            if a is None or not np.array_equal(a, b):
                raise AssertionError("%s: read %d (%r) blocks differ\n got  %s\n want %s" % (what, r, seqs[r], a, b))
        raise AssertionError("%s: block lists differ" % what)
    assert np.array_equal(sub.astype(bool), want["substring"].astype(bool)), what
    assert stats["n_occ_find"] + stats["n_occ_extract"] == want["n_occ_min"], what
    assert stats["n_blocks"] == len(want["blocks"]), what
    # no edge parity (the reference indexes .sai out of range on such sets: tests/fixtures.py), but every record must
    # name reads of the set
    n = len(seqs)
    assert np.all(edges["query"] < n) and np.all(edges["target"] < n), what
    # reads are not stretches: the direct maps are refused (sigax_tables.cpp: plan_row_tables, can_direct)
    assert info["row_direct"] == 0, what


@pytest.mark.parametrize("seed", mr.NON_ACGT_SEEDS)
def test_non_acgt_case(seed, tmp_path):
    """One case: the GPU index builder's files == the oracle builder's; per read, blocks in order, substring flag and the
    rank-evaluation count == the oracle's, on a first-pass index and on a prepared one (row tables + deep start table);
    rmdup's blocks; the order check refuses the index."""
    import siga_amd
    from siga_amd import _lib, host
    from siga_amd.overlap import name_ranks
    case = mr.non_acgt_case(seed)
    reads, m, irr, rc = case["reads"], case["m"], case["irreducible"], case["rc"]
    seqs = [s for _, s in reads]
    fa, prefix = _write_case(case, str(tmp_path))
    host.index_file(fa, prefix, threads=2)
    oracle_prefix = str(tmp_path / "o")
    po.Index.build(seqs).save(oracle_prefix + ".bwt", oracle_prefix + ".sai")
    po.Index.build(seqs, reverse=True).save(oracle_prefix + ".rbwt", oracle_prefix + ".rsai")
    gpu_prefix = str(tmp_path / "g")
    buf, offs = siga_amd.overlap.pack_reads(seqs)
    host.index_build_gpu(buf, offs, gpu_prefix)
    for ext in EXTS:
        want = open(oracle_prefix + ext, "rb").read()
        assert open(prefix + ext, "rb").read() == want, ext
        assert open(gpu_prefix + ext, "rb").read() == want, ext

    fwd = po.Index.load(prefix + ".bwt", prefix + ".sai")
    rev = po.Index.load(prefix + ".rbwt", prefix + ".rsai")
    assert fwd.nstrings == len(seqs)
    want = po.overlap_batch(fwd, rev, seqs, m, irr, rc)
    flags = (_lib.SIGAX_IRREDUCIBLE if irr else 0) | (_lib.SIGAX_RC if rc else 0) | _lib.SIGAX_EDGES
    meta = (np.array([len(s) for s in seqs], dtype=np.uint32), name_ranks([n for n, _ in reads]))

    first = siga_amd.FMIndexPair.load(prefix, resident=False)  # what one `siga overlap` runs
    try:
        first.set_reads(*meta)
        got = _run_batch(first, seqs, m, flags)
        _same_blocks(got, want, seqs, "first pass")
        # no deep table on a first pass -- unless the run overflowed its candidate slots and repeated itself
        # (SIGAX_CAND_CAP): by then the index has been asked for all its reads once and may have built it in the background
        assert got[5]["deep_k"] in ((0, _expected_deep_k(m)) if got[5]["reruns"] else (0,)), got[5]
    finally:
        first.close()

    pair = siga_amd.FMIndexPair.load(prefix)  # an index that stays open: row tables, then the deep table for m
    try:
        pair.set_reads(*meta)
        pair.prepare_overlap(m)
        got = _run_batch(pair, seqs, m, flags)
        _same_blocks(got, want, seqs, "prepared")
        info = got[5]
        if info["row_bits"] and info["row_text"]:
            assert info["deep_k"] == _expected_deep_k(m), info
        else:  # no row table + text (SIGAX_ROWEND=0, SIGAX_LOOKAHEAD=0): nothing to read the K-mers off
            assert info["deep_k"] == 0, info
        if os.environ.get("SIGAX_ROWEND") != "0":
            assert info["row_bits"] != 0, info
        dup = siga_amd.OverlapBuilder(pair).duplicate(seqs)
        wd = po.overlap_batch(fwd, rev, seqs, 0, duplicate=True)
        assert np.array_equal(dup["block_offs"], wd["block_offs"])
        assert np.array_equal(blocks_matrix(dup["blocks"]), wd["blocks"])
        assert np.array_equal(dup["substring"].astype(bool), wd["substring"].astype(bool))
        with pytest.raises(siga_amd.SigaxError) as e:  # stretches are not reads (sigax_index.cpp: sigax_index_check_order)
            pair.check_order(0)
        assert e.value.code == _lib.SIGAX_E_STATE
    finally:
        pair.close()


def test_occ_on_an_n_dense_index(tmp_path):
    """sigax_occ_batch at every position of both strands of an index whose reads all carry non-ACGT bytes == the oracle's
    Occ: the '$' count is the position's rank minus the ACGT counts, '$' rows of every non-ACGT byte included."""
    import siga_amd
    seed = mr.NON_ACGT_DENSE[0]
    case = mr.non_acgt_case(seed)
    seqs = [s for _, s in case["reads"]]
    fa, prefix = _write_case(case, str(tmp_path))
    from siga_amd import host
    host.index_file(fa, prefix, threads=2)
    pair = siga_amd.FMIndexPair.load(prefix)
    try:
        for which, ext in ((0, "bwt"), (1, "rbwt")):
            orc = po.Index.load(prefix + "." + ext)
            n = len(orc)
            assert n > 20000
            pos = np.arange(n, dtype=np.uint64)
            got = pair.occ(pos, which)
            want = np.array([orc.occ(int(p)) for p in pos], dtype=np.uint64)
            assert np.array_equal(got, want), (which, int(np.nonzero((got != want).any(axis=1))[0][0]))
            assert np.array_equal(got[:, 0], pos + 1 - got[:, 1:].sum(axis=1))
            assert int(got[-1, 0]) > len(seqs)  # '$' rows beyond one per read: the non-ACGT bytes
    finally:
        pair.close()


def test_cli_overlap_on_mixed_case_and_n(tmp_path):
    """`siga index` + `siga overlap -m 45` on a FASTA of mixed-case, IUPAC and N reads: exit 0; HT and VT lines (SS:i:
    flags) == what the host's formatter writes from the oracle's substring flags; every ED line names two reads."""
    import gzip
    import subprocess
    from siga_amd import host
    from siga_amd.overlap import EDGE_DTYPE
    seed = next(s for s in mr.NON_ACGT_SEEDS if mr.non_acgt_case(s)["m"] == 45)
    case = mr.non_acgt_case(seed)
    seqs = [s for _, s in case["reads"]]
    cwd = str(tmp_path)
    fa, prefix = _write_case(case, cwd)
    assert subprocess.run([host.CLI_PATH, "index", "r.fa"], cwd=cwd, capture_output=True).returncode == 0
    r = subprocess.run([host.CLI_PATH, "overlap", "-m", "45", "r.fa"], cwd=cwd, capture_output=True)
    assert r.returncode == 0, r.stderr
    got = gzip.open(cwd + "/r.asqg.gz", "rb").read().decode("latin-1").split("\n")
    fwd = po.Index.load(prefix + ".bwt", prefix + ".sai")
    rev = po.Index.load(prefix + ".rbwt", prefix + ".rsai")
    sub = po.overlap_batch(fwd, rev, seqs, 45)["substring"]
    host.format_asqg(fa, sub, np.zeros(0, dtype=EDGE_DTYPE), 45, cwd + "/want.asqg")
    want = open(cwd + "/want.asqg", "rb").read().decode("latin-1").split("\n")
    assert [l for l in got if l and not l.startswith("ED\t")] == [l for l in want if l]
    names = {n for n, _ in case["reads"]}
    ed = [l[3:].split(" ") for l in got if l.startswith("ED\t")]
    assert ed and all(e[0] in names and e[1] in names for e in ed)
    assert any(v.startswith("VT\t") and "SS:i:1" in v for v in want)
