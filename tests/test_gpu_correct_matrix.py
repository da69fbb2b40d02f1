"""`siga correct` on the GPU against the oracle PER READ, across k, its options and the k-mer lookup forms.

The cases come from tests/golden/make_reads.py: correct_case (tests/test_correct_cases.py checks, on the CPU, that they hold
what they claim): k from 7 to 100, seven option sets (negative thresholds among them), with and without qualities, and reads
planted where k_correct and kmer_occ change form.  Every read's output bytes and valid flag are compared, the reads that do
not become all-solid included: sigax_correct_batch against oracle.pyoracle.correct_batch, which tests/test_oracle_pin.py
ties to the file form.  tests/test_gpu_wide.py runs test_correct_case under the other lookup forms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.bigcheck import assert_same_correction, correct_on_device, correct_oracle, pack_case
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu


def _write_case(case, d, name="r"):
    """the case as FASTA / FASTQ + its index files by the host builder -> (reads path, prefix)"""
    from siga_amd import host
    path = os.path.join(d, name + (".fq" if case["quals"] else ".fa"))
    with open(path, "w") as f:
        f.write(mr.fastq_text(case["reads"], case["quals"]) if case["quals"] else mr.fasta_text(case["reads"]))
    prefix = os.path.join(d, name)
    host.index_file(path, prefix, threads=2)
    return path, prefix


def _open_forward(prefix):
    """the forward-only index `siga correct` loads (what `siga index --no-reverse` leaves): no row table of its own"""
    import siga_amd
    from siga_amd import _lib
    h = C.c_void_p()
    assert _lib.lib().sigax_index_open((prefix + ".bwt").encode(), None, None, None, 0, C.byref(h)) == 0, _lib.last_error()
    return siga_amd.FMIndexPair(h.value)


def _correct(pair, seqs, quals, offs, k, threshold, rounds, offset):
    from siga_amd import _lib
    n = len(offs) - 1
    out = np.full(len(seqs), ord("?"), dtype=np.uint8)
    valid = np.full(n, 9, dtype=np.uint8)
    r = _lib.lib().sigax_correct_batch(pair.handle, seqs.tobytes(), quals.tobytes() if quals is not None else None, offs.ctypes.data, n,
                                       k, threshold, rounds, offset, out.ctypes.data, valid.ctypes.data)
    assert r == 0, _lib.last_error()
    return out, valid


def _kmer_queries(case, rnd):
    """windows of the case's reads at its k, each also with one base replaced, and windows that hold an N"""
    k = case["k"]
    seqs = [s for _, s in case["reads"] if len(s) >= k]
    out = []
    for s in rnd.sample(seqs, 60):
        for a in {0, (len(s) - k) // 2, len(s) - k}:
            w = s[a:a + k]
            p = rnd.randrange(k)
            out += [w, w[:p] + rnd.choice([c for c in "ACGT" if c != w[p]]) + w[p + 1:]]
    with_n = [s for s in seqs if "N" in s and set(s) != {"N"}]
    for s in with_n[:40]:
        n = s.index("N")
        for a in {max(0, min(n, len(s) - k)), max(0, min(n - k + 1, len(s) - k)), max(0, min(n - k // 2, len(s) - k))}:
            out.append(s[a:a + k])
    out += ["N" * k, "A" * k]
    return out


@pytest.mark.parametrize("seed", mr.CORRECT_SEEDS)
def test_correct_case(seed, tmp_path):
    """One case: sigax_correct_batch on the forward-only index == the oracle for EVERY read -- valid[] and the output bytes,
    reads that stay unsolid (they must come back unchanged) and reads shorter than k included.  Then
    sigax_kmer_count_batch (the plain walk: a second witness when the corrector differs) == Interval::occurrences on
    windows of the case's reads, windows with one base replaced and windows with an N."""
    import random
    case = mr.correct_case(seed)
    seqs, quals, offs = pack_case(case)
    _, prefix = _write_case(case, str(tmp_path))
    index = po.Index.load(prefix + ".bwt")
    want = correct_oracle(case, index)
    args = (case["k"], case["threshold"], case["rounds"], case["offset"])
    pair = _open_forward(prefix)
    try:
        got = _correct(pair, seqs, quals, offs, *args)
        assert_same_correction(got, want, offs, "seed %d, -k %d -x %d -i %d -O %d" % ((seed,) + args))
        kmers = _kmer_queries(case, random.Random(seed))
        counts = pair.kmer_counts(kmers)
        expect = [index.occurrences(w) for w in kmers]
        assert list(map(int, counts)) == expect
        assert sum(1 for c in expect if c > 0) > 50 and any(c == 0 for c in expect)
    finally:
        pair.close()


def test_one_open_index_serves_k_after_k(tmp_path):
    """The k-mer table belongs to one k: a call with another k drops and rebuilds it (sigax_correct.cpp: ensure_kmer_table).
    One index stays open for k = 31, 21, 31, 57, 21 in turn (57 has no table: the prefix table + walk) -- first the
    forward-only index, which builds a bare row table of its own for the table builder, then a full index after
    sigax_index_prepare, whose row table it borrows.  Every call must give the oracle's bytes and flags."""
    import siga_amd
    case = mr.correct_case(1)
    assert case["quals"] is None
    seqs, _, offs = pack_case(case)
    _, prefix = _write_case(case, str(tmp_path))
    index = po.Index.load(prefix + ".bwt")
    want = {k: po.correct_batch(index, (seqs, offs), None, k, 3, 10, 1) for k in (21, 31, 57)}
    assert all(100 < int(v.sum()) < len(v) for _, v in want.values())
    assert not np.array_equal(want[21][0], want[57][0])
    for which in ("forward-only", "prepared"):
        if which == "forward-only":
            pair = _open_forward(prefix)
        else:
            pair = siga_amd.FMIndexPair.load(prefix)
            pair.prepare()
        try:
            for k in (31, 21, 31, 57, 21):
                got = _correct(pair, seqs, None, offs, k, 3, 10, 1)
                assert_same_correction(got, want[k], offs, "%s index, k = %d" % (which, k))
        finally:
            pair.close()


def test_correct_file_and_cli_with_other_options(tmp_path):
    """The host's CorrectProcessor and the CLI with options other than the defaults, one case of each format, byte for byte
    against the oracle's file form: `siga correct -k 33 -x 2 -i 3 -O 0` on FASTQ, host.correct_file at k = 100 with
    -x 5 -i 1 -O 4 on FASTA.  A negative -x reaches the reference's CorrectThreshold as the int it parses to
    (options.get<int>, src/correct_processor.cpp:78) and the CLI hands it on the same way: `-x -1` on FASTQ keeps the reads
    whose bases all score 20 and more where support 0 suffices, on FASTA writes an empty file, as does -x -2."""
    from siga_amd import host

    def cli(case, d, opts):
        os.makedirs(d)
        path, _ = _write_case(case, d, "reads")
        name = os.path.basename(path)
        for ext in (".rbwt", ".rsai"):
            os.remove(os.path.join(d, "reads" + ext))  # what `siga index --no-reverse` leaves
        r = subprocess.run([host.CLI_PATH, "correct"] + opts + ["-o", "g.ec", name], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        st = po.correct(po.Index.load(os.path.join(d, "reads.bwt")), path, os.path.join(d, "o.ec"), k=case["k"], threshold=case["threshold"],
                        rounds=case["rounds"], offset=case["offset"])
        assert open(os.path.join(d, "g.ec"), "rb").read() == open(os.path.join(d, "o.ec"), "rb").read()
        return st

    c3 = mr.correct_case(3)
    assert (c3["k"], c3["threshold"], c3["rounds"], c3["offset"], c3["quals"] is not None) == (33, 2, 3, 0, True)
    st = cli(c3, str(tmp_path / "c3"), ["-k", "33", "-x", "2", "-i", "3", "-O", "0"])
    assert st["changed"] > 500 and 1000 < st["written"] < len(c3["reads"])
    c16 = mr.correct_case(16)
    assert (c16["k"], c16["threshold"], c16["quals"] is not None) == (57, -1, True)
    st = cli(c16, str(tmp_path / "c16"), ["-k", "57", "-x", "-1"])
    assert 0 < st["written"] < len(c16["reads"])
    c2 = mr.correct_case(2)
    assert (c2["k"], c2["threshold"], c2["quals"]) == (32, -1, None)
    st = cli(c2, str(tmp_path / "c2"), ["-k", "32", "--kmer-threshold=-1"])
    assert st["written"] == 0 and os.path.getsize(str(tmp_path / "c2" / "g.ec")) == 0

    for seed, lo in ((13, 500), (9, None)):
        case = mr.correct_case(seed)
        d = str(tmp_path / ("f%d" % seed))
        os.makedirs(d)
        path, prefix = _write_case(case, d)
        args = dict(k=case["k"], threshold=case["threshold"], rounds=case["rounds"], offset=case["offset"])
        st = po.correct(po.Index.load(prefix + ".bwt"), path, os.path.join(d, "o.ec"), **args)
        host.correct_file(path, prefix, os.path.join(d, "g.ec"), **args)
        assert open(os.path.join(d, "g.ec"), "rb").read() == open(os.path.join(d, "o.ec"), "rb").read()
        if lo is None:
            assert case["threshold"] == -2 and st["written"] == 0
        else:
            assert (case["k"], case["quals"]) == (100, None) and st["changed"] > lo


def test_device_resident_form_on_mixed_lengths():
    """sigax_correct_device (every buffer on the device, the lengths unknown to the host: the small kernel form, then the
    large one for what it marked) on a case with qualities and reads of 1 to 200 bases, k = 65: the bytes and flags of
    sigax_correct_batch, which are the oracle's."""
    import tempfile
    from siga_amd import _lib
    case = mr.correct_case(12)
    assert case["k"] == 65 and case["quals"] is not None
    seqs, quals, offs = pack_case(case)
    lens = np.diff(offs.astype(np.int64))
    assert lens.min() == 1 and lens.max() == 200 and len(set(lens.tolist())) > 50
    with tempfile.TemporaryDirectory() as d:
        _, prefix = _write_case(case, d)
        index = po.Index.load(prefix + ".bwt")
        pair = _open_forward(prefix)
        try:
            args = (case["k"], case["threshold"], case["rounds"], case["offset"])
            host_form = _correct(pair, seqs, quals, offs, *args)
            out, valid, stat = correct_on_device(_lib.lib(), pair.handle, seqs, quals, offs, *args)
            assert_same_correction((out, valid), host_form, offs, "device form against host form")
            assert int(stat[0]) == 0
            assert_same_correction(host_form, correct_oracle(case, index), offs, "host form against the oracle")
        finally:
            pair.close()
