"""`siga match` on the GPU (csrc/sigax_match.hip) against the reference's loop over the oracle's Interval::occurrences
(tests/match_cases.py): every query of every case, in every form the library has -- forward-only and two-strand indexes,
with and without the corrector's prefix table and the two-step tables, 32- and 64-bit positions, the host and the device
entry point, the host class in several batches, and the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import match_cases as mc
from tests.fixtures import CACHE, ROOT
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
NONE = (1 << 64) - 1


def _files(seed):
    """the case's index files (oracle-built) and its queries as FASTA -> (prefix, queries path)"""
    case = mc.match_case(seed)
    d = os.path.join(CACHE, "match%d" % seed)
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".queries.fa")):
        seqs = [s for _, s in case["reads"]]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".queries.fa", "w") as f:
            f.write(mr.fasta_text([(n, s) for n, s, _ in case["queries"]]))
    return prefix, prefix + ".queries.fa"


def _open(prefix, both=False):
    import siga_amd
    from siga_amd import _lib
    if both:
        return siga_amd.FMIndexPair.load(prefix, device=0, with_sai=False, resident=False)
    h = C.c_void_p()
    assert _lib.lib().sigax_index_open((prefix + ".bwt").encode(), None, None, None, 0, C.byref(h)) == 0, _lib.last_error()
    return siga_amd.FMIndexPair(h.value)


def _queries(seed):
    """the case's queries plus the empty one only the C-ABI can carry"""
    case = mc.match_case(seed)
    return list(case["queries"]) + [("empty", "", "empty")]


def _assert_counts(pair, seed, what):
    case = mc.match_case(seed)
    q = _queries(seed)
    head, tail, _ = mc.expected(mc.oracle_index(seed), q, case["L"], case["rc"])
    got_h, got_t = pair.match([s for _, s, _ in q], max_length=case["L"], rc=case["rc"])
    for i, (name, s, _) in enumerate(q):
        assert int(got_h[i]) == head[i], "%s seed %d %s (%d bases): head %d, want %d" % (what, seed, name, len(s), got_h[i], head[i])
        if tail[i] is None:
            assert got_t.mask[i], "%s seed %d %s: a tail for a read that is not split" % (what, seed, name)
        else:
            assert not got_t.mask[i] and int(got_t.data[i]) == tail[i], "%s seed %d %s (%d bases): tail %d, want %d" % (
                what, seed, name, len(s), got_t.data[i], tail[i])


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_match_batch_forward_only(seed):
    prefix, _ = _files(seed)
    pair = _open(prefix)
    try:
        _assert_counts(pair, seed, "forward-only index")
    finally:
        pair.close()


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_match_batch_both_strands_and_prefix_table(seed):
    """on the two-strand index, and again once a correction call has left the table of 13-mer intervals on the device"""
    from siga_amd import _lib
    prefix, _ = _files(seed)
    pair = _open(prefix, both=True)
    try:
        _assert_counts(pair, seed, "two-strand index")
        seqs = np.frombuffer(b"ACGTACGTTGCATGCAACGTACGTTGCATGCAACGT", dtype=np.uint8)
        offs = np.array([0, len(seqs)], dtype=np.uint64)
        out, valid = np.zeros(len(seqs), dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        assert _lib.lib().sigax_correct_batch(pair.handle, seqs.tobytes(), None, offs.ctypes.data, 1, 31, 3, 10, 1, out.ctypes.data,
                                              valid.ctypes.data) == 0, _lib.last_error()
        _assert_counts(pair, seed, "with the prefix table")
    finally:
        pair.close()


def _child(env_extra, seeds):
    env = dict(os.environ, **env_extra)
    what = [os.path.join(ROOT, "tests", "test_gpu_match.py") + "::test_match_batch_both_strands_and_prefix_table[%d]" % k for k in seeds]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q"] + what, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_match_without_two_step_tables():
    _child({"SIGAX_TWO_STEP": "0"}, mc.SEEDS)


def test_match_wide_positions_small_superblocks():
    lib = os.path.join(ROOT, "build", "libsigax_super12.so")
    assert os.path.exists(lib)
    _child({"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": lib}, mc.SEEDS)
    _child({"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": lib, "SIGAX_TWO_STEP": "0"}, (1, 8))


def _match_on_device(handle, seqs, max_length, rc):
    """sigax_match_device on a stream of its own, the reads in a buffer of exactly their size -> (counts[2n], stat4)"""
    from siga_amd import _lib
    L = _lib.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    buf, offs = po.pack_reads(seqs)
    buf = np.frombuffer(buf, dtype=np.uint8)
    n = len(seqs)
    held = []

    def dbuf(nbytes, src=None):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(nbytes, 1)) == 0
        held.append(q)
        assert hip.hipMemset(q, 0xEE, max(nbytes, 1)) == 0
        if src is not None and src.nbytes:
            assert hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        return q

    stream = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    try:
        d_seqs, d_offs, d_counts, d_stat = dbuf(buf.nbytes, buf), dbuf(offs.nbytes, offs), dbuf(16 * n), dbuf(32)
        assert hip.hipDeviceSynchronize() == 0
        lim = NONE if max_length is None else max_length
        assert L.sigax_match_device(handle, d_seqs, d_offs, n, lim, 2 if rc else 0, d_counts, d_stat, stream) == 0, _lib.last_error()
        assert hip.hipStreamSynchronize(stream) == 0
        counts, stat = np.zeros(2 * n, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        assert hip.hipMemcpy(counts.ctypes.data, d_counts, 16 * n, 2) == 0 and hip.hipMemcpy(stat.ctypes.data, d_stat, 32, 2) == 0
    finally:
        for q in held:
            hip.hipFree(q)
        L.sigax_stream_destroy(0, stream)
    return counts, stat


@pytest.mark.parametrize("seed", (1, 4, 7, 10))
def test_match_device_form_and_statistics(seed):
    """same counts as the oracle on a stream of the caller's; chains run = the non-empty patterns of the case; symbols
    consumed no more than the reference's loop consumes (both from the oracle)"""
    case = mc.match_case(seed)
    fwd = mc.oracle_index(seed)
    q = _queries(seed)
    seqs = [s for _, s, _ in q]
    head, tail, _ = mc.expected(fwd, q, case["L"], case["rc"])
    prefix, _ = _files(seed)
    pair = _open(prefix)
    try:
        counts, stat = _match_on_device(pair.handle, seqs, case["L"], case["rc"])
    finally:
        pair.close()
    assert [int(x) for x in counts[0::2]] == head
    assert [int(x) for x in counts[1::2]] == [NONE if t is None else t for t in tail]
    pats = mc.patterns(seqs, case["L"], case["rc"])
    bound = sum(mc.stop_depth(fwd, w) for w in pats)
    print("seed %d: chains %d (want %d), symbols %d (bound %d, total %d), sectors %d" % (
        seed, stat[0], len(pats), stat[1], bound, sum(len(w) for w in pats), stat[2]))
    assert int(stat[0]) == len(pats)
    assert int(stat[1]) <= bound


def test_dead_chains_stop():
    fwd = mc.oracle_index(1)
    seqs = mc.half_substituted(1)
    prefix, _ = _files(1)
    pair = _open(prefix)
    try:
        counts, stat = _match_on_device(pair.handle, seqs, None, True)
    finally:
        pair.close()
    pats = mc.patterns(seqs, None, True)
    total, bound = sum(len(w) for w in pats), sum(mc.stop_depth(fwd, w) for w in pats)
    print("half substituted: symbols %d, bound %d, total %d" % (stat[1], bound, total))
    assert int(stat[0]) == len(pats)
    assert int(stat[1]) <= bound
    assert int(stat[1]) < 0.75 * total
    assert [int(x) for x in counts[0::2]] == [mc.count(fwd, s, True) for s in seqs]


def test_arguments():
    from siga_amd import _lib
    L = _lib.lib()
    prefix, _ = _files(1)
    pair = _open(prefix)
    try:
        out = np.zeros(2, dtype=np.uint64)
        offs = np.array([0, 4], dtype=np.uint64)
        assert L.sigax_match_batch(pair.handle, b"ACGT", offs.ctypes.data, 0, NONE, 2, out.ctypes.data) == 0
        assert L.sigax_match_batch(pair.handle, None, None, 0, NONE, 0, None) == 0
        for flags in (1, 4, 3, 8):
            assert L.sigax_match_batch(pair.handle, b"ACGT", offs.ctypes.data, 1, NONE, flags, out.ctypes.data) == -1
    finally:
        pair.close()


def test_consistent_with_kmer_counts_and_indexed_reads():
    case = mc.match_case(1)
    prefix, _ = _files(1)
    pair = _open(prefix)
    try:
        reads = [s for _, s in case["reads"] if set(s) <= set("ACGT")]
        head, tail = pair.match(reads, rc=False)
        assert np.array_equal(head, pair.kmer_counts(reads))
        assert tail.mask.all()
        head, _ = pair.match([s for _, s in case["reads"]])
        assert int(head.min()) >= 1
        windows = [s[7:47] for s in reads[:500]]
        assert np.array_equal(pair.match(windows, rc=False)[0], pair.kmer_counts(windows))
    finally:
        pair.close()


def _cli(args, cwd=None):
    from siga_amd import host
    return subprocess.run([host.CLI_PATH, "match"] + args, capture_output=True, cwd=cwd)


@pytest.mark.parametrize("seed", (1, 6, 9, 12))
def test_cli_two_files(seed, tmp_path):
    """FASTA + FASTQ inputs against one index, -p, -l, --no-opposite-strand, options from an ini file: stdout is the reference's"""
    case = mc.match_case(seed)
    q = case["queries"]
    prefix, _ = _files(seed)
    cut = len(q) // 2
    fa, fq = str(tmp_path / "a.fa"), str(tmp_path / "b.fastq")
    with open(fa, "w") as f:
        f.write(mr.fasta_text([(n, s) for n, s, _ in q[:cut]]))
    with open(fq, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s, _ in q[cut:]))
    _, _, want = mc.expected(mc.oracle_index(seed), q, case["L"], case["rc"])
    args = ["-p", prefix] + (["-l", str(case["L"])] if case["L"] is not None else []) + ([] if case["rc"] else ["--no-opposite-strand"])
    r = _cli(args + ["-t", "4", fa, fq])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == want
    ini = str(tmp_path / "match.ini")
    with open(ini, "w") as f:
        f.write("; options of siga match\nprefix=%s\n" % prefix)
        if case["L"] is not None:
            f.write("max-length=%d\n" % case["L"])
        if not case["rc"]:
            f.write("no-opposite-strand=1\n")
    r = _cli(["-s", ini, fa, fq])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == want


def test_cli_missing_index(tmp_path):
    _, queries = _files(1)
    r = _cli(["-p", str(tmp_path / "nothing"), queries])
    assert r.returncode != 0 and r.stdout == b""
    r = _cli([queries], cwd=str(tmp_path))  # prefix from the stem of the first READSFILE: no such index either
    assert r.returncode != 0 and r.stdout == b""


@pytest.mark.parametrize("seed", (3, 10))
def test_host_class_in_small_batches(seed, tmp_path):
    """batches of 50 reads: the lines keep the read order over four batches and more, the long query in a batch of its own"""
    from siga_amd import host
    case = mc.match_case(seed)
    prefix, queries = _files(seed)
    assert len(case["queries"]) >= 150
    _, _, want = mc.expected(mc.oracle_index(seed), case["queries"], case["L"], case["rc"])
    out = str(tmp_path / "out.txt")
    host.match_files([queries], prefix, max_length=case["L"], rc=case["rc"], out=out, batch_reads=50)
    assert open(out).read() == want
    host.match_files([queries, queries], prefix, max_length=case["L"], rc=case["rc"], out=out)
    assert open(out).read() == want + want
