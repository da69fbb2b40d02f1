"""`siga overlap -e` on the GPU (csrc/sigax_mmoverlap.hip) against the serial restatement of its rules (tests/mmoverlap_cases.py):
the device form, the batch form, the Python ends and the command line -- records with num_diff, flags and status words -- over
reads of mixed lengths, the hand-made boundary sets of every rule, the caps and the overflow protocols; and `-e 0` against the
exact overlap run."""
import ctypes as C
import functools
import gzip
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import mmoverlap_cases as mc
from tests import pileup_cases as pc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr
from tests.test_gpu_overlap_correct import _Device

pytestmark = pytest.mark.gpu


def _kw(p):
    return {mc.FIELDS[k]: v for k, v in p.items() if k not in ("P", "M", "max_len")}


def _index(refs, names, both=False):
    """the read set's files (oracle-built index, FASTA; cached under a name made of the reads) -> prefix"""
    key = hashlib.sha1("\n".join(refs + names).encode()).hexdigest()[:16]
    d = os.path.join(CACHE, "mmo_" + key)
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    if not os.path.exists(prefix + ".fa"):
        with open(prefix + ".fa", "w") as f:
            f.write(mr.fasta_text(list(zip(names, refs))))
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".sai")):
        po.Index.build(refs).save(prefix + ".bwt", prefix + ".sai")
    if both and not all(os.path.exists(prefix + e) for e in (".rbwt", ".rsai")):
        po.Index.build(refs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
    return prefix


def _open(refs, names, set_reads=True):
    import siga_amd
    pair = siga_amd.FMIndexPair.load_forward(_index(refs, names), device=0)
    if set_reads:
        pair.set_reads([len(r) for r in refs], mc.name_ranks(names))
    return pair


def _tuples(edges):
    assert not edges["reserved"].any()
    return [tuple(int(e[k]) for k in ("query", "target", "length", "af", "num_diff")) for e in edges]


def _params(p, max_len=True):
    from siga_amd import _lib
    return _lib.MmoParams(p["P"], min_overlap=p["M"], max_read_len=p["max_len"] if max_len else 0, **_kw(p))


class _Calls:
    """sigax_mmoverlap_device calls that append at one cursor, every buffer of exactly its size and prefilled with 0xEE"""

    def __init__(self, pair, refs, edges_cap):
        from siga_amd import _lib
        self.L, self._lib, self.pair, self.refs = _lib.lib(), _lib, pair, refs
        self.dev = _Device()
        self.stream = C.c_void_p()
        assert self.L.sigax_stream_create(0, C.byref(self.stream)) == 0
        self.ref = C.c_void_p()
        assert self.L.sigax_pile_ref_create(pair.handle, C.byref(self.ref)) == 0, _lib.last_error()
        self.d_text, self.d_toffs = C.c_void_p(), C.c_void_p()
        assert self.L.sigax_pile_ref_buffers(self.ref, C.byref(self.d_text), C.byref(self.d_toffs), None) == 0
        self.edges_cap = edges_cap
        self.d_edges = self.dev.buf(edges_cap * 24)
        self.d_cursor = self.dev.buf(8, np.zeros(1, dtype=np.uint64))
        self.d_contained = self.dev.buf(len(refs), np.zeros(len(refs), dtype=np.uint8))

    def workspace(self, p, count, nb, hits_cap):
        """-> (d_work, its bytes) for calls of at most these sizes"""
        wb = C.c_uint64()
        assert self.L.sigax_mmoverlap_workspace(count, nb, C.byref(_params(p)), hits_cap, C.byref(wb)) == 0, self._lib.last_error()
        return self.dev.buf(wb.value), wb.value

    def call(self, p, first, count, hits_cap, work=None):
        """-> status8; work: a workspace() to run in, as whatever ran there before has left it, in place of fresh memory"""
        nb = sum(len(r) for r in self.refs[first:first + count])
        params = _params(p)
        wb = C.c_uint64()
        assert self.L.sigax_mmoverlap_workspace(count, nb, C.byref(params), hits_cap, C.byref(wb)) == 0, self._lib.last_error()
        d_stat, d_work = self.dev.buf(64), work[0] if work else self.dev.buf(wb.value)
        assert not work or wb.value <= work[1]
        assert self.dev.hip.hipDeviceSynchronize() == 0
        assert self.L.sigax_mmoverlap_device(self.pair.handle, self.d_text, self.d_toffs, first, count, nb, C.byref(params), self.d_edges,
                                             self.edges_cap, self.d_cursor, self.d_contained, d_stat, d_work, wb.value, hits_cap,
                                             self.stream) == 0, self._lib.last_error()
        assert self.dev.hip.hipStreamSynchronize(self.stream) == 0
        return self.dev.get(d_stat, np.uint64, 8).tolist()

    def cursor(self):
        return int(self.dev.get(self.d_cursor, np.uint64, 1)[0])

    def contained(self):
        return self.dev.get(self.d_contained, np.uint8, len(self.refs)).tolist()

    def raw(self):
        """the whole record buffer, written or not"""
        return self.dev.get(self.d_edges, self._lib.MM_EDGE_DTYPE, self.edges_cap)

    def finish(self):
        """-> the ordered records"""
        n_raw = self.cursor()
        wb = C.c_uint64()
        assert self.L.sigax_mmoverlap_finish_workspace(n_raw, C.byref(wb)) == 0, self._lib.last_error()
        d_n, d_work = self.dev.buf(8), self.dev.buf(wb.value)
        assert self.dev.hip.hipDeviceSynchronize() == 0
        assert self.L.sigax_mmoverlap_finish_device(self.d_edges, n_raw, d_n, d_work, wb.value, self.stream) == 0, self._lib.last_error()
        assert self.dev.hip.hipStreamSynchronize(self.stream) == 0
        n = int(self.dev.get(d_n, np.uint64, 1)[0])
        assert n <= n_raw
        return _tuples(self.raw()[:n])

    def close(self):
        self.L.sigax_pile_ref_destroy(self.ref)
        self.dev.free()
        self.L.sigax_stream_destroy(0, self.stream)


def _check_forms(refs, names, p, device=True):
    """the batch form and one device call of exactly the sizes needed against the restatement -> the restatement's result"""
    ranks = mc.name_ranks(names)
    want = mc.expected_mm_overlaps(refs, ranks, p)
    pair = _open(refs, names)
    try:
        edges, contained, status = pair.overlap_mismatch(p["P"], p["M"], **_kw(p))
        assert _tuples(edges) == want[0]
        assert contained.tolist() == want[1] and status.tolist() == want[2]
        if device:
            calls = _Calls(pair, refs, want[2][7])
            try:
                assert calls.call(p, 0, len(refs), want[2][0]) == want[2]
                assert calls.cursor() == want[2][7] and calls.contained() == want[1]
                raw = calls.raw()
                assert not raw["reserved"].any() and sorted(set(_tuples(raw)), key=lambda r: (r[0], r[1], r[3], r[2])) == want[0]
                assert calls.finish() == want[0]
            finally:
                calls.close()
    finally:
        pair.close()
    return want


@functools.lru_cache(maxsize=None)
def _mixed():
    refs, names = mc.mixed_case()
    return refs, names, mc.name_ranks(names)


def test_mixed_lengths_all_forms():
    refs, names, _ = _mixed()
    want = _check_forms(refs, names, mc.params())
    records, contained, st = want
    assert st[1] == 3 and len(records) > 300 and sum(contained) > 20  # two reads below S and the one of 4097 bases
    assert any(r[4] for r in records) and {r[3] for r in records} == {0, 3, 5, 6}
    big, over = len(refs) - 4, len(refs) - 3  # the reads of 4096 and of 4097 bases
    assert len(refs[big]) == 4096 and len(refs[over]) == 4097
    assert any(big in r[:2] for r in records) and any(over in r[:2] for r in records)  # the long one is a target of others
    assert contained[big] == 1  # inside the one of 4097, which finds nothing itself


def test_mixed_lengths_short_seeds():
    refs, names, _ = _mixed()
    want = _check_forms(refs, names, mc.params(S=12, T=5, M=30, P=60, H=10, K=300))
    assert want[2][4] > 100 and len(want[0]) > 500  # seeds over H, and pairs found all the same


def test_every_boundary_set():
    for name, (refs, names, p, records, flagged) in sorted(mc.boundary_sets().items()):
        want = _check_forms(refs, names, p)
        assert want[0] == records and [i for i, c in enumerate(want[1]) if c] == flagged, name


def test_query_columns_from_2048_on():
    """a read of 4096 bases whose partners lie at its columns 2048 and above, where its codes are in the second register: a
    forward and a reverse-complemented read that dovetail with its last 60 columns, the first with a mismatch among them, and a
    read wholly inside"""
    g = pc.random_genome(4300, 23)
    fwd = pc.mutate(g[4036:4156], [30])
    refs = [g[0:4096], fwd, pc.revcomp(g[4036:4096] + pc.random_genome(54, 24)), g[3000:3120]]
    names = ["d", "c", "b", "a"]
    want = _check_forms(refs, names, mc.params())
    assert want[0] == [(0, 1, 60, 0, 1), (0, 2, 60, 6, 0)] and want[1] == [0, 0, 0, 1]


def test_seeded_equals_brute_force_on_the_device():
    refs, names = mc.noisy_case()
    p = mc.params(S=12, T=4, M=45, P=40, H=4096, K=4096)
    brute = mc.brute_mm_overlaps(refs, mc.name_ranks(names), p)
    want = _check_forms(refs, names, p)
    assert (want[0], want[1]) == brute


def test_read_over_k_and_seed_over_h():
    g = mc.G
    refs = [g[100:180], g[135:215], g[65:145]]  # read 0 has two partners, at K = 1 it gives up; they still report the pairs
    names = ["c", "a", "b"]
    p = mc.params(S=12, T=4, M=45, P=0, H=4096, K=1)
    want = _check_forms(refs, names, p)
    assert want[2][2] == 3 and want[0] == []  # (every read sees itself and a partner: all three are over K = 1)
    p = mc.params(S=12, T=4, M=45, P=0, H=4096, K=2)
    want = _check_forms(refs, names, p)
    assert want[2][2] == 1 and want[0] == [(0, 1, 45, 0, 0), (0, 2, 45, 3, 0)]
    # windows that occur in three reads: at H = 2 they are skipped, the others find the pairs all the same
    want = _check_forms(refs + [g[130:150] + pc.random_genome(40, 5)], names + ["d"], mc.params(S=12, T=4, M=45, P=0, H=2, K=4096))
    assert want[2][4] > 0 and len(want[0]) == 2


def test_two_calls_at_one_cursor_equal_one():
    """... the second one, of fewer reads, in the workspace the first one has used"""
    refs, names, ranks = _mixed()
    p = mc.params()
    whole = mc.expected_mm_overlaps(refs, ranks, p)
    half = len(refs) // 2 + 1
    a = mc.expected_mm_overlaps(refs, ranks, p, 0, half)
    b = mc.expected_mm_overlaps(refs, ranks, p, half, len(refs) - half)
    assert a[2][7] + b[2][7] == whole[2][7] > len(whole[0])  # pairs across the halves are written by both
    pair = _open(refs, names)
    calls = _Calls(pair, refs, whole[2][7])
    try:
        assert len(refs) - half < half
        work = calls.workspace(p, half, sum(len(r) for r in refs), max(a[2][0], b[2][0]))
        assert calls.call(p, 0, half, a[2][0], work) == a[2]
        assert calls.cursor() == a[2][7]
        assert calls.call(p, half, len(refs) - half, b[2][0], work) == b[2]  # first_read not 0
        assert calls.cursor() == whole[2][7] and calls.contained() == whole[1]
        assert calls.finish() == whole[0]
    finally:
        calls.close()
        pair.close()


def test_overflow_protocols_and_exact_buffers():
    refs, names, ranks = _mixed()
    p = mc.params()
    want = mc.expected_mm_overlaps(refs, ranks, p)
    n_rec, n_hits = want[2][7], want[2][0]
    pair = _open(refs, names)
    calls = _Calls(pair, refs, n_rec - 1)
    try:
        # records: one short -> nothing written, the cursor unchanged, the number in status[7]
        st = calls.call(p, 0, len(refs), n_hits)
        assert st == want[2] and calls.cursor() == 0
        assert calls.raw().tobytes() == b"\xee" * (24 * (n_rec - 1)) and not any(calls.contained())
        # hits: one short -> locate's protocol
        st = calls.call(p, 0, len(refs), n_hits - 1)
        assert st == [n_hits, 0, 0, 0, 0, 0, 0, 0] and calls.cursor() == 0
        assert calls.raw().tobytes() == b"\xee" * (24 * (n_rec - 1)) and not any(calls.contained())
    finally:
        calls.close()
    calls = _Calls(pair, refs, n_rec)  # the second call, with the numbers the first ones gave
    try:
        assert calls.call(p, 0, len(refs), n_hits) == want[2] and calls.cursor() == n_rec
        raw = calls.raw()
        assert b"\xee\xee\xee\xee" not in raw.tobytes() and not raw["reserved"].any()  # every field of every record written
        assert calls.contained() == want[1] and calls.finish() == want[0]
    finally:
        calls.close()
        pair.close()


def test_batch_in_pieces(monkeypatch):
    refs, names, ranks = _mixed()
    p = mc.params()
    want = mc.expected_mm_overlaps(refs, ranks, p)
    pair = _open(refs, names)
    try:
        monkeypatch.setenv("SIGAX_TEST_MMO_PIECE", "37")
        monkeypatch.setenv("SIGAX_TEST_MMO_HITS_CAP", "3")
        monkeypatch.setenv("SIGAX_TEST_MMO_EDGES_CAP", "1")
        edges, contained, status = pair.overlap_mismatch(p["P"], p["M"], **_kw(p))
        assert _tuples(edges) == want[0] and contained.tolist() == want[1] and status.tolist() == want[2]
    finally:
        pair.close()


def test_e0_equals_the_exact_exhaustive_run():
    import siga_amd
    refs, names = mc.exact_case()
    ranks = mc.name_ranks(names)
    p = mc.params(S=12, T=4, M=45, P=0, H=4096, K=4096)
    pair = siga_amd.FMIndexPair.load(_index(refs, names, both=True), device=0)
    try:
        pair.set_reads([len(r) for r in refs], ranks)
        exact = siga_amd.OverlapBuilder(pair, irreducible=False, rc=True).overlap(refs, p["M"], edges=True)
        edges, contained, status = pair.overlap_mismatch(0, p["M"], **_kw(p))
        assert not contained.any() and not exact["substring"].any() and not edges["num_diff"].any()
        got = {(q, t, l, af) for q, t, l, af, _ in _tuples(edges)}
        want = {tuple(int(e[k]) for k in ("query", "target", "length", "af")) for e in exact["edges"]}
        assert len(got) == len(edges) > 100 and got == want
    finally:
        pair.close()


def test_errors():
    import siga_amd
    from siga_amd import _lib
    from tests import test_gpu_match as tgm
    L = _lib.lib()
    refs, names = mc.exact_case()
    wb = C.c_uint64()
    for field, bad in (("seed_length", 11), ("seed_length", 65), ("seed_stride", 0), ("seed_stride", 25), ("max_seed_hits", 0),
                       ("max_seed_hits", 4097), ("min_overlap", 0), ("error_permille", 251), ("max_candidates", 0), ("max_candidates", 4097),
                       ("max_read_len", 4097)):
        kw = {"error_permille": 40}
        kw[field] = bad
        params = _lib.MmoParams(**kw)
        assert L.sigax_mmoverlap_workspace(1, 100, C.byref(params), 10, C.byref(wb)) == _lib.SIGAX_E_ARG, field
        assert field in _lib.last_error()
    params = _lib.MmoParams(40)
    assert L.sigax_mmoverlap_workspace(1, 100, None, 10, C.byref(wb)) == _lib.SIGAX_E_ARG
    assert L.sigax_mmoverlap_workspace(1, 100, C.byref(params), 10, None) == _lib.SIGAX_E_ARG
    st = np.zeros(8, dtype=np.uint64)
    pair = _open(refs, names)
    try:
        with pytest.raises(siga_amd.overlap.SigaxError):
            pair.overlap_mismatch(251)
        # NULL buffers and reads the index does not hold: refused before anything is queued
        assert L.sigax_mmoverlap_device(pair.handle, None, None, 0, 1, 100, C.byref(params), None, 0, None, None, st.ctypes.data, None, 0, 10,
                                        None) == _lib.SIGAX_E_ARG
        assert L.sigax_mmoverlap_device(pair.handle, None, None, len(refs), 1, 100, C.byref(params), None, 0, None, None, st.ctypes.data, None, 0,
                                        10, None) == _lib.SIGAX_E_ARG
        assert "holds" in _lib.last_error()
        assert L.sigax_mmoverlap_finish_device(None, 5, None, None, 0, None) == _lib.SIGAX_E_ARG
        assert L.sigax_mmoverlap_batch(pair.handle, None, C.byref(params), None, None, None, None) == _lib.SIGAX_E_ARG
    finally:
        pair.close()
    pair = _open(refs, names, set_reads=False)  # the reads' names are not known
    try:
        with pytest.raises(siga_amd.overlap.SigaxError) as e:
            pair.overlap_mismatch(40)
        assert e.value.code == _lib.SIGAX_E_STATE and "sigax_index_set_reads" in str(e.value)
    finally:
        pair.close()
    pair = siga_amd.FMIndexPair.load_forward(_index(refs, names), device=0, with_sai=False)
    try:
        with pytest.raises(siga_amd.overlap.SigaxError) as e:
            pair.overlap_mismatch(40)
        assert e.value.code == _lib.SIGAX_E_STATE and ".sai" in str(e.value)
    finally:
        pair.close()
    prefix, _ = tgm._files(1)  # an index whose reads hold an N
    pair = siga_amd.FMIndexPair.load(prefix, device=0, with_sai=True, resident=False)
    try:
        with pytest.raises(siga_amd.overlap.SigaxError) as e:
            pair.overlap_mismatch(40)
        assert e.value.code == _lib.SIGAX_E_STATE and "ACGT" in str(e.value)
    finally:
        pair.close()


# ---- the host class and the command line ----
def _cli(args, cwd):
    from siga_amd import host
    return subprocess.run([host.CLI_PATH, "overlap"] + args, capture_output=True, cwd=cwd)


def _link_index(prefix, d, exts=(".bwt", ".sai", ".fa")):
    for e in exts:
        os.symlink(prefix + e, os.path.join(d, "reads" + e))
    return os.path.join(d, "reads")


def test_cli_and_host_class(tmp_path):
    from siga_amd import host
    refs, names, ranks = _mixed()
    d = str(tmp_path)
    prefix = _link_index(_index(refs, names), d)
    p = mc.params()
    want = mc.expected_mm_overlaps(refs, ranks, p)
    r = _cli(["-e", "40", "-m", "45", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    text = gzip.open(prefix + ".asqg.gz", "rt").read()
    assert text.split("\n") == mc.asqg_text(names, refs, want[0], want[1], 45).split("\n")
    # every option on the line, the prefix given
    p = mc.params(S=16, T=4, H=100, M=30, P=60, K=300)
    want = mc.expected_mm_overlaps(refs, ranks, p)
    os.makedirs(os.path.join(d, "two"))
    r = _cli(["--error-permille=60", "--min-overlap=30", "--seed-length=16", "--seed-stride=4", "--max-seed-hits=100", "--max-candidates=300", "-p",
              prefix, "-t", "2", prefix + ".fa"], os.path.join(d, "two"))
    assert r.returncode == 0, r.stderr.decode()
    assert gzip.open(prefix + ".asqg.gz", "rt").read() == mc.asqg_text(names, refs, want[0], want[1], 30)
    out = os.path.join(d, "three.asqg")
    status = host.overlap_file(prefix + ".fa", prefix, 30, out, error_permille=60, **_kw(p))
    assert status.tolist() == want[2]
    assert open(out).read() == mc.asqg_text(names, refs, want[0], want[1], 30)


def test_cli_refusals(tmp_path):
    from tests import test_gpu_match as tgm
    refs, names = mc.exact_case()
    d = str(tmp_path)
    prefix = _link_index(_index(refs, names), d)
    for opt, name in ((["-e", "40", "--no-opposite-strand"], b"--no-opposite-strand"), (["-e", "40", "--gpus=2"], b"--gpus"),
                      (["--seed-length=16"], b"--seed-length"), (["--seed-stride=4"], b"--seed-stride"), (["--max-seed-hits=9"], b"--max-seed-hits"),
                      (["--max-candidates=9"], b"--max-candidates"), (["-e", "300"], b"error_permille"), (["-e", "40", "--seed-length=11"], b"seed_length"),
                      (["-e", "x"], b"error_permille")):
        r = _cli(opt + ["reads.fa"], d)
        assert r.returncode == 1 and name in r.stderr and not os.path.exists(prefix + ".asqg.gz"), (opt, r.stderr)
    nosai = os.path.join(d, "nosai")
    os.makedirs(nosai)
    _link_index(_index(refs, names), nosai, (".bwt", ".fa"))
    r = _cli(["-e", "40", "reads.fa"], nosai)
    assert r.returncode == 1 and b".sai" in r.stderr
    withn, fa = tgm._files(1)
    r = _cli(["-e", "40", "-p", withn, fa], d)
    assert r.returncode == 1 and b"ACGT" in r.stderr
    r = _cli(["--help"], d)
    for word in (b"--error-permille", b"--seed-length", b"--seed-stride", b"--max-seed-hits", b"--max-candidates"):
        assert word in r.stdout
