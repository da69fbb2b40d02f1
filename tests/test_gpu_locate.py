"""`siga locate` on the GPU (csrc/sigax_locate.hip) against brute-force string search (tests/locate_cases.py): every query of
the cases, through the host and the device entry point, on two-strand and forward-only indexes, with and without the
corrector's prefix table and the two-step tables, 32- and 64-bit positions, the host class and the command line."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import locate_cases as lc
from tests import match_cases as mc
from tests.fixtures import CACHE, ROOT
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
ALL = (1 << 32) - 1


def _files(name):
    """the case's index files (oracle-built) and, for `small`, its non-empty queries as FASTA -> prefix"""
    d = os.path.join(CACHE, "locate_" + name)
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".queries.fa")):
        seqs = [s for _, s in lc.small()["reads"]] if name == "small" else lc.many_seqs()
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".queries.fa", "w") as f:
            if name == "small":
                f.write(mr.fasta_text([(n, s) for n, s, _ in lc.small()["queries"] if s]))
    return prefix


def _open(prefix, both=True):
    import siga_amd
    if both:
        return siga_amd.FMIndexPair.load(prefix, device=0, with_sai=True, resident=False)
    return siga_amd.FMIndexPair.load_forward(prefix, device=0)


def _small_queries():
    return [s for _, s, _ in lc.small()["queries"]]


@functools.lru_cache(maxsize=None)
def _default_run(rc):
    """`small` through the host form on the two-strand index, everything listed: what the other forms are compared with"""
    pair = _open(_files("small"))
    try:
        return pair.locate(_small_queries(), rc=rc, max_hits=ALL)
    finally:
        pair.close()


@functools.lru_cache(maxsize=None)
def _expected(rc):
    return lc.expected([s for _, s in lc.small()["reads"]], _small_queries(), rc)


def _triples(hits):
    assert not (hits["flags"] & ~np.uint32(lc.HIT_REV)).any()
    return sorted(zip(hits["read"].tolist(), hits["offset"].tolist(), (hits["flags"] & lc.HIT_REV).tolist()))


def _check_against_brute_force(res, rc, max_hits, what):
    totals, qflags, hit_offs, hits = res
    q = lc.small()["queries"]
    exp = _expected(rc)
    assert len(totals) == len(qflags) == len(q) and len(hit_offs) == len(q) + 1
    assert int(hit_offs[0]) == 0 and int(hit_offs[-1]) == len(hits)
    for i, (name, w, _) in enumerate(q):
        a, b = int(hit_offs[i]), int(hit_offs[i + 1])
        skipped = exp[i] is None
        assert bool(qflags[i] & lc.SKIPPED) == skipped, "%s %s: SKIPPED" % (what, name)
        assert bool(qflags[i] & lc.OVER) == (int(totals[i]) > max_hits), "%s %s: OVER" % (what, name)
        assert not (qflags[i] & ~np.uint32(3))
        if not skipped:
            assert int(totals[i]) == len(exp[i]), "%s %s: total %d, want %d" % (what, name, totals[i], len(exp[i]))
        if qflags[i]:
            assert a == b, "%s %s: hits listed for a flagged query" % (what, name)
            continue
        h = hits[a:b]
        assert (h["query"] == i).all()
        assert _triples(h) == exp[i], "%s %s (%d bases)" % (what, name, len(w))
        rev = (h["flags"] & lc.HIT_REV).astype(bool)
        assert not rev[:np.count_nonzero(~rev)].any(), "%s %s: a reverse hit before a forward one" % (what, name)


@pytest.mark.parametrize("rc", (True, False))
def test_host_form_equals_brute_force(rc):
    res = _default_run(rc)
    _check_against_brute_force(res, rc, ALL, "host form")
    assert not (res[1] & lc.OVER).any()
    pair = _open(_files("small"))
    try:
        head, _ = pair.match(_small_queries(), rc=rc)
    finally:
        pair.close()
    assert np.array_equal(res[0], head)  # every query, the skipped ones too


@pytest.mark.parametrize("rc", (True, False))
def test_max_hits(rc):
    pair = _open(_files("small"))
    try:
        res = pair.locate(_small_queries(), rc=rc, max_hits=5)
    finally:
        pair.close()
    _check_against_brute_force(res, rc, 5, "max_hits 5")
    ref = _default_run(rc)
    assert np.array_equal(res[0], ref[0])
    over = (res[1] & lc.OVER).astype(bool)
    assert np.array_equal(over, ref[0] > 5) and over.any() and not over.all()
    for i in np.nonzero(res[1] == 0)[0]:  # the other queries are unchanged
        assert ref[3][int(ref[2][i]):int(ref[2][i + 1])].tobytes() == res[3][int(res[2][i]):int(res[2][i + 1])].tobytes()


@pytest.mark.parametrize("rc", (False, True))
def test_many_hits_fill_every_slot(rc):
    case = lc.many()
    pair = _open(_files("many"))
    try:
        totals, qflags, hit_offs, hits = pair.locate([s for _, s, _ in case["queries"]], rc=rc, max_hits=ALL)
    finally:
        pair.close()
    assert not qflags.any()
    for i, (name, w, _) in enumerate(case["queries"]):
        want = lc.expected_one_base(case["reads"], w, rc)
        h = hits[int(hit_offs[i]):int(hit_offs[i + 1])]
        assert int(totals[i]) == len(want) == len(h)
        assert (h["query"] == i).all() and not (h["flags"] & ~np.uint32(lc.HIT_REV)).any()
        got = np.stack([h["read"], h["offset"], h["flags"] & lc.HIT_REV], axis=1).astype(np.int64)
        got = got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))]
        assert np.array_equal(got, want), name  # no slot missing, none written twice


def _same_as_default(res, rc, what):
    ref = _default_run(rc)
    for a, b, part in zip(res, ref, ("totals", "qflags", "hit_offs", "hits")):
        assert a.tobytes() == b.tobytes(), "%s: %s differ from the default run's" % (what, part)


@pytest.mark.parametrize("rc", (True, False))
def test_forward_only_index_and_prefix_table(rc):
    """an index opened without the reverse strand, and again once a correction call has left the table of 13-mer intervals"""
    from siga_amd import _lib
    pair = _open(_files("small"), both=False)
    try:
        _same_as_default(pair.locate(_small_queries(), rc=rc, max_hits=ALL), rc, "forward-only index")
        seqs = np.frombuffer(b"ACGTACGTTGCATGCAACGTACGTTGCATGCAACGT", dtype=np.uint8)
        offs = np.array([0, len(seqs)], dtype=np.uint64)
        out, valid = np.zeros(len(seqs), dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        assert _lib.lib().sigax_correct_batch(pair.handle, seqs.tobytes(), None, offs.ctypes.data, 1, 31, 3, 10, 1, out.ctypes.data,
                                              valid.ctypes.data) == 0, _lib.last_error()
        _same_as_default(pair.locate(_small_queries(), rc=rc, max_hits=ALL), rc, "with the prefix table")
    finally:
        pair.close()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import locate_cases as lc
import siga_amd
pair = siga_amd.FMIndexPair.load(%r, device=0, with_sai=True, resident=False)
assert pair.info()["wide"] == %d
%s
for rc in (True, False):
    res = pair.locate([s for _, s, _ in lc.small()["queries"]], rc=rc, max_hits=(1 << 32) - 1)
    np.savez(%r %% int(rc), *res)
pair.close()
"""


# a correction call, which leaves the table of 13-mer intervals on the device
_WITH_TABLE = """
from siga_amd import _lib
seqs = np.frombuffer(b"ACGTACGTTGCATGCAACGTACGTTGCATGCAACGT", dtype=np.uint8)
offs = np.array([0, len(seqs)], dtype=np.uint64)
out, valid = np.zeros(len(seqs), dtype=np.uint8), np.zeros(1, dtype=np.uint8)
assert _lib.lib().sigax_correct_batch(pair.handle, seqs.tobytes(), None, offs.ctypes.data, 1, 31, 3, 10, 1, out.ctypes.data,
                                      valid.ctypes.data) == 0, _lib.last_error()
"""


def _child(env_extra, wide, tmp_path, what, prelude=""):
    out = str(tmp_path / "res%d.npz")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, _files("small"), wide, prelude, out)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rc in (True, False):
        z = np.load(out % int(rc))
        _same_as_default([z["arr_%d" % k] for k in range(4)], rc, what)


def test_without_two_step_tables(tmp_path):
    _child({"SIGAX_TWO_STEP": "0"}, 0, tmp_path, "without two-step tables")


def test_wide_positions_small_superblocks(tmp_path):
    lib = os.path.join(ROOT, "build", "libsigax_super12.so")
    assert os.path.exists(lib)
    _child({"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": lib}, 1, tmp_path, "64-bit positions")


def test_wide_positions_with_prefix_table(tmp_path):
    """the 16-byte entries of the 13-mer table under 64-bit positions (the library's ordinary superblocks)"""
    _child({"SIGAX_FORCE_WIDE": "1"}, 1, tmp_path, "64-bit positions, prefix table", prelude=_WITH_TABLE)


class _Device:
    """device buffers of exactly their size, prefilled with 0xEE, on the HIP runtime the library is bound to"""

    def __init__(self):
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.hip = hip
        self.held = []

    def buf(self, nbytes, src=None):
        q = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(q), max(nbytes, 1)) == 0
        self.held.append(q)
        assert self.hip.hipMemset(q, 0xEE, max(nbytes, 1)) == 0
        if src is not None and src.nbytes:
            assert self.hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        return q

    def get(self, q, dtype, count):
        out = np.zeros(count, dtype=dtype)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data, q, out.nbytes, 2) == 0
        return out

    def free(self):
        for q in self.held:
            self.hip.hipFree(q)


def _locate_on_device(dev, handle, seqs, rc, max_hits, max_len, hits_cap, stream):
    """-> (totals, qflags, hit_offs, hits[hits_cap], rows[hits_cap], status4, d_rows)"""
    from siga_amd import _lib
    L = _lib.lib()
    buf, offs = po.pack_reads(seqs)
    buf = np.frombuffer(buf, dtype=np.uint8)
    n = len(seqs)
    wb = C.c_uint64()
    assert L.sigax_locate_workspace(n, C.byref(wb)) == 0
    d_seqs, d_offs = dev.buf(buf.nbytes, buf), dev.buf(offs.nbytes, offs)
    d_tot, d_qf, d_ho = dev.buf(8 * n), dev.buf(4 * n), dev.buf(8 * (n + 1))
    d_hits, d_rows, d_stat, d_work = dev.buf(16 * hits_cap), dev.buf(8 * hits_cap), dev.buf(32), dev.buf(wb.value)
    assert dev.hip.hipDeviceSynchronize() == 0
    assert L.sigax_locate_device(handle, d_seqs, d_offs, n, 2 if rc else 0, max_hits, max_len, d_tot, d_qf, d_ho, d_hits, d_rows, hits_cap,
                                 d_stat, d_work, wb.value, stream) == 0, _lib.last_error()
    assert dev.hip.hipStreamSynchronize(stream) == 0
    from siga_amd._lib import HIT_DTYPE
    return (dev.get(d_tot, np.uint64, n), dev.get(d_qf, np.uint32, n), dev.get(d_ho, np.uint64, n + 1), dev.get(d_hits, HIT_DTYPE, hits_cap),
            dev.get(d_rows, np.uint64, hits_cap), dev.get(d_stat, np.uint64, 4), d_rows)


def test_device_form():
    """hits_cap one below the need: the counts are complete and no hit, no row is written; exact: the host form's hits, and
    their rows walked by sigax_string_lengths_device end at the same read and offset"""
    from siga_amd import _lib
    L = _lib.lib()
    rc = True
    ref = _default_run(rc)
    need = len(ref[3])
    seqs = _small_queries()
    pair = _open(_files("small"))
    dev = _Device()
    stream = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    try:
        tot, qf, ho, hits, rows, stat, _ = _locate_on_device(dev, pair.handle, seqs, rc, ALL, ALL, need - 1, stream)
        assert np.array_equal(tot, ref[0]) and np.array_equal(qf, ref[1]) and np.array_equal(ho, ref[2])
        assert int(stat[0]) == need and int(stat[1]) == 0 and int(stat[3]) == 0
        assert hits.tobytes() == b"\xee" * (16 * (need - 1)) and rows.tobytes() == b"\xee" * (8 * (need - 1))
        tot, qf, ho, hits, rows, stat, d_rows = _locate_on_device(dev, pair.handle, seqs, rc, ALL, ALL, need, stream)
        assert np.array_equal(tot, ref[0]) and np.array_equal(qf, ref[1]) and np.array_equal(ho, ref[2])
        assert hits.tobytes() == ref[3].tobytes()
        assert int(stat[0]) == need and int(stat[1]) == 0 and int(stat[2]) > need and int(stat[3]) == 0
        d_lens, d_stretch, d_st2 = dev.buf(4 * need), dev.buf(8 * need), dev.buf(16)
        assert L.sigax_string_lengths_device(pair.handle, 0, d_rows, need, ALL, d_lens, d_stretch, d_st2, stream) == 0, _lib.last_error()
        assert dev.hip.hipStreamSynchronize(stream) == 0
        lens, stretch = dev.get(d_lens, np.uint32, need), dev.get(d_stretch, np.uint64, need)
        assert not dev.get(d_st2, np.uint64, 2).any()
        sai = np.array(lc.oracle_index("small").sai(), dtype=np.uint32)
        assert np.array_equal(lens, hits["offset"]) and np.array_equal(sai[stretch.astype(np.int64)], hits["read"])
        for i in range(len(seqs)):  # ascending rows within each chain of a query
            a, b = int(ho[i]), int(ho[i + 1])
            nf = np.count_nonzero(~(hits["flags"][a:b] & lc.HIT_REV).astype(bool))
            for part in (rows[a:a + nf], rows[a + nf:b]):
                assert (np.diff(part.astype(np.int64)) == 1).all()
    finally:
        dev.free()
        L.sigax_stream_destroy(0, stream)
        pair.close()


def test_max_len_cuts_longer_walks():
    ref = _default_run(True)
    pair = _open(_files("small"))
    dev = _Device()
    try:
        tot, qf, ho, hits, rows, stat, _ = _locate_on_device(dev, pair.handle, _small_queries(), True, ALL, 10, len(ref[3]), None)
    finally:
        dev.free()
        pair.close()
    assert np.array_equal(ho, ref[2])
    far = ref[3]["offset"] > 10
    assert far.any() and not far.all()
    cut = (hits["flags"] & lc.HIT_CUT).astype(bool)
    assert np.array_equal(cut, far)
    assert (hits["read"][cut] == ALL).all() and (hits["offset"][cut] == ALL).all()
    assert np.array_equal(hits["query"], ref[3]["query"])
    assert np.array_equal(hits["flags"] & lc.HIT_REV, ref[3]["flags"])
    assert hits[~cut].tobytes() == ref[3][~far].tobytes()
    assert int(stat[0]) == len(hits) and int(stat[1]) == np.count_nonzero(far)


def test_errors():
    import siga_amd
    from siga_amd import _lib
    from tests import test_gpu_match as tgm
    L = _lib.lib()
    offs = np.array([0, 4], dtype=np.uint64)

    def call(pair, n, flags):
        t, f, o, h = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = L.sigax_locate_batch(pair.handle, b"ACGT", offs.ctypes.data, n, flags, 1000, ALL, C.byref(t), C.byref(f), C.byref(o), C.byref(h))
        for p in (t, f, o, h):
            L.sigax_free(p)
        return rc

    pair = _open(_files("small"))
    try:
        assert call(pair, 1, 2) == 0 and call(pair, 1, 0) == 0
        assert call(pair, 0, 2) == 0
        for flags in (4, 1, 3, 8):
            assert call(pair, 1, flags) == _lib.SIGAX_E_ARG
        t = C.c_void_p()
        assert L.sigax_locate_batch(pair.handle, b"ACGT", offs.ctypes.data, 1, 2, 1000, ALL, None, C.byref(t), C.byref(t), C.byref(t)) == _lib.SIGAX_E_ARG
        assert L.sigax_locate_device(pair.handle, None, None, 0, 2, 1000, ALL, None, None, None, None, None, 0, None, None, 0, None) == 0
        assert L.sigax_locate_device(pair.handle, None, None, 1, 2, 1000, ALL, None, None, None, None, None, 0, None, None, 0, None) == _lib.SIGAX_E_ARG
        assert L.sigax_locate_device(pair.handle, None, None, 0, 4, 1000, ALL, None, None, None, None, None, 0, None, None, 0, None) == _lib.SIGAX_E_ARG
    finally:
        pair.close()
    pair = siga_amd.FMIndexPair.load(_files("small"), device=0, with_sai=False, resident=False)  # no .sai table
    try:
        assert call(pair, 1, 2) == _lib.SIGAX_E_STATE and ".sai" in _lib.last_error()
    finally:
        pair.close()
    pair = siga_amd.FMIndexPair.load_forward(_files("small"), device=0, with_sai=False)
    try:
        assert call(pair, 1, 2) == _lib.SIGAX_E_STATE
    finally:
        pair.close()
    prefix, _ = tgm._files(1)  # reads that include `withN`
    assert any("N" in s for _, s in mc.match_case(1)["reads"])
    pair = siga_amd.FMIndexPair.load(prefix, device=0, with_sai=True, resident=False)
    try:
        assert call(pair, 1, 2) == _lib.SIGAX_E_STATE and "ACGT" in _lib.last_error()
    finally:
        pair.close()


# ---- the host class and the command line ----
def _want_text(names_seqs, rc, max_hits=1000):
    seqs = [s for _, s in lc.small()["reads"]]
    exp = lc.expected(seqs, [s for _, s in names_seqs], rc)
    fwd = lc.oracle_index("small")
    totals = [mc.count(fwd, s, rc) for _, s in names_seqs]
    listed = [None if (e is None or t > max_hits) else e for e, t in zip(exp, totals)]
    return lc.text(names_seqs, totals, listed)


def _cli(args, cwd=None):
    from siga_amd import host
    return subprocess.run([host.CLI_PATH, "locate"] + args, capture_output=True, cwd=cwd)


@pytest.mark.parametrize("rc", (True, False))
def test_cli_two_files(rc, tmp_path):
    q = [(n, s) for n, s, _ in lc.small()["queries"] if s]
    prefix = _files("small")
    cut = len(q) // 2
    fa, fq = str(tmp_path / "a.fa"), str(tmp_path / "b.fastq")
    with open(fa, "w") as f:
        f.write(mr.fasta_text(q[:cut]))
    with open(fq, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in q[cut:]))
    r = _cli(["-p", prefix, "--max-hits=100000"] + ([] if rc else ["--no-opposite-strand"]) + ["-t", "4", fa, fq])
    assert r.returncode == 0, r.stderr.decode()
    assert lc.parse_text(r.stdout.decode()) == _want_text(q, rc, 100000)
    r = _cli(["-p", prefix] + ([] if rc else ["--no-opposite-strand"]) + [fq, fa])  # the default --max-hits, the files swapped
    assert r.returncode == 0, r.stderr.decode()
    want = _want_text(q[cut:] + q[:cut], rc, 1000)
    assert any(t > 1000 for t in [int(qt.split("\t")[3]) for qt, _ in want])
    assert lc.parse_text(r.stdout.decode()) == want
    r = _cli(["-p", prefix, "--max-length=10"] + ([] if rc else ["--no-opposite-strand"]) + [fa])
    assert r.returncode == 0, r.stderr.decode()
    got = lc.parse_text(r.stdout.decode())
    full = _want_text(q[:cut], rc, 1000)
    assert [qt for qt, _ in got] == [qt for qt, _ in full]  # cut walks are counted as listed and printed without a place
    for (_, ht), (_, want_ht) in zip(got, full):
        near = sorted(l for l in want_ht if int(l.split("\t")[3]) <= 10)
        assert sorted(l for l in ht if l.split("\t")[2] != "*") == near and len(ht) == len(want_ht)


def test_cli_refuses_what_it_cannot_locate(tmp_path):
    from tests import test_gpu_match as tgm
    prefix, queries = tgm._files(1)
    r = _cli(["-p", prefix, queries])
    assert r.returncode == 255 and r.stdout == b"" and b"ACGT" in r.stderr
    d = str(tmp_path / "nosai")
    os.makedirs(d)
    small = _files("small")
    os.symlink(small + ".bwt", os.path.join(d, "reads.bwt"))
    r = _cli(["-p", os.path.join(d, "reads"), small + ".queries.fa"])
    assert r.returncode == 255 and r.stdout == b"" and b".sai" in r.stderr
    r = _cli(["-p", small])  # no QUERYFILE: the help text, as the other sub-commands
    assert r.returncode == 0 and r.stdout.startswith(b"siga locate [OPTION]") and b"--max-hits" in r.stdout


def test_host_class_in_small_batches(tmp_path):
    """batches of 7 queries: the lines keep the query order over many batches, two of them in flight"""
    from siga_amd import host
    q = [(n, s) for n, s, _ in lc.small()["queries"] if s]
    prefix = _files("small")
    out = str(tmp_path / "out.txt")
    host.locate_files([prefix + ".queries.fa"], prefix, rc=True, max_hits=100000, out=out, batch_queries=7)
    want = _want_text(q, True, 100000)
    assert lc.parse_text(open(out).read()) == want
    host.locate_files([prefix + ".queries.fa", prefix + ".queries.fa"], prefix, rc=False, out=out)
    want = _want_text(q, False, 1000)
    assert lc.parse_text(open(out).read()) == want + want
