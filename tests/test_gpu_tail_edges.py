"""The overlap tail: a run with SIGAX_EDGES makes its edge records from the blocks as filter/extract left them (stage pass,
scan, emit pass) and orders the 80-byte blocks only when they are asked for (sigax_batch_download, sigax_batch_device_outputs
with d_blocks); the scans are two launches whose second sums the partials itself; k_fx_route queues wide items through LDS.

Expected values come from the oracle: blocks from pyoracle.overlap_batch, edge records from tests.bigcheck.expected_edges (the
numpy restatement of Hit2OverlapConverter::convert) over the oracle's blocks with the fixture's .sai tables."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.fixtures import CACHE, ROOT, fixture

pytestmark = pytest.mark.gpu

# fixture -> min-overlap (those of tests/test_gpu_parity.py)
MINOV = {"toy": 45, "dup": 8, "rep": 10, "ragged": 15, "deep": 30}
_PAIRS = {}
_WANT = {}


class _Reads:
    """what a case needs of a read set: sequences, lengths, name ranks, the oracle's two indexes"""

    def __init__(self, names, seqs, fwd, rev, prefix):
        from siga_amd.overlap import name_ranks
        self.seqs = seqs
        self.lens = np.array([len(s) for s in seqs], dtype=np.uint32)
        self.ranks = name_ranks(names)
        self.fwd, self.rev, self.prefix = fwd, rev, prefix
        self.sai, self.rsai = fwd.sai(), rev.sai()


def _reads_of(name):
    fx = fixture(name)
    return _Reads([n for n, _ in fx.reads], fx.seqs, fx.fwd, fx.rev, fx.prefix)


def _pair(key, rd):
    """one resident index per read set for the whole module"""
    import siga_amd
    if key not in _PAIRS:
        pair = siga_amd.FMIndexPair.load(rd.prefix)
        pair.set_reads(rd.lens, rd.ranks)
        _PAIRS[key] = pair
    return _PAIRS[key]


def _want(key, rd, m, irr, dup, lo, hi):
    """the oracle's blocks of reads [lo, hi) and the edge records that follow from them; asked once per case"""
    from oracle import pyoracle as po
    from tests.bigcheck import expected_edges
    k = (key, m, irr, dup, lo, hi)
    if k not in _WANT:
        w = po.overlap_batch(rd.fwd, rd.rev, rd.seqs[lo:hi], 0 if dup else m, irreducible=irr, duplicate=dup)
        w["edges"] = expected_edges(w["blocks"], w["block_offs"], rd.sai, rd.rsai, rd.lens, rd.ranks, read_base=lo)
        _WANT[k] = w
    return _WANT[k]


def _d2h(ptr, dtype, count):
    """count records at a device pointer of the library's -> numpy (through the HIP runtime the library is bound to)"""
    from siga_amd import _lib
    hip = _lib.lib()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(count, dtype=dtype)
    if out.nbytes:
        assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # device to host
    return out


def _download(L, bt):
    from siga_amd import _lib
    from siga_amd.overlap import BLOCK_DTYPE, EDGE_DTYPE, _copy_records
    res = _lib.Result()
    assert L.sigax_batch_download(bt, C.byref(res)) == 0, _lib.last_error()
    try:
        n = res.n_reads
        offs = np.ctypeslib.as_array(res.block_offs, shape=(n + 1,)).copy()
        blocks = _copy_records(res.blocks, int(offs[-1]), BLOCK_DTYPE)
        sub = np.ctypeslib.as_array(res.substring, shape=(max(n, 1),))[:n].copy()
        eds = _copy_records(res.edges, int(res.n_edges), EDGE_DTYPE)
    finally:
        L.sigax_result_free(C.byref(res))
    return offs, blocks, sub, eds


def _check_blocks(offs, blocks, sub, want, what):
    from tests.bigcheck import blocks_matrix
    assert np.array_equal(offs, want["block_offs"]), what + ": block_offs differ"
    got = blocks_matrix(blocks)
    if not np.array_equal(got, want["blocks"]):
        bad = np.nonzero((got != want["blocks"]).any(axis=1))[0]
        raise AssertionError("%s: %d of %d blocks differ; first: block %d\n got  %s\n want %s" % (
            what, len(bad), len(got), bad[0], got[bad[0]], want["blocks"][bad[0]]))
    assert np.array_equal(sub.astype(bool), want["substring"].astype(bool)), what + ": substring flags differ"


def _check_edges(eds, want, what):
    from tests.bigcheck import edges_matrix
    got = edges_matrix(eds) if len(eds) else np.zeros((0, 4), dtype=np.uint32)
    exp = want["edges"]
    assert len(got) == len(exp), "%s: %d edge records, the oracle's blocks give %d" % (what, len(got), len(exp))
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        raise AssertionError("%s: %d of %d edge records differ; first: record %d\n got  %s\n want %s" % (
            what, len(bad), len(got), bad[0], got[bad[0]], exp[bad[0]]))


def _edges_then_blocks(L, bt, rd, lo, hi, m, flags, want, what):
    """one run of the batch object over reads [lo, hi): (a) edges before anything asks for blocks, (b) download, (c) the
    device blocks asked for twice"""
    from siga_amd import _lib
    from siga_amd.overlap import BLOCK_DTYPE, EDGE_DTYPE, pack_reads
    part = rd.seqs[lo:hi]
    buf, offs = pack_reads(part)
    assert L.sigax_batch_upload(bt, buf, offs.ctypes.data, len(part), None) == 0, _lib.last_error()
    assert L.sigax_batch_run(bt, lo, m, flags, None) == 0, _lib.last_error()
    stats = _lib.Stats()
    assert L.sigax_batch_finish(bt, None, C.byref(stats)) == 0, _lib.last_error()
    assert stats.n_blocks == len(want["blocks"]), what
    # (a) substring flags and edge records straight from the device, the blocks not asked for
    p_sub, p_edges = C.c_void_p(), C.c_void_p()
    assert L.sigax_batch_device_outputs(bt, None, None, C.byref(p_sub), C.byref(p_edges)) == 0, _lib.last_error()
    assert stats.n_edges == len(want["edges"]), "%s: %d edge records, the oracle's blocks give %d" % (what, stats.n_edges, len(want["edges"]))
    _check_edges(_d2h(p_edges, EDGE_DTYPE, int(stats.n_edges)), want, what + " (a)")
    assert np.array_equal(_d2h(p_sub, np.uint8, len(part)).astype(bool), want["substring"].astype(bool)), what + " (a): substring flags differ"
    # (b) everything through the download
    boffs, blocks, sub, eds = _download(L, bt)
    _check_blocks(boffs, blocks, sub, want, what + " (b)")
    _check_edges(eds, want, what + " (b)")
    # (c) the ordered blocks on the device: same pointer, same bytes, both times; the edge records are still there
    seen = []
    for _ in range(2):
        p_blocks, p_offs, p_edges2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert L.sigax_batch_device_outputs(bt, C.byref(p_blocks), C.byref(p_offs), None, C.byref(p_edges2)) == 0, _lib.last_error()
        assert p_edges2.value == p_edges.value
        seen.append((p_blocks.value, _d2h(p_blocks, BLOCK_DTYPE, len(blocks)).tobytes(), _d2h(p_offs, np.uint64, len(part) + 1).tobytes()))
    assert seen[0][0] == seen[1][0], what + " (c): the blocks moved"
    assert seen[0][1] == seen[1][1] == blocks.tobytes(), what + " (c): device blocks differ from the downloaded ones"
    assert seen[0][2] == seen[1][2] == boffs.tobytes(), what + " (c): block_offs differ"
    _check_edges(_d2h(p_edges, EDGE_DTYPE, int(stats.n_edges)), want, what + " (c)")


def _blocks_after_edges(key, rd, m, irr, dup=False):
    from siga_amd import _lib
    from siga_amd.overlap import pack_reads
    L = _lib.lib()
    pair = _pair(key, rd)
    n = len(rd.seqs)
    if dup:
        flags = _lib.SIGAX_DUPLICATE | _lib.SIGAX_EDGES
    else:
        flags = (_lib.SIGAX_IRREDUCIBLE if irr else 0) | _lib.SIGAX_RC | _lib.SIGAX_EDGES
        pair.prepare_overlap(m)
    bt = C.c_void_p()
    assert L.sigax_batch_create(pair.handle, n, sum(len(s) for s in rd.seqs), int(rd.lens.max()), C.byref(bt)) == 0, _lib.last_error()
    try:
        what = "%s m=%d irr=%d dup=%d" % (key, m, irr, dup)
        _edges_then_blocks(L, bt, rd, 0, n, m, flags, _want(key, rd, m, irr, dup, 0, n), what + " all reads")
        # (d) the same batch object again on another slice of the reads: edges first, blocks after
        lo, hi = n // 3, n - n // 5
        _edges_then_blocks(L, bt, rd, lo, hi, m, flags, _want(key, rd, m, irr, dup, lo, hi), what + " reads %d..%d" % (lo, hi))
        # and one run without SIGAX_EDGES: the blocks are its result and are ordered in the run
        buf, offs = pack_reads(rd.seqs)
        assert L.sigax_batch_upload(bt, buf, offs.ctypes.data, n, None) == 0, _lib.last_error()
        assert L.sigax_batch_run(bt, 0, m, flags & ~_lib.SIGAX_EDGES, None) == 0, _lib.last_error()
        stats = _lib.Stats()
        assert L.sigax_batch_finish(bt, None, C.byref(stats)) == 0, _lib.last_error()
        boffs, blocks, sub, eds = _download(L, bt)
        _check_blocks(boffs, blocks, sub, _want(key, rd, m, irr, dup, 0, n), what + " without SIGAX_EDGES")
        assert len(eds) == 0 and stats.n_edges == 0
    finally:
        L.sigax_batch_destroy(bt)


@pytest.mark.parametrize("irr", [True, False], ids=["irreducible", "exhaustive"])
@pytest.mark.parametrize("name", ["toy", "dup", "rep", "ragged", "deep"])
def test_blocks_after_edges(name, irr):
    """Edge records first, ordered blocks when asked, twice, again on another slice, and a run without edge records."""
    _blocks_after_edges(name, _reads_of(name), MINOV[name], irr)


def test_blocks_after_edges_duplicate_mode():
    """SIGAX_DUPLICATE | SIGAX_EDGES on `dup`: blocks whose range holds several targets (the stage pass leaves them to the
    emit pass's walk) beside blocks with one."""
    rd = _reads_of("dup")
    want = _want("dup", rd, 0, True, True, 0, len(rd.seqs))
    multi = want["blocks"][:, 1] > want["blocks"][:, 0]
    assert multi.any() and not multi.all() and len(want["edges"]) > 0  # the fixture is what the case is meant for
    _blocks_after_edges("dup", rd, 0, True, dup=True)


def test_equal_names_make_no_edge():
    """reads that share a name (query.name != target.name, src/overlap_builder.cpp:358): `dup` with every third read named as
    its neighbour, in single-target and multi-target ranges alike"""
    fx = fixture("dup")
    names = [n for n, _ in fx.reads]
    for i in range(0, len(names) - 1, 3):
        names[i + 1] = names[i]
    rd = _Reads(names, fx.seqs, fx.fwd, fx.rev, fx.prefix)
    plain = _want("dup", _reads_of("dup"), MINOV["dup"], True, False, 0, len(names))
    renamed = _want("dup_names", rd, MINOV["dup"], True, False, 0, len(names))
    assert not np.array_equal(renamed["edges"], plain["edges"])  # the names matter to this fixture's records
    _blocks_after_edges("dup_names", rd, MINOV["dup"], True)
    _blocks_after_edges("dup_names", rd, 0, True, dup=True)


def test_growing_arenas():
    """Tiny first sizes for the final-block arena and the edge buffer: the overflowing run stays inside its buffers (staged
    records included), sigax_batch_finish grows them and repeats the run, and the repeated run's edges and blocks -- ordered
    after the repeat -- are the oracle's."""
    env = dict(os.environ, SIGAX_TEST_FIN_CAP="64", SIGAX_TEST_EDGE_CAP="16")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", os.path.join(ROOT, "tests", "test_gpu_tail_edges.py"),
                        "-k", "test_blocks_after_edges and (toy or dup or rep)"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "7 passed" in r.stdout, r.stdout[-1000:]  # three fixtures x two modes + the duplicate-mode case


def test_wide_and_narrow_items_in_one_sub_batch():
    """4000 x 100 bp from 2.5 kb (160x: every item has more blocks than a 32-lane group holds) followed by 2400 x 100 bp from
    20 kb (12x: none has): whole workgroup tiles of the route kernel are all wide, others hold no wide item, and the flushes
    of its LDS buffer fall inside the run of wide tiles.  All blocks and edges against the oracle."""
    from oracle import pyoracle as po
    from tests.golden import make_reads as mr
    reads = mr.survey_reads(2500, 100, 4000, 21) + [("s%d" % i, s) for i, (_, s) in enumerate(mr.survey_reads(20000, 100, 2400, 22))]
    d = os.path.join(CACHE, "tail_mix")
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "tail_mix")
    seqs = [s for _, s in reads]
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai")):
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
    fwd, rev = po.Index.load(prefix + ".bwt", prefix + ".sai"), po.Index.load(prefix + ".rbwt", prefix + ".rsai")
    rd = _Reads([n for n, _ in reads], seqs, fwd, rev, prefix)
    want = _want("tail_mix", rd, 45, True, False, 0, len(seqs))
    from siga_amd import _lib
    L = _lib.lib()
    pair = _pair("tail_mix", rd)
    pair.prepare_overlap(45)
    bt = C.c_void_p()
    assert L.sigax_batch_create(pair.handle, len(seqs), 100 * len(seqs), 100, C.byref(bt)) == 0, _lib.last_error()
    try:
        flags = _lib.SIGAX_IRREDUCIBLE | _lib.SIGAX_RC | _lib.SIGAX_EDGES
        _edges_then_blocks(L, bt, rd, 0, len(seqs), 45, flags, want, "tail_mix")
    finally:
        L.sigax_batch_destroy(bt)


def test_scan_across_more_than_256_partials():
    """300 000 x 60 bp reads from 600 kb: 600 000 (read, side) items, more than 256 x 2048 -- a scan workgroup sums more
    partials than it has threads, and the total is written by a workgroup that is not the first.  Index built on the GPU;
    tests.test_gpu_configs._big_case checks the whole batch: edge records == expected_edges over the GPU's blocks, the
    blocks of a seeded sample of 2000 reads == the oracle's, idempotence, invariance under re-sharding, self-containment
    blocks, dedup rule and order of the edge records."""
    from tests.test_gpu_configs import _big_case
    N, L = 300000, 60
    assert 2 * N > 256 * 2048
    info = _big_case("tail_scan", N, 600000, L, 7, world=1, sample=2000, M=30)
    assert info["n_symbols"] == N * (L + 1) and info["wide"] == 0
