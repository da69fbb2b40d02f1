"""The read order of key-sharded edge records on the GPU (csrc/sigax_order.hip): sigax_edges_restore_order, its host form and
sigax_flags_by_read_id against the numpy restatement (siga_amd/sharding.py, itself held against a grouping by hand in
tests/test_restore_order_cases.py) on synthetic records, the refusals with guard words around every buffer, and
OverlapBuilder.overlap_sharded against the one-batch run and the oracle's ASQG -- bytes, not counts."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.fixtures import GOLDEN, fixture, md5_prefix
from tests.test_restore_order_cases import run_layout

pytestmark = pytest.mark.gpu

PAD = 32  # guard bytes (0x5A) on either side of a buffer: keeps its start 16-byte aligned


def _lib():
    from siga_amd import _lib
    return _lib


class Guarded:
    """nbytes of device memory between two stretches of guard words"""

    def __init__(self, nbytes, fill=None):
        self.nbytes = nbytes
        room = (nbytes + 7) // 8 * 8
        self.bytes = torch.full((2 * PAD + room,), 0x5A, dtype=torch.uint8, device="cuda")
        if fill is not None:
            self.bytes[PAD:PAD + nbytes] = torch.from_numpy(np.frombuffer(fill, dtype=np.uint8).copy()).cuda()
        self.ptr = self.bytes.data_ptr() + PAD
        self._inside = self.bytes[PAD:PAD + nbytes].clone()

    def inside(self):
        return self.bytes[PAD:PAD + self.nbytes].cpu().numpy()

    def guards_intact(self):
        b = self.bytes.cpu().numpy()
        return (b[:PAD] == 0x5A).all() and (b[PAD + self.nbytes:] == 0x5A).all()

    def untouched(self):
        return self.guards_intact() and bool(torch.equal(self.bytes[PAD:PAD + self.nbytes], self._inside))


def _workspace(n_edges, n_reads):
    need = C.c_uint64()
    assert _lib().lib().sigax_edges_order_workspace(n_edges, n_reads, C.byref(need)) == 0
    return int(need.value)


def _restore_device(recs, n_reads, with_offs=True):
    """sigax_edges_restore_order on `recs` with guard words around every buffer -> (out, offs or None, status)"""
    L = _lib().lib()
    k = len(recs)
    d_in = Guarded(16 * k, recs.tobytes())
    d_out = Guarded(16 * k)
    d_offs = Guarded(8 * (n_reads + 1)) if with_offs else None
    wb = _workspace(k, n_reads)
    d_work = Guarded(wb)
    d_status = Guarded(16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.sigax_edges_restore_order(0, d_in.ptr, k, n_reads, d_out.ptr, d_offs.ptr if with_offs else None, d_work.ptr, wb, d_status.ptr, st)
    assert rc == 0, _lib().last_error()
    torch.cuda.synchronize()
    assert d_in.untouched()
    for g in (d_out, d_offs, d_work, d_status):
        assert g is None or g.guards_intact()
    out = d_out.inside().view(_lib().EDGE_DTYPE)
    offs = d_offs.inside().view(np.uint64) if with_offs else None
    return out, offs, d_status.inside().view(np.uint64).tolist()


def _restore_host(recs, n_reads, with_offs=True):
    L = _lib().lib()
    recs = np.ascontiguousarray(recs)
    out = np.zeros(len(recs), dtype=_lib().EDGE_DTYPE)
    offs = np.full(n_reads + 1, 77, dtype=np.uint64)
    rc = L.sigax_edges_restore_order_host(0, recs.ctypes.data, len(recs), n_reads, out.ctypes.data, offs.ctypes.data if with_offs else None)
    return rc, out, offs


LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025]


def _lengths_for(n_reads):
    # many queries absent; the long runs thinned out where there are many reads, so that a case stays a few MB
    return [0] * 6 + [1, 1, 2, 2] + LENGTHS if n_reads <= 1000 else [0] * 400 + [1] * 200 + [2] * 100 + LENGTHS


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 257, 1000, 70001])
def test_synthetic_records_against_the_restatement(n_reads):
    from siga_amd.sharding import restore_order
    for seed, last_present in ((0, True), (1, False)):
        ordered, shuffled, _, starts = run_layout(n_reads, _lengths_for(n_reads), seed, last_present)
        if len(shuffled) == 0:
            continue
        want, want_offs = restore_order(shuffled, n_reads)  # the numpy restatement
        assert want.tobytes() == ordered.tobytes() and np.array_equal(want_offs, starts)
        out, offs, status = _restore_device(shuffled, n_reads)
        assert status == [0, 0]
        assert out.tobytes() == want.tobytes() and np.array_equal(offs, want_offs)
        rc, out, offs = _restore_host(shuffled, n_reads)
        assert rc == 0, _lib().last_error()
        assert out.tobytes() == want.tobytes() and np.array_equal(offs, want_offs)
        if seed:
            continue
        # the Python entry point on the device: arrays in, arrays out; a tensor in, tensors out
        got, offs = restore_order(shuffled, n_reads, device="cuda")
        assert got.tobytes() == want.tobytes() and offs.dtype == np.uint64 and np.array_equal(offs, want_offs)
        t = torch.from_numpy(shuffled.view(np.int32).reshape(-1, 4).copy()).cuda()
        got_t, offs_t = restore_order(t, n_reads)
        assert got_t.is_cuda and got_t.cpu().numpy().tobytes() == want.tobytes() and offs_t.cpu().tolist() == want_offs.tolist()


def test_no_records_no_offsets_and_one_run():
    L = _lib().lib()
    # n_edges = 0: d_query_offs all zeros, status zeros, buffers may be missing
    d_offs, d_status = Guarded(8 * 11), Guarded(16)
    assert L.sigax_edges_restore_order(0, None, 0, 10, None, d_offs.ptr, None, 0, d_status.ptr, None) == 0, _lib().last_error()
    torch.cuda.synchronize()
    assert not d_offs.inside().any() and not d_status.inside().any() and d_offs.guards_intact() and d_status.guards_intact()
    rc, out, offs = _restore_host(np.zeros(0, dtype=_lib().EDGE_DTYPE), 10)
    assert rc == 0 and not offs.any()
    # d_query_offs = NULL
    ordered, shuffled, _, _ = run_layout(300, [0, 1, 2, 65], 3)
    out, offs, status = _restore_device(shuffled, 300, with_offs=False)
    assert status == [0, 0] and offs is None and out.tobytes() == ordered.tobytes()
    rc, out, _ = _restore_host(shuffled, 300, with_offs=False)
    assert rc == 0 and out.tobytes() == ordered.tobytes()
    # one run that is the whole list, of the last read
    one = np.zeros(3000, dtype=_lib().EDGE_DTYPE)
    one["query"] = 4
    one["target"] = np.arange(3000)
    out, offs, status = _restore_device(one, 5)
    assert status == [0, 0] and out.tobytes() == one.tobytes() and offs.tolist() == [0, 0, 0, 0, 0, 3000]


def test_refusals_are_counted_or_coded_and_stay_inside_the_buffers():
    """None of these may fault: they are argument errors the kernels survive by construction (bounds checked before every
    table access and every store)."""
    from siga_amd.sharding import restore_order
    lib = _lib()
    L = lib.lib()
    n = 500
    ordered, shuffled, _, _ = run_layout(n, [0, 1, 2, 63, 64, 65, 257], 5)
    k = len(shuffled)
    # one record with query == n_reads
    beyond = shuffled.copy()
    beyond["query"][k // 2] = n
    _, _, status = _restore_device(beyond, n)
    assert status[0] == 1
    rc, _, _ = _restore_host(beyond, n)
    assert rc == lib.SIGAX_E_ARG and "beyond" in lib.last_error()
    with pytest.raises(ValueError, match="beyond"):
        restore_order(beyond, n, device="cuda")
    # n_reads = 0 with records: every record is out of range
    _, _, status = _restore_device(shuffled[:100], 0)
    assert status == [100, 0]
    # one query whose run is split in two
    q = shuffled["query"][0]
    run = shuffled[shuffled["query"] == q]
    split = np.concatenate([shuffled, run[:1]])
    assert split["query"][-2] != q
    _, _, status = _restore_device(split, n)
    assert status == [0, 1]
    rc, _, _ = _restore_host(split, n)
    assert rc == lib.SIGAX_E_ARG and "runs beyond the first" in lib.last_error()
    with pytest.raises(ValueError, match="runs beyond the first"):
        restore_order(split, n, device="cuda")
    # argument errors: codes, and nothing written
    d_in, d_out, d_offs, d_status = Guarded(16 * k, shuffled.tobytes()), Guarded(16 * k), Guarded(8 * (n + 1)), Guarded(16)
    wb = _workspace(k, n)
    d_work = Guarded(wb)
    bad_calls = [
        (d_in.ptr, d_in.ptr, d_work.ptr, wb, d_status.ptr),           # d_out aliasing d_in
        (d_in.ptr, d_in.ptr + 16 * (k - 1), d_work.ptr, wb, d_status.ptr),  # ... overlapping its last record
        (d_in.ptr, d_out.ptr, d_work.ptr, wb - 1, d_status.ptr),      # a workspace one byte short
        (None, d_out.ptr, d_work.ptr, wb, d_status.ptr),              # NULL buffers
        (d_in.ptr, None, d_work.ptr, wb, d_status.ptr),
        (d_in.ptr, d_out.ptr, None, wb, d_status.ptr),
        (d_in.ptr, d_out.ptr, d_work.ptr, wb, None),
    ]
    for a_in, a_out, a_work, a_wb, a_status in bad_calls:
        assert L.sigax_edges_restore_order(0, a_in, k, n, a_out, d_offs.ptr, a_work, a_wb, a_status, None) == lib.SIGAX_E_ARG
    torch.cuda.synchronize()
    for g in (d_in, d_out, d_offs, d_work, d_status):
        assert g.untouched()
    out = np.zeros(k, dtype=lib.EDGE_DTYPE)
    assert L.sigax_edges_restore_order_host(0, shuffled.ctypes.data, k, n, shuffled.ctypes.data, None) == lib.SIGAX_E_ARG
    assert L.sigax_edges_restore_order_host(0, None, k, n, out.ctypes.data, None) == lib.SIGAX_E_ARG
    assert L.sigax_flags_by_read_id(0, None, d_in.ptr, 5, 10, d_out.ptr, d_status.ptr, None) == lib.SIGAX_E_ARG
    assert L.sigax_flags_by_read_id(0, d_in.ptr, d_in.ptr, 5, 10, d_out.ptr, None, None) == lib.SIGAX_E_ARG


def test_flags_by_read_id():
    from siga_amd.sharding import flags_by_read_id
    L = _lib().lib()
    rng = np.random.default_rng(9)
    n = 70001

    def scatter(flags, ids, n_reads):
        d_flags, d_ids = Guarded(len(flags), flags.tobytes()), Guarded(4 * len(ids), ids.tobytes())
        d_out, d_status = Guarded(n_reads, bytes([9]) * n_reads), Guarded(8)
        rc = L.sigax_flags_by_read_id(0, d_flags.ptr, d_ids.ptr, len(ids), n_reads, d_out.ptr, d_status.ptr, None)
        assert rc == 0, _lib().last_error()
        torch.cuda.synchronize()
        assert d_flags.untouched() and d_ids.untouched() and d_out.guards_intact() and d_status.guards_intact()
        return d_out.inside().copy(), int(d_status.inside().view(np.uint64)[0])

    # a random permutation
    ids = rng.permutation(n).astype(np.uint32)
    flags = rng.integers(0, 2, size=n).astype(np.uint8)
    out, beyond = scatter(flags, ids, n)
    want = np.zeros(n, dtype=np.uint8)
    want[ids] = flags
    assert beyond == 0 and np.array_equal(out, want)
    assert np.array_equal(flags_by_read_id(flags, ids, n, device="cuda"), want)
    assert np.array_equal(flags_by_read_id(flags, ids, n), want)
    # a strict subset: the other positions keep their value
    sub = ids[:1000]
    out, beyond = scatter(flags[:1000], sub, n)
    want = np.full(n, 9, dtype=np.uint8)
    want[sub] = flags[:1000]
    assert beyond == 0 and np.array_equal(out, want)
    # one id out of range: counted, not written
    bad = sub.copy()
    bad[500] = n
    out, beyond = scatter(flags[:1000], bad, n)
    want[sub[500]] = 9
    assert beyond == 1 and np.array_equal(out, want)
    with pytest.raises(ValueError, match="beyond"):
        flags_by_read_id(flags[:1000], bad, n, device="cuda")
    # no reads at all
    d_status = Guarded(8)
    assert L.sigax_flags_by_read_id(0, None, None, 0, 0, None, d_status.ptr, None) == 0
    torch.cuda.synchronize()
    assert not d_status.inside().any()


_ONE_BATCH = {}


def _one_batch(name):
    """the index with its reads set and the one-batch run at m = 45, irreducible + rc: computed once, never changed"""
    if name not in _ONE_BATCH:
        import siga_amd
        from siga_amd.overlap import name_ranks, read_sequences
        fx = fixture(name)
        reads = read_sequences(fx.fa)
        seqs = [r[2] for r in reads]
        pair = siga_amd.FMIndexPair.load(fx.prefix)
        pair.set_reads(np.array([len(s) for s in seqs], dtype=np.uint32), name_ranks([r[0] for r in reads]))
        builder = siga_amd.OverlapBuilder(pair, fx.prefix)
        res = builder.overlap(seqs, 45, edges=True)
        want_asqg, _, _ = fx.oracle_asqg(45)
        _ONE_BATCH[name] = (fx, reads, seqs, builder, res, want_asqg)
    return _ONE_BATCH[name]


def _shards(name, seqs, n_shards):
    from siga_amd.sharding import key_order, locality_keys
    if name == "ragged":  # mixed lengths: no key matrix, a seeded random permutation instead
        order = np.random.default_rng(17).permutation(len(seqs))
    else:
        order = key_order(locality_keys(np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), -1)))
    return np.array_split(order, n_shards)


@pytest.mark.parametrize("n_shards", [2, 3])
@pytest.mark.parametrize("name", ["toy", "ragged", "deep"])
def test_overlap_sharded_gives_the_one_batch_bytes(name, n_shards):
    from siga_amd.overlap import format_asqg
    fx, reads, seqs, builder, one, want_asqg = _one_batch(name)
    shards = _shards(name, seqs, n_shards)
    assert not np.array_equal(np.concatenate(shards), np.arange(len(seqs)))
    res = builder.overlap_sharded(seqs, 45, shards)
    edges, substring = res
    assert len(one["edges"]) > 0 and edges.dtype == one["edges"].dtype
    assert edges.tobytes() == one["edges"].tobytes()
    assert substring.tobytes() == one["substring"].tobytes()
    text = format_asqg(reads, res, 45)
    assert text == want_asqg
    if name == "toy":
        assert GOLDEN["toy"]["min_overlap"] == 45 and md5_prefix(text) == GOLDEN["toy"]["md5"]["asqg_t1"]
    # the order in which the shards' records are concatenated does not matter
    back = builder.overlap_sharded(seqs, 45, shards[::-1])
    assert back["edges"].tobytes() == one["edges"].tobytes() and back["substring"].tobytes() == one["substring"].tobytes()


def test_overlap_sharded_refuses_shards_that_are_no_partition():
    fx, reads, seqs, builder, one, _ = _one_batch("toy")
    n = len(seqs)
    with pytest.raises(ValueError, match="exactly once"):
        builder.overlap_sharded(seqs, 45, [np.arange(n - 1)])
    with pytest.raises(ValueError, match="exactly once"):
        builder.overlap_sharded(seqs, 45, [np.arange(n), np.array([0])])


def test_gather_with_one_rank_then_restore():
    """sigax_gather_edges with a communicator of one rank, as in test_rccl_exchange_step_with_one_rank, followed by
    sigax_edges_restore_order on the gathered list of shuffled shards."""
    lib = _lib()
    L = lib.lib()
    idb = (C.c_uint8 * 128)()
    if L.sigax_comm_unique_id(idb) != 0:
        pytest.skip("RCCL cannot be bound: " + lib.last_error())
    comm = C.c_void_p()
    assert L.sigax_comm_create(0, 0, 1, idb, C.byref(comm)) == 0, lib.last_error()
    try:
        n = 5000
        ordered, shuffled, _, starts = run_layout(n, [0, 0, 1, 1, 2, 65, 257], 11)
        k = len(shuffled)
        d_local = torch.from_numpy(shuffled.view(np.int32).reshape(-1, 4).copy()).cuda()
        d_all = torch.zeros((k, 4), dtype=torch.int32, device="cuda")
        cnt = (C.c_uint64 * 1)()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.sigax_gather_counts(comm, k, cnt, st) == 0, lib.last_error()
        assert int(cnt[0]) == k
        assert L.sigax_gather_edges(comm, C.c_void_p(d_local.data_ptr()), cnt, 0, C.c_void_p(d_all.data_ptr()), st) == 0, lib.last_error()
        d_out = torch.zeros_like(d_all)
        d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        wb = _workspace(k, n)
        d_work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        d_status = torch.ones(2, dtype=torch.int64, device="cuda")
        assert L.sigax_edges_restore_order(0, d_all.data_ptr(), k, n, d_out.data_ptr(), d_offs.data_ptr(), d_work.data_ptr(), wb,
                                           d_status.data_ptr(), st) == 0, lib.last_error()
        torch.cuda.synchronize()
        assert d_status.tolist() == [0, 0]
        assert d_out.cpu().numpy().tobytes() == ordered.tobytes()
        assert np.array_equal(d_offs.cpu().numpy().astype(np.uint64), starts)
    finally:
        L.sigax_comm_destroy(comm)
