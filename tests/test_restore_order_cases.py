"""The read order of key-sharded edge records, on the CPU: the numpy restatement of csrc/sigax_order.hip
(siga_amd/sharding.py::restore_order, what tests/test_gpu_restore_order.py holds the kernels against) against a grouping made
by hand, its two refusals, flags_by_read_id, the new calls in the bindings and the header, and gather_edges(..., n_reads=n)
through a gloo world of two."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from siga_amd import _lib
from siga_amd._lib import EDGE_DTYPE
from tests.fixtures import ROOT

NEW_CALLS = ["sigax_edges_order_workspace", "sigax_edges_restore_order", "sigax_edges_restore_order_host", "sigax_flags_by_read_id"]


def run_layout(n_reads, lengths, seed, last_present=None):
    """Records of a one-batch run over n_reads reads whose runs have lengths drawn from `lengths` (0 = a read without
    records): (the list in read order, the same runs in shuffled order, the shuffled order of the queries that have records).
    target/length/af number the records, so that any two differ and a run's inner order shows."""
    rng = np.random.default_rng(seed)
    cnt = rng.choice(np.asarray(lengths, dtype=np.int64), size=n_reads)
    if last_present is not None and n_reads:
        cnt[-1] = (max(lengths) or 1) if last_present else 0
    ordered = np.zeros(int(cnt.sum()), dtype=EDGE_DTYPE)
    ordered["query"] = np.repeat(np.arange(n_reads, dtype=np.uint32), cnt)
    ordered["target"] = np.arange(len(ordered), dtype=np.uint32) * 7 + 1
    ordered["length"] = np.arange(len(ordered), dtype=np.uint32) % 101 + 45
    ordered["af"] = np.arange(len(ordered), dtype=np.uint32) % 8
    starts = np.zeros(n_reads + 1, dtype=np.int64)
    starts[1:] = np.cumsum(cnt)
    queries = rng.permutation(np.flatnonzero(cnt))
    parts = [ordered[starts[q]:starts[q + 1]] for q in queries]
    shuffled = np.concatenate(parts) if parts else ordered[:0].copy()
    return ordered, shuffled, queries, starts.astype(np.uint64)


def group_by_hand(shuffled, n_reads):
    """stable grouping by query, record by record"""
    bins = [[] for _ in range(n_reads)]
    for e in shuffled:
        bins[int(e["query"])].append(e)
    flat = [e for b in bins for e in b]
    offs = np.zeros(n_reads + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(b) for b in bins])
    out = np.array(flat, dtype=EDGE_DTYPE) if flat else np.zeros(0, dtype=EDGE_DTYPE)
    return out, offs


@pytest.mark.parametrize("n_reads,lengths", [(1, [3]), (1, [0]), (7, [0, 1, 2]), (65, [0, 0, 1, 5]), (300, [0, 1, 2, 63, 64, 65]), (40, [1])])
def test_restatement_is_the_stable_grouping(n_reads, lengths):
    from siga_amd.sharding import restore_order
    for seed in range(3):
        ordered, shuffled, _, starts = run_layout(n_reads, lengths, seed)
        want, want_offs = group_by_hand(shuffled, n_reads)
        assert want.tobytes() == ordered.tobytes() and np.array_equal(want_offs, starts)
        got, offs = restore_order(shuffled, n_reads)
        assert got.dtype == EDGE_DTYPE and got.tobytes() == want.tobytes()
        assert offs.dtype == np.uint64 and offs.shape == (n_reads + 1,) and np.array_equal(offs, want_offs)
        # the tensor form gather_edges returns
        t = torch.from_numpy(shuffled.view(np.int32).reshape(-1, 4).copy())
        got_t, offs_t = restore_order(t, n_reads)
        assert got_t.dtype == torch.int32 and got_t.numpy().tobytes() == want.tobytes()
        assert offs_t.dtype == torch.int64 and offs_t.tolist() == want_offs.tolist()


def test_restatement_of_nothing():
    from siga_amd.sharding import restore_order
    got, offs = restore_order(np.zeros(0, dtype=EDGE_DTYPE), 5)
    assert len(got) == 0 and offs.tolist() == [0] * 6
    got, offs = restore_order(np.zeros(0, dtype=EDGE_DTYPE), 0)
    assert len(got) == 0 and offs.tolist() == [0]


def test_both_refusals_raise():
    from siga_amd.sharding import restore_order
    _, shuffled, _, _ = run_layout(50, [0, 1, 2, 3], 1)
    beyond = shuffled.copy()
    beyond["query"][len(beyond) // 2] = 50
    with pytest.raises(ValueError, match="beyond"):
        restore_order(beyond, 50)
    with pytest.raises(ValueError, match="beyond"):
        restore_order(shuffled[:1], 0)
    q = shuffled["query"][0]
    run = shuffled[shuffled["query"] == q]
    split = np.concatenate([shuffled, run[:1]])  # the first query's run comes back at the end of the list
    assert split["query"][-2] != q
    with pytest.raises(ValueError, match="runs beyond the first"):
        restore_order(split, 50)
    with pytest.raises(ValueError, match="runs beyond the first"):
        restore_order(torch.from_numpy(split.view(np.int32).reshape(-1, 4).copy()), 50)


def test_flags_by_read_id_scatters():
    from siga_amd.sharding import flags_by_read_id
    rng = np.random.default_rng(2)
    ids = rng.permutation(100)[:37].astype(np.uint32)
    flags = rng.integers(1, 4, size=37).astype(np.uint8)
    out = flags_by_read_id(flags, ids, 100)
    assert out.dtype == np.uint8 and out.shape == (100,)
    want = np.zeros(100, dtype=np.uint8)
    for r in range(37):
        want[ids[r]] = flags[r]
    assert np.array_equal(out, want)
    bad = ids.copy()
    bad[5] = 100
    with pytest.raises(ValueError, match="beyond"):
        flags_by_read_id(flags, bad, 100)


def test_new_calls_are_bound_and_declared():
    header = open(os.path.join(ROOT, "include", "sigax.h")).read()
    for name in NEW_CALLS:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
    # ... and the library exports them with the rest
    L = _lib.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name), name
    need = (_lib.C.c_uint64 * 1)()
    assert L.sigax_edges_order_workspace(1000, 100, need) == 0 and need[0] >= 100 * 8  # host arithmetic: no device touched
    assert L.sigax_edges_order_workspace(1000, 100, None) == _lib.SIGAX_E_ARG


def _shares(n_reads, seed):
    """a synthetic record list split into two ranks by a random permutation of its queries"""
    ordered, _, _, _ = run_layout(n_reads, [0, 1, 2, 5], seed)
    side = np.random.default_rng(seed + 1).permutation(n_reads) % 2
    order = np.random.default_rng(seed + 2).permutation(n_reads)  # each rank holds its reads in an order of its own
    shares = []
    for rank in range(2):
        parts = [ordered[ordered["query"] == q] for q in order if side[q] == rank]
        shares.append(np.concatenate(parts) if parts else ordered[:0])
    return ordered, shares


def _tensor(e):
    return torch.from_numpy(e.view(np.int32).reshape(-1, 4).copy())


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from siga_amd.sharding import gather_edges, gather_edges_async
        n = 200
        ordered, shares = _shares(n, 7)
        got, counts = gather_edges(_tensor(shares[rank]), n_reads=n)
        plain, counts2 = gather_edges(_tensor(shares[rank]))
        late, counts3 = gather_edges_async(_tensor(shares[rank]), n_reads=n).wait()
        if rank == 0:
            cat = np.concatenate(shares)
            out.put((got.numpy().tobytes() == ordered.tobytes(), plain.numpy().tobytes() == cat.tobytes(),
                     late.numpy().tobytes() == ordered.tobytes(), cat.tobytes() != ordered.tobytes(),
                     counts == counts2 == counts3 == [len(shares[0]), len(shares[1])]))
        else:
            assert got is None and plain is None and late is None
    finally:
        dist.destroy_process_group()


def test_gather_edges_restores_the_read_order_gloo_world2():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    restored, plain_is_cat, late, permuted, counts_ok = q.get(timeout=10)
    assert restored and plain_is_cat and late and permuted and counts_ok
