"""The child-process bodies of tests/test_gpu_comm_ranks.py: `python -m tests.comm_ranks_child <group> <W> [<workdir>]` with
SIGAX_RCCL_LIB naming the stand-in (tests/rccl_standin.cpp).  The ranks of a world are Python threads of this one process on
the one GPU: ctypes releases the GIL, so W calls into the library are in flight at once, as W processes' would be.  A failed
check or a thread that does not come back ends the child with a non-zero status and the cause on stdout."""
import ctypes as C
import os
import sys
import threading
import traceback

import numpy as np
import torch  # noqa: F401  (before libsigax.so: one HIP runtime per process)

from siga_amd import _lib
from siga_amd._lib import EDGE_DTYPE
from siga_amd.overlap import _DeviceBytes
from tests.test_gpu_multi import _edges

E_ARG, E_DEVICE = -1, -3
H2D, D2H, D2D = 1, 2, 3
REC = EDGE_DTYPE.itemsize
GUARD = 64  # bytes of 0xEE behind the root's records
JOIN_SECONDS = 120
VALUES = (0, 1, 7, 1000, 12345)


class Hip:
    """the few asynchronous HIP calls the ranks need, through the runtime libsigax.so is bound to"""

    def __init__(self):
        h = _lib.lib()
        vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
        h.hipMemcpyAsync.argtypes = [vp, vp, sz, ci, vp]
        h.hipMemsetAsync.argtypes = [vp, ci, sz, vp]
        h.hipStreamSynchronize.argtypes = [vp]
        h.hipHostMalloc.argtypes = [C.POINTER(vp), sz, C.c_uint]
        h.hipHostFree.argtypes = [vp]
        self.h = h

    def ok(self, err, where):
        if err != 0:
            raise RuntimeError("%s failed: HIP error %d" % (where, err))

    def copy_async(self, dst, src, nbytes, kind, stream):
        if nbytes:
            self.ok(self.h.hipMemcpyAsync(dst, src, nbytes, kind, stream), "hipMemcpyAsync")

    def fill_async(self, dst, byte, nbytes, stream):
        if nbytes:
            self.ok(self.h.hipMemsetAsync(dst, byte, nbytes, stream), "hipMemsetAsync")

    def wait(self, stream):
        self.ok(self.h.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def pinned(self, nbytes):
        p = C.c_void_p()
        self.ok(self.h.hipHostMalloc(C.byref(p), max(nbytes, 16), 0), "hipHostMalloc")
        return p

    def unpin(self, p):
        self.h.hipHostFree(p)


def run_ranks(W, body):
    """W threads, each with its communicator of one fresh world and a stream of its own, run body(rank, comm, stream, L);
    every thread must come back in time and without an exception"""
    L = _lib.lib()
    idb = (C.c_uint8 * 128)()
    assert L.sigax_comm_unique_id(idb) == 0, _lib.last_error()
    errors = []

    def rank_thread(rank):
        comm, st = C.c_void_p(), C.c_void_p()
        try:
            assert L.sigax_comm_create(0, rank, W, idb, C.byref(comm)) == 0, _lib.last_error()
            assert L.sigax_stream_create(0, C.byref(st)) == 0, _lib.last_error()
            body(rank, comm, st, L)
        except BaseException:
            errors.append("rank %d of %d:\n%s" % (rank, W, traceback.format_exc()))
        finally:
            if st:
                L.sigax_stream_destroy(0, st)
            if comm:
                L.sigax_comm_destroy(comm)

    threads = [threading.Thread(target=rank_thread, args=(r,), daemon=True) for r in range(W)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    stuck = [r for r, t in enumerate(threads) if t.is_alive()]
    if stuck or errors:
        print("\n".join(errors))
        if stuck:
            print("ranks that did not come back within %d s: %s" % (JOIN_SECONDS, stuck))
        sys.stdout.flush()
        os._exit(1)  # (a rank may still sit in a call: no waiting for it)


# ----------------------------------------------------------------------------------------------------------------------
# a. synthetic records
# ----------------------------------------------------------------------------------------------------------------------
def synthetic_cases(W):
    """(root, counts) with the root first, last and in the middle, counts drawn from VALUES so that the root's own share is
    empty, a non-root's is, all are, and one rank holds everything -- on the root and off it"""
    rng = np.random.default_rng(100 + W)
    cases = []
    for root in sorted({0, W // 2, W - 1}):
        other = (root + 1) % W
        cases.append((root, [0] * W))
        cases.append((root, [12345 if r == root else 0 for r in range(W)]))    # everything on the root: nobody sends
        cases.append((root, [12345 if r == other else 0 for r in range(W)]))   # everything on one sender, the root's own share empty
        cases.append((root, [VALUES[1 + (r + root) % 4] for r in range(W)]))   # nobody empty
        c = [VALUES[1 + (r + 2 * root) % 4] for r in range(W)]
        c[root] = 0                                                            # the root's own share empty, every sender's not
        cases.append((root, c))
        c = [VALUES[1 + (3 * r + root) % 4] for r in range(W)]
        c[other] = 0                                                           # one sender's share empty, the root's not
        cases.append((root, c))
        cases.append((root, [int(x) for x in rng.choice(VALUES, size=W)]))
    seen = [c for _, c in cases]
    assert any(not any(c) for c in seen) and any(sorted(c)[-2] == 0 and max(c) for c in seen)
    assert any(c[root] == 0 and any(c) for root, c in cases) and any(c[root] and 0 in c for root, c in cases)
    return cases


def synthetic(W):
    hip = Hip()
    cases = synthetic_cases(W)
    most = max(VALUES)

    def body(rank, comm, st, L):
        h_in, h_back = hip.pinned(most * REC), hip.pinned(W * most * REC + GUARD)
        d_in, d_out = _DeviceBytes(most * REC, 0), _DeviceBytes(W * most * REC + GUARD, 0)
        try:
            for root, counts in cases:
                total = sum(counts)
                n = counts[rank]
                for run in (0, 1):  # twice on the same communicators, other records the second time
                    e = _edges(rank + W * run, n)
                    C.memmove(h_in, e.ctypes.data, e.nbytes)

                    def upload():  # on this rank's stream, no host wait behind it
                        hip.fill_async(d_in.ptr, 0xCD, most * REC, st)
                        hip.copy_async(d_in.ptr, h_in, e.nbytes, H2D, st)

                    if rank == root:
                        hip.fill_async(d_out.ptr, 0xEE, W * most * REC + GUARD, st)
                    if run == 0:
                        upload()
                    cnt = (C.c_uint64 * W)()
                    assert L.sigax_gather_counts(comm, n, cnt, st) == 0, _lib.last_error()
                    assert [int(c) for c in cnt] == counts, ([int(c) for c in cnt], counts)
                    if run == 1:  # ... and here between the two calls: sigax_gather_edges alone must honour the stream
                        upload()
                    # a buffer that may be NULL (nothing to send, nothing to receive) is NULL in the second run
                    p_in = None if (n == 0 and run == 1) else d_in.ptr
                    p_out = d_out.ptr if rank == root and not (total == 0 and run == 1) else None
                    assert L.sigax_gather_edges(comm, p_in, cnt, root, p_out, st) == 0, _lib.last_error()
                    if rank == root:
                        hip.copy_async(h_back, d_out.ptr, total * REC + GUARD, D2H, st)  # behind the gather on the root's stream
                    hip.wait(st)
                    if rank == root:
                        got = C.string_at(h_back, total * REC + GUARD)
                        want = b"".join(_edges(r + W * run, counts[r]).tobytes() for r in range(W))
                        assert len(want) == total * REC
                        where = "W %d root %d counts %s run %d" % (W, root, counts, run)
                        assert got[:total * REC] == want, "records differ: " + where
                        assert got[total * REC:] == b"\xEE" * GUARD, "bytes behind the records written: " + where
        finally:
            d_in.free()
            d_out.free()
            hip.unpin(h_in)
            hip.unpin(h_back)

    run_ranks(W, body)
    print("synthetic: W %d, %d cases twice" % (W, len(cases)))


# ----------------------------------------------------------------------------------------------------------------------
# b. refusals with a world above one
# ----------------------------------------------------------------------------------------------------------------------
def refusals(W):
    hip = Hip()
    true_counts = [5, 7, 3, 11, 2, 1, 9, 4][:W]
    liar = 1  # the rank whose counts[] says 9 where everyone else's says 7
    results = {}

    def body(rank, comm, st, L):
        d_in, d_out = _DeviceBytes(16 * REC, 0), _DeviceBytes(sum(true_counts) * REC + 16 * REC + GUARD, 0)
        h_back = hip.pinned(sum(true_counts) * REC)
        try:
            cnt = (C.c_uint64 * W)(*true_counts)
            # nothing of this is posted (every rank is refused by itself), so no other rank waits
            for root in (-1, W, W + 5):
                assert L.sigax_gather_edges(comm, d_in.ptr, cnt, root, d_out.ptr, st) == E_ARG
            assert L.sigax_gather_edges(comm, None, cnt, (rank + 1) % W, None, st) == E_ARG      # NULL d_local, own count above zero
            assert L.sigax_gather_edges(comm, None, cnt, rank, d_out.ptr, st) == E_ARG
            assert L.sigax_gather_edges(comm, d_in.ptr, cnt, rank, None, st) == E_ARG             # NULL d_out on the root
            assert "NULL record buffer" in _lib.last_error()
            assert L.sigax_gather_edges(comm, d_in.ptr, None, 0, d_out.ptr, st) == E_ARG
            # the communicators are as they were: a gather pairs up
            e = _edges(rank, true_counts[rank])
            d_in.upload(e)
            got = (C.c_uint64 * W)()
            assert L.sigax_gather_counts(comm, true_counts[rank], got, st) == 0, _lib.last_error()
            assert [int(c) for c in got] == true_counts
            root = W - 1
            assert L.sigax_gather_edges(comm, d_in.ptr, got, root, d_out.ptr if rank == root else None, st) == 0, _lib.last_error()
            if rank == root:
                hip.copy_async(h_back, d_out.ptr, sum(true_counts) * REC, D2H, st)
            hip.wait(st)
            if rank == root:
                assert C.string_at(h_back, sum(true_counts) * REC) == b"".join(_edges(r, true_counts[r]).tobytes() for r in range(W))
            # one sender's counts[] differs from the root's: the Send and its Recv disagree, both sides hear of it
            if rank == liar:
                cnt[liar] = 9
            rc = L.sigax_gather_edges(comm, d_in.ptr, cnt, 0, d_out.ptr if rank == 0 else None, st)
            results[rank] = (rc, _lib.last_error() if rc else "")
            hip.wait(st)
        finally:
            d_in.free()
            d_out.free()
            hip.unpin(h_back)

    run_ranks(W, body)
    for rank in range(W):
        rc, text = results[rank]
        if rank in (0, liar):
            assert rc == E_DEVICE and "mismatch" in text, (rank, rc, text)
        else:
            assert rc == 0, (rank, rc, text)
    print("refusals: W %d" % W)


# ----------------------------------------------------------------------------------------------------------------------
# c. the step end to end
# ----------------------------------------------------------------------------------------------------------------------
def _read_sets(workdir):
    """(tag, reads as (name, comment, seq), index prefix, min overlap, irreducible, rc, the oracle's ASQG text)"""
    from oracle import pyoracle as po
    from siga_amd import host
    from siga_amd.overlap import read_sequences
    from tests.fixtures import fixture
    from tests.test_gpu_random import make_case
    for name, m in (("toy", 45), ("ragged", 15), ("dup", 8)):
        fx = fixture(name)
        yield name, read_sequences(fx.fa), fx.prefix, m, True, True, fx.oracle_asqg(m)[0]
    reads, m, irr, rc = make_case(8)
    fa = os.path.join(workdir, "r.fa")
    with open(fa, "w") as f:
        for n, s in reads:
            f.write(">%s\n%s\n" % (n, s))
    prefix = os.path.join(workdir, "r")
    host.index_file(fa, prefix, threads=2)
    fwd = po.Index.load(prefix + ".bwt", prefix + ".sai")
    rev = po.Index.load(prefix + ".rbwt", prefix + ".rsai")
    po.build_asqg(fwd, rev, fa, m, os.path.join(workdir, "o.asqg"), "", irr, rc)
    yield "random8", read_sequences(fa), prefix, m, irr, rc, open(os.path.join(workdir, "o.asqg")).read()


def _key_shards(seqs, W):
    """np.array_split(key_order(locality_keys(...)), W); reads of mixed lengths are padded with 'A' for the key alone (a key
    only decides placement)"""
    from siga_amd.sharding import key_order, locality_keys
    width = max(len(s) for s in seqs)
    mat = np.frombuffer("".join(s.ljust(width, "A") for s in seqs).encode(), dtype=np.uint8).reshape(len(seqs), width)
    return np.array_split(key_order(locality_keys(mat)), W)


def _run_rank_by_rank(builder, seqs, m, shards, by_key, held):
    """each rank's overlap run on the main thread -> per rank (edge records, how many, substring flags, read ids) in device
    memory (ids None for a contiguous range: the run went under read_base)"""
    from siga_amd.overlap import _check, pack_reads
    L = _lib.lib()
    fmi = builder.fmi
    bt = C.c_void_p()
    _check(L.sigax_batch_create(fmi.handle, max(max(len(s) for s in shards), 1), 0, max(len(s) for s in seqs), C.byref(bt)), "sigax_batch_create")
    out = []

    def dev(nbytes):
        held.append(_DeviceBytes(nbytes, 0))
        return held[-1]

    try:
        for ids in shards:
            ids = np.ascontiguousarray(ids, dtype=np.uint32)
            if len(ids) == 0:
                out.append((dev(0), 0, dev(0), None))
                continue
            buf, offs = pack_reads([seqs[i] for i in ids])
            _check(L.sigax_batch_upload(bt, buf, offs.ctypes.data, len(ids), None), "sigax_batch_upload")
            d_ids = None
            if by_key:
                d_ids = dev(ids.nbytes).upload(ids)
                _check(L.sigax_batch_set_device_read_ids(bt, d_ids.ptr, len(ids)), "sigax_batch_set_device_read_ids")
            else:
                assert np.array_equal(ids, np.arange(ids[0], ids[0] + len(ids)))
            _check(L.sigax_batch_run(bt, 0 if by_key else int(ids[0]), m, builder._flags(True), None), "sigax_batch_run")
            stats = _lib.Stats()
            _check(L.sigax_batch_finish(bt, None, C.byref(stats)), "sigax_batch_finish")
            p_sub, p_edges = C.c_void_p(), C.c_void_p()
            _check(L.sigax_batch_device_outputs(bt, None, None, C.byref(p_sub), C.byref(p_edges)), "sigax_batch_device_outputs")
            k = int(stats.n_edges)
            d_edges, d_flags = dev(k * REC), dev(len(ids))
            d_edges.copy_from_device(0, p_edges, k * REC)  # (the batch object's own buffers serve the next rank)
            d_flags.copy_from_device(0, p_sub, len(ids))
            out.append((d_edges, k, d_flags, d_ids))
    finally:
        L.sigax_batch_destroy(bt)
    return out


def _exchange(W, root, parts, held):
    """the exchange alone on W threads -> (the root's gathered records in device memory behind a guard, how many)"""
    hip = Hip()
    counts = [k for _, k, _, _ in parts]
    total = sum(counts)
    held.append(_DeviceBytes(total * REC + GUARD, 0))
    d_all = held[-1]

    def body(rank, comm, st, L):
        cnt = (C.c_uint64 * W)()
        assert L.sigax_gather_counts(comm, counts[rank], cnt, st) == 0, _lib.last_error()
        assert [int(c) for c in cnt] == counts
        if rank == root:
            hip.fill_async(d_all.ptr, 0xEE, total * REC + GUARD, st)
        assert L.sigax_gather_edges(comm, parts[rank][0].ptr if counts[rank] else None, cnt, root, d_all.ptr if rank == root else None,
                                    st) == 0, _lib.last_error()
        hip.wait(st)

    run_ranks(W, body)
    assert d_all.download(np.uint8, total * REC + GUARD)[total * REC:].tobytes() == b"\xEE" * GUARD
    return d_all, total


def end_to_end(W, workdir):
    import siga_amd
    from siga_amd.overlap import _check, format_asqg, name_ranks
    from siga_amd.sharding import shard_range
    L = _lib.lib()
    for tag, reads, prefix, m, irr, rc, want_asqg in _read_sets(workdir):
        seqs = [r[2] for r in reads]
        n = len(seqs)
        pair = siga_amd.FMIndexPair.load(prefix)
        pair.set_reads(np.array([len(s) for s in seqs], dtype=np.uint32), name_ranks([r[0] for r in reads]))
        builder = siga_amd.OverlapBuilder(pair, prefix, irreducible=irr, rc=rc)
        one = builder.overlap(seqs, m, edges=True)
        assert len(one["edges"]) > 0 and format_asqg(reads, one, m) == want_asqg, tag
        shardings = (("contiguous", False, [np.arange(*shard_range(n, r, W)) for r in range(W)], 0),
                     ("key", True, _key_shards(seqs, W), W // 2))
        for how, by_key, shards, root in shardings:
            where = "%s, %d ranks, %s shards" % (tag, W, how)
            held = []
            try:
                parts = _run_rank_by_rank(builder, seqs, m, shards, by_key, held)
                d_all, total = _exchange(W, root, parts, held)
                assert total == len(one["edges"]), where
                d_sub = _DeviceBytes(n, 0).zero()
                held.append(d_sub)
                if not by_key:  # rank order is read order: the gathered buffer as it is, the flags one range behind the other
                    edges = d_all.download(EDGE_DTYPE, total)
                    at = 0
                    for _, _, d_flags, _ in parts:
                        d_sub.copy_from_device(at, d_flags.ptr, d_flags.nbytes)
                        at += d_flags.nbytes
                    assert at == n
                else:
                    assert not np.array_equal(np.concatenate(shards), np.arange(n)), where  # (a real permutation of the reads)
                    d_out, d_status = _DeviceBytes(total * REC, 0), _DeviceBytes(16, 0)
                    held += [d_out, d_status]
                    need = C.c_uint64()
                    _check(L.sigax_edges_order_workspace(total, n, C.byref(need)), "sigax_edges_order_workspace")
                    d_work = _DeviceBytes(need.value, 0)
                    held.append(d_work)
                    _check(L.sigax_edges_restore_order(0, d_all.ptr, total, n, d_out.ptr, None, d_work.ptr, need.value, d_status.ptr, None),
                           "sigax_edges_restore_order")
                    assert not d_status.download(np.uint64, 2).any(), where
                    edges = d_out.download(EDGE_DTYPE, total)
                    for (_, _, d_flags, d_ids), ids in zip(parts, shards):
                        if len(ids):
                            _check(L.sigax_flags_by_read_id(0, d_flags.ptr, d_ids.ptr, len(ids), n, d_sub.ptr, d_status.ptr, None),
                                   "sigax_flags_by_read_id")
                            assert not d_status.download(np.uint64, 1).any(), where
                substring = d_sub.download(np.uint8, n)
                assert edges.tobytes() == one["edges"].tobytes(), "edge records differ: " + where
                assert substring.tobytes() == one["substring"].tobytes(), "substring flags differ: " + where
                assert format_asqg(reads, {"edges": edges, "substring": substring}, m) == want_asqg, "ASQG differs: " + where
            finally:
                for d in held:
                    d.free()
        pair.close()
        print("end to end: %s, W %d" % (tag, W))


if __name__ == "__main__":
    assert os.environ.get("SIGAX_RCCL_LIB"), "SIGAX_RCCL_LIB must name the stand-in"
    group, W = sys.argv[1], int(sys.argv[2])
    if group == "synthetic":
        synthetic(W)
    elif group == "refusals":
        refusals(W)
    elif group == "end_to_end":
        end_to_end(W, sys.argv[3])
    else:
        raise SystemExit("unknown group " + group)
    sys.stdout.flush()
