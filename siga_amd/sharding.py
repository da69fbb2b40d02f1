"""Read sharding and the one exchange step of the multi-GPU path.

Every read's result depends only on the immutable index, so the index is replicated on every GPU and the reads
are cut into `world` contiguous ranges (contiguous keeps VT order and hits order trivial).  The only exchange is
a variable-length gather of fixed-size edge records to rank 0: an all_gather of the per-rank counts, then one
padded gather of the records (RCCL over xGMI when the backend is "nccl"; gloo on CPU in the tests).

Ranks that run key-range shards instead (`locality_keys` / `key_order`, every read under its own id) emit their records in
key order; `restore_order` -- or `gather_edges(..., n_reads=n)` -- puts the gathered list back into the ED order of a
one-GPU run, and `flags_by_read_id` does the same for the per-read substring flags.
"""
import torch
import torch.distributed as dist


def shard_range(n_reads, rank, world):
    """Contiguous, balanced [lo, hi) of reads for `rank`; the first n_reads % world ranks get one more."""
    q, r = divmod(n_reads, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


class PendingGather:
    """An edge gather in flight: `wait()` returns what `gather_edges` returns."""

    def __init__(self, work, bufs, counts, is_dst, local=None, n_reads=None):
        self._work, self._bufs, self.counts, self._is_dst, self._local = work, bufs, counts, is_dst, local
        self._n_reads = n_reads

    def wait(self):
        if self._work is not None:
            self._work.wait()
        if self._local is not None:
            return _restored(self._local, self._n_reads), self.counts
        if not self._is_dst:
            return None, self.counts
        return _restored(torch.cat([self._bufs[r][: self.counts[r]] for r in range(len(self._bufs))], dim=0), self._n_reads), self.counts


def _restored(edges, n_reads):
    """what the destination rank returns: the gathered list as it is, or back in read order when the caller says how many
    reads the queries index"""
    return edges if n_reads is None else restore_order(edges, n_reads)[0]


def gather_edges_async(local_edges, group=None, dst=0, n_reads=None):
    """Like gather_edges, but the record gather itself is asynchronous so that it overlaps the next batch's kernels
    (the caller must not touch `local_edges` until wait()).  The tiny count exchange is synchronous; with `n_reads` the
    destination's wait() restores the read order."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return PendingGather(None, None, [int(local_edges.shape[0])], True, local=local_edges, n_reads=n_reads)
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    dev = local_edges.device
    cnt = torch.tensor([local_edges.shape[0]], dtype=torch.int64, device=dev)
    allc = torch.zeros(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(allc, cnt, group=group)
    counts = [int(c) for c in allc.tolist()]
    mx = max(max(counts), 1)
    padded = torch.zeros((mx, 4), dtype=torch.int32, device=dev)
    padded[: local_edges.shape[0]] = local_edges
    if rank == dst:
        bufs = [torch.empty((mx, 4), dtype=torch.int32, device=dev) for _ in range(world)]
        work = dist.gather(padded, gather_list=bufs, dst=dst, group=group, async_op=True)
        return PendingGather(work, bufs, counts, True, n_reads=n_reads)
    work = dist.gather(padded, gather_list=None, dst=dst, group=group, async_op=True)
    pg = PendingGather(work, None, counts, False)
    pg._keep = padded
    return pg


def gather_edges(local_edges, group=None, dst=0, n_reads=None):
    """local_edges: int32 tensor [k, 4] (query, target, length, af) on this rank's device.

    Returns on `dst` the concatenation over ranks in rank order and the per-rank counts; on other ranks (None, counts).
    Rank order is read order -- the ED order of a single-GPU run -- when the ranks ran contiguous ranges of the file
    (`shard_range`).  Ranks that ran key-range shards under their own ids pass `n_reads`, the number of indexed reads: `dst`
    then returns the list put back into that order (`restore_order`)."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return _restored(local_edges, n_reads), [int(local_edges.shape[0])]
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    dev = local_edges.device
    cnt = torch.tensor([local_edges.shape[0]], dtype=torch.int64, device=dev)
    allc = torch.zeros(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(allc, cnt, group=group)
    counts = [int(c) for c in allc.tolist()]  # one device->host sync for all ranks' counts
    mx = max(max(counts), 1)
    padded = torch.zeros((mx, 4), dtype=torch.int32, device=dev)
    padded[: local_edges.shape[0]] = local_edges
    if rank == dst:
        bufs = [torch.empty((mx, 4), dtype=torch.int32, device=dev) for _ in range(world)]
        dist.gather(padded, gather_list=bufs, dst=dst, group=group)
        return _restored(torch.cat([bufs[r][: counts[r]] for r in range(world)], dim=0), n_reads), counts
    dist.gather(padded, gather_list=None, dst=dst, group=group)
    return None, counts


# ------------------------------------------------------------------------------------------------------------------
# Key-range sharding: the read order of what the ranks return
# ------------------------------------------------------------------------------------------------------------------
def _restore_order_numpy(query, n_reads):
    """the restatement of csrc/sigax_order.hip in numpy: (stable order of the records by query, query_offs u64[n_reads + 1]);
    the kernel's two refusals are ValueErrors"""
    import numpy as np
    query = np.ascontiguousarray(query, dtype=np.uint32)
    beyond = int((query >= n_reads).sum())
    if beyond:
        raise ValueError("%d records with a query beyond the %d reads" % (beyond, n_reads))
    heads = np.ones(len(query), dtype=bool)
    heads[1:] = query[1:] != query[:-1]
    extra = int(heads.sum()) - len(np.unique(query))
    if extra:
        raise ValueError("%d runs beyond the first of their query: some query's records are not contiguous" % extra)
    offs = np.zeros(n_reads + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.bincount(query, minlength=n_reads), dtype=np.uint64)
    return np.argsort(query, kind="stable"), offs


def _status_error(status, n_reads):
    if status[0]:
        return ValueError("%d records with a query beyond the %d reads" % (status[0], n_reads))
    return ValueError("%d runs beyond the first of their query: some query's records are not contiguous" % status[1])


def restore_order(edges, n_reads, device=None):
    """The concatenation of any number of key-range shards' edge records, in any shard order -> (the records in the ED order of
    a one-batch run over the `n_reads` indexed reads, query_offs[n_reads + 1]: the records of read q are ordered[offs[q] :
    offs[q + 1]]).  Every query's records must be contiguous in `edges` (a read runs in one batch, and a batch emits a query's
    records together): the result is then the stable order by query.  A query beyond `n_reads`, or a query with a second run,
    is a ValueError.

    edges: a numpy `EDGE_DTYPE` array (numpy arrays come back) or an int32 tensor [k, 4] as `gather_edges` returns (an int32
    tensor and an int64 tensor come back, on the tensor's device).  On a GPU (`device` a cuda device, or a tensor that lives on
    one) the order comes from the library's kernels (sigax_edges_restore_order, csrc/sigax_order.hip); on the CPU from the numpy
    restatement above, which the tests hold the kernels against."""
    import numpy as np
    from ._lib import EDGE_DTYPE
    n_reads = int(n_reads)
    as_tensor = isinstance(edges, torch.Tensor)
    if as_tensor:
        if edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 4:
            raise ValueError("edges: an int32 tensor [k, 4]")
        dev = torch.device(device) if device is not None else edges.device
    else:
        edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        dev = torch.device(device) if device is not None else torch.device("cpu")
    if dev.type != "cuda":
        rec = edges.cpu().contiguous().numpy().view(EDGE_DTYPE).reshape(-1) if as_tensor else edges
        order, offs = _restore_order_numpy(rec["query"], n_reads)
        out = rec[order]
        if as_tensor:
            return torch.from_numpy(out.view(np.int32).reshape(-1, 4)).to(edges.device), torch.from_numpy(offs.astype(np.int64)).to(edges.device)
        return out, offs
    from . import _lib
    lib = _lib.lib()
    d_in = edges.to(dev).contiguous() if as_tensor else torch.from_numpy(edges.view(np.int32).reshape(-1, 4)).to(dev)
    k = int(d_in.shape[0])
    import ctypes as C
    need = C.c_uint64()
    if lib.sigax_edges_order_workspace(k, n_reads, C.byref(need)) != 0:
        raise ValueError("sigax_edges_order_workspace: " + _lib.last_error())
    d_out = torch.empty_like(d_in)
    d_offs = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    d_work = torch.empty(max(int(need.value), 16), dtype=torch.uint8, device=dev)
    d_status = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.sigax_edges_restore_order(dev.index or 0, d_in.data_ptr(), k, n_reads, d_out.data_ptr(), d_offs.data_ptr(),
                                           d_work.data_ptr(), int(need.value), d_status.data_ptr(), C.c_void_p(st))
    if rc != 0:
        raise RuntimeError("sigax_edges_restore_order: " + _lib.last_error())
    status = d_status.tolist()  # (waits for the stream)
    if status[0] or status[1]:
        raise _status_error(status, n_reads)
    if as_tensor:
        return d_out.to(edges.device), d_offs.to(edges.device)
    return d_out.cpu().numpy().view(EDGE_DTYPE).reshape(-1), d_offs.cpu().numpy().astype(np.uint64)


def flags_by_read_id(flags, ids, n_reads, device=None):
    """One byte per read of a shard (its substring flags) to the reads' places: out[ids[r]] = flags[r] in a zeroed uint8 array
    [n_reads]; an id beyond `n_reads` is a ValueError.  On a cuda `device` by the library's kernel (sigax_flags_by_read_id),
    else in numpy."""
    import numpy as np
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    n_reads = int(n_reads)
    if flags.shape != ids.shape or flags.ndim != 1:
        raise ValueError("flags and ids: one entry per read of the shard")
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if dev.type != "cuda":
        beyond = int((ids >= n_reads).sum())
        if beyond:
            raise ValueError("%d read ids beyond the %d reads" % (beyond, n_reads))
        out = np.zeros(n_reads, dtype=np.uint8)
        out[ids] = flags
        return out
    import ctypes as C
    from . import _lib
    d_flags = torch.from_numpy(flags).to(dev)
    d_ids = torch.from_numpy(ids.view(np.int32)).to(dev)
    d_out = torch.zeros(max(n_reads, 1), dtype=torch.uint8, device=dev)
    d_status = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        rc = _lib.lib().sigax_flags_by_read_id(dev.index or 0, d_flags.data_ptr(), d_ids.data_ptr(), len(ids), n_reads, d_out.data_ptr(),
                                               d_status.data_ptr(), C.c_void_p(st))
    if rc != 0:
        raise RuntimeError("sigax_flags_by_read_id: " + _lib.last_error())
    beyond = int(d_status.item())
    if beyond:
        raise ValueError("%d read ids beyond the %d reads" % (beyond, n_reads))
    return d_out[:n_reads].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# Key-range sharding: which reads go to which rank
# ------------------------------------------------------------------------------------------------------------------
LOCALITY_K = 16  # bases of the minimizer


def locality_keys(reads, device=None, chunk=1 << 20):
    """reads: uint8 array [n, L] of ASCII bases -> int64 array [n] of locality keys, computed from the sequences alone.

    key = min over the read's 16-mers of  hash(canonical 16-mer) << 16 | (L - 16 - off): the read's minimizer -- the canonical
    16-mer (the smaller of a 16-mer and its reverse complement) with the smallest hash, so a read and the reverse complement of
    its neighbour on the genome share it -- above, and below it where the read starts before the minimizer on the canonical
    strand (off), turned so that an earlier start sorts first.  Reads that share a minimizer cover the same 2L-wide stretch of
    the genome: sorted by key they are neighbours, and a contiguous slice of that order (one rank's share: `key_order` /
    `shard_range`) covers its part of the genome as deep as the whole read set covers the whole genome -- the backward searches
    of a rank then walk a fraction of the index's rows (a non-ACGT base counts as 'A' here; the key only decides placement,
    never a result).

    On a GPU (`device` a cuda device) the keys come from the library's kernel (sigax_locality_keys, csrc/sigax_keys.hip); on
    the CPU from the torch restatement below, which the tests hold the kernel against."""
    import numpy as np
    n, L = reads.shape
    out = np.empty(n, dtype=np.int64)
    if L < LOCALITY_K:
        out[:] = 0
        return out
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if dev.type == "cuda":
        from . import _lib
        lib = _lib.lib()
        d_offs = torch.arange(0, (min(chunk, n) + 1) * L, L, dtype=torch.int64, device=dev)
        for lo in range(0, n, chunk):
            m = min(chunk, n - lo)
            r = torch.from_numpy(np.ascontiguousarray(reads[lo:lo + m]).reshape(-1)).to(dev)
            k = torch.empty(m, dtype=torch.int64, device=dev)
            torch.cuda.current_stream(dev).synchronize()  # (the library launches on the default stream)
            rc = lib.sigax_locality_keys(dev.index or 0, r.data_ptr(), d_offs.data_ptr(), m, k.data_ptr(), None)
            if rc != 0:
                raise RuntimeError("sigax_locality_keys: " + _lib.last_error())
            out[lo:lo + m] = k.cpu().numpy()
        return out
    return _locality_keys_torch(reads, dev, chunk)


def _locality_keys_torch(reads, dev, chunk=1 << 20):
    """the restatement of csrc/sigax_keys.hip in torch ops (any device)"""
    import numpy as np
    n, L = reads.shape
    k = LOCALITY_K
    out = np.empty(n, dtype=np.int64)
    lut = torch.zeros(256, dtype=torch.int64, device=dev)
    for ch, v in ((b"C", 1), (b"G", 2), (b"T", 3), (b"c", 1), (b"g", 2), (b"t", 3)):
        lut[ch[0]] = v
    at = torch.arange(L - k + 1, dtype=torch.int64, device=dev)[None, :]
    for lo in range(0, n, chunk):
        r = torch.from_numpy(np.ascontiguousarray(reads[lo:lo + chunk])).to(dev)
        f = lut[r.long()]          # [m, L] codes, most significant base first in a k-mer
        g = 3 - f                  # complement; the reverse complement reads it the other way round
        w = 1
        while w < k:               # k-mers by doubling: f[i] = f[i] << 2w | f[i + w]; g[i] = g[i] | g[i + w] << 2w
            f = (f[:, :-w] << (2 * w)) | f[:, w:]
            g = g[:, :-w] | (g[:, w:] << (2 * w))
            w *= 2
        fw = f <= g
        c = torch.where(fw, f, g)  # canonical 16-mer (32 bits)
        h = (c * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF   # wraps like uint64 arithmetic, sign bit dropped
        h = (h >> 31) & 0xFFFFFFFF                             # bits 31..62 of the product: 32-bit hash
        # the read starts `at` bases before the 16-mer on its own strand; seen from the canonical strand a read whose 16-mer
        # is the larger one of the pair starts L - k - at before it
        off = torch.where(fw, at, (L - k) - at)
        key = ((h << 16) | ((L - k) - off)).min(dim=1).values  # earlier start on the canonical strand = smaller key
        out[lo:lo + r.shape[0]] = key.cpu().numpy()
    return out


def key_order(keys, device=None):
    """stable order of the reads by locality key -> int64 permutation (read ids in key order); sorted on `device` if given"""
    import numpy as np
    if device is not None and torch.device(device).type == "cuda":
        return torch.sort(torch.from_numpy(np.ascontiguousarray(keys)).to(device), stable=True).indices.cpu().numpy()
    return np.argsort(keys, kind="stable")
