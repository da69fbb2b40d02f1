#!/usr/bin/env python3
"""Measures `siga locate` at BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1) for two query sets, 31-mers cut
from the reads and whole reads:
  search      device time of sigax_locate_device with hits_cap = 0: the search, the flags and the prefix sum, nothing walked
  locate      device time of the whole call; walk = locate - search, step by step (the two run back to back on one stream,
              so the difference is k_locate_walk and its launch)
  walk_k_walk device time of sigax_string_lengths_device over the rows the call returned through d_rows: the one-lane-per-row
              launch of k_walk, what the library had for the walk half before (lengths and stretches, no hit records)
by HIP events, median of --steps after --warmup, with their spread; hits/s, LF steps per hit and rank-table sectors per hit
of the walk.  Checks that the plain walk ends where the hits say.  One JSON document on stdout (and in --out).  Needs a
GPU; nothing but this repository.

    python tools/locate_bench.py --out profiles/locate_configs1.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALL = (1 << 32) - 1


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    return hip


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "stdev_ms": statistics.pstdev(ms)}


def measure(hip, L, handle, flat, offs, max_hits, steps, warmup):
    from siga_amd._lib import HIT_DTYPE
    n = len(offs) - 1
    held = []

    def dbuf(nbytes, src=None):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(nbytes, 16)) == 0
        held.append(q)
        if src is not None:
            assert hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        return q

    def get(q, dtype, count):
        out = np.zeros(count, dtype=dtype)
        assert hip.hipMemcpy(out.ctypes.data, q, out.nbytes, 2) == 0
        return out

    stream = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    ev = [C.c_void_p() for _ in range(3)]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def elapsed(a, b):
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), a, b) == 0
        return float(t.value)

    try:
        wb = C.c_uint64()
        assert L.sigax_locate_workspace(n, C.byref(wb)) == 0
        d_seqs, d_offs = dbuf(flat.nbytes, flat), dbuf(offs.nbytes, offs)
        d_tot, d_qf, d_ho, d_stat, d_work = dbuf(8 * n), dbuf(4 * n), dbuf(8 * (n + 1)), dbuf(32), dbuf(wb.value)

        def locate(d_hits, d_rows, cap):
            assert L.sigax_locate_device(handle, d_seqs, d_offs, n, 2, max_hits, ALL, d_tot, d_qf, d_ho, d_hits, d_rows, cap, d_stat, d_work,
                                         wb.value, stream) == 0

        locate(None, None, 0)
        assert hip.hipStreamSynchronize(stream) == 0
        search_stat = get(d_stat, np.uint64, 4)
        need = int(search_stat[0])
        d_hits, d_rows = dbuf(16 * need), dbuf(8 * need)
        search_ms, locate_ms, walk_ms = [], [], []
        for i in range(warmup + steps):
            assert hip.hipEventRecord(ev[0], stream) == 0
            locate(None, None, 0)
            assert hip.hipEventRecord(ev[1], stream) == 0
            locate(d_hits, d_rows, need)
            assert hip.hipEventRecord(ev[2], stream) == 0
            assert hip.hipEventSynchronize(ev[2]) == 0
            if i >= warmup:
                search_ms.append(elapsed(ev[0], ev[1]))
                locate_ms.append(elapsed(ev[1], ev[2]))
                walk_ms.append(locate_ms[-1] - search_ms[-1])
        stat = get(d_stat, np.uint64, 4)
        hits = get(d_hits, HIT_DTYPE, need)
        d_lens, d_stretch, d_st2 = dbuf(4 * need), dbuf(8 * need), dbuf(16)
        plain_ms = []
        for i in range(warmup + steps):
            assert hip.hipEventRecord(ev[0], stream) == 0
            assert L.sigax_string_lengths_device(handle, 0, d_rows, need, ALL, d_lens, d_stretch, d_st2, stream) == 0
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            if i >= warmup:
                plain_ms.append(elapsed(ev[0], ev[1]))
        lens = get(d_lens, np.uint32, need)
        same = bool(np.array_equal(lens, hits["offset"]) and int(stat[1]) == 0 and not (hits["flags"] & 2).any())
        qflags = get(d_qf, np.uint32, n)
    finally:
        for q in held:
            hip.hipFree(q)
        L.sigax_stream_destroy(0, stream)
    w = statistics.median(walk_ms)
    return {"queries": n, "hits": need, "queries_over_max_hits": int(np.count_nonzero(qflags & 2)),
            "search": spread(search_ms), "locate": spread(locate_ms), "walk": spread(walk_ms), "walk_k_walk": spread(plain_ms),
            "k_walk_over_walk": statistics.median(plain_ms) / w if w > 0 else None,
            "hits_per_s_walk": need / (w * 1e-3) if w > 0 else None,
            "hits_per_s_locate": need / (statistics.median(locate_ms) * 1e-3),
            "lf_steps_per_hit": float(hits["offset"].astype(np.float64).mean()) if need else 0.0,
            "sectors_per_hit_walk": float(int(stat[2]) - int(search_stat[2])) / need if need else 0.0,
            "sectors_search": int(search_stat[2]), "plain_walk_agrees": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--queries", type=int, default=250000, help="queries per set")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--max-hits", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import siga_amd
    from siga_amd import _lib, host
    from tests.golden.make_reads import fast_reads
    hip, L = hip_runtime(), _lib.lib()
    N, K, Q = args.reads, args.length, min(args.queries, args.reads)
    reads, _ = fast_reads(args.genome, K, N, args.seed)
    offs = np.arange(N + 1, dtype=np.uint64) * np.uint64(K)
    rng = np.random.default_rng(args.seed + 7)
    pick = rng.choice(N, size=Q, replace=False)
    start = rng.integers(0, K - args.k + 1, size=Q)
    kmers = np.ascontiguousarray(np.stack([reads[r, s:s + args.k] for r, s in zip(pick, start)]))
    whole = np.ascontiguousarray(reads[pick])
    result = {"config": {"reads": N, "read_length": K, "genome": args.genome, "seed": args.seed, "queries_per_set": Q, "k": args.k,
                         "max_hits": args.max_hits, "steps": args.steps, "warmup": args.warmup, "strands": "both"}, "sets": {}}
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "reads")
        host.index_build_gpu(reads.reshape(-1), offs, prefix)
        pair = siga_amd.FMIndexPair.load_forward(prefix, device=0)
        for name, q in (("kmers_%d" % args.k, kmers), ("whole_reads", whole)):
            qo = np.arange(Q + 1, dtype=np.uint64) * np.uint64(q.shape[1])
            result["sets"][name] = measure(hip, L, pair.handle, q.reshape(-1), qo, args.max_hits, args.steps, args.warmup)
        pair.close()
    result["accepted"] = all(s["plain_walk_agrees"] for s in result["sets"].values())
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if result["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
