#!/usr/bin/env python3
"""Measures `siga match` at BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1), once with the reads as indexed
and once with 1 % substitutions:
  (a) device time of sigax_match_device, both strands, by HIP events: median of --steps launches after --warmup
  (b) wall time of sigax_match_batch
  (c) the same numbers without the match kernel: host reverse complement + two sigax_kmer_count_batch(k = 150) calls
  (d) the CPU oracle's Interval::occurrences over the same queries on the threads the machine gives
and checks (b) <= (c), equal counts, and symbols consumed < total chain length on the 1 % set.  One JSON document on stdout
(and in --out).  Needs a GPU; nothing but this repository.

    python tools/match_bench.py --out profiles/match_configs1.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def device_time(hip, L, handle, reads, offs, steps, warmup):
    """-> (median ms, all ms, stat4, counts) of sigax_match_device with SIGAX_RC on a stream of its own"""
    n = len(offs) - 1
    held = []

    def dbuf(nbytes, src=None):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), nbytes) == 0
        held.append(q)
        if src is not None:
            assert hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        return q

    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    try:
        d_seqs, d_offs, d_counts, d_stat = dbuf(reads.nbytes, reads), dbuf(offs.nbytes, offs), dbuf(16 * n), dbuf(32)
        ms = []
        for i in range(warmup + steps):
            assert hip.hipEventRecord(e0, stream) == 0
            assert L.sigax_match_device(handle, d_seqs, d_offs, n, (1 << 64) - 1, 2, d_counts, d_stat, stream) == 0
            assert hip.hipEventRecord(e1, stream) == 0
            assert hip.hipEventSynchronize(e1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            if i >= warmup:
                ms.append(float(t.value))
        counts, stat = np.zeros(2 * n, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        assert hip.hipMemcpy(counts.ctypes.data, d_counts, 16 * n, 2) == 0 and hip.hipMemcpy(stat.ctypes.data, d_stat, 32, 2) == 0
    finally:
        for q in held:
            hip.hipFree(q)
        L.sigax_stream_destroy(0, stream)
    return statistics.median(ms), ms, [int(x) for x in stat], counts[0::2].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--wall-repeats", type=int, default=5)
    ap.add_argument("--oracle-reads", type=int, default=100000, help="queries of (d): the oracle's time is scaled to the whole set")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import siga_amd
    from oracle import pyoracle as po
    from siga_amd import _lib, host
    from tests.golden.make_reads import fast_reads, substitute
    hip, L = hip_runtime(), _lib.lib()
    N, K = args.reads, args.length
    clean, _ = fast_reads(args.genome, K, N, args.seed)
    offs = np.arange(N + 1, dtype=np.uint64) * np.uint64(K)
    comp = np.zeros(256, dtype=np.uint8)
    comp[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
    result = {"config": {"reads": N, "read_length": K, "genome": args.genome, "seed": args.seed, "steps": args.steps, "warmup": args.warmup,
                         "wall_repeats": args.wall_repeats, "oracle_threads": args.threads, "oracle_reads": min(args.oracle_reads, N)},
              "sets": {}}
    ok = True
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "reads")
        host.index_build_gpu(clean.reshape(-1), offs, prefix)
        h = C.c_void_p()
        assert L.sigax_index_open((prefix + ".bwt").encode(), None, None, None, 0, C.byref(h)) == 0, _lib.last_error()
        pair = siga_amd.FMIndexPair(h.value)
        oracle = po.Index.load(prefix + ".bwt")
        for name, reads in (("as_indexed", clean), ("substituted_1pct", substitute(clean, 0.01, args.seed + 100))):
            flat = np.ascontiguousarray(reads.reshape(-1))
            a_ms, a_all, stat, dev_counts = device_time(hip, L, pair.handle, flat, offs, args.steps, args.warmup)
            b_s, c_s = [], []
            got = want = None
            for _ in range(args.wall_repeats + 1):  # the first of each is warm-up
                t0 = time.perf_counter()
                got, _ = pair.match((flat, offs), rc=True)
                b_s.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                rc = np.ascontiguousarray(comp[reads][:, ::-1])
                out = np.zeros(N, dtype=np.uint64)
                out2 = np.zeros(N, dtype=np.uint64)
                assert L.sigax_kmer_count_batch(pair.handle, C.c_char_p(flat.ctypes.data), K, N, out.ctypes.data) == 0
                assert L.sigax_kmer_count_batch(pair.handle, C.c_char_p(rc.ctypes.data), K, N, out2.ctypes.data) == 0
                want = out + out2
                c_s.append(time.perf_counter() - t0)
            same = bool(np.array_equal(got, want) and np.array_equal(dev_counts, want))
            m = min(args.oracle_reads, N)
            rows = [reads[i].tobytes() for i in range(m)]
            rows_rc = [comp[reads[i]][::-1].tobytes() for i in range(m)]

            def occ(lo_hi):
                return [oracle.occurrences(rows[i]) + oracle.occurrences(rows_rc[i]) for i in range(*lo_hi)]

            t0 = time.perf_counter()
            cuts = [(m * t // args.threads, m * (t + 1) // args.threads) for t in range(args.threads)]
            with ThreadPoolExecutor(args.threads) as ex:
                parts = list(ex.map(occ, cuts))
            d_s = (time.perf_counter() - t0) * N / m
            same = same and [int(x) for x in want[:m]] == [x for p in parts for x in p]
            b, c = statistics.median(b_s[1:]), statistics.median(c_s[1:])
            total = 2 * N * K
            result["sets"][name] = {
                "a_device_ms_median": a_ms, "a_device_ms_min": min(a_all), "a_device_ms_max": max(a_all),
                "a_reads_per_s": N / (a_ms * 1e-3), "b_match_batch_wall_s": b, "c_kmer_count_route_wall_s": c,
                "d_oracle_wall_s_scaled": d_s, "ratio_c_over_b": c / b, "ratio_d_over_b": d_s / b,
                "chains_run": stat[0], "symbols_consumed": stat[1], "total_chain_symbols": total, "sectors": stat[2],
                "counts_equal": same, "reads_found": int((want > 0).sum())}
            ok = ok and same and b <= c and (name == "as_indexed" or stat[1] < total)
        pair.close()
    result["accepted"] = ok
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
