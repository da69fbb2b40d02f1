#!/usr/bin/env python3
"""Measures `siga overlap -e` at BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1), error-free and with the 1 %
substitutions tools/e2e_aux.py and tools/pileup_bench.py draw.
  device      by HIP events, median of --steps after --warmup, with their spread, one call over all reads: the seeds and their
              hits alone, those and k_mmo (sigax_mmoverlap_stages_device), the whole call, and the finish; k_mmo = the difference
              of the first two, the commit the difference of the next two
  counts      raw and unique records, flags, records by num_diff, the status words
  error-free  at -e 0: the records against the non-containment records of the exhaustive exact run (FMIndexPair.overlap with
              edges), both counts and the records only one of them has
  1 % set     recall at the default seeds (24, 12) and at (16, 4): records found over the true overlaps the reads' places in the
              genome imply (length >= M, mismatches within P, neither read inside the other), and the seconds each setting takes
              through the batch call
One JSON document on stdout (and in --out).  Needs a GPU; nothing but this repository.  --device-only measures the device
section of the 1 % set alone (for A/B runs of two builds of the library, SIGAX_LIB selecting one).

    python tools/mmoverlap_bench.py --out profiles/mmoverlap_configs1.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    return hip


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "stdev_ms": statistics.pstdev(ms)}


def device_times(hip, L, pair, n, nb, params, steps, warmup):
    from siga_amd import _lib
    held = []

    def dbuf(nbytes):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(nbytes, 16)) == 0
        held.append(q)
        return q

    def get(q, dtype, count):
        out = np.zeros(count, dtype=dtype)
        assert hip.hipMemcpy(out.ctypes.data, q, out.nbytes, 2) == 0
        return out

    stream = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    ev = [C.c_void_p() for _ in range(5)]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def elapsed(a, b):
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), a, b) == 0
        return float(t.value)

    ref = C.c_void_p()
    assert L.sigax_pile_ref_create(pair.handle, C.byref(ref)) == 0, _lib.last_error()
    try:
        d_text, d_toffs = C.c_void_p(), C.c_void_p()
        assert L.sigax_pile_ref_buffers(ref, C.byref(d_text), C.byref(d_toffs), None) == 0
        d_cursor, d_contained, d_stat, d_n = dbuf(8), dbuf(n), dbuf(64), dbuf(8)
        wb = C.c_uint64()

        def call(d_edges, cap, d_work, hits_cap, stages=3):
            a = (pair.handle, d_text, d_toffs, 0, n, nb, C.byref(params), d_edges, cap, d_cursor, d_contained, d_stat, d_work, wb.value,
                 hits_cap, stream)
            rc = L.sigax_mmoverlap_device(*a) if stages == 3 else L.sigax_mmoverlap_stages_device(*(a + (stages,)))
            assert rc == 0, _lib.last_error()

        def reset():
            assert hip.hipMemsetAsync(d_cursor, 0, 8, stream) == 0
            assert hip.hipMemsetAsync(d_contained, 0, n, stream) == 0

        # the sizes: the hits the seeds list, then the records the reads emit
        assert L.sigax_mmoverlap_workspace(n, nb, C.byref(params), 0, C.byref(wb)) == 0, _lib.last_error()
        d_work = dbuf(wb.value)
        reset()
        call(None, 0, d_work, 0)
        assert hip.hipStreamSynchronize(stream) == 0
        hits = int(get(d_stat, np.uint64, 8)[0])
        hip.hipFree(held.pop())
        assert L.sigax_mmoverlap_workspace(n, nb, C.byref(params), hits, C.byref(wb)) == 0, _lib.last_error()
        d_work = dbuf(wb.value)
        call(None, 0, d_work, hits)
        assert hip.hipStreamSynchronize(stream) == 0
        n_raw = int(get(d_stat, np.uint64, 8)[7])
        d_edges = dbuf(24 * n_raw)
        fb = C.c_uint64()
        assert L.sigax_mmoverlap_finish_workspace(n_raw, C.byref(fb)) == 0, _lib.last_error()
        d_fwork = dbuf(fb.value)
        seeds_ms, upto_ms, whole_ms, finish_ms = [], [], [], []
        for i in range(warmup + steps):
            reset()
            assert hip.hipEventRecord(ev[0], stream) == 0
            call(d_edges, n_raw, d_work, hits, 1)
            assert hip.hipEventRecord(ev[1], stream) == 0
            call(d_edges, n_raw, d_work, hits, 2)
            assert hip.hipEventRecord(ev[2], stream) == 0
            call(d_edges, n_raw, d_work, hits)
            assert hip.hipEventRecord(ev[3], stream) == 0
            assert L.sigax_mmoverlap_finish_device(d_edges, n_raw, d_n, d_fwork, fb.value, stream) == 0, _lib.last_error()
            assert hip.hipEventRecord(ev[4], stream) == 0
            assert hip.hipEventSynchronize(ev[4]) == 0
            if i >= warmup:
                seeds_ms.append(elapsed(ev[0], ev[1]))
                upto_ms.append(elapsed(ev[1], ev[2]))
                whole_ms.append(elapsed(ev[2], ev[3]))
                finish_ms.append(elapsed(ev[3], ev[4]))
        stat = get(d_stat, np.uint64, 8)
        n_unique = int(get(d_n, np.uint64, 1)[0])
        edges = get(d_edges, _lib.MM_EDGE_DTYPE, n_unique)
        contained = get(d_contained, np.uint8, n)
    finally:
        L.sigax_pile_ref_destroy(ref)
        for q in held:
            hip.hipFree(q)
        L.sigax_stream_destroy(0, stream)
    out = {"reads": n, "bases": nb, "seeds_and_locate": spread(seeds_ms), "seeds_locate_and_k_mmo": spread(upto_ms),
           "k_mmo": spread([b - a for a, b in zip(seeds_ms, upto_ms)]), "whole_call": spread(whole_ms),
           "commit": spread([b - a for a, b in zip(upto_ms, whole_ms)]), "finish": spread(finish_ms),
           "workspace_bytes": int(wb.value), "finish_workspace_bytes": int(fb.value), "status8": [int(v) for v in stat],
           "records_raw": n_raw, "records_unique": n_unique, "reads_flagged": int(np.count_nonzero(contained)),
           "records_by_num_diff": {str(k): int(v) for k, v in enumerate(np.bincount(edges["num_diff"])) if v},
           "pileup_round_ms_for_comparison": 140.0}
    return out, edges, contained


def record_keys(q, t, af, length, n):
    return ((q.astype(np.uint64) * np.uint64(n) + t.astype(np.uint64)) * np.uint64(8) + af.astype(np.uint64)) * np.uint64(4096) + length.astype(np.uint64)


def pair_keys(a, b):
    lo, hi = np.minimum(a, b).astype(np.uint64), np.maximum(a, b).astype(np.uint64)
    return (lo << np.uint64(32)) | hi


def places(reads, genome_codes, K):
    """where every error-free read lies: (position, reversed) from its first 31 bases, forward or reverse-complemented"""
    w = 31
    lut = np.zeros(256, dtype=np.uint64)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    g = genome_codes.astype(np.uint64)
    gk = np.zeros(len(g) - w + 1, dtype=np.uint64)
    for j in range(w):
        gk = gk * np.uint64(4) + g[j:len(g) - w + 1 + j]
    order = np.argsort(gk, kind="stable")
    gs = gk[order]
    codes = lut[reads]
    fk = np.zeros(len(reads), dtype=np.uint64)
    rk = np.zeros(len(reads), dtype=np.uint64)
    for j in range(w):
        fk = fk * np.uint64(4) + codes[:, j]
        rk = rk * np.uint64(4) + (np.uint64(3) - codes[:, K - 1 - j])
    at = np.searchsorted(gs, fk)
    hit = (at < len(gs)) & (gs[np.minimum(at, len(gs) - 1)] == fk)
    at2 = np.searchsorted(gs, rk)
    pos = np.where(hit, order[np.minimum(at, len(gs) - 1)], order[np.minimum(at2, len(gs) - 1)])
    return pos.astype(np.int64), ~hit


def true_overlaps(noisy, pos, rev, K, M, P):
    """the pairs whose places overlap in M .. K - 1 columns with mismatches within P -> their keys"""
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    fwd = noisy.copy()
    fwd[rev] = comp[noisy[rev]][:, ::-1]
    order = np.argsort(pos, kind="stable")
    sp, sf = pos[order], fwd[order]
    keys = []
    k = 1
    while True:
        delta = sp[k:] - sp[:-k]
        near = np.nonzero((delta >= 1) & (delta <= K - M))[0]
        if not np.any(delta <= K - M):
            break
        for d in np.unique(delta[near]):
            i = near[delta[near] == d]
            m = (sf[i][:, d:] != sf[i + k][:, :K - d]).sum(axis=1)
            ok = m <= ((K - d) * P) // 1000
            keys.append(pair_keys(order[i[ok]], order[i[ok] + k]))
        k += 1
    return np.unique(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.uint64)


def emit(result, out):
    text = json.dumps(result, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--permille", type=int, default=40)
    ap.add_argument("--min-overlap", type=int, default=45)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()

    import siga_amd
    from siga_amd import _lib, host
    from tests.golden.make_reads import fast_reads, rank_of_r_names
    hip, L = hip_runtime(), _lib.lib()
    N, K, M, P = args.reads, args.length, args.min_overlap, args.permille
    reads, genome = fast_reads(5 * N, K, N, args.seed)
    rng = np.random.default_rng(4)
    noisy = reads.copy()
    flips = rng.random(noisy.shape) < args.error
    noisy[flips] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(flips.sum()))]
    offs = np.arange(N + 1, dtype=np.uint64) * np.uint64(K)
    lengths, ranks = np.full(N, K, dtype=np.uint32), rank_of_r_names(N)
    result = {"config": {"reads": N, "read_length": K, "genome": 5 * N, "seed": args.seed, "substitution_rate": args.error, "min_overlap": M,
                         "error_permille": P, "steps": args.steps, "warmup": args.warmup}}

    with tempfile.TemporaryDirectory() as d:
        if args.device_only:
            prefix = os.path.join(d, "noisy")
            host.index_build_gpu(noisy.reshape(-1), offs, prefix)
            pair = siga_amd.FMIndexPair.load_forward(prefix, device=0)
            pair.set_reads(lengths, ranks)
            result["noisy_defaults"] = device_times(hip, L, pair, N, N * K, _lib.MmoParams(P, min_overlap=M, max_read_len=K), args.steps, args.warmup)[0]
            pair.close()
            return emit(result, args.out)
        # ---- error-free, -e 0 ----
        prefix = os.path.join(d, "clean")
        host.index_build_gpu(reads.reshape(-1), offs, prefix)
        pair = siga_amd.FMIndexPair.load(prefix, device=0, resident=False)
        pair.set_reads(lengths, ranks)
        dev, edges, contained = device_times(hip, L, pair, N, N * K, _lib.MmoParams(0, min_overlap=M, max_read_len=K), args.steps, args.warmup)
        seqs = [bytes(r) for r in reads]
        exact = siga_amd.OverlapBuilder(pair, irreducible=False, rc=True).overlap(seqs, M, edges=True)
        pair.close()
        ex = exact["edges"]
        a = np.unique(record_keys(edges["query"], edges["target"], edges["af"], edges["length"], N))
        b = np.unique(record_keys(ex["query"], ex["target"], ex["af"], ex["length"], N))
        dev["against_exact_exhaustive"] = {"records": int(len(a)), "exact_records": int(len(b)), "exact_edges_listed": int(len(ex)),
                                           "only_mismatch_path": int(len(np.setdiff1d(a, b, assume_unique=True))),
                                           "only_exact_path": int(len(np.setdiff1d(b, a, assume_unique=True))),
                                           "exact_substring_reads": int(np.count_nonzero(exact["substring"]))}
        result["error_free_e0"] = dev

        # ---- 1 % substitutions ----
        prefix = os.path.join(d, "noisy")
        host.index_build_gpu(noisy.reshape(-1), offs, prefix)
        pair = siga_amd.FMIndexPair.load_forward(prefix, device=0)
        pair.set_reads(lengths, ranks)
        dev, edges, contained = device_times(hip, L, pair, N, N * K, _lib.MmoParams(P, min_overlap=M, max_read_len=K), args.steps, args.warmup)
        result["noisy_defaults"] = dev
        pos, rev = places(reads, genome, K)
        truth = true_overlaps(noisy, pos, rev, K, M, P)
        recall = []
        for S, T in ((24, 12), (16, 4)):
            t0 = time.time()
            e, c, st = pair.overlap_mismatch(P, M, seed_length=S, seed_stride=T)
            secs = time.time() - t0
            found = np.unique(pair_keys(e["query"], e["target"]))
            recall.append({"seed_length": S, "seed_stride": T, "seconds_batch_call": secs, "records": int(len(e)), "pairs_found": int(len(found)),
                           "true_pairs": int(len(truth)), "true_pairs_found": int(np.isin(truth, found, assume_unique=True).sum()),
                           "recall": float(np.isin(truth, found, assume_unique=True).sum()) / max(len(truth), 1),
                           "pairs_found_not_true": int((~np.isin(found, truth, assume_unique=True)).sum()), "reads_flagged": int(np.count_nonzero(c)),
                           "status8": [int(v) for v in st]})
        pair.close()
        result["noisy_recall"] = recall
    return emit(result, args.out)


if __name__ == "__main__":
    sys.exit(main())
