#!/usr/bin/env python3
"""Measures the mate-pair pass of `siga unitig --pairs` (sigax_unitigs_pairs_device) next to the unitig call that feeds it, on
read sets shaped like BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1, m = 45) but drawn in pairs at a fixed
insert: read 2k is the genome at a random place, on a random strand, read 2k + 1 the other strand --insert bases on, so the two
point at each other; the ids are then shuffled.  Error-free, and with the bench's 1 % substitutions.  Per read set two GPU steps,
each a child process under a `timeout` of its own; a step is not started when the one before it failed:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run in one device batch, its records left on the device; then by HIP events on the caller's stream,
            median of --steps calls after --warmup: sigax_unitigs_device, and sigax_unitigs_pairs_device over what it left; then
            sigax_unitigs_trim_device at 10 rounds and the pairs call over that (a layout with reads missing)
Reports per call the time and the counts.  One JSON document on stdout (and in --out).  Needs a GPU; nothing but this repository.

    python tools/pairs_bench.py --out profiles/pairs_configs1.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATUS6 = ("unitigs", "bases", "malformed", "below_min_overlap", "merged", "cycles")


def reads_of(args):
    """-> (uint8 [N, L] of ASCII, offs u64[N + 1], mate u32[N])"""
    from tests.golden.make_reads import substitute
    rng = np.random.default_rng(args.seed)
    n, L, I = args.reads, args.length, args.insert
    assert n % 2 == 0 and I >= L
    genome = rng.integers(0, 4, size=args.genome, dtype=np.uint8)
    pos = rng.permutation(args.genome - I + 1)[:n // 2].astype(np.int64)  # distinct places
    win = np.lib.stride_tricks.sliding_window_view(genome, L)
    left, right = win[pos], (3 - win[pos + I - L])[:, ::-1]  # the left read forward, the right read reverse-complemented
    flip = rng.random(n // 2) < 0.5  # which of the two is read 2k
    codes = np.empty((n, L), dtype=np.uint8)
    codes[0::2] = np.where(flip[:, None], right, left)
    codes[1::2] = np.where(flip[:, None], left, right)
    order = rng.permutation(n)  # read 2k, 2k + 1 get the ids order[2k], order[2k + 1]
    reads = np.empty((n, L), dtype=np.uint8)
    reads[order] = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    mate = np.empty(n, dtype=np.uint32)
    mate[order[0::2]] = order[1::2]
    mate[order[1::2]] = order[0::2]
    if args.error_rate:
        reads = substitute(reads, args.error_rate, args.seed + 100)
    return reads, np.arange(n + 1, dtype=np.uint64) * np.uint64(L), mate


def step_index(args):
    from siga_amd import host
    reads, offs, _ = reads_of(args)
    host.index_build_gpu(reads.reshape(-1), offs, os.path.join(args.dir, "reads"))
    return 0


def step_measure(args):
    import siga_amd
    from siga_amd import _lib
    from tools.locate_bench import hip_runtime
    from tools.unitig_bench import spread
    hip, L = hip_runtime(), _lib.lib()
    reads, offs, mate = reads_of(args)
    n, nb = args.reads, reads.size
    lengths = np.full(n, args.length, dtype=np.uint32)
    flat = np.ascontiguousarray(reads.reshape(-1))
    held = []

    def dbuf(nbytes, src=None):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(nbytes, 16)) == 0
        held.append(q)
        if src is not None and src.nbytes:
            assert hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        return q

    stream = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed(call):
        ms = []
        for i in range(args.warmup + args.steps):
            assert hip.hipEventRecord(ev[0], stream) == 0
            assert call() == 0, _lib.last_error()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
            if i >= args.warmup:
                ms.append(float(t.value))
        return spread(ms)

    pair = siga_amd.FMIndexPair.load(os.path.join(args.dir, "reads"), device=0, with_sai=True, resident=True)
    bt = C.c_void_p()
    try:
        pair.set_reads(lengths, np.arange(n, dtype=np.uint32))
        pair.prepare_overlap(args.min_overlap)
        assert L.sigax_batch_create(pair.handle, n, nb, args.length, C.byref(bt)) == 0, _lib.last_error()
        flags = _lib.SIGAX_EDGES | _lib.SIGAX_IRREDUCIBLE | _lib.SIGAX_RC
        stats = _lib.Stats()
        assert L.sigax_batch_upload(bt, C.c_char_p(flat.ctypes.data), offs.ctypes.data, n, stream) == 0, _lib.last_error()
        assert L.sigax_batch_run(bt, 0, args.min_overlap, flags, stream) == 0, _lib.last_error()
        assert L.sigax_batch_finish(bt, stream, C.byref(stats)) == 0, _lib.last_error()
        d_edges = C.c_void_p()
        assert L.sigax_batch_device_outputs(bt, None, None, None, C.byref(d_edges)) == 0, _lib.last_error()
        ne = int(stats.n_edges)
        wt, wq = C.c_uint64(), C.c_uint64()
        assert L.sigax_unitigs_trim_workspace(n, ne, 0, C.byref(wt)) == 0 and L.sigax_unitigs_pairs_workspace(0, n, C.byref(wq)) == 0
        d_len, d_seqs, d_offs, d_mate = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs), dbuf(mate.nbytes, mate)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_rm, d_stat, d_work = dbuf(4 * n), dbuf(96), dbuf(wt.value)
        bins = args.bins
        d_hist, d_links, d_st24, d_pwork = dbuf(8 * bins), dbuf(24 * (n // 2)), dbuf(192), dbuf(wq.value)
        popts = _lib.PairsOpts(0, bins, 0, 0, args.max_span)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "error_rate": args.error_rate, "insert": args.insert, "hist_bins": bins, "hist_shift": 0, "max_span": args.max_span,
                          "steps": args.steps, "warmup": args.warmup},
               "edges": ne, "workspace_bytes": {"trim": int(wt.value), "pairs": int(wq.value)}, "calls": []}

        def pairs_call():
            return L.sigax_unitigs_pairs_device(0, d_mate, d_len, n, d_stat, d_so, d_lo, d_uf, d_lay, C.byref(popts), d_hist, d_links, d_st24,
                                                d_pwork, wq.value, stream)

        def pairs_status():
            s = np.zeros(24, dtype=np.uint64)
            assert hip.hipMemcpy(s.ctypes.data, d_st24, 192, 2) == 0
            d = dict(zip(_lib.PAIRS_STATUS, (int(x) for x in s)))
            d["insert_size"], d["delta"], d["span_mean"], d["span_sd"] = siga_amd.pairs_estimate(s)
            return d

        def unitig_status(k):
            s = np.zeros(12, dtype=np.uint64)
            assert hip.hipMemcpy(s.ctypes.data, d_stat, 8 * k, 2) == 0
            return {name: int(x) for name, x in zip(STATUS6 + ("trim_rounds", "islands", "dead_ends", "reads_removed", "records_dropped", "lifted"), s[:k])}

        t = timed(lambda: L.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo, d_uf, d_lay, d_us, d_stat,
                                                 d_work, wt.value, stream))
        t.update({"call": "unitigs_device", "status": unitig_status(6)})
        out["calls"].append(t)
        t = timed(pairs_call)
        t.update({"call": "pairs_device after unitigs_device", "status": pairs_status()})
        out["calls"].append(t)
        topts = _lib.TrimOpts(10, 150, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
        t = timed(lambda: L.sigax_unitigs_trim_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(topts), d_so, d_lo, d_uf,
                                                      d_lay, d_us, d_rm, None, d_stat, d_work, wt.value, stream))
        t.update({"call": "unitigs_trim_device, 10 rounds", "status": unitig_status(12)})
        out["calls"].append(t)
        t = timed(pairs_call)
        t.update({"call": "pairs_device after unitigs_trim_device", "status": pairs_status()})
        out["calls"].append(t)
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    with open(os.path.join(args.dir, "pairs.json"), "w") as f:
        json.dump(out, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--insert", type=int, default=500)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--min-overlap", type=int, default=45)
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--max-span", type=int, default=0)
    ap.add_argument("--sets", default="0,0.01", help="read sets to measure: error rates, comma separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--error-rate", type=float, default=0.0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "index":
        return step_index(args)
    if args.step == "measure":
        return step_measure(args)
    result = {"sets": []}
    for rate in (float(s) for s in args.sets.split(",")):
        with tempfile.TemporaryDirectory() as d:
            for step in ("index", "measure"):  # the next step only after a clean exit of the one before
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d,
                       "--error-rate", str(rate)]
                for key in ("reads", "genome", "length", "insert", "seed", "min_overlap", "bins", "max_span", "steps", "warmup"):
                    cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
                rc = subprocess.call(cmd, cwd=ROOT)
                if rc != 0:
                    print("step %s (error rate %g) ended with status %d" % (step, rate, rc), file=sys.stderr)
                    return 1
            with open(os.path.join(d, "pairs.json")) as f:
                result["sets"].append(json.load(f))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
