#!/usr/bin/env python3
"""Measures non-maximal overlap cutting in the rounds of `siga unitig` (sigax_unitigs_prune_device) on the inputs of
tools/trim_bench.py: the edge records of one overlap run over BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1,
m = 45), error-free and with the bench's 1 % substitutions.  Per read set two GPU steps, each a child process under a `timeout`
of its own; a step is not started when the one before it failed:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run in one device batch, its records left on the device; then by HIP events on the caller's stream,
            median of --steps calls after --warmup: the unchanged sigax_unitigs_device and sigax_unitigs_trim_device (0, 1 and
            10 rounds), and sigax_unitigs_prune_device at 0, 1 and 10 rounds for delta 1 and 10, plain and careful, N = the
            reads, G = --genome, T = 13, L = 150, no coverage test, no graph; one call with the graph per setting at 10 rounds
            for the lifted records
Reports per call the time and the 16 counts, the records cut per round (from cut[]), and derives what a first round costs
(rounds 1 against 0) beside the trim-only round of the same session, the difference being the cut step.  One JSON document on
stdout (and in --out).  Needs a GPU; nothing but this repository.

    python tools/prune_bench.py --out profiles/prune_configs1.json
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
from tools.trim_bench import STATUS12, reads_of, step_index  # noqa: E402

STATUS16 = STATUS12 + ("records_cut", "cut_rounds", "unique_unitigs_round_1", "zero")


def step_measure(args):
    import siga_amd
    from siga_amd import _lib
    from tools.locate_bench import hip_runtime
    from tools.unitig_bench import spread
    hip, L = hip_runtime(), _lib.lib()
    reads, offs = reads_of(args)
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

    def timed(call, steps=None):
        ms = []
        for i in range(args.warmup + (steps or args.steps)):
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
        w0, wt, wp, wc, wg = (C.c_uint64() for _ in range(5))
        assert L.sigax_unitigs_workspace(n, ne, C.byref(w0)) == 0 and L.sigax_unitigs_trim_workspace(n, ne, 0, C.byref(wt)) == 0
        assert L.sigax_unitigs_prune_workspace(n, ne, 0, 0, C.byref(wp)) == 0 and L.sigax_unitigs_prune_workspace(n, ne, 0, 1, C.byref(wc)) == 0
        assert L.sigax_unitigs_prune_workspace(n, ne, 1, 1, C.byref(wg)) == 0
        d_len, d_seqs, d_offs = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_rm, d_ct, d_ue, d_stat, d_work = dbuf(4 * n), dbuf(4 * ne), dbuf(16 * ne), dbuf(128), dbuf(wg.value)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "error_rate": args.error_rate, "min_branch_length": args.min_branch_length, "num_reads": n, "genome_size": args.genome,
                          "uniq_threshold": 13.0, "steps": args.steps, "warmup": args.warmup},
               "edges": ne, "workspace_bytes": {"unitigs": int(w0.value), "trim": int(wt.value), "prune": int(wp.value),
                                                "prune_careful": int(wc.value), "prune_careful_with_graph": int(wg.value)}}

        def status(k):
            s = np.zeros(16, dtype=np.uint64)
            assert hip.hipMemcpy(s.ctypes.data, d_stat, 8 * k, 2) == 0
            return dict(zip(STATUS16[:k], (int(x) for x in s[:k])))

        out["unitigs_call"] = timed(lambda: L.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo, d_uf,
                                                                   d_lay, d_us, d_stat, d_work, w0.value, stream))
        out["trim"] = []
        for rounds in (0, 1, 10):
            opts = _lib.TrimOpts(rounds, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
            for graph in ((False, True) if rounds else (False,)):
                t = timed(lambda: L.sigax_unitigs_trim_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(opts), d_so, d_lo,
                                                              d_uf, d_lay, d_us, d_rm, d_ue if graph else None, d_stat, d_work, wg.value, stream),
                          2 if graph else None)
                t.update({"max_rounds": rounds, "graph": graph, "status": status(12)})
                out["trim"].append(t)
        out["prune"] = []
        for delta in (1, 10):
            for careful in (0, 1):
                for rounds in (0, 1, 10):
                    opts = _lib.PruneOpts(rounds, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, delta, careful, 0, n, args.genome, 13.0)
                    for graph in ((False, True) if rounds else (False,)):
                        t = timed(lambda: L.sigax_unitigs_prune_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(opts),
                                                                       d_so, d_lo, d_uf, d_lay, d_us, d_rm, d_ct, d_ue if graph else None, d_stat,
                                                                       d_work, wg.value, stream), 2 if graph else None)
                        cut = np.zeros(ne, dtype=np.uint32)
                        if ne:
                            assert hip.hipMemcpy(cut.ctypes.data, d_ct, 4 * ne, 2) == 0
                        t.update({"delta": delta, "careful": bool(careful), "max_rounds": rounds, "graph": graph, "status": status(16),
                                  "cut_per_round": np.bincount(cut, minlength=rounds + 1)[1:].tolist()})
                        out["prune"].append(t)
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    tr = {t["max_rounds"]: t for t in out["trim"] if not t["graph"]}
    out["derived"] = []
    for delta in (1, 10):
        for careful in (False, True):
            pr = {t["max_rounds"]: t for t in out["prune"] if t["delta"] == delta and t["careful"] == careful and not t["graph"]}
            round_1, trim_1 = pr[1]["median_ms"] - pr[0]["median_ms"], tr[1]["median_ms"] - tr[0]["median_ms"]
            out["derived"].append({"delta": delta, "careful": careful, "round_1_ms": round_1, "trim_only_round_1_ms": trim_1,
                                   "cut_step_ms": round_1 - trim_1, "cut_step_over_trim_step": (round_1 - trim_1) / trim_1 if trim_1 else None,
                                   "ten_rounds_ms": pr[10]["median_ms"] - pr[0]["median_ms"],
                                   "trim_only_ten_rounds_ms": tr[10]["median_ms"] - tr[0]["median_ms"]})
    for x in out["derived"]:  # what the careful mode adds to a first round: clearing, filling and probing its table
        if x["careful"]:
            plain = next(y for y in out["derived"] if y["delta"] == x["delta"] and not y["careful"])
            x["careful_over_plain_round_1_ms"] = x["round_1_ms"] - plain["round_1_ms"]
            x["key_table_bytes"] = out["workspace_bytes"]["prune_careful"] - out["workspace_bytes"]["prune"] - 8 * n
    with open(os.path.join(args.dir, "prune.json"), "w") as f:
        json.dump(out, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--min-overlap", type=int, default=45)
    ap.add_argument("--min-branch-length", type=int, default=150)
    ap.add_argument("--error-rates", default="0,0.01", help="substitutions per base of the read sets to measure, comma separated")
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
    for rate in [float(x) for x in args.error_rates.split(",")]:
        with tempfile.TemporaryDirectory() as d:
            for step in ("index", "measure"):  # the next step only after a clean exit of the one before
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d,
                       "--error-rate", str(rate)]
                for k in ("reads", "genome", "length", "seed", "min_overlap", "min_branch_length", "steps", "warmup"):
                    cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
                rc = subprocess.call(cmd, cwd=ROOT)
                if rc != 0:
                    print("step %s (error rate %g) ended with status %d" % (step, rate, rc), file=sys.stderr)
                    return 1
            with open(os.path.join(d, "prune.json")) as f:
                result["sets"].append(json.load(f))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
