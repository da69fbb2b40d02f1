#!/usr/bin/env python3
"""Measures chimeric unitig removal in the rounds of `siga unitig` (sigax_unitigs_chimeric_device) on the inputs of
tools/prune_bench.py: the edge records of one overlap run over BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1,
m = 45), error-free, with the bench's 1 % substitutions, and the 1 % set with --bridges of its reads replaced by reads made of
the halves of two other reads (a bridge between two places of the genome).  Per read set two GPU steps, each a child process
under a `timeout` of its own; a step is not started when the one before it failed:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run in one device batch, its records left on the device; then by HIP events on the caller's stream,
            median of --steps calls after --warmup: sigax_unitigs_prune_device and sigax_unitigs_chimeric_device with the same
            options at 1 and 10 rounds, without and with -d 10; N = the reads, G = --genome, T = 13, Tc = 0, L = Lc = 150, no
            coverage tests, no graph
            with --ab-lib: also sigax_unitigs_device, sigax_unitigs_trim_device and sigax_unitigs_prune_device through that
            library (the parent commit's build) and through this one, over the same buffers, in the order parent, this, this,
            parent, parent, this
Reports per call the time and the counts, the chimeric unitigs' reads per round (from removed[]), and derives what a chimeric
step costs: the difference to the prune call, an estimate.  One JSON document on stdout (and in --out; the A/B in --ab-out).
Needs a GPU; nothing but this repository.

    python tools/chimeric_bench.py --out profiles/chimeric_configs1.json
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
from tools import trim_bench  # noqa: E402
from tools.prune_bench import STATUS16  # noqa: E402

STATUS20 = STATUS16 + ("chimeric_unitigs", "chimeric_reads", "chimeric_rounds", "zero2")
CHIMERIC = 0x80000000


def reads_of(args):
    reads, offs = trim_bench.reads_of(args)
    if args.bridges:  # the last reads become bridges: the first half of one read, the second half of another
        rng = np.random.default_rng(args.seed + 200)
        n, half = args.reads, args.length // 2
        a, b = rng.integers(0, n - args.bridges, args.bridges), rng.integers(0, n - args.bridges, args.bridges)
        reads = reads.reshape(n, args.length).copy()
        reads[n - args.bridges:, :half] = reads[a, :half]
        reads[n - args.bridges:, half:] = reads[b, half:]
    return reads, offs


def step_index(args):
    from siga_amd import host
    reads, offs = reads_of(args)
    host.index_build_gpu(reads.reshape(-1), offs, os.path.join(args.dir, "reads"))
    return 0


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
        wp, wc = C.c_uint64(), C.c_uint64()
        assert L.sigax_unitigs_prune_workspace(n, ne, 0, 0, C.byref(wp)) == 0 and L.sigax_unitigs_chimeric_workspace(n, ne, 0, 0, C.byref(wc)) == 0
        d_len, d_seqs, d_offs = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_rm, d_ct, d_stat, d_work = dbuf(4 * n), dbuf(4 * ne), dbuf(160), dbuf(wc.value)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "error_rate": args.error_rate, "bridges": args.bridges, "min_branch_length": args.min_branch_length,
                          "min_chimeric_length": args.min_chimeric_length, "num_reads": n, "genome_size": args.genome, "uniq_threshold": 13.0,
                          "chimeric_threshold": 0.0, "steps": args.steps, "warmup": args.warmup},
               "edges": ne, "workspace_bytes": {"prune": int(wp.value), "chimeric": int(wc.value)}, "calls": []}

        def status(k):
            s = np.zeros(20, dtype=np.uint64)
            assert hip.hipMemcpy(s.ctypes.data, d_stat, 8 * k, 2) == 0
            return dict(zip(STATUS20[:k], (int(x) for x in s[:k])))

        for delta in (0, 10):
            for rounds in (1, 10):
                prune = _lib.PruneOpts(rounds, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, delta, 0, 0, n, args.genome, 13.0)
                opts = _lib.ChimericOpts(prune, args.min_chimeric_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0, 0, 0.0)
                t = timed(lambda: L.sigax_unitigs_prune_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(prune), d_so, d_lo,
                                                               d_uf, d_lay, d_us, d_rm, d_ct, None, d_stat, d_work, wc.value, stream))
                t.update({"call": "prune", "delta": delta, "max_rounds": rounds, "status": status(16)})
                out["calls"].append(t)
                t = timed(lambda: L.sigax_unitigs_chimeric_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(opts), d_so,
                                                                  d_lo, d_uf, d_lay, d_us, d_rm, d_ct, None, d_stat, d_work, wc.value, stream))
                removed = np.zeros(n, dtype=np.uint32)
                assert hip.hipMemcpy(removed.ctypes.data, d_rm, 4 * n, 2) == 0
                chim = removed[(removed & CHIMERIC) != 0] & ~np.uint32(CHIMERIC)
                planted = removed[n - args.bridges:] if args.bridges else removed[:0]
                t.update({"call": "chimeric", "delta": delta, "max_rounds": rounds, "status": status(20),
                          "chimeric_reads_per_round": np.bincount(chim, minlength=rounds + 1)[1:].tolist(),
                          "planted_removed_as_chimeric": int(((planted & CHIMERIC) != 0).sum()), "planted_removed_at_all": int((planted != 0).sum())})
                out["calls"].append(t)
        out["derived"] = []
        for delta in (0, 10):
            by = {(c["call"], c["max_rounds"]): c for c in out["calls"] if c["delta"] == delta}
            for rounds in (1, 10):
                p, c = by[("prune", rounds)], by[("chimeric", rounds)]
                out["derived"].append({"delta": delta, "max_rounds": rounds, "prune_ms": p["median_ms"], "chimeric_ms": c["median_ms"],
                                       "chimeric_steps_ms": c["median_ms"] - p["median_ms"],
                                       "per_round_ms": (c["median_ms"] - p["median_ms"]) / rounds,
                                       "unitigs_left": {"prune": p["status"]["unitigs"], "chimeric": c["status"]["unitigs"]}})
        if args.ab_lib:
            P = C.CDLL(args.ab_lib)
            for name in ("sigax_unitigs_device", "sigax_unitigs_trim_device", "sigax_unitigs_prune_device"):
                getattr(P, name).argtypes = getattr(L, name).argtypes
            topts = _lib.TrimOpts(10, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
            popts = _lib.PruneOpts(10, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 10, 0, 0, n, args.genome, 13.0)
            runs = []
            for order, tree in enumerate(("parent", "this", "this", "parent", "parent", "this"), 1):
                X = P if tree == "parent" else L
                run = {"order": order, "tree": tree}
                run["unitigs_device"] = timed(lambda: X.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo,
                                                                             d_uf, d_lay, d_us, d_stat, d_work, wc.value, stream))
                run["trim_device_10_rounds"] = timed(lambda: X.sigax_unitigs_trim_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap,
                                                                                         C.byref(topts), d_so, d_lo, d_uf, d_lay, d_us, d_rm, None,
                                                                                         d_stat, d_work, wc.value, stream))
                run["prune_device_10_rounds"] = timed(lambda: X.sigax_unitigs_prune_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap,
                                                                                           C.byref(popts), d_so, d_lo, d_uf, d_lay, d_us, d_rm, d_ct,
                                                                                           None, d_stat, d_work, wc.value, stream))
                runs.append(run)
            summary = {}
            for call in ("unitigs_device", "trim_device_10_rounds", "prune_device_10_rounds"):
                mean = {tree: float(np.mean([r[call]["median_ms"] for r in runs if r["tree"] == tree])) for tree in ("parent", "this")}
                spreads = [(r[call]["max_ms"] - r[call]["min_ms"]) / r[call]["median_ms"] for r in runs]
                summary[call] = {"mean_of_medians_ms": mean, "this_over_parent": mean["this"] / mean["parent"],
                                 "largest_spread_of_a_run": max(spreads), "smallest_spread_of_a_run": min(spreads)}
            out["old_entry_ab"] = {"what": "the three older device entry points through the parent commit's library and through this tree's, over "
                                           "the same device buffers in one process, HIP events, median of %d calls after %d, in the order "
                                           "given" % (args.steps, args.warmup), "config": out["config"], "runs": runs, "summary": summary}
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    with open(os.path.join(args.dir, "chimeric.json"), "w") as f:
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
    ap.add_argument("--min-chimeric-length", type=int, default=150)
    ap.add_argument("--sets", default="0:0,0.01:0,0.01:2000", help="read sets to measure, error rate:bridge reads, comma separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-lib", default=None, help="the parent commit's libsigax.so: A/B of the older entry points on the last read set")
    ap.add_argument("--ab-out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--error-rate", type=float, default=0.0, help=argparse.SUPPRESS)
    ap.add_argument("--bridges", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "index":
        return step_index(args)
    if args.step == "measure":
        return step_measure(args)
    result = {"sets": []}
    sets = [(float(s.split(":")[0]), int(s.split(":")[1])) for s in args.sets.split(",")]
    for k, (rate, bridges) in enumerate(sets):
        with tempfile.TemporaryDirectory() as d:
            for step in ("index", "measure"):  # the next step only after a clean exit of the one before
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d,
                       "--error-rate", str(rate), "--bridges", str(bridges)]
                for key in ("reads", "genome", "length", "seed", "min_overlap", "min_branch_length", "min_chimeric_length", "steps", "warmup"):
                    cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
                if step == "measure" and args.ab_lib and k == len(sets) - 1:
                    cmd += ["--ab-lib", os.path.abspath(args.ab_lib)]
                rc = subprocess.call(cmd, cwd=ROOT)
                if rc != 0:
                    print("step %s (error rate %g, %d bridges) ended with status %d" % (step, rate, bridges, rc), file=sys.stderr)
                    return 1
            with open(os.path.join(d, "chimeric.json")) as f:
                one = json.load(f)
            ab = one.pop("old_entry_ab", None)
            result["sets"].append(one)
            if ab and args.ab_out:
                with open(args.ab_out, "w") as f:
                    f.write(json.dumps(ab, indent=1) + "\n")
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
