#!/usr/bin/env python3
"""Measures tip trimming and the lifted records of `siga unitig` (sigax_unitigs_trim_device) on the inputs of
tools/unitig_bench.py: the edge records of one overlap run over BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed
1, m = 45), error-free and with the bench's 1 % substitutions (tests/golden/make_reads.substitute, seed + 100).  Per read set
two GPU steps, each a child process under a `timeout` of its own; a step is not started when the one before it failed:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run in one device batch, its records left on the device; then by HIP events on the caller's stream,
            median of --steps calls after --warmup: sigax_unitigs_device with and without its bases pass (the latter is what
            a trim round repeats), and sigax_unitigs_trim_device at max_rounds 0, 1 and 10, L = 150, no coverage test, with
            and without the graph
Reports per call the time, the rounds that removed something, the reads removed and the unitigs left, and derives the cost of
a round that removes something (rounds 1 against 0) and of the launches of a round that finds nothing to do (what 10 rounds
cost beyond the removing ones).  One JSON document on stdout (and in --out).  Needs a GPU; nothing but this repository.

    python tools/trim_bench.py --out profiles/trim_configs1.json

Where a round's time goes (profiles/trim_round_trace.json): after `--step index --dir D --error-rate 0.01`, run `--step trace` with
the same arguments under `rocprofv3 --kernel-trace -f csv`, then `--analyse <the kernel trace CSV>`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STATUS12 = ("unitigs", "unitig_bases", "malformed", "below_min_overlap", "merged", "cycles", "rounds", "islands", "dead_ends", "reads_removed",
            "records_dropped", "records_lifted")


def reads_of(args):
    from tests.golden.make_reads import fast_reads, substitute
    reads, _ = fast_reads(args.genome, args.length, args.reads, args.seed)
    if args.error_rate:
        reads = substitute(reads, args.error_rate, args.seed + 100)
    return reads, np.arange(args.reads + 1, dtype=np.uint64) * np.uint64(args.length)


def step_index(args):
    from siga_amd import host
    reads, offs = reads_of(args)
    host.index_build_gpu(reads.reshape(-1), offs, os.path.join(args.dir, "reads"))
    return 0


def step_measure(args, trace=False):
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
        wb, wg, w0 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert L.sigax_unitigs_workspace(n, ne, C.byref(w0)) == 0
        assert L.sigax_unitigs_trim_workspace(n, ne, 0, C.byref(wb)) == 0 and L.sigax_unitigs_trim_workspace(n, ne, 1, C.byref(wg)) == 0
        d_len, d_seqs, d_offs = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_rm, d_ue, d_stat, d_work = dbuf(4 * n), dbuf(16 * ne), dbuf(96), dbuf(wg.value)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "error_rate": args.error_rate, "min_branch_length": args.min_branch_length, "steps": args.steps, "warmup": args.warmup},
               "edges": ne, "workspace_bytes": {"unitigs": int(w0.value), "trim": int(wb.value), "trim_with_graph": int(wg.value)}}
        if trace:  # two calls without rounds, two with one: tools/trim_bench.py --analyse reads the second of each off a kernel trace
            for rounds in (0, 0, 1, 1):
                opts = _lib.TrimOpts(rounds, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
                assert L.sigax_unitigs_trim_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(opts), d_so, d_lo, d_uf,
                                                   d_lay, d_us, d_rm, None, d_stat, d_work, wb.value, stream) == 0, _lib.last_error()
                assert hip.hipStreamSynchronize(stream) == 0
            return 0
        out["unitigs_call"] = timed(lambda: L.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo, d_uf,
                                                                   d_lay, d_us, d_stat, d_work, w0.value, stream))
        out["unitigs_call_without_bases"] = timed(lambda: L.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so,
                                                                                 d_lo, d_uf, d_lay, None, d_stat, d_work, w0.value, stream))
        out["trim"] = []
        for graph in (False, True):
            for rounds in (0, 1, 10):
                opts = _lib.TrimOpts(rounds, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
                t = timed(lambda: L.sigax_unitigs_trim_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(opts), d_so, d_lo,
                                                              d_uf, d_lay, d_us, d_rm, d_ue if graph else None, d_stat, d_work,
                                                              wg.value if graph else wb.value, stream))
                status = np.zeros(12, dtype=np.uint64)
                assert hip.hipMemcpy(status.ctypes.data, d_stat, 96, 2) == 0
                t.update({"max_rounds": rounds, "graph": graph, "status": dict(zip(STATUS12, (int(x) for x in status)))})
                out["trim"].append(t)
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    by = {(t["graph"], t["max_rounds"]): t for t in out["trim"]}
    t0, t1, t10 = (by[(False, r)]["median_ms"] for r in (0, 1, 10))
    active = by[(False, 10)]["status"]["rounds"]
    full = min(active + 1, 10)  # the round that finds nothing to remove still runs in full; the ones after it only launch and leave
    out["derived"] = {
        "trim_0_rounds_over_unitigs_call": t0 / out["unitigs_call"]["median_ms"],
        "round_1_ms": t1 - t0,  # (with what the removals change in the pass that writes the result)
        "round_1_over_unitigs_call_without_bases": (t1 - t0) / out["unitigs_call_without_bases"]["median_ms"],
        "rounds_that_removed": active, "rounds_run_in_full": full,
        "ten_rounds_ms": t10 - t0,
        # measurable apart only where round 1 is the one round run in full
        "idle_round_ms": (t10 - t1) / 9 if full == 1 else None,
        "graph_ms": by[(True, 0)]["median_ms"] - t0,
    }
    with open(os.path.join(args.dir, "trim.json"), "w") as f:
        json.dump(out, f)
    return 0


def analyse(path):
    """a rocprofv3 kernel trace (CSV) of `--step trace` -> per kernel the microseconds of the second call without rounds, and of
    the second call with one round split into the round and the pass that writes the result; k_trim_status ends every call,
    k_step_mark the round"""
    import csv
    with open(path) as f:
        rows = list(csv.DictReader(f))
    key = lambda names: next(k for k in rows[0] if k.lower() in names)  # noqa: E731
    kn, ks, ke = key(("kernel_name",)), key(("start_timestamp",)), key(("end_timestamp",))
    rows.sort(key=lambda r: int(r[ks]))
    ends = [i for i, r in enumerate(rows) if "k_trim_status" in r[kn]]
    assert len(ends) == 4, "expected the four calls of --step trace, found %d" % len(ends)

    def part(lo, hi):
        by = {}
        for r in rows[lo:hi]:
            name = r[kn].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            e = by.setdefault(name, {"launches": 0, "us": 0.0})
            e["launches"] += 1
            e["us"] += (int(r[ke]) - int(r[ks])) / 1e3
        return {"span_us": (int(rows[hi - 1][ke]) - int(rows[lo][ks])) / 1e3, "kernel_us": sum(e["us"] for e in by.values()),
                "launches": hi - lo, "kernels": by}

    # (a call's first kernel follows the k_trim_status of the call before it)
    mark = max(i for i in range(ends[2], ends[3]) if "k_step_mark" in rows[i][kn])
    return {"no_rounds": part(ends[0] + 1, ends[1] + 1), "round_1": part(ends[2] + 1, mark + 1), "result_pass_after_round_1": part(mark + 1, ends[3] + 1)}


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
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--error-rate", type=float, default=0.0, help=argparse.SUPPRESS)
    ap.add_argument("--analyse", default=None, help="a rocprofv3 --kernel-trace CSV of `--step trace --dir D` (after `--step index --dir D`): "
                                                    "prints where a round's time goes")
    args = ap.parse_args()
    if args.analyse:
        print(json.dumps(analyse(args.analyse), indent=1))
        return 0
    if args.step == "trace":
        return step_measure(args, trace=True)
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
            with open(os.path.join(d, "trim.json")) as f:
                result["sets"].append(json.load(f))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
