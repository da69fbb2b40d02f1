#!/usr/bin/env python3
"""Measures `siga unitig --scaffold` (sigax_scaffold_device) next to the unitig call and the pairs call it follows, on the paired
read sets of tools/pairs_bench.py (BASELINE configs[1] shape: 1 M x 150 bp reads of a 5 Mb genome, seed 1, m = 45, drawn in pairs
at a fixed insert; error-free, and with the bench's 1 % substitutions).  Per read set two GPU steps, each a child process under
a `timeout` of its own; a step is not started when the one before it failed:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run in one device batch, its records left on the device; then by HIP events on the caller's stream,
            median of --steps calls after --warmup: sigax_unitigs_device, sigax_unitigs_pairs_device over what it left,
            sigax_scaffold_device over both (the layout alone, then with a bases buffer of exactly the size the layout gave), and
            the bases pass alone: its bytes (unitig bases in, scaffold bases out), GB/s and share of an 8 TB/s peak
With --ab-lib (the parent commit's libsigax.so) the unitig and the pairs entry points also run through that library and through
this tree's over the same device buffers, in alternating order, on the last read set.
One JSON document on stdout (and in --out).  Needs a GPU; nothing but this repository.

    python tools/scaffold_bench.py --out profiles/scaffold_configs1.json
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

from tools.pairs_bench import STATUS6, reads_of, step_index  # noqa: E402

PEAK_GBS = 8000.0


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
        wu, wq, ws = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert L.sigax_unitigs_workspace(n, ne, C.byref(wu)) == 0 and L.sigax_unitigs_pairs_workspace(0, n, C.byref(wq)) == 0
        assert L.sigax_scaffold_workspace(n, n // 2, C.byref(ws)) == 0
        d_len, d_seqs, d_offs, d_mate = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs), dbuf(mate.nbytes, mate)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_stat, d_work = dbuf(96), dbuf(wu.value)
        bins = args.bins
        d_hist, d_links, d_st24, d_pwork = dbuf(8 * bins), dbuf(24 * (n // 2)), dbuf(192), dbuf(wq.value)
        d_sco, d_scl, d_scf, d_slay, d_st16, d_swork = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(128), dbuf(ws.value)
        popts = _lib.PairsOpts(0, bins, 0, 0, args.max_span)
        sopts = _lib.ScaffoldOpts(_lib.SIGAX_SCAFFOLD_INSERT_FROM_STATUS, args.min_pairs, args.link_ratio, args.min_unitig_bases, 0, 1, args.max_gap)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "error_rate": args.error_rate, "insert": args.insert, "hist_bins": bins, "max_span": args.max_span,
                          "min_pairs": args.min_pairs, "link_ratio": args.link_ratio, "min_unitig_bases": args.min_unitig_bases, "min_gap": 1,
                          "max_gap": args.max_gap, "insert_size": "from the pairs status, on the device", "steps": args.steps, "warmup": args.warmup},
               "edges": ne, "workspace_bytes": {"unitigs": int(wu.value), "pairs": int(wq.value), "scaffold": int(ws.value)}, "calls": []}
        d_status_nl = C.c_void_p(d_st24.value + 22 * 8)

        def unitigs_call(X=L):
            return X.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo, d_uf, d_lay, d_us, d_stat, d_work,
                                          wu.value, stream)

        def pairs_call(X=L):
            return X.sigax_unitigs_pairs_device(0, d_mate, d_len, n, d_stat, d_so, d_lo, d_uf, d_lay, C.byref(popts), d_hist, d_links, d_st24,
                                                d_pwork, wq.value, stream)

        def scaffold_call(d_out, cap, fn=None):
            fn = fn or L.sigax_scaffold_device
            return fn(0, d_stat, n, d_so, d_uf, d_us, nb, d_links, d_status_nl, n // 2, d_st24, C.byref(sopts), d_sco, d_scl, d_scf, d_slay, d_out, cap,
                      d_st16, d_swork, ws.value, stream)

        def fetch(ptr, k):
            s = np.zeros(k, dtype=np.uint64)
            assert hip.hipMemcpy(s.ctypes.data, ptr, 8 * k, 2) == 0
            return [int(x) for x in s]

        t = timed(unitigs_call)
        ustat = dict(zip(STATUS6, fetch(d_stat, 6)))
        t.update({"call": "unitigs_device", "status": ustat})
        out["calls"].append(t)
        t = timed(pairs_call)
        pstat = dict(zip(_lib.PAIRS_STATUS, fetch(d_st24, 24)))
        t.update({"call": "pairs_device", "status": pstat})
        out["calls"].append(t)
        t = timed(lambda: scaffold_call(None, 0))
        layout_only = dict(zip(_lib.SCAFFOLD_STATUS, fetch(d_st16, 16)))
        t.update({"call": "scaffold_device, the layout alone", "status": layout_only})
        out["calls"].append(t)
        total = layout_only["bases"]
        d_out = dbuf(total)
        t = timed(lambda: scaffold_call(d_out, total))
        sstat = dict(zip(_lib.SCAFFOLD_STATUS, fetch(d_st16, 16)))
        assert sstat["bases_not_written"] == 0
        t.update({"call": "scaffold_device", "status": sstat})
        out["calls"].append(t)
        t = timed(lambda: scaffold_call(d_out, total, L.sigax_scaffold_bases_device))
        moved = ustat["bases"] + total
        t.update({"call": "scaffold bases pass alone", "bytes_in": ustat["bases"], "bytes_out": total,
                  "mean_unitig_bases": ustat["bases"] / max(ustat["unitigs"], 1), "gb_per_s": moved / (t["median_ms"] * 1e6),
                  "share_of_8_tb_per_s": moved / (t["median_ms"] * 1e6) / PEAK_GBS})
        out["calls"].append(t)
        if args.ab_lib:
            P = C.CDLL(args.ab_lib)
            for name in ("sigax_unitigs_device", "sigax_unitigs_pairs_device"):
                getattr(P, name).argtypes = getattr(L, name).argtypes
            runs = []
            for order, tree in enumerate(("parent", "this", "this", "parent", "parent", "this"), 1):
                X = P if tree == "parent" else L
                runs.append({"order": order, "tree": tree, "unitigs_device": timed(lambda: unitigs_call(X)), "pairs_device": timed(lambda: pairs_call(X))})
            summary = {}
            for call in ("unitigs_device", "pairs_device"):
                mean = {tree: float(np.mean([r[call]["median_ms"] for r in runs if r["tree"] == tree])) for tree in ("parent", "this")}
                spreads = [(r[call]["max_ms"] - r[call]["min_ms"]) / r[call]["median_ms"] for r in runs]
                summary[call] = {"mean_of_medians_ms": mean, "this_over_parent": mean["this"] / mean["parent"],
                                 "largest_spread_of_a_run": max(spreads), "smallest_spread_of_a_run": min(spreads)}
            out["old_entry_ab"] = {"what": "the unitig and the pairs device entry points through the parent commit's library and through this "
                                           "tree's, over the same device buffers in one process, HIP events, median of %d calls after %d, in the "
                                           "order given" % (args.steps, args.warmup), "runs": runs, "summary": summary}
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    with open(os.path.join(args.dir, "scaffold.json"), "w") as f:
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
    ap.add_argument("--min-pairs", type=int, default=2)
    ap.add_argument("--link-ratio", type=int, default=0)
    ap.add_argument("--min-unitig-bases", type=int, default=0)
    ap.add_argument("--max-gap", type=int, default=1000000)
    ap.add_argument("--sets", default="0,0.01", help="read sets to measure: error rates, comma separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-lib", default=None, help="the parent commit's libsigax.so: A/B of the unitig and pairs entry points on the last read set")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--error-rate", type=float, default=0.0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "index":
        return step_index(args)
    if args.step == "measure":
        return step_measure(args)
    result = {"sets": []}
    rates = [float(s) for s in args.sets.split(",")]
    for k, rate in enumerate(rates):
        with tempfile.TemporaryDirectory() as d:
            for step in ("index", "measure"):  # the next step only after a clean exit of the one before
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d,
                       "--error-rate", str(rate)]
                for key in ("reads", "genome", "length", "insert", "seed", "min_overlap", "bins", "max_span", "min_pairs", "link_ratio",
                            "min_unitig_bases", "max_gap", "steps", "warmup"):
                    cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
                if step == "measure" and args.ab_lib and k == len(rates) - 1:
                    cmd += ["--ab-lib", os.path.abspath(args.ab_lib)]
                rc = subprocess.call(cmd, cwd=ROOT)
                if rc != 0:
                    print("step %s (error rate %g) ended with status %d" % (step, rate, rc), file=sys.stderr)
                    return 1
            with open(os.path.join(d, "scaffold.json")) as f:
                result["sets"].append(json.load(f))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
