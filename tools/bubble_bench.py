#!/usr/bin/env python3
"""Measures bubble popping in the rounds of `siga unitig` (sigax_unitigs_bubble_device) on a two-haplotype read set of BASELINE
configs[1] shape: 1 M x 150 bp reads, m = 45, drawn half each from a 5 Mb genome (seed 1) and from a copy of it with a substitution
every --snp-every bases; error-free, and with the bench's 1 % substitutions.  Per read set two GPU steps, each a child process under
a `timeout` of its own; a step is not started when the one before it failed:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run in one device batch, its records left on the device; then by HIP events on the caller's stream,
            median of --steps calls after --warmup: sigax_unitigs_chimeric_device and sigax_unitigs_bubble_device with the same
            options at 1 and 10 rounds, the bubble call with the bases test (--divergence per mille) and without; N = the reads,
            G = --genome, T = 13, Tc = 0, L = Lc = 150, no coverage tests, no cut step, no graph
            with --ab-lib: also sigax_unitigs_device, _trim_device, _prune_device, _chimeric_device and _bubble_device (10 rounds,
            with the bases test) through that library (the parent commit's build) and through this one, over the same buffers, in
            the order parent, this, this, parent, parent, this; in the same runs the wall-clock time of sigax_unitigs_trim_host and
            sigax_unitigs_bubble_host over host copies of the same arrays, three calls each (allocation and copies included: reported,
            no yardstick); and the chimeric call of the table above is the parent's
Reports per call the time and the counts, the reads the bubble steps removed per round (from removed[]), and derives what a bubble
step costs: the difference to the chimeric call per enqueued round.  Arms and groups are not counted on the device: status24 holds
arms popped and losers kept.  One JSON document on stdout (and in --out; the A/B in --ab-out).  Needs a GPU; nothing but this
repository.

    python tools/bubble_bench.py --out profiles/bubble_configs1.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.chimeric_bench import STATUS20  # noqa: E402

STATUS24 = STATUS20 + ("bubble_arms_popped", "bubble_reads", "bubble_rounds", "bubble_losers_kept")
BUBBLE = 0x40000000


def reads_of(args):
    """unique (position, strand) draws in random order, each from one of the two haplotypes"""
    from tests.golden.make_reads import substitute
    rng = np.random.default_rng(args.seed)
    G, L, N = args.genome, args.length, args.reads
    genome = rng.integers(0, 4, size=G, dtype=np.uint8)
    hap = genome.copy()
    at = np.arange(args.snp_every // 2, G, args.snp_every)
    hap[at] = (hap[at] + rng.integers(1, 4, size=len(at), dtype=np.uint8)) & 3
    npos = G - L + 1
    keys = np.unique(rng.integers(0, 2 * npos, size=int(N * 1.25) + 64, dtype=np.int64))
    while len(keys) < N:
        keys = np.unique(np.concatenate([keys, rng.integers(0, 2 * npos, size=N, dtype=np.int64)]))
    rng.shuffle(keys)
    keys = keys[:N]
    pos, strand = (keys >> 1).astype(np.int64), (keys & 1).astype(bool)
    second = rng.random(N) < 0.5
    codes = np.lib.stride_tricks.sliding_window_view(genome, L)[pos]
    codes[second] = np.lib.stride_tricks.sliding_window_view(hap, L)[pos[second]]
    codes[strand] = (3 - codes[strand])[:, ::-1]
    reads = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    if args.error_rate:
        reads = substitute(reads, args.error_rate, args.seed + 100)
    return reads, np.arange(N + 1, dtype=np.uint64) * np.uint64(L)


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

    OLD = ("sigax_unitigs_device", "sigax_unitigs_trim_device", "sigax_unitigs_prune_device", "sigax_unitigs_chimeric_device",
           "sigax_unitigs_bubble_device", "sigax_unitigs_trim_host", "sigax_unitigs_bubble_host", "sigax_free")
    P = None
    if args.ab_lib:
        P = C.CDLL(args.ab_lib)
        for name in OLD:
            getattr(P, name).argtypes = getattr(L, name).argtypes
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
        wc, wb = C.c_uint64(), C.c_uint64()
        assert L.sigax_unitigs_chimeric_workspace(n, ne, 0, 0, C.byref(wc)) == 0 and L.sigax_unitigs_bubble_workspace(n, ne, 0, 0, C.byref(wb)) == 0
        d_len, d_seqs, d_offs = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_rm, d_ct, d_stat, d_work = dbuf(4 * n), dbuf(4 * ne), dbuf(192), dbuf(wb.value)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "error_rate": args.error_rate, "snp_every": args.snp_every, "min_branch_length": args.min_branch_length,
                          "min_chimeric_length": args.min_chimeric_length, "max_bubble_span": args.max_bubble_span,
                          "divergence_permille": args.divergence, "num_reads": n, "genome_size": args.genome, "uniq_threshold": 13.0,
                          "chimeric_threshold": 0.0, "steps": args.steps, "warmup": args.warmup,
                          "chimeric_call_through": "the parent commit's library" if P else "this tree's library"},
               "edges": ne, "workspace_bytes": {"chimeric": int(wc.value), "bubble": int(wb.value)}, "calls": []}

        def status(k):
            s = np.zeros(24, dtype=np.uint64)
            assert hip.hipMemcpy(s.ctypes.data, d_stat, 8 * k, 2) == 0
            return dict(zip(STATUS24[:k], (int(x) for x in s[:k])))

        X = P or L
        for rounds in (1, 10):
            prune = _lib.PruneOpts(rounds, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0, 0, 0, n, args.genome, 13.0)
            chim = _lib.ChimericOpts(prune, args.min_chimeric_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0, 0, 0.0)
            t = timed(lambda: X.sigax_unitigs_chimeric_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(chim), d_so,
                                                              d_lo, d_uf, d_lay, d_us, d_rm, d_ct, None, d_stat, d_work, wb.value, stream))
            t.update({"call": "chimeric", "max_rounds": rounds, "status": status(20)})
            out["calls"].append(t)
            for name, div in (("bubble", args.divergence), ("bubble_no_bases", _lib.SIGAX_BUBBLE_NO_BASES)):
                opts = _lib.BubbleOpts(chim, args.max_bubble_span, div, (C.c_uint32 * 2)(0, 0))
                t = timed(lambda: L.sigax_unitigs_bubble_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(opts), d_so,
                                                                d_lo, d_uf, d_lay, d_us, d_rm, d_ct, None, d_stat, d_work, wb.value, stream))
                removed = np.zeros(n, dtype=np.uint32)
                assert hip.hipMemcpy(removed.ctypes.data, d_rm, 4 * n, 2) == 0
                bub = removed[(removed & BUBBLE) != 0] & ~np.uint32(BUBBLE)
                t.update({"call": name, "max_rounds": rounds, "status": status(24),
                          "bubble_reads_per_round": np.bincount(bub, minlength=rounds + 1)[1:].tolist()})
                out["calls"].append(t)
        out["derived"] = []
        by = {(c["call"], c["max_rounds"]): c for c in out["calls"]}
        for rounds in (1, 10):
            c = by[("chimeric", rounds)]
            for name in ("bubble", "bubble_no_bases"):
                b = by[(name, rounds)]
                out["derived"].append({"call": name, "max_rounds": rounds, "chimeric_ms": c["median_ms"], "bubble_ms": b["median_ms"],
                                       "bubble_steps_ms": b["median_ms"] - c["median_ms"],
                                       "per_enqueued_round_ms": (b["median_ms"] - c["median_ms"]) / rounds,
                                       "unitigs_left": {"chimeric": c["status"]["unitigs"], name: b["status"]["unitigs"]}})
        if P:
            topts = _lib.TrimOpts(10, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
            popts = _lib.PruneOpts(10, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 10, 0, 0, n, args.genome, 13.0)
            copts = _lib.ChimericOpts(popts, args.min_chimeric_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0, 0, 0.0)
            bopts = _lib.BubbleOpts(copts, args.max_bubble_span, args.divergence, (C.c_uint32 * 2)(0, 0))
            h_edges = np.zeros(ne, dtype=_lib.EDGE_DTYPE)
            if ne:
                assert hip.hipMemcpy(h_edges.ctypes.data, d_edges, 16 * ne, 2) == 0

            def timed_host(X, call, calls=3):
                """wall clock of a host form, its arrays handed back after the clock has stopped"""
                ms = []
                for _ in range(calls):
                    nu, o, st = C.c_uint64(), [C.c_void_p() for _ in range(7)], np.zeros(24, dtype=np.uint64)
                    t0 = time.perf_counter()
                    rc = call(nu, o, st)
                    ms.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, _lib.last_error()
                    for q in o:
                        X.sigax_free(q)
                return spread(ms)

            runs = []
            for order, tree in enumerate(("parent", "this", "this", "parent", "parent", "this"), 1):
                X = P if tree == "parent" else L
                run = {"order": order, "tree": tree}
                run["unitigs_device"] = timed(lambda: X.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo,
                                                                             d_uf, d_lay, d_us, d_stat, d_work, wb.value, stream))
                run["trim_device_10_rounds"] = timed(lambda: X.sigax_unitigs_trim_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap,
                                                                                         C.byref(topts), d_so, d_lo, d_uf, d_lay, d_us, d_rm, None,
                                                                                         d_stat, d_work, wb.value, stream))
                run["prune_device_10_rounds"] = timed(lambda: X.sigax_unitigs_prune_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap,
                                                                                           C.byref(popts), d_so, d_lo, d_uf, d_lay, d_us, d_rm, d_ct,
                                                                                           None, d_stat, d_work, wb.value, stream))
                run["chimeric_device_10_rounds"] = timed(lambda: X.sigax_unitigs_chimeric_device(0, d_edges, ne, d_len, d_seqs, d_offs, n,
                                                                                                 args.min_overlap, C.byref(copts), d_so, d_lo, d_uf,
                                                                                                 d_lay, d_us, d_rm, d_ct, None, d_stat, d_work,
                                                                                                 wb.value, stream))
                run["bubble_device_10_rounds"] = timed(lambda: X.sigax_unitigs_bubble_device(0, d_edges, ne, d_len, d_seqs, d_offs, n,
                                                                                             args.min_overlap, C.byref(bopts), d_so, d_lo, d_uf,
                                                                                             d_lay, d_us, d_rm, d_ct, None, d_stat, d_work,
                                                                                             wb.value, stream))
                run["trim_host_10_rounds"] = timed_host(X, lambda nu, o, st: X.sigax_unitigs_trim_host(
                    0, h_edges.ctypes.data, ne, lengths.ctypes.data, C.c_char_p(flat.ctypes.data), offs.ctypes.data, n, args.min_overlap,
                    C.byref(topts), C.byref(nu), *[C.byref(q) for q in o[:6]], None, st.ctypes.data))
                run["bubble_host_10_rounds"] = timed_host(X, lambda nu, o, st: X.sigax_unitigs_bubble_host(
                    0, h_edges.ctypes.data, ne, lengths.ctypes.data, C.c_char_p(flat.ctypes.data), offs.ctypes.data, n, args.min_overlap,
                    C.byref(bopts), C.byref(nu), *[C.byref(q) for q in o[:7]], None, st.ctypes.data))
                runs.append(run)
            summary = {}
            for call in ("unitigs_device", "trim_device_10_rounds", "prune_device_10_rounds", "chimeric_device_10_rounds", "bubble_device_10_rounds",
                         "trim_host_10_rounds", "bubble_host_10_rounds"):
                mean = {tree: float(np.mean([r[call]["median_ms"] for r in runs if r["tree"] == tree])) for tree in ("parent", "this")}
                spreads = [(r[call]["max_ms"] - r[call]["min_ms"]) / r[call]["median_ms"] for r in runs]
                summary[call] = {"mean_of_medians_ms": mean, "this_over_parent": mean["this"] / mean["parent"],
                                 "largest_spread_of_a_run": max(spreads), "smallest_spread_of_a_run": min(spreads)}
            out["old_entry_ab"] = {"what": "the five device entry points through the parent commit's library and through this tree's, over "
                                           "the same device buffers in one process, HIP events, median of %d calls after %d, in the order "
                                           "given; the two host forms over host copies of the same arrays, wall clock, median of 3 calls"
                                           % (args.steps, args.warmup), "config": out["config"], "runs": runs, "summary": summary}
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    with open(os.path.join(args.dir, "bubble.json"), "w") as f:
        json.dump(out, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--snp-every", type=int, default=1000)
    ap.add_argument("--min-overlap", type=int, default=45)
    ap.add_argument("--min-branch-length", type=int, default=150)
    ap.add_argument("--min-chimeric-length", type=int, default=150)
    ap.add_argument("--max-bubble-span", type=int, default=150)
    ap.add_argument("--divergence", type=int, default=50)
    ap.add_argument("--sets", default="0,0.01", help="read sets to measure: error rates, comma separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-lib", default=None, help="the parent commit's libsigax.so: its chimeric call is the yardstick, and the A/B of the older "
                                                   "entry points runs on the last read set")
    ap.add_argument("--ab-out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--error-rate", type=float, default=0.0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "index":
        return step_index(args)
    if args.step == "measure":
        return step_measure(args)
    result = {"sets": []}
    sets = [float(s) for s in args.sets.split(",")]
    for k, rate in enumerate(sets):
        with tempfile.TemporaryDirectory() as d:
            for step in ("index", "measure"):  # the next step only after a clean exit of the one before
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d,
                       "--error-rate", str(rate)]
                for key in ("reads", "genome", "length", "seed", "snp_every", "min_overlap", "min_branch_length", "min_chimeric_length",
                            "max_bubble_span", "divergence", "steps", "warmup"):
                    cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
                if step == "measure" and args.ab_lib:
                    cmd += ["--ab-lib", os.path.abspath(args.ab_lib)]
                rc = subprocess.call(cmd, cwd=ROOT)
                if rc != 0:
                    print("step %s (error rate %g) ended with status %d" % (step, rate, rc), file=sys.stderr)
                    return 1
            with open(os.path.join(d, "bubble.json")) as f:
                one = json.load(f)
            ab = one.pop("old_entry_ab", None)
            result["sets"].append(one)
            if ab and args.ab_out and k == len(sets) - 1:
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
