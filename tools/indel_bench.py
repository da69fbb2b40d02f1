#!/usr/bin/env python3
"""Measures indel bubble popping in the rounds of `siga unitig` (sigax_unitigs_indel_device) on a two-haplotype read set of BASELINE
configs[1] shape: 1 M x 150 bp error-free reads, m = 45, drawn half each from a 5 Mb genome (seed 1) and from a copy of it with, every
--every bases in turn, a substitution, a 1-base indel and a 3-base indel (deletions and insertions alternate).  Two GPU steps, each a
child process under a `timeout` of its own; the second is not started when the first failed:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run in one device batch, its records left on the device; then by HIP events on the caller's stream, median of
            --steps calls after --warmup: sigax_unitigs_bubble_device (through --ab-lib, the parent commit's library, when given)
            and sigax_unitigs_indel_device with the same options at 1 and 10 rounds, E = --edits with De = 50 and De = 1000; N = the
            reads, G = --genome, T = 13, Tc = 0, L = Lc = Lb = 150, D = --divergence, no coverage tests, no cut step, no graph
            with --ab-lib: also sigax_unitigs_device, _trim_device, _prune_device, _chimeric_device and _bubble_device (10 rounds)
            through that library and through this one, over the same buffers, in the order parent, this, this, parent, parent, this
Reports per call the time and the counts, the reads the indel steps removed per round (from removed[]), and derives what an indel step
costs: the difference to the bubble call per enqueued round.  How many arms the step leaves out because their span is below 1 is not
counted on the device (tests/indel_cases.py::left_out counts it on the host, at sizes a serial restatement can walk).  One JSON
document on stdout (and in --out; the A/B in --ab-out).  Needs a GPU; nothing but this repository.

    python tools/indel_bench.py --out profiles/indel_configs1.json
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
from tools.bubble_bench import STATUS24  # noqa: E402

STATUS32 = STATUS24 + ("indel_arms_popped", "indel_reads", "indel_rounds", "indel_losers_kept", "indel_losers_not_compared", "_29", "_30", "_31")
INDEL = 0x20000000


def haplotype(genome, every, rng):
    """the copy: at every // 2, + every, ... in turn a substitution, a 1-base indel and a 3-base indel -> (codes, the three counts)"""
    parts, last, counts = [], 0, [0, 0, 0]
    for k, at in enumerate(range(every // 2, len(genome) - 4, every)):
        kind, insertion = k % 3, (k // 3) % 2 == 1
        parts.append(genome[last:at])
        width = (0, 1, 3)[kind]
        if kind == 0:
            parts.append(np.array([(genome[at] + rng.integers(1, 4)) & 3], dtype=np.uint8))
            last = at + 1
        elif insertion:
            parts.append(rng.integers(0, 4, size=width, dtype=np.uint8))
            last = at
        else:
            last = at + width
        counts[kind] += 1
    parts.append(genome[last:])
    return np.concatenate(parts), counts


def reads_of(args):
    """random (position, strand) draws, each from one of the two haplotypes, no read twice from one place, strand and haplotype"""
    rng = np.random.default_rng(args.seed)
    G, L, N = args.genome, args.length, args.reads
    genome = rng.integers(0, 4, size=G, dtype=np.uint8)
    hap, counts = haplotype(genome, args.every, rng)
    npos = min(len(genome), len(hap)) - L + 1
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
    return reads, np.arange(N + 1, dtype=np.uint64) * np.uint64(L), counts


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
    reads, offs, variants = reads_of(args)
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
           "sigax_unitigs_bubble_device")
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
        wb, wi = C.c_uint64(), C.c_uint64()
        assert L.sigax_unitigs_bubble_workspace(n, ne, 0, 0, C.byref(wb)) == 0 and L.sigax_unitigs_indel_workspace(n, ne, 0, 0, C.byref(wi)) == 0
        d_len, d_seqs, d_offs = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_rm, d_ct, d_stat, d_work = dbuf(4 * n), dbuf(4 * ne), dbuf(256), dbuf(wi.value)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "variant_every": args.every, "variants": dict(zip(("substitutions", "indels_of_1", "indels_of_3"), variants)),
                          "min_branch_length": args.min_branch_length, "min_chimeric_length": args.min_chimeric_length,
                          "max_bubble_span": args.max_bubble_span, "divergence_permille": args.divergence, "max_edits": args.edits,
                          "num_reads": n, "genome_size": args.genome, "uniq_threshold": 13.0, "chimeric_threshold": 0.0, "steps": args.steps,
                          "warmup": args.warmup, "bubble_call_through": "the parent commit's library" if P else "this tree's library"},
               "edges": ne, "workspace_bytes": {"bubble": int(wb.value), "indel": int(wi.value)}, "calls": [],
               "arms_left_out_for_span_below_1": "not measured: not counted on the device, and a serial restatement does not walk 1 M reads"}

        def status(k):
            s = np.zeros(32, dtype=np.uint64)
            assert hip.hipMemcpy(s.ctypes.data, d_stat, 8 * k, 2) == 0
            return dict(zip(STATUS32[:k], (int(x) for x in s[:k])))

        def bubble_opts(rounds, delta=0):
            prune = _lib.PruneOpts(rounds, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, delta, 0, 0, n, args.genome, 13.0)
            chim = _lib.ChimericOpts(prune, args.min_chimeric_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0, 0, 0.0)
            return _lib.BubbleOpts(chim, args.max_bubble_span, args.divergence, (C.c_uint32 * 2)(0, 0))

        X = P or L
        for rounds in (1, 10):
            bopts = bubble_opts(rounds)
            t = timed(lambda: X.sigax_unitigs_bubble_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(bopts), d_so,
                                                            d_lo, d_uf, d_lay, d_us, d_rm, d_ct, None, d_stat, d_work, wi.value, stream))
            t.update({"call": "bubble", "max_rounds": rounds, "status": status(24)})
            out["calls"].append(t)
            for permille in (50, 1000):
                iopts = _lib.IndelOpts(bopts, args.edits, permille, (C.c_uint32 * 2)(0, 0))
                t = timed(lambda: L.sigax_unitigs_indel_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(iopts), d_so,
                                                               d_lo, d_uf, d_lay, d_us, d_rm, d_ct, None, d_stat, d_work, wi.value, stream))
                removed = np.zeros(n, dtype=np.uint32)
                assert hip.hipMemcpy(removed.ctypes.data, d_rm, 4 * n, 2) == 0
                ind = removed[(removed & INDEL) != 0] & ~np.uint32(INDEL)
                t.update({"call": "indel_de%d" % permille, "max_rounds": rounds, "status": status(32),
                          "indel_reads_per_round": np.bincount(ind, minlength=rounds + 1)[1:].tolist()})
                out["calls"].append(t)
        out["derived"] = []
        by = {(c["call"], c["max_rounds"]): c for c in out["calls"]}
        for rounds in (1, 10):
            b = by[("bubble", rounds)]
            for name in ("indel_de50", "indel_de1000"):
                i = by[(name, rounds)]
                out["derived"].append({"call": name, "max_rounds": rounds, "bubble_ms": b["median_ms"], "indel_ms": i["median_ms"],
                                       "indel_steps_ms": i["median_ms"] - b["median_ms"],
                                       "per_enqueued_round_ms": (i["median_ms"] - b["median_ms"]) / rounds,
                                       "arms_popped": i["status"]["indel_arms_popped"], "losers_kept": i["status"]["indel_losers_kept"],
                                       "losers_same_span_or_far": i["status"]["indel_losers_not_compared"],
                                       "unitigs_left": {"bubble": b["status"]["unitigs"], name: i["status"]["unitigs"]}})
        if P:
            topts = _lib.TrimOpts(10, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
            bopts = bubble_opts(10, delta=10)
            copts, popts = bopts.chimeric, bopts.chimeric.prune
            runs = []
            for order, tree in enumerate(("parent", "this", "this", "parent", "parent", "this"), 1):
                X = P if tree == "parent" else L
                run = {"order": order, "tree": tree}
                run["unitigs_device"] = timed(lambda: X.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo,
                                                                             d_uf, d_lay, d_us, d_stat, d_work, wi.value, stream))
                run["trim_device_10_rounds"] = timed(lambda: X.sigax_unitigs_trim_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap,
                                                                                         C.byref(topts), d_so, d_lo, d_uf, d_lay, d_us, d_rm, None,
                                                                                         d_stat, d_work, wi.value, stream))
                for name, fn, o in (("prune", X.sigax_unitigs_prune_device, popts), ("chimeric", X.sigax_unitigs_chimeric_device, copts),
                                    ("bubble", X.sigax_unitigs_bubble_device, bopts)):
                    run[name + "_device_10_rounds"] = timed(lambda: fn(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(o), d_so, d_lo,
                                                                       d_uf, d_lay, d_us, d_rm, d_ct, None, d_stat, d_work, wi.value, stream))
                runs.append(run)
            summary = {}
            for call in ("unitigs_device", "trim_device_10_rounds", "prune_device_10_rounds", "chimeric_device_10_rounds", "bubble_device_10_rounds"):
                med = {tree: [r[call]["median_ms"] for r in runs if r["tree"] == tree] for tree in ("parent", "this")}
                mean = {tree: float(np.mean(v)) for tree, v in med.items()}
                spreads = [(r[call]["max_ms"] - r[call]["min_ms"]) / r[call]["median_ms"] for r in runs]
                gap = (max(med["parent"]) - min(med["parent"])) / mean["parent"]
                summary[call] = {"mean_of_medians_ms": mean, "this_over_parent": mean["this"] / mean["parent"],
                                 "widest_gap_between_parent_medians": gap, "largest_spread_of_a_run": max(spreads),
                                 "margin": max(gap, max(spreads)), "within_margin": abs(mean["this"] / mean["parent"] - 1.0) <= max(gap, max(spreads))}
            out["old_entry_ab"] = {"what": "the five older device entry points through the parent commit's library and through this tree's, over "
                                           "the same device buffers in one process, HIP events, median of %d calls after %d, in the order given; "
                                           "margin = the larger of the widest gap between two parent medians and the largest spread of a run"
                                           % (args.steps, args.warmup), "config": out["config"], "runs": runs, "summary": summary}
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    with open(os.path.join(args.dir, "indel.json"), "w") as f:
        json.dump(out, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--every", type=int, default=1000)
    ap.add_argument("--min-overlap", type=int, default=45)
    ap.add_argument("--min-branch-length", type=int, default=150)
    ap.add_argument("--min-chimeric-length", type=int, default=150)
    ap.add_argument("--max-bubble-span", type=int, default=150)
    ap.add_argument("--divergence", type=int, default=50)
    ap.add_argument("--edits", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-lib", default=None, help="the parent commit's libsigax.so: its bubble call is the yardstick, and the A/B of the older "
                                                   "entry points runs")
    ap.add_argument("--ab-out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "index":
        return step_index(args)
    if args.step == "measure":
        return step_measure(args)
    with tempfile.TemporaryDirectory() as d:
        for step in ("index", "measure"):  # the next step only after a clean exit of the one before
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d]
            for key in ("reads", "genome", "length", "seed", "every", "min_overlap", "min_branch_length", "min_chimeric_length", "max_bubble_span",
                        "divergence", "edits", "steps", "warmup"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            if step == "measure" and args.ab_lib:
                cmd += ["--ab-lib", os.path.abspath(args.ab_lib)]
            rc = subprocess.call(cmd, cwd=ROOT)
            if rc != 0:
                print("step %s ended with status %d" % (step, rc), file=sys.stderr)
                return 1
        with open(os.path.join(d, "indel.json")) as f:
            result = json.load(f)
    ab = result.pop("old_entry_ab", None)
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
