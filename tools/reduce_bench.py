#!/usr/bin/env python3
"""Measures the transitive reduction in the rounds of `siga unitig` (sigax_unitigs_reduce_device) at BASELINE configs[1]: 1 M x 150 bp
error-free reads of a 5 Mb genome (seed 1), m = 45, over the records of an EXHAUSTIVE overlap run, next to the irreducible run of the
same reads.  Two GPU steps, each a child process under a `timeout` of its own; the second is not started when the first failed:
  index     the reads' FM-index files, built on the GPU
  measure   two overlap runs in one device batch, irreducible (its records copied aside on the device) and exhaustive; then by HIP events
            on the caller's stream, median of --steps calls after --warmup, sigax_unitigs_reduce_device
              over the exhaustive records with reduce = 0 and reduce = 1 at 0 rounds (the difference is one pass), at 1 and at 10 rounds
              with -l (N = the reads, G = --genome, T = 13, Tc = 0, L = Lc = 150, no coverage tests, no cut step, no bubbles, no graph),
              over the irreducible records with reduce = 0 at 0, 1 and 10 rounds (the difference of the first two is a round: with no
              cut, bubble or chimeric removal to do that is its trim step plus one idle-free chimeric step), and with reduce = 1 at 10
            and, on the host, the records the pass left unflagged against the irreducible run's, as unordered (read end, read end,
            overlap) keys, with the containment records and the reads that occur twice (either strand) counted
            with --ab-lib (the parent commit's library): sigax_unitigs_device and the trim, prune, chimeric, bubble, indel and reduce
            device calls (10 rounds) over the irreducible records through that library and through this one, three runs each, in the
            order parent, this, this, parent, parent, this; a call passes when this_over_parent <= 1 + the spread of the parent's medians
One JSON document on stdout (and in --out; the A/B in --ab-out).  Needs a GPU; nothing but this repository.

    python tools/reduce_bench.py --out profiles/reduce_configs1.json
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
from tools.indel_bench import STATUS32  # noqa: E402
from tools.unitig_bench import reads_of, spread, step_index  # noqa: E402

STATUS40 = STATUS32 + ("reduce_flagged_first_pass", "reduce_flagged_final", "reduce_passes", "reduce_participants_last_pass", "_36", "_37",
                       "_38", "_39")
TRANSITIVE = 0x80000000


def keys_of(e):
    """sigax_edge records -> one u64 per record: (smaller state, larger state, overlap), the same whichever read is the query"""
    a = 2 * e["query"].astype(np.uint64) + np.where(e["af"] & 1, 0, 1).astype(np.uint64)
    b = 2 * e["target"].astype(np.uint64) + np.where(e["af"] & 2, 1, 0).astype(np.uint64)
    return (np.minimum(a, b) << np.uint64(40)) | (np.maximum(a, b) << np.uint64(12)) | e["length"].astype(np.uint64)


def step_measure(args):
    import siga_amd
    from siga_amd import _lib
    from tools.locate_bench import hip_runtime
    hip, L = hip_runtime(), _lib.lib()
    reads, offs = reads_of(args)
    n, nb = args.reads, reads.size
    assert n < (1 << 22) and args.length < (1 << 12)  # (keys_of packs two states and a length into 64 bits)
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
           "sigax_unitigs_bubble_device", "sigax_unitigs_indel_device", "sigax_unitigs_reduce_device")
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
        assert L.sigax_batch_upload(bt, C.c_char_p(flat.ctypes.data), offs.ctypes.data, n, stream) == 0, _lib.last_error()
        stats = _lib.Stats()
        d_edges = C.c_void_p()

        def overlap(flags):
            assert L.sigax_batch_run(bt, 0, args.min_overlap, flags, stream) == 0, _lib.last_error()
            assert L.sigax_batch_finish(bt, stream, C.byref(stats)) == 0, _lib.last_error()
            assert L.sigax_batch_device_outputs(bt, None, None, None, C.byref(d_edges)) == 0, _lib.last_error()
            return int(stats.n_edges)

        ne_irr = overlap(_lib.SIGAX_EDGES | _lib.SIGAX_IRREDUCIBLE | _lib.SIGAX_RC)
        d_irr = dbuf(16 * ne_irr)
        assert hip.hipMemcpy(d_irr, d_edges, 16 * ne_irr, 3) == 0
        ne = overlap(_lib.SIGAX_EDGES | _lib.SIGAX_RC)
        d_exh = C.c_void_p(d_edges.value)
        wr, wi = C.c_uint64(), C.c_uint64()
        assert L.sigax_unitigs_reduce_workspace(n, ne, 0, 0, C.byref(wr)) == 0 and L.sigax_unitigs_indel_workspace(n, ne, 0, 0, C.byref(wi)) == 0
        d_len, d_seqs, d_offs = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_rm, d_ct, d_stat, d_work = dbuf(4 * n), dbuf(4 * ne), dbuf(320), dbuf(wr.value)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "min_branch_length": args.min_branch_length, "min_chimeric_length": args.min_chimeric_length, "num_reads": n,
                          "genome_size": args.genome, "uniq_threshold": 13.0, "chimeric_threshold": 0.0, "steps": args.steps, "warmup": args.warmup},
               "records": {"exhaustive": ne, "irreducible": ne_irr, "exhaustive_minus_irreducible": ne - ne_irr},
               "workspace_bytes": {"indel": int(wi.value), "reduce": int(wr.value)}, "calls": []}

        def status():
            s = np.zeros(40, dtype=np.uint64)
            assert hip.hipMemcpy(s.ctypes.data, d_stat, 320, 2) == 0
            return dict(zip(STATUS40, (int(x) for x in s)))

        def opts(rounds, reduce, lc=None, lb=0, edits=0, delta=0):
            prune = _lib.PruneOpts(rounds, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, delta, 0, 0, n, args.genome, 13.0)
            chim = _lib.ChimericOpts(prune, args.min_chimeric_length if lc is None else lc, _lib.SIGAX_TRIM_NO_COVERAGE, 0, 0, 0.0)
            bub = _lib.BubbleOpts(chim, lb, 50, (C.c_uint32 * 2)(0, 0))
            return _lib.ReduceOpts(_lib.IndelOpts(bub, edits, 50, (C.c_uint32 * 2)(0, 0)), reduce, (C.c_uint32 * 3)(0, 0, 0))

        def reduce_call(d_e, k, o):
            return L.sigax_unitigs_reduce_device(0, d_e, k, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(o), d_so, d_lo, d_uf, d_lay, d_us,
                                                 d_rm, d_ct, None, d_stat, d_work, wr.value, stream)

        first_cut = None
        for records, d_e, k, reduce, rounds in (("exhaustive", d_exh, ne, 0, 0), ("exhaustive", d_exh, ne, 1, 0), ("exhaustive", d_exh, ne, 1, 1),
                                                ("exhaustive", d_exh, ne, 1, 10), ("exhaustive", d_exh, ne, 0, 10), ("irreducible", d_irr, ne_irr, 0, 0),
                                                ("irreducible", d_irr, ne_irr, 0, 1), ("irreducible", d_irr, ne_irr, 0, 10),
                                                ("irreducible", d_irr, ne_irr, 1, 10)):
            o = opts(rounds, reduce)
            t = timed(lambda: reduce_call(d_e, k, o))
            t.update({"records": records, "reduce": reduce, "max_rounds": rounds, "status": status()})
            out["calls"].append(t)
            if records == "exhaustive" and reduce == 1 and rounds == 0:
                first_cut = np.zeros(ne, dtype=np.uint32)
                assert hip.hipMemcpy(first_cut.ctypes.data, d_ct, 4 * ne, 2) == 0
        by = {(c["records"], c["reduce"], c["max_rounds"]): c for c in out["calls"]}
        ms = lambda *key: by[key]["median_ms"]  # noqa: E731
        un = lambda *key: by[key]["status"]["unitigs"]  # noqa: E731
        out["derived"] = {
            "one_pass_ms": ms("exhaustive", 1, 0) - ms("exhaustive", 0, 0),
            "a_round_on_the_irreducible_records_ms": ms("irreducible", 0, 1) - ms("irreducible", 0, 0),
            "whole_call_ms": {"exhaustive_reduce_0_rounds": ms("exhaustive", 1, 0), "exhaustive_reduce_1_round": ms("exhaustive", 1, 1),
                              "exhaustive_reduce_10_rounds": ms("exhaustive", 1, 10), "irreducible_10_rounds": ms("irreducible", 0, 10),
                              "irreducible_reduce_10_rounds": ms("irreducible", 1, 10)},
            "flagged_by_the_first_pass": by[("exhaustive", 1, 0)]["status"]["reduce_flagged_first_pass"],
            "unitigs": {"exhaustive_reduce_x10_l": un("exhaustive", 1, 10), "irreducible_x10_l": un("irreducible", 0, 10),
                        "irreducible_reduce_x10_l": un("irreducible", 1, 10), "exhaustive_x10_l_without_reduce": un("exhaustive", 0, 10),
                        "exhaustive_reduce_no_rounds": un("exhaustive", 1, 0), "irreducible_no_rounds": un("irreducible", 0, 0)}}
        # the records the pass left against the irreducible run's, on the host
        exh = np.zeros(ne, dtype=_lib.EDGE_DTYPE)
        irr = np.zeros(ne_irr, dtype=_lib.EDGE_DTYPE)
        assert hip.hipMemcpy(exh.ctypes.data, d_exh, 16 * ne, 2) == 0 and hip.hipMemcpy(irr.ctypes.data, d_irr, 16 * ne_irr, 2) == 0
        left = exh[(first_cut & TRANSITIVE) == 0]
        kl, ki = np.unique(keys_of(left)), np.unique(keys_of(irr))
        only_left, only_irr = np.setdiff1d(kl, ki, assume_unique=True), np.setdiff1d(ki, kl, assume_unique=True)
        codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), reads)  # a read as the smaller of itself and its reverse complement
        rc = (3 - codes)[:, ::-1]
        first_diff = (codes != rc).argmax(axis=1)
        take_rc = rc[np.arange(n), first_diff] < codes[np.arange(n), first_diff]
        canon = np.where(take_rc[:, None], rc, codes).astype(np.uint8)
        rows = np.ascontiguousarray(canon).view(np.dtype((np.void, canon.shape[1]))).reshape(-1)
        _, inverse, counts = np.unique(rows, return_inverse=True, return_counts=True)
        twice = counts[inverse] > 1  # reads that occur more than once, on either strand
        contain = exh["length"] == args.length

        def touching(keys):
            a, b = (keys >> np.uint64(40)).astype(np.int64) >> 1, ((keys >> np.uint64(12)) & np.uint64((1 << 28) - 1)).astype(np.int64) >> 1
            return int((twice[a] | twice[b]).sum())

        out["against_the_irreducible_run"] = {
            "unflagged_exhaustive_records": int(len(left)), "their_distinct_keys": int(len(kl)), "irreducible_records": ne_irr,
            "their_distinct_keys_": int(len(ki)), "keys_only_unflagged": int(len(only_left)), "keys_only_irreducible": int(len(only_irr)),
            "keys_only_unflagged_that_touch_a_read_occurring_twice": touching(only_left),
            "keys_only_irreducible_that_touch_a_read_occurring_twice": touching(only_irr),
            "containment_records_in_the_exhaustive_run": int(contain.sum()), "reads_occurring_twice_either_strand": int(twice.sum()),
            "equal": bool(len(only_left) == 0 and len(only_irr) == 0)}
        if P:
            topts = _lib.TrimOpts(10, args.min_branch_length, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
            ropts = opts(10, 1, lb=150, edits=4, delta=10)
            iopts = ropts.indel
            bopts = iopts.bubble
            copts, popts = bopts.chimeric, bopts.chimeric.prune
            runs = []
            for order, tree in enumerate(("parent", "this", "this", "parent", "parent", "this")):
                X = P if tree == "parent" else L
                run = {"order": order + 1, "tree": tree}
                run["unitigs_device"] = timed(lambda: X.sigax_unitigs_device(0, d_irr, ne_irr, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo,
                                                                             d_uf, d_lay, d_us, d_stat, d_work, wr.value, stream))
                run["trim_device_10_rounds"] = timed(lambda: X.sigax_unitigs_trim_device(0, d_irr, ne_irr, d_len, d_seqs, d_offs, n, args.min_overlap,
                                                                                         C.byref(topts), d_so, d_lo, d_uf, d_lay, d_us, d_rm, None,
                                                                                         d_stat, d_work, wr.value, stream))
                for name, fn, o in (("prune", X.sigax_unitigs_prune_device, popts), ("chimeric", X.sigax_unitigs_chimeric_device, copts),
                                    ("bubble", X.sigax_unitigs_bubble_device, bopts), ("indel", X.sigax_unitigs_indel_device, iopts)):
                    run[name + "_device_10_rounds"] = timed(lambda: fn(0, d_irr, ne_irr, d_len, d_seqs, d_offs, n, args.min_overlap, C.byref(o), d_so,
                                                                       d_lo, d_uf, d_lay, d_us, d_rm, d_ct, None, d_stat, d_work, wr.value, stream))
                run["reduce_device_10_rounds"] = timed(lambda: X.sigax_unitigs_reduce_device(0, d_irr, ne_irr, d_len, d_seqs, d_offs, n, args.min_overlap,
                                                                                             C.byref(ropts), d_so, d_lo, d_uf, d_lay, d_us, d_rm, d_ct,
                                                                                             None, d_stat, d_work, wr.value, stream))
                runs.append(run)
            summary = {}
            for call in [k for k in runs[0] if k not in ("order", "tree")]:
                med = {tree: [r[call]["median_ms"] for r in runs if r["tree"] == tree] for tree in ("parent", "this")}
                rng = {tree: [min(v), max(v)] for tree, v in med.items()}
                ratio = float(np.mean(med["this"]) / np.mean(med["parent"]))
                margin = float((rng["parent"][1] - rng["parent"][0]) / np.mean(med["parent"]))
                summary[call] = {"range_of_medians_ms": rng, "this_over_parent": ratio, "margin": margin, "passes": bool(ratio <= 1.0 + margin)}
            out["old_entry_ab"] = {"what": "the seven device entry points over the irreducible records through the parent commit's library and "
                                           "through this tree's, over the same device buffers in one process, HIP events, median of %d calls after "
                                           "%d, three runs each in the order parent, this, this, parent, parent, this; this_over_parent is the ratio "
                                           "of the means of the medians, the margin the spread of the parent's own medians, (max - min) / mean"
                                           % (args.steps, args.warmup), "config": out["config"], "runs": runs, "summary": summary}
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    with open(os.path.join(args.dir, "reduce.json"), "w") as f:
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-lib", default=None, help="the parent commit's libsigax.so: the A/B of the older entry points runs")
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
            for key in ("reads", "genome", "length", "seed", "min_overlap", "min_branch_length", "min_chimeric_length", "steps", "warmup"):
                cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
            if step == "measure" and args.ab_lib:
                cmd += ["--ab-lib", os.path.abspath(args.ab_lib)]
            rc = subprocess.call(cmd, cwd=ROOT)
            if rc != 0:
                print("step %s ended with status %d" % (step, rc), file=sys.stderr)
                return 1
        with open(os.path.join(d, "reduce.json")) as f:
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
