#!/usr/bin/env python3
"""Measures `siga unitig` at BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1, m = 45).  Two GPU steps, each a
child process of this script under a `timeout` of its own; the second is not started when the first fails:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run over all reads in one device batch (irreducible, both strands; run twice, the second timed: HIP
            events on the caller's stream round sigax_batch_run, and the library's own per-kernel events,
            sigax_batch_kernel_ms).  Its edge records stay where the run left them (sigax_batch_device_outputs), and
            sigax_unitigs_device runs over them --steps times after --warmup, by HIP events: the whole call, and its bases
            pass alone (the library's measurement aid, over the scratch the call left)
Reports the medians with their spread, the bases pass's bytes (bases read + unitig bases written) per second as a fraction
of the 8 TB/s HBM peak DESIGN.md uses, and the call's share of the overlap run's device time.  One JSON document on stdout
(and in --out).  Needs a GPU; nothing but this repository.

    python tools/unitig_bench.py --out profiles/unitig_configs1.json
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
HBM_PEAK = 8.0e12


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "stdev_ms": statistics.pstdev(ms)}


def reads_of(args):
    from tests.golden.make_reads import fast_reads
    reads, _ = fast_reads(args.genome, args.length, args.reads, args.seed)
    return reads, np.arange(args.reads + 1, dtype=np.uint64) * np.uint64(args.length)


def step_index(args):
    from siga_amd import host
    reads, offs = reads_of(args)
    host.index_build_gpu(reads.reshape(-1), offs, os.path.join(args.dir, "reads"))
    return 0


def step_measure(args):
    import siga_amd
    from siga_amd import _lib
    from tools.locate_bench import hip_runtime
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
    ev = [C.c_void_p() for _ in range(3)]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def elapsed(a, b):
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), a, b) == 0
        return float(t.value)

    pair = siga_amd.FMIndexPair.load(os.path.join(args.dir, "reads"), device=0, with_sai=True, resident=True)
    bt = C.c_void_p()
    try:
        pair.set_reads(lengths, np.arange(n, dtype=np.uint32))
        pair.prepare_overlap(args.min_overlap)
        assert L.sigax_batch_create(pair.handle, n, nb, args.length, C.byref(bt)) == 0, _lib.last_error()
        flags = _lib.SIGAX_EDGES | _lib.SIGAX_IRREDUCIBLE | _lib.SIGAX_RC
        stats = _lib.Stats()
        assert L.sigax_batch_upload(bt, C.c_char_p(flat.ctypes.data), offs.ctypes.data, n, stream) == 0, _lib.last_error()
        overlap_ms = []
        for i in range(2):  # the first run grows arenas and warms tables
            assert hip.hipEventRecord(ev[0], stream) == 0
            assert L.sigax_batch_run(bt, 0, args.min_overlap, flags, stream) == 0, _lib.last_error()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert L.sigax_batch_finish(bt, stream, C.byref(stats)) == 0, _lib.last_error()
            overlap_ms.append(elapsed(ev[0], ev[1]))
        kms, nsub = (C.c_float * 5)(), C.c_uint32()
        assert L.sigax_batch_kernel_ms(bt, C.byref(kms), C.byref(nsub)) == 0
        d_edges = C.c_void_p()
        assert L.sigax_batch_device_outputs(bt, None, None, None, C.byref(d_edges)) == 0, _lib.last_error()
        ne = int(stats.n_edges)
        wb = C.c_uint64()
        assert L.sigax_unitigs_workspace(n, ne, C.byref(wb)) == 0
        d_len, d_seqs, d_offs = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_stat, d_work = dbuf(48), dbuf(wb.value)
        call_ms, bases_ms = [], []
        for i in range(args.warmup + args.steps):
            assert hip.hipEventRecord(ev[0], stream) == 0
            assert L.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo, d_uf, d_lay, d_us, d_stat,
                                          d_work, wb.value, stream) == 0, _lib.last_error()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert L.sigax_unitigs_bases_device(0, d_seqs, d_offs, n, ne, d_us, d_work, wb.value, stream) == 0, _lib.last_error()
            assert hip.hipEventRecord(ev[2], stream) == 0
            assert hip.hipEventSynchronize(ev[2]) == 0
            if i >= args.warmup:
                call_ms.append(elapsed(ev[0], ev[1]))
                bases_ms.append(elapsed(ev[1], ev[2]))
        status = np.zeros(6, dtype=np.uint64)
        assert hip.hipMemcpy(status.ctypes.data, d_stat, 48, 2) == 0
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    b = statistics.median(bases_ms) * 1e-3
    c = statistics.median(call_ms)
    moved = int(nb) + int(status[1])
    out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                      "steps": args.steps, "warmup": args.warmup},
           "edges": ne, "workspace_bytes": int(wb.value),
           "status": dict(zip(("unitigs", "unitig_bases", "malformed", "below_min_overlap", "merged", "cycles"), (int(x) for x in status))),
           "call": spread(call_ms), "bases_pass": spread(bases_ms), "rounds_per_ranking": int(np.ceil(np.log2(n))) + 1,
           "bases_pass_bytes": moved, "bases_pass_bytes_per_s": moved / b if b > 0 else None,
           "bases_pass_fraction_of_hbm_peak": moved / b / HBM_PEAK if b > 0 else None,
           "reads_per_s_call": n / (c * 1e-3),
           "overlap_run_device_ms": overlap_ms[1], "overlap_first_run_device_ms": overlap_ms[0],
           "overlap_kernel_ms": {k: float(v) for k, v in zip(("find", "filter_extract", "filter_extract_general", "order", "edges"), kms)},
           "call_share_of_overlap_run": c / overlap_ms[1]}
    with open(os.path.join(args.dir, "unitigs.json"), "w") as f:
        json.dump(out, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--min-overlap", type=int, default=45)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
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
            for k in ("reads", "genome", "length", "seed", "min_overlap", "steps", "warmup"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
            rc = subprocess.call(cmd, cwd=ROOT)
            if rc != 0:
                print("step %s ended with status %d" % (step, rc), file=sys.stderr)
                return 1
        with open(os.path.join(d, "unitigs.json")) as f:
            result = json.load(f)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
