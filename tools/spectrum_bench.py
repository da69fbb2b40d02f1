#!/usr/bin/env python3
"""Measures `siga preqc` at BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1), every read once (--all):
  index     builds the index files of the read set into --dir
  measure   rows 0 .. n-1 -> lengths -> strings (k_walk, both passes) -> spectrum (k_spectrum) at k = 13, 31, 41, without and
            with the table of 13-mer intervals: device time of each kernel by HIP events (median of --steps after --warmup),
            windows/s, rank-table sectors per window; and the wall time of sigax_kmer_spectrum_rows at k = 31.
            Run it a second time under SIGAX_TWO_STEP=0 with --form one_step for the numbers without two-step lines.
  compose   what the library could do for the same windows before it had the kernel: the windows of --compose-reads reads cut
            out on the host, sigax_kmer_count_batch over them and over their reverse complements, numpy's bincount; against
            sigax_kmer_spectrum_batch on the same strings.  Both wall times, their ratio, equal bins.
  collect   the steps' JSON files -> one document (--out), with the commit it was taken at
Every step is a process of its own; tools/spectrum_bench.sh runs them under their own time limits, chained with &&.
Needs a GPU (not `collect`); nothing but this repository."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (13, 31, 41)


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    return hip


def reads_of(args):
    from tests.golden.make_reads import fast_reads
    reads, _ = fast_reads(args.genome, args.length, args.reads, args.seed)
    return reads, np.arange(args.reads + 1, dtype=np.uint64) * np.uint64(args.length)


def open_forward(prefix):
    import siga_amd
    from siga_amd import _lib
    h = C.c_void_p()
    assert _lib.lib().sigax_index_open((prefix + ".bwt").encode(), None, None, None, 0, C.byref(h)) == 0, _lib.last_error()
    return siga_amd.FMIndexPair(h.value)


def step_index(args, prefix):
    from siga_amd import host
    reads, offs = reads_of(args)
    t0 = time.perf_counter()
    host.index_build_gpu(reads.reshape(-1), offs, prefix)
    return {"index_build_s": time.perf_counter() - t0}


def step_measure(args, prefix):
    from siga_amd import _lib
    hip, L = hip_runtime(), _lib.lib()
    pair = open_forward(prefix)
    n = pair.info()["n_strings"]
    held = []

    def dbuf(nbytes, src=None):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(nbytes, 16)) == 0
        held.append(q)
        if src is not None:
            assert hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        return q

    def down(q, dtype, count):
        out = np.zeros(count, dtype=dtype)
        assert hip.hipMemcpy(out.ctypes.data, q, out.nbytes, 2) == 0
        return out

    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    def timed(call):
        ms = []
        for i in range(args.warmup + args.steps):
            assert hip.hipEventRecord(e0, stream) == 0
            assert call() == 0, _lib.last_error()
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            if i >= args.warmup:
                ms.append(float(t.value))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    out = {"form": args.form, "two_step_env": os.environ.get("SIGAX_TWO_STEP"), "rows": n, "steps": args.steps, "warmup": args.warmup}
    try:
        rows = np.arange(n, dtype=np.uint64)
        d_rows, d_lens, d_status = dbuf(rows.nbytes, rows), dbuf(4 * n), dbuf(24)
        out["k_walk_lengths"] = timed(lambda: L.sigax_string_lengths_device(pair.handle, 0, d_rows, n, 1 << 20, d_lens, None, d_status, stream))
        lens = down(d_lens, np.uint32, n)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens, dtype=np.uint64)
        total = int(offs[-1])
        d_offs, d_seqs = dbuf(offs.nbytes, offs), dbuf(total + 16)
        out["k_walk_write"] = timed(lambda: L.sigax_get_strings_device(pair.handle, 0, d_rows, n, 1 << 20, d_offs, d_seqs, d_status, stream))
        out["walk_status"] = [int(x) for x in down(d_status, np.uint64, 3)]
        out["bases"] = total
        need = C.c_uint64()
        assert L.sigax_kmer_spectrum_workspace(n, C.byref(need)) == 0
        d_hist, d_stat, d_work = dbuf(8 * args.bins), dbuf(32), dbuf(need.value)
        out["k_spectrum"] = {}
        bins = {}
        for table in ("without_13mer_table", "with_13mer_table"):
            if table == "with_13mer_table":  # one correction call leaves it on the device
                seq = np.frombuffer(b"ACGTACGTTGCATGCAACGTACGTTGCATGCAACGT", dtype=np.uint8)
                o2 = np.array([0, len(seq)], dtype=np.uint64)
                cs, cv = np.zeros(len(seq), dtype=np.uint8), np.zeros(1, dtype=np.uint8)
                assert L.sigax_correct_batch(pair.handle, seq.tobytes(), None, o2.ctypes.data, 1, 31, 3, 10, 1, cs.ctypes.data, cv.ctypes.data) == 0
            for k in KS:
                t = timed(lambda: L.sigax_kmer_spectrum_device(pair.handle, d_seqs, d_offs, n, k, args.bins, d_hist, d_stat, d_work, need.value, stream))
                stat = [int(x) for x in down(d_stat, np.uint64, 4)]
                assert hip.hipMemset(d_hist, 0, 8 * args.bins) == 0
                assert L.sigax_kmer_spectrum_device(pair.handle, d_seqs, d_offs, n, k, args.bins, d_hist, d_stat, d_work, need.value, stream) == 0
                assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
                h = down(d_hist, np.uint64, args.bins)
                same = bins.setdefault(k, h) is h or bool(np.array_equal(bins[k], h))
                t.update({"strings": stat[0], "bases": stat[1], "windows": stat[2], "sectors": stat[3],
                          "windows_per_s": stat[2] / (t["ms_median"] * 1e-3), "sectors_per_window": stat[3] / max(stat[2], 1),
                          "bins_sum_is_windows": int(h.sum()) == stat[2], "bins_equal_across_tables": same,
                          "mode_count": int(np.argmax(h[1:]) + 1)})
                out["k_spectrum"]["k%d_%s" % (k, table)] = t
        wall = []
        for _ in range(args.wall_repeats + 1):
            t0 = time.perf_counter()
            pair.kmer_spectrum(31, args.bins, rows=rows)
            wall.append(time.perf_counter() - t0)
        out["rows_call_wall_s_k31"] = statistics.median(wall[1:])
    finally:
        for q in held:
            hip.hipFree(q)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    return out


def step_compose(args, prefix):
    from siga_amd import _lib
    L = _lib.lib()
    pair = open_forward(prefix)
    reads, _ = reads_of(args)
    m, k, K = min(args.compose_reads, args.reads), 31, args.length
    sub = np.ascontiguousarray(reads[:m])
    offs = np.arange(m + 1, dtype=np.uint64) * np.uint64(K)
    comp = np.zeros(256, dtype=np.uint8)
    comp[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
    a_s, b_s = [], []
    fused = composed = None
    try:
        for _ in range(args.wall_repeats + 1):  # the first of each is warm-up
            t0 = time.perf_counter()
            fused, _ = pair.kmer_spectrum(k, args.bins, seqs=(sub.reshape(-1), offs))
            a_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            win = np.lib.stride_tricks.sliding_window_view(sub, k, axis=1)[:, :K - k]  # j = k .. len - 1: not the last window
            fw = np.ascontiguousarray(win).reshape(-1, k)
            rc = np.ascontiguousarray(comp[fw][:, ::-1])
            c1, c2 = np.zeros(len(fw), dtype=np.uint64), np.zeros(len(fw), dtype=np.uint64)
            assert L.sigax_kmer_count_batch(pair.handle, C.c_char_p(fw.ctypes.data), k, len(fw), c1.ctypes.data) == 0
            assert L.sigax_kmer_count_batch(pair.handle, C.c_char_p(rc.ctypes.data), k, len(fw), c2.ctypes.data) == 0
            composed = np.bincount(np.minimum(c1 + c2, np.uint64(args.bins - 1)).astype(np.int64), minlength=args.bins).astype(np.uint64)
            b_s.append(time.perf_counter() - t0)
    finally:
        pair.close()
    a, b = statistics.median(a_s[1:]), statistics.median(b_s[1:])
    return {"reads": m, "k": k, "windows": int(m * (K - k)), "fused_spectrum_batch_wall_s": a, "kmer_count_composition_wall_s": b,
            "ratio_composition_over_fused": b / a, "bins_equal": bool(np.array_equal(fused, composed))}


def step_collect(args):
    doc = {"config": {"reads": args.reads, "read_length": args.length, "genome": args.genome, "seed": args.seed, "bins": args.bins,
                      "rows": "--all: 0 .. n_strings - 1"}}
    for name in ("index", "measure_two_step", "measure_one_step", "compose"):
        p = os.path.join(args.dir, name + ".json")
        doc[name] = json.load(open(p)) if os.path.exists(p) else None
    try:
        head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "status", "--porcelain", "--", "siga_amd", "include"], cwd=ROOT, capture_output=True, text=True).stdout.strip())
    except OSError:
        head, dirty = None, None
    rec = os.path.join(ROOT, "build", "build_record.json")
    doc["taken_at"] = {"commit": head, "sources_changed_since": dirty,
                       "sources_sha256": json.load(open(rec)).get("sources_sha256") if os.path.exists(rec) else None}
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=("index", "measure", "compose", "collect"))
    ap.add_argument("--dir", default=os.path.join(ROOT, "build", "spectrum_bench"))
    ap.add_argument("--form", default="two_step", choices=("two_step", "one_step"))
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bins", type=int, default=1025)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--wall-repeats", type=int, default=3)
    ap.add_argument("--compose-reads", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmer_spectrum.json"))
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    prefix = os.path.join(args.dir, "reads")
    if args.step == "collect":
        step_collect(args)
        return 0
    res = {"index": step_index, "measure": step_measure, "compose": step_compose}[args.step](args, prefix)
    name = "measure_" + args.form if args.step == "measure" else args.step
    with open(os.path.join(args.dir, name + ".json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
