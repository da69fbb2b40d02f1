#!/usr/bin/env python3
"""Measures `siga correct -a overlap` at BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1) with 1 % substitutions,
the set tools/e2e_aux.py draws; the index is built from the noisy reads, and the error-free reads are the truth.
  device      by HIP events, median of --steps after --warmup, with their spread: the reference-text build
              (sigax_reference_text_device), one whole round (sigax_pileup_device) and the pile-up kernel alone over the hits
              that round left (sigax_pileup_pile_device); seeds + locate = round - pile-up.  The pile-up kernel's bytes are
              counted from what it reads and writes -- 16 per hit, the candidates' text (at most a read's length each), three
              offsets a candidate, the read in and out -- and set against the HBM peak
  accuracy    through the command line: reads written and wrong bases before and after for `-a kmer`, `-a overlap`, and `-a kmer`
              followed by `-a overlap` over the reads the k-mer path dropped; reads over --max-candidates and seeds over
              --max-seed-hits at the defaults
One JSON document on stdout (and in --out).  Needs a GPU; nothing but this repository.  --device-only ends after the device
section (for A/B runs of two builds of the library, SIGAX_LIB selecting one).

    python tools/pileup_bench.py --out profiles/pileup_configs1.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12  # bytes/s, the MI355X data sheet


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    return hip


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "stdev_ms": statistics.pstdev(ms)}


def device_times(hip, L, handle, flat, offs, params, steps, warmup):
    from siga_amd import _lib
    n, nb = len(offs) - 1, int(offs[-1])
    held = []

    def dbuf(nbytes, src=None):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(nbytes, 16)) == 0
        held.append(q)
        if src is not None:
            assert hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        return q

    def get(q, dtype, count):
        out = np.zeros(count, dtype=dtype)
        assert hip.hipMemcpy(out.ctypes.data, q, out.nbytes, 2) == 0
        return out

    stream = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    ev = [C.c_void_p() for _ in range(3)]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def elapsed(a, b):
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), a, b) == 0
        return float(t.value)

    try:
        tb, wb = C.c_uint64(), C.c_uint64()
        assert L.sigax_reference_text_workspace(handle, C.byref(tb), C.byref(wb)) == 0, _lib.last_error()
        d_text, d_toffs, d_tstat, d_twork = dbuf(tb.value), dbuf(8 * (n + 1)), dbuf(32), dbuf(wb.value)
        ref_ms = []
        for i in range(warmup + steps):
            assert hip.hipEventRecord(ev[0], stream) == 0
            assert L.sigax_reference_text_device(handle, d_text, tb.value, d_toffs, d_tstat, d_twork, wb.value, stream) == 0, _lib.last_error()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            if i >= warmup:
                ref_ms.append(elapsed(ev[0], ev[1]))
        tstat = get(d_tstat, np.uint64, 4)

        d_seqs, d_offs = dbuf(flat.nbytes + 16, flat), dbuf(offs.nbytes, offs)
        d_out, d_valid, d_changed, d_stat = dbuf(flat.nbytes + 16), dbuf(n), dbuf(n), dbuf(64)
        args = lambda d_work, wbytes, cap: (handle, d_seqs, d_offs, n, nb, C.byref(params), d_text, d_toffs, d_out, d_valid, d_changed,  # noqa: E731
                                             d_stat, d_work, wbytes, cap, stream)
        assert L.sigax_pileup_workspace(n, nb, C.byref(params), 0, C.byref(wb)) == 0, _lib.last_error()
        d_work = dbuf(wb.value)
        assert L.sigax_pileup_device(*args(d_work, wb.value, 0)) == 0, _lib.last_error()  # nothing walked: the hits the seeds list
        assert hip.hipStreamSynchronize(stream) == 0
        need = int(get(d_stat, np.uint64, 8)[0])
        hip.hipFree(held.pop())
        assert L.sigax_pileup_workspace(n, nb, C.byref(params), need, C.byref(wb)) == 0, _lib.last_error()
        d_work = dbuf(wb.value)
        round_ms, pile_ms = [], []
        for i in range(warmup + steps):
            assert hip.hipEventRecord(ev[0], stream) == 0
            assert L.sigax_pileup_device(*args(d_work, wb.value, need)) == 0, _lib.last_error()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert L.sigax_pileup_pile_device(*args(d_work, wb.value, need)) == 0, _lib.last_error()
            assert hip.hipEventRecord(ev[2], stream) == 0
            assert hip.hipEventSynchronize(ev[2]) == 0
            if i >= warmup:
                round_ms.append(elapsed(ev[0], ev[1]))
                pile_ms.append(elapsed(ev[1], ev[2]))
        stat = get(d_stat, np.uint64, 8)
        valid = get(d_valid, np.uint8, n)
    finally:
        for q in held:
            hip.hipFree(q)
        L.sigax_stream_destroy(0, stream)
    longest = int((offs[1:] - offs[:-1]).max())
    pile_bytes = 16 * need + int(stat[5]) * (longest + 24) + 2 * nb + 2 * n
    p = statistics.median(pile_ms)
    return {"reads": n, "bases": nb, "reference_text": dict(spread(ref_ms), status4=[int(v) for v in tstat]),
            "round": spread(round_ms), "pileup_kernel": spread(pile_ms),
            "seeds_and_locate": spread([a - b for a, b in zip(round_ms, pile_ms)]),
            "workspace_bytes": int(wb.value), "status8": [int(v) for v in stat], "reads_valid": int(np.count_nonzero(valid == 1)),
            "pileup_bytes_counted": pile_bytes, "pileup_bytes_per_s": pile_bytes / (p * 1e-3),
            "pileup_fraction_of_hbm_peak": pile_bytes / (p * 1e-3) / HBM_PEAK,
            "reads_per_s_round": n / (statistics.median(round_ms) * 1e-3)}


def fasta(path, reads, ids):
    with open(path, "wb") as f:
        f.write(b"".join(b">r%d\n%s\n" % (i, bytes(reads[i])) for i in ids))


def parse(path, length):
    """-> (ids, [n, length] uint8) of a FASTA the CLI wrote from reads named r<i>"""
    lines = open(path, "rb").read().split(b"\n")
    names, seqs = lines[0:-1:2], lines[1::2]
    ids = np.array([int(nm.split()[0][2:]) for nm in names], dtype=np.int64)
    if len(ids) == 0:
        return ids, np.zeros((0, length), dtype=np.uint8)
    return ids, np.frombuffer(b"".join(seqs[:len(ids)]), dtype=np.uint8).reshape(-1, length)


def emit(result, out):
    text = json.dumps(result, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()

    import siga_amd
    from siga_amd import _lib, host
    from tests.golden.make_reads import fast_reads
    hip, L = hip_runtime(), _lib.lib()
    N, K = args.reads, args.length
    reads, _ = fast_reads(5 * N, K, N, args.seed)
    rng = np.random.default_rng(4)
    noisy = reads.copy()
    flips = rng.random(noisy.shape) < args.error
    noisy[flips] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(flips.sum()))]
    offs = np.arange(N + 1, dtype=np.uint64) * np.uint64(K)
    params = _lib.PileParams(max_read_len=K)
    result = {"config": {"reads": N, "read_length": K, "genome": 5 * N, "seed": args.seed, "substitution_rate": args.error,
                         "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                         "params": {n: int(getattr(params, n)) for n, _ in params._fields_}},
              "wrong_bases_in": int((noisy != reads).sum())}

    def run(cli_args, cwd):
        t0 = time.time()
        r = subprocess.run([host.CLI_PATH, "correct"] + cli_args, cwd=cwd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return time.time() - t0, r.stderr.strip().splitlines()[-1:] if r.stderr.strip() else []

    def score(path, name, seconds, note):
        ids, fixed = parse(path, K)
        return {"name": name, "seconds_end_to_end": seconds, "reads_written": int(len(ids)),
                "wrong_bases_before_over_written": int((noisy[ids] != reads[ids]).sum()),
                "wrong_bases_after_over_written": int((fixed != reads[ids]).sum()), "cli": note}, ids

    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "noisy")
        fasta(prefix + ".fa", noisy, range(N))
        host.index_build_gpu(noisy.reshape(-1), offs, prefix)
        pair = siga_amd.FMIndexPair.load_forward(prefix, device=0)
        result["device"] = device_times(hip, L, pair.handle, noisy.reshape(-1), offs, params, args.steps, args.warmup)
        pair.close()
        if args.device_only:
            return emit(result, args.out)
        t, note = run(["-a", "kmer", "-k", "31", "-p", prefix, "-o", "kmer.fa", "noisy.fa"], d)
        kmer, kept = score(os.path.join(d, "kmer.fa"), "kmer", t, note)
        t, note = run(["-a", "overlap", "-i", str(args.rounds), "-p", prefix, "-o", "overlap.fa", "noisy.fa"], d)
        over, _ = score(os.path.join(d, "overlap.fa"), "overlap", t, note)
        dropped = np.setdiff1d(np.arange(N), kept)
        fasta(os.path.join(d, "dropped.fa"), noisy, dropped)
        t, note = run(["-a", "overlap", "-i", str(args.rounds), "-p", prefix, "-o", "rescued.fa", "dropped.fa"], d)
        resc, _ = score(os.path.join(d, "rescued.fa"), "overlap over the reads kmer dropped", t, note)
        both = {"name": "kmer, then overlap over the reads it dropped", "reads_written": kmer["reads_written"] + resc["reads_written"],
                "wrong_bases_before_over_written": kmer["wrong_bases_before_over_written"] + resc["wrong_bases_before_over_written"],
                "wrong_bases_after_over_written": kmer["wrong_bases_after_over_written"] + resc["wrong_bases_after_over_written"]}
        result["accuracy"] = [kmer, over, resc, both]
        result["kmer_dropped"] = int(len(dropped))
    st = result["device"]["status8"]
    result["caps_at_defaults"] = {"reads_over_max_candidates": st[2], "seeds_located": st[3], "seeds_over_max_seed_hits": st[4]}
    return emit(result, args.out)


if __name__ == "__main__":
    sys.exit(main())
