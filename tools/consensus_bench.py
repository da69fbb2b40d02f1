#!/usr/bin/env python3
"""Measures `siga unitig -e` and its consensus pass at BASELINE configs[1] (1 M x 150 bp reads of a 5 Mb genome, seed 1) with the
1 % substitutions tools/mmoverlap_bench.py draws, the reads' places in the genome known.
  assembly    -e 40 --reduce -x 10 at the default seeds through the library's calls (the mismatch overlaps, the records that touch
              a contained read dropped, sigax_unitigs_reduce_host, the consensus pass): unitigs, contained reads, status8, and the
              wrong bases against the genome in the unitigs with copy bases and with consensus, by unitig length class.  A unitig
              is laid on the genome at its first read's place; one whose copy differs there in more than a tenth of its bases is
              counted as misplaced and left out of the sums.
  device      sigax_consensus_device by HIP events, median of --steps after --warmup with min and max, over the layout of that
              assembly, next to sigax_unitigs_device over the same records and that call's bases pass alone; the bytes the
              pass must move (placed read bases + twice the unitig bases + 16 per placement) over its time, against 8 TB/s
  error-free  (--clean) the same reads without substitutions at -e 0: `changed` must be 0 in every unitig
One JSON document on stdout (and in --out).  Needs a GPU; nothing but this repository.

    python tools/consensus_bench.py --clean --out profiles/consensus_configs1.json
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch  # before the library loads: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def _mmoverlap_bench():
    spec = importlib.util.spec_from_file_location("mmoverlap_bench", os.path.join(ROOT, "tools", "mmoverlap_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def assemble(pair, seqs, lengths, offs, P, M, rounds):
    """-> (kept records as EDGE_DTYPE, contained, mismatch status, the unitig call's dict, seconds of the two calls)"""
    import siga_amd
    from siga_amd import _lib
    t0 = time.time()
    e, contained, st = pair.overlap_mismatch(P, M)
    t1 = time.time()
    keep = (contained[e["query"]] == 0) & (contained[e["target"]] == 0)
    edges = np.zeros(int(keep.sum()), dtype=_lib.EDGE_DTYPE)
    for k in ("query", "target", "length", "af"):
        edges[k] = e[k][keep]
    t2 = time.time()
    res = siga_amd.unitigs_reduce(edges, lengths, seqs, offs, M, rounds, 150, reduce=True)
    t3 = time.time()
    return edges, contained, st, res, {"mismatch_overlaps_s": t1 - t0, "unitigs_reduce_host_s": t3 - t2}


def wrong_bases(res, cons, contained, pos, rev, genome_ascii, K):
    """wrong bases against the genome, copy and consensus, by unitig length class"""
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    so, lo, lay = res["seq_offs"].astype(np.int64), res["lay_offs"].astype(np.int64), res["layout"]
    copy = res["useqs"]
    classes = ((1, 150), (151, 1000), (1001, 10000), (10001, 1 << 62))
    out = [{"bases_from": a, "bases_to": b, "unitigs": 0, "bases": 0, "wrong_copy": 0, "wrong_consensus": 0, "misplaced": 0} for a, b in classes]
    hidden = 0
    for u in range(len(so) - 1):
        p0 = lo[u]
        r = int(lay["read"][p0])
        if lo[u + 1] - p0 == 1 and contained[r]:
            hidden += 1
            continue
        U = int(so[u + 1] - so[u])
        flip = bool(rev[r]) != bool(lay["flags"][p0] & 1)  # the unitig runs against the genome
        start = int(pos[r]) + K - U if flip else int(pos[r])
        row = next(c for c in out if c["bases_from"] <= U <= c["bases_to"])
        if start < 0 or start + U > len(genome_ascii):
            row["misplaced"] += 1
            continue
        g = genome_ascii[start:start + U]
        if flip:
            g = comp[g][::-1]
        w0 = int((copy[so[u]:so[u + 1]] != g).sum())
        if 10 * w0 > U:
            row["misplaced"] += 1
            continue
        row["unitigs"] += 1
        row["bases"] += U
        row["wrong_copy"] += w0
        row["wrong_consensus"] += int((cons[so[u]:so[u + 1]] != g).sum())
    return out, hidden


def device_times(res, edges, lengths, seqs, offs, M, steps, warmup):
    """HIP events on the null stream: the consensus call over res, sigax_unitigs_device over the records and its bases pass"""
    from siga_amd import _lib
    L = _lib.lib()
    L.sigax_unitigs_bases_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    n, nb, ne = len(lengths), len(seqs), len(edges)

    def up(a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return torch.from_numpy(a).to("cuda:0") if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda:0")

    def timed(fn, before=None):
        ms = []
        for i in range(warmup + steps):
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert fn() == 0, _lib.last_error()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        return spread(ms)

    d_len, d_seqs, d_offs = up(lengths), up(seqs), up(offs)
    nu = len(res["uflags"])
    so, lo = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    so[:nu + 1], lo[:nu + 1] = res["seq_offs"], res["lay_offs"]
    so[nu + 1:], lo[nu + 1:] = res["seq_offs"][-1], res["lay_offs"][-1]
    lay = np.zeros(n, dtype=_lib.PLACEMENT_DTYPE)
    lay[:len(res["layout"])] = res["layout"]
    d_nu, d_so, d_lo, d_lay, d_own = up(np.array([nu], dtype=np.uint64)), up(so), up(lo), up(lay), up(res["useqs"])
    d_us = torch.zeros(nb, dtype=torch.uint8, device="cuda:0")
    d_ch, d_sup, d_st = (torch.zeros(k, dtype=torch.uint8, device="cuda:0") for k in (4 * n, nb, 64))
    wb = C.c_uint64()
    assert L.sigax_consensus_workspace(n, n, C.byref(wb)) == 0
    d_work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")
    opts = _lib.ConsensusOpts(1, (0, 0, 0))

    def restore():
        d_us[:len(res["useqs"])] = d_own

    def consensus(sup):
        return L.sigax_consensus_device(0, d_nu.data_ptr(), n, d_so.data_ptr(), d_lo.data_ptr(), d_lay.data_ptr(), d_len.data_ptr(), d_seqs.data_ptr(),
                                        d_offs.data_ptr(), n, C.byref(opts), d_us.data_ptr(), d_ch.data_ptr(), d_sup.data_ptr() if sup else None,
                                        d_st.data_ptr(), d_work.data_ptr(), wb.value, None)

    out = {"consensus": timed(lambda: consensus(False), restore), "consensus_with_support": timed(lambda: consensus(True), restore)}
    status = d_st.cpu().numpy().view(np.uint64)
    placed = int(lengths[res["layout"]["read"]].astype(np.int64).sum())
    moved = placed + 2 * int(res["seq_offs"][-1]) + 16 * len(res["layout"])
    out["bytes_to_move"] = moved
    out["fraction_of_8TBps"] = moved / (out["consensus"]["median_ms"] * 1e-3) / PEAK
    out["status8_device"] = [int(x) for x in status]
    # the plain unitig call over the same records, and its bases pass
    d_edges = up(edges)
    ub = C.c_uint64()
    assert L.sigax_unitigs_workspace(n, ne, C.byref(ub)) == 0
    bufs = [torch.zeros(k, dtype=torch.uint8, device="cuda:0") for k in (8 * (n + 1), 8 * (n + 1), 4 * n, 16 * n, nb, 64, ub.value)]
    p = [b.data_ptr() for b in bufs]
    out["unitigs_device"] = timed(lambda: L.sigax_unitigs_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, M,
                                                                 p[0], p[1], p[2], p[3], p[4], p[5], p[6], ub.value, None))
    out["unitigs_bases_pass"] = timed(lambda: L.sigax_unitigs_bases_device(0, d_seqs.data_ptr(), d_offs.data_ptr(), n, ne, p[4], p[6], ub.value, None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--permille", type=int, default=40)
    ap.add_argument("--min-overlap", type=int, default=45)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clean", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import siga_amd
    from siga_amd import host
    from tests.golden.make_reads import fast_reads, rank_of_r_names
    mb = _mmoverlap_bench()
    N, K, M, P = args.reads, args.length, args.min_overlap, args.permille
    reads, genome = fast_reads(5 * N, K, N, args.seed)
    rng = np.random.default_rng(4)
    noisy = reads.copy()
    flips = rng.random(noisy.shape) < args.error
    noisy[flips] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(flips.sum()))]
    offs = np.arange(N + 1, dtype=np.uint64) * np.uint64(K)
    lengths, ranks = np.full(N, K, dtype=np.uint32), rank_of_r_names(N)
    pos, rev = mb.places(reads, genome, K)
    genome_ascii = np.frombuffer(b"ACGT", dtype=np.uint8)[genome]
    result = {"config": {"reads": N, "read_length": K, "genome": 5 * N, "seed": args.seed, "substitution_rate": args.error, "min_overlap": M,
                         "error_permille": P, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup},
              "exact_path_unitigs_after_10_rounds": 198657}

    def run(name, data, permille, device):
        with tempfile.TemporaryDirectory() as d:
            prefix = os.path.join(d, name)
            t0 = time.time()
            host.index_build_gpu(data.reshape(-1), offs, prefix)
            pair = siga_amd.FMIndexPair.load_forward(prefix, device=0)
            pair.set_reads(lengths, ranks)
            t1 = time.time()
            flat = data.reshape(-1)
            edges, contained, st, res, secs = assemble(pair, flat, lengths, offs, permille, M, args.rounds)
            pair.close()
        t2 = time.time()
        cons = siga_amd.unitigs_consensus(res, lengths, flat, offs)
        secs.update(index_build_and_load_s=t1 - t0, consensus_host_s=time.time() - t2)
        by_class, hidden = wrong_bases(res, cons["useqs"], contained, pos, rev, genome_ascii, K)
        nu = len(res["uflags"])
        doc = {"records_kept": int(len(edges)), "contained_reads": int(np.count_nonzero(contained)), "mismatch_status8": [int(v) for v in st],
               "unitigs_of_the_call": nu, "unitigs_shown": nu - hidden, "unitig_bases": int(res["seq_offs"][-1]),
               "placements": int(len(res["layout"])), "reduce_status40": [int(v) for v in res["status"]],
               "consensus_status8": [int(v) for v in cons["status"]], "unitigs_with_a_change": int(np.count_nonzero(cons["changed"])),
               "wrong_bases_by_unitig_length": by_class, "seconds": secs}
        if device:
            doc["device"] = device_times(res, edges, lengths, flat, offs, M, args.steps, args.warmup)
        return doc

    result["noisy_e40_reduce_x%d" % args.rounds] = run("noisy", noisy, P, True)
    if args.clean:
        clean = run("clean", reads, 0, False)
        assert clean["consensus_status8"][2] == 0 and clean["unitigs_with_a_change"] == 0, "the vote changed error-free bases"
        result["error_free_e0_reduce_x%d" % args.rounds] = clean
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
