#!/usr/bin/env python3
"""Measures the placement of contained reads (`siga unitig -e --place-contained`, sigax_contained_place_*) at BASELINE configs[1]
(1 M x 150 bp reads of a 5 Mb genome, seed 1) with the 1 % substitutions tools/mmoverlap_bench.py draws, on that set and on the same
reads cut to 100 .. 150 bases at their 3' end, the reads' places in the genome known.
  counts      contained reads, reads per placement class, the longest chain, the containment records
  wrong bases against the genome per unitig length band (those of tools/consensus_bench.py): copy bases, the vote over the call's
              own layout, the vote over the layout with the contained reads placed
  pairs       reads 2k and 2k + 1 taken as mates: pairs with a contained mate (no pair today), and those of them whose contained
              mates are all placed (pairs again); counted on the host from contained[] and place_class[], no pairs call is run
  device      sigax_contained_place_device by HIP events, median of --steps after --warmup with min and max, next to
              sigax_unitigs_device over the same records and sigax_consensus_device over the placed layout
  --ab LIB    the mismatch overlap call with flags = 0 in this build and in the build LIB (the parent's sigax_mmoverlap sources),
              the two alternating in child processes, --ab-rounds medians each; the verify kernel with flags = 1 beside it
One JSON document on stdout (and in --out).  Needs a GPU; nothing but this repository.

    python tools/contained_bench.py --out profiles/contained_configs1.json
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch  # before the library loads: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BANDS = ((1, 150), (151, 1000), (1001, 10000), (10001, 1 << 62))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_sets(N, K, seed, error):
    """-> {name: (flat bases, lengths, offs, pos, rev)}, genome as ASCII, name ranks"""
    from tests.golden.make_reads import fast_reads, rank_of_r_names
    reads, genome = fast_reads(5 * N, K, N, seed)
    rng = np.random.default_rng(4)
    noisy = reads.copy()
    flips = rng.random(noisy.shape) < error
    noisy[flips] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(flips.sum()))]
    pos, rev = _tool("mmoverlap_bench").places(reads, genome, K)
    pos, rev = np.asarray(pos, dtype=np.int64), np.asarray(rev, dtype=bool)
    full = np.full(N, K, dtype=np.uint32)
    sets = {"equal_150": (noisy.reshape(-1), full, np.arange(N + 1, dtype=np.uint64) * np.uint64(K), pos, rev)}
    cut = np.random.default_rng(5).integers(100, K + 1, size=N).astype(np.uint32)
    keep = np.arange(K)[None, :] < cut[:, None]
    offs = np.zeros(N + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(cut, dtype=np.uint64)
    # a read on the reverse strand loses the genome's columns at its low end
    sets["cut_100_150"] = (noisy[keep], cut, offs, np.where(rev, pos + K - cut.astype(np.int64), pos), rev)
    return sets, np.frombuffer(b"ACGT", dtype=np.uint8)[genome], rank_of_r_names(N)


def wrong_bases(res, lengths, contained, pos, rev, genome_ascii, variants):
    """per band: unitigs, bases, and the wrong bases of every variant (name -> unitig bases); a unitig is laid on the genome at
    its first read's place, and one whose copy differs there in more than a tenth of its bases is counted as misplaced"""
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    so, lo, lay = res["seq_offs"].astype(np.int64), res["lay_offs"].astype(np.int64), res["layout"]
    out = [dict({"bases_from": a, "bases_to": b, "unitigs": 0, "bases": 0, "misplaced": 0}, **{"wrong_" + k: 0 for k in variants}) for a, b in BANDS]
    for u in range(len(so) - 1):
        p0 = lo[u]
        r = int(lay["read"][p0])
        if lo[u + 1] - p0 == 1 and contained[r]:
            continue
        U = int(so[u + 1] - so[u])
        flip = bool(rev[r]) != bool(lay["flags"][p0] & 1)
        start = int(pos[r]) + int(lengths[r]) - U if flip else int(pos[r])
        row = next(c for c in out if c["bases_from"] <= U <= c["bases_to"])
        if start < 0 or start + U > len(genome_ascii):
            row["misplaced"] += 1
            continue
        g = genome_ascii[start:start + U]
        if flip:
            g = comp[g][::-1]
        if 10 * int((variants["copy"][so[u]:so[u + 1]] != g).sum()) > U:
            row["misplaced"] += 1
            continue
        row["unitigs"] += 1
        row["bases"] += U
        for k, bases in variants.items():
            row["wrong_" + k] += int((bases[so[u]:so[u + 1]] != g).sum())
    return out


def place_device_time(res, lengths, contained, conts, steps, warmup):
    from siga_amd import _lib
    L = _lib.lib()
    n, nu = len(lengths), len(res["uflags"])

    def up(a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return torch.from_numpy(a).to("cuda:0") if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda:0")

    so, lo = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    so[:nu + 1], lo[:nu + 1] = res["seq_offs"], res["lay_offs"]
    so[nu + 1:], lo[nu + 1:] = res["seq_offs"][-1], res["lay_offs"][-1]
    lay = np.full(16 * n, 0xFF, dtype=np.uint8).view(_lib.PLACEMENT_DTYPE)
    lay[:len(res["layout"])] = res["layout"]
    d_nu, d_so, d_lo, d_lay = up(np.array([nu], dtype=np.uint64)), up(so), up(lo), up(lay)
    d_len, d_cont, d_recs = up(lengths), up(contained), up(conts)
    wb = C.c_uint64()
    assert L.sigax_contained_place_workspace(n, n, len(conts), C.byref(wb)) == 0, _lib.last_error()
    d_lo2, d_lay2, d_cls, d_st, d_work = (torch.zeros(k, dtype=torch.uint8, device="cuda:0") for k in (8 * (n + 1), 16 * n, n, 64, wb.value))
    opts = _lib.ContainedOpts()
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = L.sigax_contained_place_device(0, d_nu.data_ptr(), n, d_so.data_ptr(), d_lo.data_ptr(), d_lay.data_ptr(), d_len.data_ptr(), n,
                                            d_cont.data_ptr(), d_recs.data_ptr(), len(conts), C.byref(opts), d_lo2.data_ptr(), d_lay2.data_ptr(),
                                            d_cls.data_ptr(), d_st.data_ptr(), d_work.data_ptr(), wb.value, None)
        assert rc == 0, _lib.last_error()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    out = _tool("consensus_bench").spread(ms)
    out["workspace_bytes"] = int(wb.value)
    out["status8_device"] = [int(x) for x in d_st.cpu().numpy().view(np.uint64)]
    return out


def run_set(name, data, ranks, genome_ascii, args):
    import siga_amd
    from siga_amd import _lib, host
    flat, lengths, offs, pos, rev = data
    M, P = args.min_overlap, args.permille
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, name)
        host.index_build_gpu(flat, offs, prefix)
        pair = siga_amd.FMIndexPair.load_forward(prefix, device=0)
        pair.set_reads(lengths, ranks)
        t0 = time.time()
        e, contained, st, conts = pair.overlap_mismatch(P, M, containments=True)
        secs = {"mismatch_overlaps_with_containments_s": time.time() - t0}
        pair.close()
    keep = (contained[e["query"]] == 0) & (contained[e["target"]] == 0)
    edges = np.zeros(int(keep.sum()), dtype=_lib.EDGE_DTYPE)
    for k in ("query", "target", "length", "af"):
        edges[k] = e[k][keep]
    res = siga_amd.unitigs_reduce(edges, lengths, flat, offs, M, args.rounds, 150, reduce=True)
    t0 = time.time()
    placed = siga_amd.unitigs_place_contained(res, lengths, contained, conts)
    secs["place_host_s"] = time.time() - t0
    cons_old = siga_amd.unitigs_consensus(res, lengths, flat, offs)
    cons_new = siga_amd.unitigs_consensus(placed, lengths, flat, offs)
    cls = placed["place_class"]
    n = len(lengths)
    c0, c1 = contained[0:n - 1:2] != 0, contained[1:n:2] != 0
    ok0, ok1 = ~c0 | (cls[0:n - 1:2] == 1), ~c1 | (cls[1:n:2] == 1)
    doc = {"reads": n, "bases": int(offs[-1]), "records_kept": int(len(edges)), "containment_records": int(len(conts)),
           "mismatch_status8": [int(v) for v in st], "contained_reads": int(np.count_nonzero(contained)),
           "reads_by_class": {k: int((cls == i).sum()) for i, k in enumerate(_lib.CP_CLASSES)},
           "place_status8": dict(zip(_lib.CONTAINED_STATUS, (int(v) for v in placed["place_status"]))),
           "unitigs_of_the_call": len(res["uflags"]), "placements_before": int(len(res["layout"])), "placements_after": int(len(placed["layout"])),
           "consensus_status8_before": [int(v) for v in cons_old["status"]], "consensus_status8_after": [int(v) for v in cons_new["status"]],
           "wrong_bases_by_unitig_length": wrong_bases(res, lengths, contained, pos, rev, genome_ascii,
                                                       {"copy": res["useqs"], "consensus": cons_old["useqs"], "consensus_placed": cons_new["useqs"]}),
           "pairs_of_neighbouring_ids": {"pairs": n // 2, "with_a_contained_mate": int((c0 | c1).sum()),
                                         "regained": int(((c0 | c1) & ok0 & ok1).sum()), "still_lost": int(((c0 | c1) & ~(ok0 & ok1)).sum())},
           "seconds": secs}
    cb = _tool("consensus_bench")
    dev = cb.device_times(placed, edges, lengths, flat, offs, M, args.steps, args.warmup)
    doc["device"] = {"place": place_device_time(res, lengths, contained, conts, args.steps, args.warmup),
                     "consensus_over_the_placed_layout": dev["consensus"], "unitigs_device": dev["unitigs_device"]}
    return doc


def ab_child(args):
    """one build (SIGAX_LIB), one measurement of the mismatch overlap call on the equal-length set -> JSON on stdout"""
    import siga_amd
    from siga_amd import _lib, host
    mb = _tool("mmoverlap_bench")
    sets, _, ranks = make_sets(args.reads, args.length, args.seed, args.error)
    flat, lengths, offs, _, _ = sets["equal_150"]
    prefix = args.ab_child
    if not os.path.exists(prefix + ".sai"):
        host.index_build_gpu(flat, offs, prefix)
    pair = siga_amd.FMIndexPair.load_forward(prefix, device=0)
    pair.set_reads(lengths, ranks)
    params = _lib.MmoParams(args.permille, min_overlap=args.min_overlap, max_read_len=args.length, flags=args.ab_flags)
    dev = mb.device_times(mb.hip_runtime(), _lib.lib(), pair, len(lengths), int(offs[-1]), params, args.steps, args.warmup)[0]
    pair.close()
    print("AB " + json.dumps({k: dev[k]["median_ms"] for k in ("seeds_and_locate", "k_mmo", "commit", "whole_call", "finish")} |
                             {"records_raw": dev["records_raw"]}))
    return 0


def ab(args):
    runs = {"parent": [], "new": [], "new_flags1": []}
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "ab")
        order = [("parent", args.ab, 0), ("new", None, 0)] * args.ab_rounds + [("new_flags1", None, 1)] * 2
        for name, libpath, flags in order:
            env = dict(os.environ)
            if libpath:
                env["SIGAX_LIB"] = os.path.abspath(libpath)
            cmd = [sys.executable, os.path.abspath(__file__), "--ab-child", prefix, "--ab-flags", str(flags), "--reads", str(args.reads), "--steps",
                   str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:  # a fault or an abort: nothing more is started on the GPU
                raise SystemExit("%s run ended with %d: %s" % (name, r.returncode, r.stderr[-2000:]))
            runs[name].append(json.loads(next(l for l in r.stdout.split("\n") if l.startswith("AB "))[3:]))
            print(name, runs[name][-1], file=sys.stderr, flush=True)
    doc = {"what": "sigax_mmoverlap_device on the equal-length set, median ms of %d steps after %d per run; the runs alternate" % (args.steps, args.warmup),
           "runs": runs}
    for key in ("whole_call", "k_mmo", "commit", "finish"):
        a, b = [r[key] for r in runs["parent"]], [r[key] for r in runs["new"]]
        doc[key] = {"parent_min": min(a), "parent_max": max(a), "new_min": min(b), "new_max": max(b), "ranges_overlap": min(a) <= max(b) and min(b) <= max(a)}
    return doc


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
    ap.add_argument("--sets", default="equal_150,cut_100_150")
    ap.add_argument("--ab", default=None, help="a libsigax.so built with the parent's sigax_mmoverlap sources")
    ap.add_argument("--ab-rounds", type=int, default=5)
    ap.add_argument("--ab-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--ab-flags", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.ab_child:
        return ab_child(args)
    result = {"config": {"reads": args.reads, "read_length": args.length, "genome": 5 * args.reads, "seed": args.seed, "substitution_rate": args.error,
                         "min_overlap": args.min_overlap, "error_permille": args.permille, "rounds": args.rounds, "steps": args.steps,
                         "warmup": args.warmup}}
    if args.sets:
        sets, genome_ascii, ranks = make_sets(args.reads, args.length, args.seed, args.error)
        for name in args.sets.split(","):
            result[name] = run_set(name, sets[name], ranks, genome_ascii, args)
            print(name, "done", file=sys.stderr, flush=True)
    if args.ab:
        result["mmoverlap_flags0_ab"] = ab(args)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
