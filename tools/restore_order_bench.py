#!/usr/bin/env python3
"""Measures sigax_edges_restore_order (csrc/sigax_order.hip) against what a caller could do before it existed, on the same
device and the same input: torch.sort(query, stable=True) followed by an index-select of the records.

Input: synthetic records generated on the device with the edge density the project has recorded -- configs[1]: 1 103 193
records over 1 M reads; configs[2]: about 22 M records over 20 M reads.  Run lengths are Poisson with that mean; the reads are
dealt to 8 shards by a random permutation and each shard holds its reads in the permutation's order: the worst case for the
move's locality.  Device time by HIP events on the current stream, warm, the two routes alternating, median of --steps
repetitions.  Both routes must give the same bytes.  One JSON document on stdout (and in --out).  Needs a GPU.

    python tools/restore_order_bench.py --out profiles/restore_order.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"configs1": (1000000, 1103193), "configs2": (20000000, 22000000)}
RANK_STEP_MS = 18.6  # one rank's step at configs[2], 2.5 M reads


def synthetic(torch, n_reads, n_edges, shards, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    cnt = torch.poisson(torch.full((n_reads,), n_edges / n_reads, device="cuda"), generator=g).to(torch.int64)
    perm = torch.randperm(n_reads, device="cuda", generator=g)  # shard s = perm[s * n / shards : (s + 1) * n / shards]
    query = torch.repeat_interleave(perm, cnt[perm])
    k = int(query.shape[0])
    at = torch.arange(k, device="cuda", dtype=torch.int64)
    recs = torch.stack([query, (at * 7 + 1) % n_reads, at % 101 + 45, at % 8], dim=1).to(torch.int32).contiguous()
    return recs, k, float(cnt.float().mean()), int(cnt.max())


def measure(torch, L, recs, n_reads, steps, warmup):
    k = int(recs.shape[0])
    need = C.c_uint64()
    assert L.sigax_edges_order_workspace(k, n_reads, C.byref(need)) == 0
    out = torch.empty_like(recs)
    work = torch.empty(int(need.value), dtype=torch.uint8, device="cuda")
    status = torch.empty(2, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ours():
        rc = L.sigax_edges_restore_order(0, recs.data_ptr(), k, n_reads, out.data_ptr(), None, work.data_ptr(), int(need.value),
                                         status.data_ptr(), st)
        assert rc == 0
        return out

    def torch_route():
        order = torch.sort(recs[:, 0].contiguous(), stable=True).indices
        return recs.index_select(0, order)

    ms = {"restore_order": [], "torch_sort_index_select": []}
    same = None
    for i in range(warmup + steps):
        for name, fn in (("restore_order", ours), ("torch_sort_index_select", torch_route)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            got = fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                ms[name].append(e0.elapsed_time(e1))
            if i == 0:
                same = bool(torch.equal(got, same)) if name == "torch_sort_index_select" else got.clone()
    return ms, same, status.tolist(), int(need.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="configs1,configs2")
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from siga_amd import _lib
    if not torch.cuda.is_available():
        sys.exit("restore_order_bench.py measures device time: it needs a GPU")
    L = _lib.lib()
    result = {"config": {"shards": args.shards, "steps": args.steps, "warmup": args.warmup, "seed": args.seed,
                         "timing": "HIP events on the current stream, routes alternating, median",
                         "bytes_moved": "32 bytes per record: each record read once and written once at its place"},
              "shapes": {}}
    ok = True
    for name in args.shapes.split(","):
        n_reads, n_edges = SHAPES[name]
        recs, k, mean, longest = synthetic(torch, n_reads, n_edges, args.shards, args.seed)
        ms, same, status, work_bytes = measure(torch, L, recs, n_reads, args.steps, args.warmup)
        a, b = statistics.median(ms["restore_order"]), statistics.median(ms["torch_sort_index_select"])
        row = {"reads": n_reads, "records": k, "mean_run": mean, "longest_run": longest, "workspace_bytes": work_bytes,
               "restore_order_ms_median": a, "restore_order_ms_min": min(ms["restore_order"]), "restore_order_ms_max": max(ms["restore_order"]),
               "torch_sort_index_select_ms_median": b, "torch_sort_index_select_ms_min": min(ms["torch_sort_index_select"]),
               "torch_sort_index_select_ms_max": max(ms["torch_sort_index_select"]),
               "ratio_torch_over_restore_order": b / a, "restore_order_GB_per_s": 32 * k / (a * 1e-3) / 1e9,
               "torch_route_GB_per_s": 32 * k / (b * 1e-3) / 1e9, "same_bytes": same, "status": status,
               "restore_order_not_slower": a <= b}
        if name == "configs2":
            row["share_of_one_rank_step"] = a / RANK_STEP_MS
            row["one_rank_step_ms"] = RANK_STEP_MS
        result["shapes"][name] = row
        ok = ok and same and status == [0, 0] and a <= b
        del recs
        torch.cuda.empty_cache()
    result["accepted"] = ok
    if not ok:
        result["verdict"] = "sigax_edges_restore_order is SLOWER than torch.sort + index_select at one shape at least, or the bytes differ: see the rows"
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
