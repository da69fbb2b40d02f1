#!/usr/bin/env python3
"""Measures `siga unitig --scaffold --gapfill --join-overlaps` (sigax_join_device) next to the scaffold and gapfill calls it
follows, on the paired read sets of tools/pairs_bench.py (BASELINE configs[1] shape: 1 M x 150 bp reads of a 5 Mb genome, seed 1,
m = 45, drawn in pairs at a fixed insert; error-free, and with the bench's 1 % substitutions).  Per read set two GPU steps, each a
child process under a `timeout` of its own; a step is not started when the one before it failed:
  index     the reads' FM-index files, built on the GPU
  measure   one overlap run in one device batch, its records left on the device; sigax_unitigs_device, sigax_unitigs_pairs_device,
            sigax_scaffold_device, sigax_gapfill_device and sigax_join_device over them in one process; then by HIP events on the
            caller's stream, median of --steps calls after --warmup: the scaffold, the gapfill and the join call at their
            defaults, each with a bases buffer of exactly its size.  From the join call's status and records: gaps by class, how
            many of the gaps the gapfill call left open are now joined (by the gapfill call's class), the N left, candidate
            overlaps tested and junction windows looked up.  Every joined junction is then looked up in the simulated genome:
            the k bases on either side of it must occur there on one strand or the other.  With --mismatches N > 0 then
            sigax_join_approx_device over the same tables (--permille M), timed likewise next to the exact call: gaps by class,
            approximate joins, their columns taken from the left and from the right neighbour, and every approximately joined
            junction -- its whole overlap and the k bases on either side -- looked up in the genome.  The ends of the gaps that
            stay NONE are then compared on the host, without the half rule: per gap the overlap length in lo .. hi whose two
            copies differ in the smallest share of their bases, so that the profile says what keeps those ends apart.
One JSON document on stdout (and in --out).  Needs a GPU; nothing but this repository.

    python tools/join_bench.py --out profiles/join_configs1.json
    python tools/join_bench.py --mismatches 2 --out profiles/join_approx_configs1.json
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

from tools.gapfill_bench import genome_of  # noqa: E402
from tools.pairs_bench import STATUS6, reads_of, step_index  # noqa: E402


def nearest_overlaps(seqs, sco, scl, lay, so, recs, sel, lo, max_overlap):
    """for the gaps sel (numbered in placement order, as the records are): the v in lo .. min(max_overlap, |L| - 1, |R| - 1) whose
    two copies differ in the smallest share of their bases (all of them ACGT) -> a summary over those gaps"""
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGT")] = True
    buf = np.frombuffer(seqs, dtype=np.uint8)
    rows, g = [], 0
    for s in range(len(scl) - 1):
        for p in range(int(scl[s]), int(scl[s + 1]) - 1):
            if sel[g]:
                ends = []
                for q in (p, p + 1):
                    u = int(lay[q]["read"])
                    at = int(sco[s]) + int(lay[q]["offset"])
                    ends.append(buf[at:at + int(so[u + 1] - so[u])])
                L, R = ends
                hi = min(max_overlap, len(L) - 1, len(R) - 1)
                best = None
                for v in range(lo, hi + 1):
                    a, b = L[len(L) - v:], R[:v]
                    if not (ok[a].all() and ok[b].all()):
                        continue
                    d = int((a != b).sum())
                    if best is None or d * best[0] < best[1] * v:
                        best = (v, d)
                rows.append((len(L), len(R), hi) + (best or (0, -1)))
            g += 1
    assert g == len(recs)
    near = [r for r in rows if r[4] >= 0 and 20 * r[4] <= r[3]]  # at most 5 % of the bases differ
    return {"gaps": len(rows), "with_an_overlap_within_50_permille": len(near),
            "of_them_beyond_half_of_the_shorter_unitig": sum(1 for r in near if r[3] > min(r[0], r[1]) // 2),
            "their_differing_bases": {str(d): sum(1 for r in near if r[4] == d) for d in sorted(set(r[4] for r in near))},
            "their_overlap_lengths": {"min": min((r[3] for r in near), default=0), "max": max((r[3] for r in near), default=0)},
            "unitig_bases_at_those_gaps": {"min": min((min(r[0], r[1]) for r in rows), default=0), "max": max((max(r[0], r[1]) for r in rows), default=0)},
            "smallest_share_elsewhere_permille": sorted(1000 * r[4] // r[3] for r in rows if r[4] >= 0 and 20 * r[4] > r[3])[:5]}


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
        wu, wq, ws, wg, wj = (C.c_uint64() for _ in range(5))
        assert L.sigax_unitigs_workspace(n, ne, C.byref(wu)) == 0 and L.sigax_unitigs_pairs_workspace(0, n, C.byref(wq)) == 0
        assert L.sigax_scaffold_workspace(n, n // 2, C.byref(ws)) == 0 and L.sigax_gapfill_workspace(n, args.walk_bases, C.byref(wg)) == 0
        assert L.sigax_join_workspace(n, C.byref(wj)) == 0
        d_len, d_seqs, d_offs, d_mate = dbuf(lengths.nbytes, lengths), dbuf(nb, flat), dbuf(offs.nbytes, offs), dbuf(mate.nbytes, mate)
        d_so, d_lo, d_uf, d_lay, d_us = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(nb)
        d_stat, d_work = dbuf(96), dbuf(wu.value)
        bins = args.bins
        d_hist, d_links, d_st24, d_pwork = dbuf(8 * bins), dbuf(24 * (n // 2)), dbuf(192), dbuf(wq.value)
        d_sco, d_scl, d_scf, d_slay, d_st16, d_swork = dbuf(8 * (n + 1)), dbuf(8 * (n + 1)), dbuf(4 * n), dbuf(16 * n), dbuf(128), dbuf(ws.value)
        d_gco, d_glay, d_gaps, d_gst, d_gwork = dbuf(8 * (n + 1)), dbuf(16 * n), dbuf(32 * n), dbuf(192), dbuf(wg.value)
        d_jco, d_jlay, d_joins, d_jst, d_jwork = dbuf(8 * (n + 1)), dbuf(16 * n), dbuf(32 * n), dbuf(128), dbuf(wj.value)
        popts = _lib.PairsOpts(0, bins, 0, 0, args.max_span)
        sopts = _lib.ScaffoldOpts(_lib.SIGAX_SCAFFOLD_INSERT_FROM_STATUS, args.min_pairs, args.link_ratio, args.min_unitig_bases, 0, 1, args.max_gap)
        gopts = _lib.GapfillOpts(0, args.gap_kmer, args.gap_min_count, args.gap_slack, args.gap_max_fill, 0)
        jopts = _lib.JoinOpts(0, args.join_min_overlap, args.join_max_overlap, args.join_slack, args.join_kmer, args.join_min_count, 0)
        out = {"config": {"reads": n, "read_length": args.length, "genome": args.genome, "seed": args.seed, "min_overlap": args.min_overlap,
                          "error_rate": args.error_rate, "insert": args.insert, "min_pairs": args.min_pairs, "link_ratio": args.link_ratio,
                          "min_unitig_bases": args.min_unitig_bases, "min_gap": 1, "max_gap": args.max_gap,
                          "gapfill": {"k": args.gap_kmer, "min_count": args.gap_min_count, "slack": args.gap_slack, "max_fill": args.gap_max_fill,
                                      "walk_bases": args.walk_bases},
                          "join": {"min_overlap": args.join_min_overlap, "max_overlap": args.join_max_overlap, "slack": args.join_slack,
                                   "k": args.join_kmer, "min_count": args.join_min_count},
                          "steps": args.steps, "warmup": args.warmup},
               "edges": ne, "workspace_bytes": {"scaffold": int(ws.value), "gapfill": int(wg.value), "join": int(wj.value)}, "calls": []}
        d_status_nl = C.c_void_p(d_st24.value + 22 * 8)

        def scaffold_call(d_out, cap):
            return L.sigax_scaffold_device(0, d_stat, n, d_so, d_uf, d_us, nb, d_links, d_status_nl, n // 2, d_st24, C.byref(sopts), d_sco, d_scl, d_scf,
                                           d_slay, d_out, cap, d_st16, d_swork, ws.value, stream)

        def gapfill_call(d_out, cap):
            return L.sigax_gapfill_device(pair.handle, d_stat, n, d_so, d_us, nb, d_st16, d_scl, d_slay, C.byref(gopts), d_gco, d_glay, d_out, cap, d_gaps,
                                          d_gst, d_gwork, wg.value, args.walk_bases, stream)

        def fetch(ptr, k, dtype=np.uint64):
            s = np.zeros(k, dtype=dtype)
            assert hip.hipMemcpy(s.ctypes.data, ptr, s.nbytes, 2) == 0
            return s

        assert L.sigax_unitigs_device(0, d_edges, ne, d_len, d_seqs, d_offs, n, args.min_overlap, d_so, d_lo, d_uf, d_lay, d_us, d_stat, d_work, wu.value,
                                      stream) == 0, _lib.last_error()
        assert L.sigax_unitigs_pairs_device(0, d_mate, d_len, n, d_stat, d_so, d_lo, d_uf, d_lay, C.byref(popts), d_hist, d_links, d_st24, d_pwork,
                                            wq.value, stream) == 0, _lib.last_error()
        assert scaffold_call(None, 0) == 0, _lib.last_error()
        assert hip.hipStreamSynchronize(stream) == 0
        ustat = dict(zip(STATUS6, [int(x) for x in fetch(d_stat, 6)]))
        total = int(fetch(d_st16, 16)[1])
        d_out = dbuf(total)
        t = timed(lambda: scaffold_call(d_out, total))
        sstat = dict(zip(_lib.SCAFFOLD_STATUS, [int(x) for x in fetch(d_st16, 16)]))
        t.update({"call": "scaffold_device", "status": sstat, "unitigs": ustat})
        out["calls"].append(t)
        scaffold_ms = t["median_ms"]
        assert gapfill_call(None, 0) == 0, _lib.last_error()
        assert hip.hipStreamSynchronize(stream) == 0
        gtotal = int(fetch(d_gst, 24)[16])
        d_gout = dbuf(gtotal)
        t = timed(lambda: gapfill_call(d_gout, gtotal))
        gstat = dict(zip(_lib.GAPFILL_STATUS, [int(x) for x in fetch(d_gst, 24)]))
        assert gstat["bases_not_written"] == 0
        t.update({"call": "gapfill_device", "status": gstat, "over_scaffold_device": t["median_ms"] / scaffold_ms})
        out["calls"].append(t)
        gapfill_ms = t["median_ms"]

        def join_call(d_jout, cap):
            return L.sigax_join_device(pair.handle, d_stat, n, d_so, d_st16, d_gco, d_scl, d_glay, d_gout, gtotal, C.byref(jopts), d_jco, d_jlay, d_jout, cap,
                                       d_joins, d_jst, d_jwork, wj.value, stream)

        assert join_call(None, 0) == 0, _lib.last_error()
        assert hip.hipStreamSynchronize(stream) == 0
        jtotal = int(fetch(d_jst, 16)[11])
        d_jout = dbuf(jtotal)
        t = timed(lambda: join_call(d_jout, jtotal))
        jstat = dict(zip(_lib.JOIN_STATUS, [int(x) for x in fetch(d_jst, 16)]))
        assert jstat["bases_not_written"] == 0 and jstat["gaps"] == gstat["gaps"]
        # the two calls number the gaps alike: record g of either is the same pair of neighbours
        grecs = fetch(d_gaps, gstat["gaps"], _lib.GAP_DTYPE)
        jrecs = fetch(d_joins, jstat["gaps"], _lib.JOIN_DTYPE)
        still_open = grecs["cls"] != 0
        now = {}
        for gcls in sorted(set(int(x) for x in grecs["cls"][still_open])):
            sel = still_open & (grecs["cls"] == gcls)
            now[_lib.GAP_CLASSES[gcls]] = {"gaps": int(sel.sum()),
                                          "by_join_class": {_lib.JOIN_CLASSES[c]: int((jrecs["cls"][sel] == c).sum())
                                                            for c in sorted(set(int(x) for x in jrecs["cls"][sel]))}}
        t.update({"call": "join_device", "status": jstat, "over_scaffold_device": t["median_ms"] / scaffold_ms,
                  "over_gapfill_device": t["median_ms"] / gapfill_ms, "gaps_left_open_by_gapfill": int(still_open.sum()),
                  "of_them_joined": int((jrecs["cls"][still_open] == 0).sum()), "open_gaps_by_gapfill_class": now,
                  "n_bases_left": gstat["n_bases_left"] - jstat["n_bases_removed"],
                  "overlap_lengths_joined": {"min": int(jrecs["overlap"][jrecs["cls"] == 0].min()) if jstat["joined"] else 0,
                                             "max": int(jrecs["overlap"][jrecs["cls"] == 0].max()) if jstat["joined"] else 0}})
        out["calls"].append(t)
        # every joined junction against the genome: the k bases on either side of where L ended must lie there on one strand
        seqs = fetch(d_jout, jtotal, np.uint8).tobytes()
        sco = fetch(d_jco, sstat["scaffolds"] + 1)
        genome = genome_of(args)
        other = genome.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
        k, checked, differ = args.join_kmer, 0, 0
        for r in jrecs[jrecs["cls"] == 0][:args.check]:
            at = int(sco[r["scaffold"]]) + int(r["offset"]) + int(r["overlap"])
            piece = seqs[max(at - k, int(sco[r["scaffold"]])):min(at + k, int(sco[r["scaffold"] + 1]))]
            checked += 1
            differ += piece not in genome and piece not in other
        out["junctions_checked"] = checked
        out["junctions_that_differ_from_the_genome"] = differ
        if args.mismatches > 0:
            wa = C.c_uint64()
            assert L.sigax_join_approx_workspace(n, C.byref(wa)) == 0
            d_mm, d_ast, d_awork = dbuf(4 * n), dbuf(192), dbuf(wa.value)
            aopts = _lib.JoinApproxOpts(0, args.join_min_overlap, args.join_max_overlap, args.join_slack, args.join_kmer, args.join_min_count,
                                        args.mismatches, args.permille, 0)

            def approx_call(d_aout, cap):
                return L.sigax_join_approx_device(pair.handle, d_stat, n, d_so, d_st16, d_gco, d_scl, d_glay, d_gout, gtotal, C.byref(aopts), d_jco, d_jlay,
                                                  d_aout, cap, d_joins, d_mm, d_ast, d_awork, wa.value, stream)

            assert approx_call(None, 0) == 0, _lib.last_error()
            assert hip.hipStreamSynchronize(stream) == 0
            atotal = int(fetch(d_ast, 24)[11])
            d_aout = dbuf(atotal)
            exact_ms = t["median_ms"]
            t = timed(lambda: approx_call(d_aout, atotal))
            astat = dict(zip(_lib.JOIN_APPROX_STATUS, [int(x) for x in fetch(d_ast, 24)]))
            assert astat["bases_not_written"] == 0 and astat["gaps"] == jstat["gaps"]
            arecs = fetch(d_joins, astat["gaps"], _lib.JOIN_DTYPE)
            mm = fetch(d_mm, astat["gaps"], np.uint32)
            approx = (arecs["cls"] == 0) & (mm >> 16 != 0)
            was = jrecs["cls"]  # the exact call's class of the same gap
            assert bool(((arecs["cls"] == was) | (was == 4)).all()), "a gap the exact call did not class NONE changed"
            aseqs = fetch(d_aout, atotal, np.uint8).tobytes()
            asco = fetch(d_jco, sstat["scaffolds"] + 1)
            checked = differ = 0
            for r in arecs[approx][:args.check]:
                lo_, hi_ = int(asco[r["scaffold"]]), int(asco[r["scaffold"] + 1])
                at = lo_ + int(r["offset"])  # where the overlap begins
                piece = aseqs[max(at - k, lo_):min(at + int(r["overlap"]) + k, hi_)]
                checked += 1
                differ += piece not in genome and piece not in other
            t.update({"call": "join_approx_device", "max_mismatches": args.mismatches, "mismatch_permille": args.permille, "status": astat,
                      "over_join_device": t["median_ms"] / exact_ms, "workspace_bytes": int(wa.value),
                      "approximate_joins": int(approx.sum()), "columns_taken_left": astat["mismatch_columns"] - astat["columns_from_right"],
                      "columns_taken_right": astat["columns_from_right"],
                      "exact_NONE_gaps_now": {_lib.JOIN_CLASSES[c]: int((arecs["cls"][was == 4] == c).sum())
                                              for c in sorted(set(int(x) for x in arecs["cls"][was == 4]))},
                      "mismatches_of_approximate_joins": {str(d): int(((mm & 0xFF)[approx] == d).sum()) for d in sorted(set(int(x) for x in (mm & 0xFF)[approx]))},
                      "overlap_lengths_joined_approximately": {"min": int(arecs["overlap"][approx].min()) if approx.any() else 0,
                                                               "max": int(arecs["overlap"][approx].max()) if approx.any() else 0},
                      "approximate_junctions_checked": checked, "approximate_junctions_that_differ_from_the_genome": differ})
            t["ends_of_the_gaps_still_NONE"] = nearest_overlaps(fetch(d_gout, gtotal, np.uint8).tobytes(), fetch(d_gco, sstat["scaffolds"] + 1),
                                                                fetch(d_scl, sstat["scaffolds"] + 1), fetch(d_glay, n, _lib.PLACEMENT_DTYPE),
                                                                fetch(d_so, n + 1), arecs, arecs["cls"] == 4, args.join_min_overlap, args.join_max_overlap)
            out["calls"].append(t)
    finally:
        for q in held:
            hip.hipFree(q)
        if bt:
            L.sigax_batch_destroy(bt)
        L.sigax_stream_destroy(0, stream)
        pair.close()
    with open(os.path.join(args.dir, "join.json"), "w") as f:
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
    ap.add_argument("--gap-kmer", type=int, default=31)
    ap.add_argument("--gap-min-count", type=int, default=3)
    ap.add_argument("--gap-slack", type=int, default=100)
    ap.add_argument("--gap-max-fill", type=int, default=10000)
    ap.add_argument("--walk-bases", type=int, default=1 << 28, help="bytes of walk scratch")
    ap.add_argument("--join-min-overlap", type=int, default=16)
    ap.add_argument("--join-max-overlap", type=int, default=1000)
    ap.add_argument("--join-slack", type=int, default=100)
    ap.add_argument("--join-kmer", type=int, default=31)
    ap.add_argument("--join-min-count", type=int, default=3)
    ap.add_argument("--mismatches", type=int, default=0, help="also measure sigax_join_approx_device with this max_mismatches (0: the exact call alone)")
    ap.add_argument("--permille", type=int, default=50, help="its mismatch_permille")
    ap.add_argument("--check", type=int, default=20000, help="joined junctions to look up in the genome, at most")
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
    for rate in rates:
        with tempfile.TemporaryDirectory() as d:
            for step in ("index", "measure"):  # the next step only after a clean exit of the one before
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d,
                       "--error-rate", str(rate)]
                for key in ("reads", "genome", "length", "insert", "seed", "min_overlap", "bins", "max_span", "min_pairs", "link_ratio",
                            "min_unitig_bases", "max_gap", "steps", "warmup", "check", "gap_kmer", "gap_min_count", "gap_slack", "gap_max_fill", "walk_bases",
                            "join_min_overlap", "join_max_overlap", "join_slack", "join_kmer", "join_min_count", "mismatches", "permille"):
                    cmd += ["--" + key.replace("_", "-"), str(getattr(args, key))]
                rc = subprocess.call(cmd, cwd=ROOT)
                if rc != 0:
                    print("step %s (error rate %g) ended with status %d" % (step, rate, rc), file=sys.stderr)
                    return 1
            with open(os.path.join(d, "join.json")) as f:
                result["sets"].append(json.load(f))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
