#!/usr/bin/env python3
"""Pins what the backward-search kernels (sigax_match.hip, sigax_spectrum.hip, sigax_locate.hip) compute AND how much work they
count for it: runs sigax_match_device, sigax_kmer_spectrum_device, sigax_locate_device and the row walks
(sigax_string_lengths_device, sigax_get_strings_device) on generated queries over the `small` read set of tests/locate_cases.py,
in every form of the index the tests build (FORMS), and writes checksums of the results and the status words to
tests/golden/search_counters.json.  tests/test_gpu_search_counters.py runs the same cases and compares word for word, so the
file is recorded with the library of the commit BEFORE a change to those kernels and committed with the change.
Left out: d_stat4[3] of match, the chain counter's final value, which depends on the grid.  Every other word is a sum over
chains or walks of work each of them determines by itself.  Needs a GPU; nothing but this repository.

    python tools/record_search_counters.py            # all forms -> tests/golden/search_counters.json
    python tools/record_search_counters.py --form F   # one form, in this process, JSON on stdout
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "search_counters.json")
SEED = 4242
ALL = (1 << 32) - 1
SUPER12 = os.path.join(ROOT, "build", "libsigax_super12.so")
# form -> (environment of the process that loads the library, 64-bit positions, a correction call leaves the 13-mer table first)
FORMS = {
    "default": ({}, 0, False),
    "one_step": ({"SIGAX_TWO_STEP": "0"}, 0, False),
    "wide_super12": ({"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": SUPER12}, 1, False),
    "prefix_table": ({}, 0, True),
    "wide_prefix_table": ({"SIGAX_FORCE_WIDE": "1"}, 1, True),
}
MATCH_CASES = ((True, None), (False, None), (True, 50), (False, 25))  # (rc, max_length): 50 splits whole reads only
SPECTRUM_KS = (12, 13, 14, 31)                                       # pk - 1, pk, pk + 1, and an odd k of many double steps
SPECTRUM_BINS = 64
LOCATE_CASES = ((True, ALL, ALL), (False, ALL, ALL), (True, 5, 10))  # (rc, max_hits, max_len)
WALK_MAX_LENS = (1 << 20, 10)


def queries():
    """every class of chain the shared search code treats differently, from the reads of locate_cases.small()"""
    from tests import locate_cases as lc
    small = lc.small()
    reads = [s for _, s in small["reads"]]
    rnd = random.Random(SEED)
    q = [s for _, s, _ in small["queries"]]  # duplicates, a palindrome, periodic reads: intervals that stay wide
    for l in (0, 1, 2, 12, 13, 14, 27, 40):  # pk - 1, pk, pk + 1; odd and even: a single step left after the double steps or not
        for _ in range(4):
            s = reads[rnd.randrange(lc.SMALL_READS)]
            a = rnd.randrange(0, lc.SMALL_LEN - l + 1)
            q.append(s[a:a + l])
    q += reads[:40] + [reads[-1]]  # long chains, the 300-base read among them
    sub = {"A": "C", "C": "G", "G": "T", "T": "A"}
    for i in range(40, 80):  # one substitution: chains that die early, on one strand or the other
        s = reads[i]
        p = rnd.randrange(len(s))
        q.append(s[:p] + sub[s[p]] + s[p + 1:])
    for i, p in enumerate((0, 1, 2, 5, 6, 19, 20, 33, 34, 37, 38, 39)):  # a byte outside ACGT as either symbol of a pair, in
        s = reads[100 + i][10:50]                                      # both directions, and inside the first 13 symbols
        q.append(s[:p] + "N" + s[p + 1:])
    q += ["N", "NN", "AN", "NA", "ACGTACGTACGTN", "NACGTACGTACGT"]
    return q


def describe_input():
    from tests import locate_cases as lc
    return {"seed": SEED, "reads": "tests/locate_cases.py small()", "n_reads": len(lc.small()["reads"]), "n_queries": len(queries()),
            "match": [[rc, L] for rc, L in MATCH_CASES], "spectrum_k": list(SPECTRUM_KS), "spectrum_bins": SPECTRUM_BINS,
            "locate": [list(c) for c in LOCATE_CASES], "walk_max_len": list(WALK_MAX_LENS)}


def _sum(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _words(a):
    return [int(x) for x in a]


def run_cases(with_table, wide):
    """the cases on the library this process has loaded -> {case: {checksums, status words}}"""
    from oracle import pyoracle as po
    from tests import test_gpu_locate as tgl
    from tests import test_gpu_match as tgm
    from tests import test_gpu_spectrum as tgs
    q = queries()
    out = {}
    pair = tgl._open(tgl._files("small"))
    try:
        info = pair.info()
        assert info["wide"] == wide
        if with_table:
            tgs._leave_prefix_table(pair)
        for rc, L in MATCH_CASES:
            counts, stat = tgm._match_on_device(pair.handle, q, L, rc)
            out["match rc=%d L=%s" % (rc, L)] = {"counts": _sum(counts), "stat3": _words(stat[:3])}
        dev = tgs.Device()
        try:
            buf, offs = po.pack_reads(q)
            buf = np.frombuffer(buf, dtype=np.uint8)
            need = C.c_uint64()
            assert dev.L.sigax_kmer_spectrum_workspace(len(q), C.byref(need)) == 0
            d_seqs, d_offs, d_stat, d_work = dev.buf(buf.nbytes, buf), dev.buf(offs.nbytes, offs), dev.buf(32), dev.buf(need.value)
            for k in SPECTRUM_KS:
                d_hist = dev.buf(8 * SPECTRUM_BINS, fill=0)
                assert dev.L.sigax_kmer_spectrum_device(pair.handle, d_seqs, d_offs, len(q), k, SPECTRUM_BINS, d_hist, d_stat, d_work,
                                                        need.value, dev.stream) == 0
                out["spectrum k=%d" % k] = {"hist": _words(dev.get(d_hist, np.uint64, SPECTRUM_BINS)), "stat4": _words(dev.get(d_stat, np.uint64, 4))}
            n = info["n_symbols"]
            rows = np.concatenate([np.arange(0, n, 7, dtype=np.uint64), np.array([n - 1, n, (1 << 64) - 1], dtype=np.uint64)])
            m = len(rows)
            d_rows = dev.buf(rows.nbytes, rows)
            for which in (0, 1):
                for max_len in WALK_MAX_LENS:  # the second cuts most walks
                    d_lens, d_stretch, d_status = dev.buf(4 * m), dev.buf(8 * m), dev.buf(24)
                    assert dev.L.sigax_string_lengths_device(pair.handle, which, d_rows, m, max_len, d_lens, d_stretch, d_status, dev.stream) == 0
                    lens = dev.get(d_lens, np.uint32, m)
                    rec = {"lens": _sum(lens), "stretch": _sum(dev.get(d_stretch, np.uint64, m)), "status2": _words(dev.get(d_status, np.uint64, 2))}
                    o = np.zeros(m + 1, dtype=np.uint64)
                    o[1:] = np.cumsum(lens, dtype=np.uint64)
                    d_o, d_text = dev.buf(o.nbytes, o), dev.buf(int(o[-1]) + 16)
                    assert dev.L.sigax_get_strings_device(pair.handle, which, d_rows, m, max_len, d_o, d_text, d_status, dev.stream) == 0
                    rec.update({"text": _sum(dev.get(d_text, np.uint8, int(o[-1]))), "status3": _words(dev.get(d_status, np.uint64, 3))})
                    out["walk strand=%d max_len=%d" % (which, max_len)] = rec
        finally:
            dev.close()
        dl = tgl._Device()
        try:
            for rc, max_hits, max_len in LOCATE_CASES:
                none = tgl._locate_on_device(dl, pair.handle, q, rc, max_hits, max_len, 0, None)
                need = int(none[5][0])
                tot, qf, ho, hits, rows, stat, _ = tgl._locate_on_device(dl, pair.handle, q, rc, max_hits, max_len, need, None)
                out["locate rc=%d max_hits=%d max_len=%d" % (rc, max_hits, max_len)] = {
                    "search_status4": _words(none[5]), "totals": _sum(tot), "qflags": _sum(qf), "hit_offs": _sum(ho), "hits": _sum(hits),
                    "rows": _sum(rows), "status4": _words(stat), "over": int(np.count_nonzero(qf & 2)),
                    "cut": int(np.count_nonzero(hits["flags"] & 2))}
        finally:
            dl.free()
    finally:
        pair.close()
    return out


def run_form(form):
    """-> the form's cases; a form whose environment differs from this process's runs in a child (the library and its switches
    are chosen when it is loaded)"""
    env_extra, wide, with_table = FORMS[form]
    if not env_extra:
        return run_cases(with_table, wide)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--form", form], cwd=ROOT, env=dict(os.environ, **env_extra),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=sorted(FORMS), default=None)
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if args.form:
        _, wide, with_table = FORMS[args.form]
        print(json.dumps(run_cases(with_table, wide)))
        return 0
    doc = {"input": describe_input(), "forms": {form: run_form(form) for form in FORMS}}
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({form: len(cases) for form, cases in doc["forms"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
