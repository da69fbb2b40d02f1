"""Helpers shared by the BASELINE-sized GPU tests: compare a GPU result with the oracle's batch call, and a numpy
restatement of Hit2OverlapConverter::convert (src/overlap_builder.cpp:345-375) for the edge records; the corrector's
cases against the oracle, and its device-resident entry point driven through the HIP runtime."""
import ctypes as C
import hashlib
import os

import numpy as np

COLS = ["capped0_lo", "capped0_hi", "capped1_lo", "capped1_hi", "raw0_lo", "raw0_hi", "raw1_lo", "raw1_hi", "length", "af"]


def blocks_matrix(blocks):
    """structured sigax_block array -> u64 [k, 10] in the oracle's column order"""
    out = np.empty((len(blocks), 10), dtype=np.uint64)
    for i, c in enumerate(COLS):
        out[:, i] = blocks[c]
    return out


def assert_same_blocks(res, want, what=""):
    """res: siga_amd OverlapBuilder.overlap result; want: oracle.pyoracle.overlap_batch result"""
    assert np.array_equal(res["block_offs"], want["block_offs"]), what + " block_offs differ"
    got = blocks_matrix(res["blocks"])
    if not np.array_equal(got, want["blocks"]):
        bad = np.nonzero((got != want["blocks"]).any(axis=1))[0]
        owner = np.searchsorted(want["block_offs"], bad[0], side="right") - 1
        raise AssertionError("%s %d blocks differ; first: block %d of read %d\n got  %s\n want %s" % (
            what, len(bad), bad[0], owner, got[bad[0]], want["blocks"][bad[0]]))
    assert np.array_equal(res["substring"].astype(bool), want["substring"].astype(bool)), what + " substring flags differ"
    s = res["stats"]
    assert s["n_occ_find"] + s["n_occ_extract"] == want["n_occ_min"], what + " N_occ_min differs"


def expected_edges(blocks10, block_offs, sai, rsai, read_len, name_rank, read_base=0):
    """Hit2OverlapConverter::convert over all blocks in hits order -> u32 [e, 4] (query, target, length, af)."""
    nb = len(blocks10)
    lo, hi = blocks10[:, 0].astype(np.int64), blocks10[:, 1].astype(np.int64)
    length, af = blocks10[:, 8].astype(np.int64), blocks10[:, 9].astype(np.int64)
    owner = np.repeat(np.arange(len(block_offs) - 1, dtype=np.int64), np.diff(block_offs.astype(np.int64))) + read_base
    cnt = np.maximum(hi - lo + 1, 0)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if nb else np.zeros(0, dtype=np.int64)
    total = int(cnt.sum())
    bi = np.repeat(np.arange(nb, dtype=np.int64), cnt)
    j = lo[bi] + (np.arange(total, dtype=np.int64) - start[bi])
    rev = (af[bi] & 2) != 0
    t = np.where(rev, rsai[j], sai[j]).astype(np.int64)
    q = owner[bi]
    nq, nt = name_rank[q].astype(np.int64), name_rank[t].astype(np.int64)
    ln = length[bi]
    contained = (ln == read_len[q]) | (ln == read_len[t])          # Match::isContainment (coord.h:150-152)
    keep = (nq != nt) & ~((nq < nt) | (contained & ((af[bi] & 1) != 0)))  # :358, :365
    out = np.stack([q[keep], t[keep], ln[keep], af[bi][keep]], axis=1).astype(np.uint32)
    return out


def edges_matrix(edges):
    return np.stack([edges["query"], edges["target"], edges["length"], edges["af"]], axis=1).astype(np.uint32)


def read_sai(path):
    """.sai text (src/suffix_array.cpp:17-44) -> read ids"""
    data = np.fromfile(path, dtype=np.uint8)
    txt = data.tobytes().split(b"\n", 3)
    body = np.frombuffer(txt[3], dtype=np.uint8)
    # lines "<id> 0": parse with numpy: split on newline via loadtxt is slow for 20M lines; use a vectorised digit parse
    nl = np.nonzero(body == 10)[0]
    starts = np.concatenate([[0], nl[:-1] + 1])
    sp = nl - 2  # position of the space before the trailing '0'
    lens = sp - starts
    out = np.zeros(len(nl), dtype=np.int64)
    maxlen = int(lens.max()) if len(lens) else 0
    for k in range(maxlen):
        has = lens > k
        d = body[np.minimum(starts + k, len(body) - 1)].astype(np.int64) - 48
        out = np.where(has, out * 10 + d, out)
    return out.astype(np.uint32)


# ---- `siga correct` ------------------------------------------------------------------------------------------------------
def pack_case(case):
    """a case of make_reads.correct_case -> (seqs uint8[total], quals uint8[total] or None, offs u64[n+1])"""
    from oracle import pyoracle as po
    b, offs = po.pack_reads([s for _, s in case["reads"]])
    q = None if case["quals"] is None else np.frombuffer("".join(case["quals"]).encode(), dtype=np.uint8)
    return np.frombuffer(b, dtype=np.uint8), q, offs


def correct_oracle(case, index=None):
    """the oracle's (out_seqs, valid) for a case.  With SIGA_CORRECT_ORACLE_CACHE set to a directory the result is kept
    there under a hash of the case: tests/test_gpu_wide.py runs every case under many kernel forms and asks once."""
    from oracle import pyoracle as po
    seqs, quals, offs = pack_case(case)
    args = (case["k"], case["threshold"], case["rounds"], case["offset"])
    cache = os.environ.get("SIGA_CORRECT_ORACLE_CACHE")
    path = None
    if cache:
        h = hashlib.sha1(seqs.tobytes() + b"|" + (quals.tobytes() if quals is not None else b"-") + offs.tobytes() + repr(args).encode())
        path = os.path.join(cache, "correct_%s.npz" % h.hexdigest()[:20])
        if os.path.exists(path):
            z = np.load(path)
            return z["out"], z["valid"]
    index = index or po.Index.build([s for _, s in case["reads"]])
    out, valid = po.correct_batch(index, (seqs, offs), quals, *args)
    if path:
        tmp = path + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, out=out, valid=valid)
        os.replace(tmp, path)
    return out, valid


def assert_same_correction(got, want, offs, what=""):
    """got, want: (out_seqs, valid); every read's bytes and flag must be equal"""
    go, gv = got
    wo, wv = want
    if np.array_equal(gv, wv) and np.array_equal(go, wo):
        return
    offs = offs.astype(np.int64)
    bad_b = np.nonzero(go != wo)[0]
    r_b = int(np.searchsorted(offs, bad_b[0], side="right") - 1) if len(bad_b) else len(gv)
    bad_v = np.nonzero(gv != wv)[0]
    r = min(r_b, int(bad_v[0]) if len(bad_v) else len(gv))
    a, b = int(offs[r]), int(offs[r + 1])
    raise AssertionError("%s: %d reads differ in valid[], %d bytes differ; first: read %d, %d bases\n got  valid=%d %s\n want valid=%d %s" % (
        what, len(bad_v), len(bad_b), r, b - a, gv[r], go[a:b].tobytes().decode("latin-1"), wv[r], wo[a:b].tobytes().decode("latin-1")))


def correct_on_device(L, handle, seqs, quals, offs, k, threshold, rounds, offset):
    """sigax_correct_device on buffers made through the HIP runtime the library itself runs on (torch brings a second copy of
    it) -> (out_seqs, valid, stat4)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    held = []

    def dbuf(nbytes, src=None):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), nbytes) == 0
        held.append(q)
        assert hip.hipMemset(q, 0, nbytes) == 0
        if src is not None:
            assert hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0  # host to device
        return q

    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = len(offs) - 1
    try:
        d_seqs, d_offs = dbuf(len(seqs) + 16, seqs), dbuf(offs.nbytes, offs)
        d_quals = dbuf(len(seqs) + 16, np.ascontiguousarray(quals, dtype=np.uint8)) if quals is not None else None
        d_out, d_val, d_stat = dbuf(len(seqs) + 16), dbuf(n + 16), dbuf(32)
        assert hip.hipDeviceSynchronize() == 0
        from siga_amd import _lib
        assert L.sigax_correct_device(handle, d_seqs, d_quals, d_offs, n, k, threshold, rounds, offset, d_out, d_val, d_stat, None) == 0, _lib.last_error()
        assert hip.hipDeviceSynchronize() == 0
        out, val, stat = np.zeros(len(seqs), dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(4, dtype=np.uint64)
        assert hip.hipMemcpy(out.ctypes.data, d_out, len(seqs), 2) == 0 and hip.hipMemcpy(val.ctypes.data, d_val, n, 2) == 0
        assert hip.hipMemcpy(stat.ctypes.data, d_stat, 32, 2) == 0
    finally:
        for q in held:
            hip.hipFree(q)
    return out, val, stat
