// siga_amd/csrc/sigax_correct.cpp -- `siga correct` on the device: its prefix and k-mer tables and entry points.
#include <algorithm>
#include <chrono>
#include <cstdio>

#include "sigax_internal.h"

// the 12-mer table of the k-mer lookups, built on first use (an accelerator: without it every lookup walks all its steps)
// Built by the first correction call ON THAT CALL'S STREAM (no device-wide wait: sigax_correct_device stays asynchronous;
// the allocation itself is the one synchronous step); later calls on other streams wait for the build's event.
static void ensure_prefix_table(sigax_index* ix, hipStream_t st) {
  std::lock_guard<std::mutex> lock(*ix->enqueue_mu);
  if (ix->ptab_tried) {
    if (ix->d_ptab && ix->ptab_ev) (void)hipStreamWaitEvent(st, ix->ptab_ev, 0);
    return;
  }
  ix->ptab_tried = true;
  // 0 = none, 8 .. 14 = that many symbols.  Default 13 (537 MB): measured at BASELINE configs[3], k = 31, 28.1 / 31.3 / 29.5 M
  // reads/s with 12 / 13 / 14 symbols (21.1 M without) -- the 2 GB table of all 14-mers no longer sits in the caches
  uint32_t pk = settings().kmer_prefix;
  if (pk == 0) return;
  pk = std::min(std::max(pk, 8u), 14u);
  void* tab = nullptr;
  if (hipMalloc(&tab, prefix_table_bytes(ix->wide, pk)) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  launch_prefix_build(ix->st[0], ix->wide, tab, pk, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ix->ptab_ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(ix->ptab_ev, st);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(st);
    hipFree(tab);
    return;
  }
  ix->d_ptab = tab;
  ix->ptab_k = pk;
  ix->device_bytes += prefix_table_bytes(ix->wide, pk);
}

// The corrector's k-mer table (see sigax_index): (re)built when a correction call comes with another k.  Synchronous (the
// build takes 0.1 s at BASELINE configs[3]; it happens once per index and k); an accelerator: whatever fails leaves the
// prefix-table + walk path in charge.  SIGAX_KMER_TABLE=0 turns it off.
static void ensure_kmer_table(sigax_index* ix, uint32_t k) {
  std::lock_guard<std::mutex> lock(*ix->enqueue_mu);
  if (ix->ktab_k == k || ix->ktab_tried_k == k) return;
  ix->ktab_tried_k = k;
  if (settings().kmer_table_off || k < 8 || k > SIGAX_DEEP_KMAX || ix->n_symbols == 0 || ix->st[0].C[1] >= 0xFFFFFFFFull) return;
  const bool verbose = settings().verbose;
  const auto t0 = std::chrono::steady_clock::now();
  if (ix->d_ktab) {  // a table for another k: no correction call is running on it (the caller serialises calls that change k)
    (void)hipDeviceSynchronize();
    hipFree(ix->d_ktab);
    ix->d_ktab = nullptr;
    ix->device_bytes -= ix->ktab_bytes;
    ix->ktab_k = 0;
    ix->ktab_bytes = 0;
  }
  const u64 n_stretch = ix->st[0].C[1];
  FmStrand f = ix->st[0];
  hipStream_t sb = nullptr;
  if (hipStreamCreateWithFlags(&sb, hipStreamNonBlocking) != hipSuccess) return;
  bool ok = true;
  const uint32_t* slen = ix->d_slen[0];
  if (!(f.sa && f.text && slen)) {
    // forward row table (bare entries) + text + stretch lengths of our own
    if (!ix->d_csa) {
      void* info = nullptr;
      u32* d_max = nullptr;
      uint32_t maxlen = 0;
      ok = hipMalloc(&info, std::max<u64>(n_stretch, 1) * 8) == hipSuccess && hipMalloc((void**)&d_max, 8) == hipSuccess &&
           hipMemsetAsync(d_max, 0, 8, sb) == hipSuccess;
      if (ok) {
        launch_stretch_scan(ix->st[0], ix->wide, n_stretch, (u64*)info, d_max, sb);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(&maxlen, d_max, 4, hipMemcpyDeviceToHost, sb) == hipSuccess &&
             hipStreamSynchronize(sb) == hipSuccess;
      }
      RowTabGeom g = row_tab_geom(ix, maxlen, 0);
      ok = ok && g.sa_bits <= 57;
      size_t mfree = 0, mtotal = 0;
      (void)hipMemGetInfo(&mfree, &mtotal);
      ok = ok && g.sa_bytes + g.text_bytes + n_stretch * 4 < (u64)mfree / 2;
      ok = ok && hipMalloc(&ix->d_csa, g.sa_bytes) == hipSuccess && hipMalloc(&ix->d_ctext, g.text_bytes) == hipSuccess &&
           hipMalloc((void**)&ix->d_cslen, std::max<u64>(n_stretch, 1) * 4) == hipSuccess &&
           hipMemsetAsync(ix->d_csa, 0, g.sa_bytes, sb) == hipSuccess && hipMemsetAsync(ix->d_ctext, 0, g.text_bytes, sb) == hipSuccess;
      if (ok) {
        launch_rows_fill(ix->st[0], ix->wide, n_stretch, (const u64*)info, (unsigned char*)ix->d_csa, g.sa_bits, g.ld_bits, g.t_bits,
                         (unsigned char*)ix->d_ctext, g.text_stride, ix->d_cslen, sb);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(sb) == hipSuccess;
      }
      if (info) hipFree(info);
      if (d_max) hipFree(d_max);
      if (ok) {
        ix->csa_bits = g.sa_bits;
        ix->cld_bits = g.ld_bits;
        ix->ct_bits = g.t_bits;
        ix->ctext_stride = g.text_stride;
        ix->device_bytes += g.sa_bytes + g.text_bytes + n_stretch * 4;
      } else {
        (void)hipGetLastError();
        if (ix->d_csa) hipFree(ix->d_csa);
        if (ix->d_ctext) hipFree(ix->d_ctext);
        if (ix->d_cslen) hipFree(ix->d_cslen);
        ix->d_csa = ix->d_ctext = nullptr;
        ix->d_cslen = nullptr;
      }
    }
    if (ok && ix->d_csa) {
      f.sa = (const unsigned char*)ix->d_csa;
      f.text = (const unsigned char*)ix->d_ctext;
      f.xmap = nullptr;
      f.sa_bits = ix->csa_bits;
      f.ld_bits = ix->cld_bits;
      f.t_bits = ix->ct_bits;
      f.text_stride = ix->ctext_stride;
      slen = ix->d_cslen;
    } else {
      ok = false;
    }
  }
  u64* d_cnt = nullptr;
  u64* list = nullptr;
  void* tab = nullptr;
  u64 h[2] = {0, 0}, distinct = 0, slots = 0;
  ok = ok && hipMalloc((void**)&d_cnt, 16) == hipSuccess && hipMemsetAsync(d_cnt, 0, 16, sb) == hipSuccess;
  if (ok) {
    launch_deep_scan(f, slen, n_stretch, k, d_cnt, nullptr, 0, sb);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h, d_cnt, 16, hipMemcpyDeviceToHost, sb) == hipSuccess && hipStreamSynchronize(sb) == hipSuccess;
    distinct = h[0];
  }
  if (ok) {
    size_t mfree = 0, mtotal = 0;
    (void)hipMemGetInfo(&mfree, &mtotal);
    slots = std::max<u64>(64, distinct * 2 + 16);
    ok = distinct < (1ull << 32) - 256 && slots * deep_entry_bytes() + distinct * 8 < (u64)mfree / 100 * 45;
  }
  ok = ok && hipMalloc((void**)&list, std::max<u64>(distinct, 1) * 8) == hipSuccess && hipMalloc(&tab, slots * deep_entry_bytes()) == hipSuccess &&
       hipMemsetAsync(tab, 0, slots * deep_entry_bytes(), sb) == hipSuccess && hipMemsetAsync(d_cnt, 0, 16, sb) == hipSuccess;
  if (ok) {
    launch_deep_scan(f, slen, n_stretch, k, d_cnt, list, distinct, sb);
    launch_deep_fill(f, f, ix->wide, slen, n_stretch, k, list, distinct, tab, slots, d_cnt + 1, sb);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h, d_cnt, 16, hipMemcpyDeviceToHost, sb) == hipSuccess && hipStreamSynchronize(sb) == hipSuccess &&
         h[0] == distinct && h[1] == 0;
  }
  if (list) hipFree(list);
  if (d_cnt) hipFree(d_cnt);
  (void)hipStreamDestroy(sb);
  if (!ok) {
    (void)hipGetLastError();
    if (tab) hipFree(tab);
    if (verbose) fprintf(stderr, "[sigax] k-mer table for k = %u not built: the corrector walks\n", k);
    return;
  }
  ix->d_ktab = tab;
  ix->ktab_slots = slots;
  ix->ktab_k = k;
  ix->ktab_bytes = slots * deep_entry_bytes();
  ix->device_bytes += ix->ktab_bytes;
  if (verbose)
    fprintf(stderr, "[sigax] k-mer table: k = %u, %llu distinct k-mers, %.2f GB, %.3f s\n", k, distinct, ix->ktab_bytes / 1e9,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

static CorrectArgs correct_args(sigax_index* ix, const unsigned char* d_seqs, const unsigned char* d_quals, const u64* d_offs, u64 n_reads,
                                uint32_t kmer_size, int32_t kmer_threshold, uint32_t kmer_rounds, uint32_t count_offset,
                                unsigned char* d_out, unsigned char* d_valid, u64* d_stat, hipStream_t st) {
  CorrectArgs ca;
  ca.fwd = ix->st[0];
  ca.seqs = d_seqs;
  ca.quals = d_quals;
  ca.offs = d_offs;
  ca.n_reads = n_reads;
  ca.k = kmer_size;
  // CorrectThreshold::minSupport (src/correct_processor.cpp:28-37) keeps two ints and hands them out as size_t: a negative
  // one is a support no count reaches (-1: low unreachable, high = 0; -2 and below: both unreachable)
  ca.low = kmer_threshold < 0 ? CORRECT_NEVER : (uint32_t)kmer_threshold;
  ca.high = kmer_threshold < -1 ? CORRECT_NEVER : (uint32_t)((long long)kmer_threshold + 1);
  ca.cutoff = 20;
  ca.rounds = kmer_rounds;
  ca.offset = count_offset;
  ca.out = d_out;
  ca.valid = d_valid;
  ca.dstat = d_stat;
  ensure_kmer_table(ix, kmer_size);
  ca.ktab = ix->ktab_k == kmer_size ? ix->d_ktab : nullptr;
  ca.ktab_slots = ix->ktab_slots;
  ensure_prefix_table(ix, st);
  ca.ptab = ix->d_ptab;
  ca.pk = ix->ptab_k;
  ca.max_len = 0;  // unknown here: sigax_correct_batch sees the offsets and says
  ca.only_deferred = 0;
  return ca;
}

extern "C" int sigax_correct_device(sigax_index* ix, const void* d_seqs, const void* d_quals, const void* d_offs, uint64_t n_reads,
                                    uint32_t kmer_size, int32_t kmer_threshold, uint32_t kmer_rounds, uint32_t count_offset,
                                    void* d_out_seqs, void* d_valid, void* d_stat4, void* stream) {
  if (!ix || kmer_size == 0 || (n_reads && (!d_seqs || !d_offs || !d_out_seqs || !d_valid || !d_stat4))) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (n_reads == 0) return SIGAX_OK;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_stat4, 0, 32, st));
  CorrectArgs ca = correct_args(ix, (const unsigned char*)d_seqs, (const unsigned char*)d_quals, (const u64*)d_offs, n_reads, kmer_size,
                                kmer_threshold, kmer_rounds, count_offset, (unsigned char*)d_out_seqs, (unsigned char*)d_valid, (u64*)d_stat4, st);
  launch_correct(ca, ix->wide, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_correct_batch(sigax_index* ix, const char* seqs, const char* quals, const uint64_t* offs, uint32_t n_reads,
                                   uint32_t kmer_size, int32_t kmer_threshold, uint32_t kmer_rounds, uint32_t count_offset,
                                   char* out_seqs, uint8_t* valid) {
  if (!ix || kmer_size == 0 || (n_reads && (!seqs || !offs || !out_seqs || !valid))) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (n_reads == 0) return SIGAX_OK;
  const u64 nb = offs[n_reads];
  unsigned char *d_seqs = nullptr, *d_quals = nullptr, *d_out = nullptr, *d_valid = nullptr;
  u64 *d_offs = nullptr, *d_stat = nullptr;
  DevGuard g;
  HIP_TRY(g.alloc((void**)&d_seqs, nb + 16));
  HIP_TRY(g.alloc((void**)&d_out, nb + 16));
  HIP_TRY(g.alloc((void**)&d_offs, ((size_t)n_reads + 1) * 8));
  HIP_TRY(g.alloc((void**)&d_valid, (size_t)n_reads + 16));
  HIP_TRY(g.alloc((void**)&d_stat, 64));
  HIP_TRY(hipMemset(d_stat, 0, 64));
  HIP_TRY(hipMemcpy(d_seqs, seqs, nb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_offs, offs, ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice));
  if (quals) {
    HIP_TRY(g.alloc((void**)&d_quals, nb + 16));
    HIP_TRY(hipMemcpy(d_quals, quals, nb, hipMemcpyHostToDevice));
  }
  CorrectArgs ca = correct_args(ix, d_seqs, d_quals, d_offs, n_reads, kmer_size, kmer_threshold, kmer_rounds, count_offset, d_out,
                                d_valid, d_stat, (hipStream_t)0);
  for (uint32_t i = 0; i < n_reads; ++i) ca.max_len = std::max<uint32_t>(ca.max_len, (uint32_t)std::min<u64>(offs[i + 1] - offs[i], 0xFFFFFFFFull));
  ca.max_len = std::max(ca.max_len, 1u);
  launch_correct(ca, ix->wide, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  u64 toolong = 0;
  HIP_TRY(hipMemcpy(&toolong, d_stat, 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_seqs, d_out, nb, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(valid, d_valid, n_reads, hipMemcpyDeviceToHost));
  if (toolong) return sigax_fail(SIGAX_E_ARG, "%llu reads are longer than the 1024 bases the correction kernel supports", toolong);
  return SIGAX_OK;
}

