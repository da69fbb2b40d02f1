// siga_amd/csrc/sigax_tables.cpp -- the optional tables of an index: row tables, direct maps, stretch texts and deep
// start tables (plan, allocation, fill, publishing, side threads); sigax_index_prepare{,_overlap}.
#include <algorithm>
#include <chrono>
#include <cstdio>

#include "sigax_internal.h"

// Row tables for the irreducible extractor (fm_layout.h: the suffix array as (stretch, offset), bit-packed, plus the
// stretches' text): a single-row block's extension rounds are read off its read's text instead of computed from rank
// lines, and a branch that leaves ONE single-row block in a group -- what a substitution in an overlapping read does -- is
// resolved by one lookup instead of a walk to the end of that read (~100 dependent rounds).  An accelerator like the
// two-step tables: skipped when memory is short or SIGAX_ROWEND=0 (SIGAX_LOOKAHEAD=0: no text, countdowns only), and the
// extractor then walks.  Built on the index's own device (a clone builds its own: 2 n LF steps on the spot beat copying
// the tables between GPUs).
static u32 bits_for(u64 maxval) {  // bits that hold 0 .. maxval
  u32 b = 1;
  while (b < 64 && (maxval >> b) != 0) ++b;
  return b;
}
// syms = symbols an entry carries at most (as many as keep it within the 57 bits one unaligned 8-byte load delivers)
RowTabGeom row_tab_geom(const sigax_index* ix, u32 maxlen, u32 syms) {
  RowTabGeom g;
  const u64 n_stretch = ix->st[0].C[1];
  g.ld_bits = bits_for(n_stretch ? n_stretch - 1 : 0);
  g.t_bits = bits_for(maxlen);
  g.sa_bits = g.ld_bits + g.t_bits;
  if (g.sa_bits < 57) g.sa_bits += 2 * std::min<u32>(syms, std::min<u32>(14u, (57 - g.sa_bits) / 2));
  g.text_stride = ((2 * maxlen + 7) / 8 + 8 + 7) & ~7u;  // 2 bits per symbol; the build ORs whole 8-byte words in
  g.sa_bytes = ((ix->n_symbols * g.sa_bits + 63) / 64) * 8 + 16;
  g.text_bytes = n_stretch * (u64)g.text_stride + 16;
  return g;
}
// the longest stretch this index can hold, as far as the host knows: no stretch is longer than the longest read
static u32 maxlen_bound(const sigax_index* ix) {
  if (ix->max_read_len) return ix->max_read_len;
  const u64 n_stretch = std::max<u64>(ix->st[0].C[1], 1);
  const u64 avg = ix->n_symbols / n_stretch;
  return (u32)std::min<u64>(std::max<u64>(2 * avg, avg + 64), (1u << 28) - 1);
}
// Which tables does this index get?  Decided from the free memory of that moment.
void plan_row_tables(sigax_index* ix) {
  const Settings& cfg = settings();
  ix->tab_plan = 0;
  if (cfg.rowend_off || ix->st[0].C[1] >= 0xFFFFFFFFull || ix->n_symbols == 0) return;
  size_t mfree = 0, mtotal = 0;
  (void)hipMemGetInfo(&mfree, &mtotal);
  ix->tab_text = !cfg.lookahead_off;
  // Row table with as many of its entries' first symbols (14 at most) as fit half of the free memory (one lookup then
  // serves an item's first rounds: at BASELINE configs[1] 14 symbols, 56 bits per row); bare entries when they fit 70 %;
  // else -- when the .sai tables are there and every stretch is a read (no non-ACGT bases) -- the DIRECT MAPS (fm_layout.h):
  // text + 8 bytes per read and strand, no table per BWT symbol.  Measured (gpurun_out/r3u/): one lookup in the big table
  // beats two in small ones -- configs[1] 119.9 M reads/s on the row table, 108.8 M on direct maps (whose 112 MB compete
  // with the finder's table for the Infinity Cache: the finder goes from 8.3 to 9.1 ms), configs[2] shape 86.4 vs 77.4 M,
  // configs[4] (bare entries: two lookups either way) 38.4 vs 37.3 M with 188 vs 79 GB on the device -- so the direct maps
  // are what an index too big for a row table gets instead of nothing.  SIGAX_XMAP=1 forces them, =0 forbids them.
  const bool can_direct = ix->tab_text && cfg.xmap != '0' && ix->d_sai[0] && ix->d_sai[1] && ix->n_sai == ix->n_strings &&
                          ix->st[0].C[1] == ix->n_strings && ix->st[1].C[1] == ix->n_strings;
  auto plan_direct = [&]() -> bool {
    const RowTabGeom g = row_tab_geom(ix, maxlen_bound(ix), 0);
    const u64 want = 2 * (g.text_bytes + 8 * ix->n_strings);
    if (!can_direct || want >= mfree / 10 * 7) return false;
    ix->tab_direct = true;
    ix->tab_plan = want;
    ix->tab_syms = 0;
    return true;
  };
  ix->tab_direct = false;
  if (cfg.xmap == '1' && plan_direct()) return;
  for (u32 syms = ix->tab_text ? cfg.row_syms : 0u;; --syms) {
    const RowTabGeom g = row_tab_geom(ix, maxlen_bound(ix), syms);
    if (g.sa_bits > 57) break;
    const u64 want = 2 * (g.sa_bytes + (ix->tab_text ? g.text_bytes : 0));
    if (want < mfree / 10 * (syms ? 5 : 7)) {
      ix->tab_plan = want;
      ix->tab_syms = syms;
      return;
    }
    if (syms == 0) break;
  }
  (void)plan_direct();
}

static void free_row_tables(sigax_index* ix) {
  for (int s = 0; s < 2; ++s) {
    if (ix->d_sa[s]) hipFree(ix->d_sa[s]);
    if (ix->d_text[s]) hipFree(ix->d_text[s]);
    if (ix->d_xmap[s]) hipFree(ix->d_xmap[s]);
    ix->d_sa[s] = ix->d_text[s] = ix->d_xmap[s] = nullptr;
    ix->sa_alloc[s] = ix->text_alloc[s] = 0;
  }
}

// Allocation, on the caller's thread (by the bound of the longest stretch) ...
static bool alloc_row_tables(sigax_index* ix) {
  const RowTabGeom g = row_tab_geom(ix, maxlen_bound(ix), ix->tab_syms);
  ix->tab_plan = 0;
  hipError_t e = hipSuccess;
  for (int s = 0; s < 2 && e == hipSuccess; ++s) {
    if (!ix->tab_direct) {
      e = hipMalloc(&ix->d_sa[s], g.sa_bytes);
      if (e == hipSuccess) ix->sa_alloc[s] = g.sa_bytes;
    } else {
      e = hipMalloc(&ix->d_xmap[s], std::max<u64>(ix->n_strings, 1) * 8);
    }
    if (e == hipSuccess && ix->tab_text) {
      e = hipMalloc(&ix->d_text[s], g.text_bytes);
      if (e == hipSuccess) ix->text_alloc[s] = g.text_bytes;
    }
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    free_row_tables(ix);
    if (settings().verbose) fprintf(stderr, "[sigax] row tables not allocated (%s): the extractor walks\n", hipGetErrorString(e));
    return false;
  }
  return true;
}

// ... and the fill, on a stream of its own (possibly on a side thread): the first walk measures the longest stretch, which
// fixes the entry width; buffers that turn out too small for it (the bound was an estimate) are allocated again here
static void fill_row_tables(sigax_index* ix, FmStrand out[2], u64* out_bytes) {
  out[0] = ix->st[0];
  out[1] = ix->st[1];
  *out_bytes = 0;
  const u64 n_stretch = ix->st[0].C[1];
  hipStream_t sb = nullptr;
  void* info = nullptr;
  u32* d_max = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&sb, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(&info, std::max<u64>(n_stretch, 1) * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&d_max, 8);
  u32 maxlen[2] = {0, 0};
  RowTabGeom g[2];
  const bool direct = ix->tab_direct;
  // the stretches' lengths by '$' rank: what the direct maps are composed from, and what the deep start table's build reads
  // a row's remaining symbols off (kept with the index: 4 bytes per read and strand)
  u32* slen[2] = {nullptr, nullptr};
  u32* isai = nullptr;
  if (ix->tab_text) {
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
      if (!ix->d_slen[s]) e = hipMalloc((void**)&ix->d_slen[s], std::max<u64>(n_stretch, 1) * 4);
      slen[s] = ix->d_slen[s];
    }
  }
  if (direct && e == hipSuccess) e = hipMalloc((void**)&isai, std::max<u64>(n_stretch, 1) * 4);
  for (int s = 0; s < 2 && e == hipSuccess; ++s) {
    e = hipMemsetAsync(d_max, 0, 8, sb);
    if (e != hipSuccess) break;
    launch_stretch_scan(ix->st[s], ix->wide, n_stretch, (u64*)info, d_max, sb);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&maxlen[s], d_max, 4, hipMemcpyDeviceToHost, sb);
    if (e == hipSuccess) e = hipStreamSynchronize(sb);
    if (e != hipSuccess) break;
    g[s] = row_tab_geom(ix, maxlen[s], ix->tab_syms);
    if (g[s].sa_bits > 57) { e = hipErrorInvalidValue; break; }
    if (!direct && g[s].sa_bytes > ix->sa_alloc[s]) {
      hipFree(ix->d_sa[s]);
      ix->d_sa[s] = nullptr;
      ix->sa_alloc[s] = 0;
      e = hipMalloc(&ix->d_sa[s], g[s].sa_bytes);
      if (e != hipSuccess) break;
      ix->sa_alloc[s] = g[s].sa_bytes;
    }
    if (ix->tab_text && g[s].text_bytes > ix->text_alloc[s]) {
      hipFree(ix->d_text[s]);
      ix->d_text[s] = nullptr;
      ix->text_alloc[s] = 0;
      e = hipMalloc(&ix->d_text[s], g[s].text_bytes);
      if (e != hipSuccess) break;
      ix->text_alloc[s] = g[s].text_bytes;
    }
    if (!direct) e = hipMemsetAsync(ix->d_sa[s], 0, ix->sa_alloc[s], sb);
    if (e == hipSuccess && ix->tab_text) e = hipMemsetAsync(ix->d_text[s], 0, ix->text_alloc[s], sb);
    if (e != hipSuccess) break;
    launch_rows_fill(ix->st[s], ix->wide, n_stretch, (const u64*)info, direct ? nullptr : (unsigned char*)ix->d_sa[s], g[s].sa_bits, g[s].ld_bits,
                     g[s].t_bits, ix->tab_text ? (unsigned char*)ix->d_text[s] : nullptr, g[s].text_stride, slen[s], sb);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(sb);
  }
  // direct maps: strand s as extension index serves the blocks whose capped[0] counts the OTHER strand's '$' rows
  for (int s = 0; direct && s < 2 && e == hipSuccess; ++s) {
    launch_xmap(ix->d_sai[1 - s], ix->d_sai[s], isai, slen[s], ix->n_strings, (u64*)ix->d_xmap[s], sb);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(sb);
  }
  if (isai) hipFree(isai);
  if (sb) (void)hipStreamDestroy(sb);
  if (info) hipFree(info);
  if (d_max) hipFree(d_max);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (settings().verbose) fprintf(stderr, "[sigax] row tables not built (%s): the extractor walks\n", hipGetErrorString(e));
    return;  // the buffers are freed with the index
  }
  for (int s = 0; s < 2; ++s) {
    out[s].sa = direct ? nullptr : (const unsigned char*)ix->d_sa[s];
    out[s].xmap = direct ? (const u64*)ix->d_xmap[s] : nullptr;
    if (direct) *out_bytes += 8 * ix->n_strings;
    if (ix->d_slen[s]) *out_bytes += 4 * n_stretch;
    out[s].text = ix->tab_text ? (const unsigned char*)ix->d_text[s] : nullptr;
    out[s].sa_bits = g[s].sa_bits;
    out[s].ld_bits = g[s].ld_bits;
    out[s].t_bits = g[s].t_bits;
    out[s].text_stride = g[s].text_stride;
    *out_bytes += ix->sa_alloc[s] + ix->text_alloc[s];
  }
  if (settings().verbose && direct)
    fprintf(stderr, "[sigax] direct maps (8 bytes per read and strand) + text rows of %u bytes, %.2f GB\n", g[0].text_stride, *out_bytes / 1e9);
  else if (settings().verbose)
    fprintf(stderr, "[sigax] row tables: %u bits per row (stretch %u + offset %u + %u symbols), text rows of %u bytes, %.2f GB\n", g[0].sa_bits,
            g[0].ld_bits, g[0].t_bits, (g[0].sa_bits - g[0].ld_bits - g[0].t_bits) / 2, ix->tab_text ? g[0].text_stride : 0u, *out_bytes / 1e9);
}

// the tables of a finished build become visible to the runs enqueued from now on
void publish_tables(sigax_index* ix) {
  if (!ix->tab_state || ix->tab_state->load(std::memory_order_acquire) != 2) return;
  for (int s = 0; s < 2; ++s) {
    ix->st[s].sa = ix->tab_st[s].sa;
    ix->st[s].xmap = ix->tab_st[s].xmap;
    ix->st[s].text = ix->tab_st[s].text;
    ix->st[s].sa_bits = ix->tab_st[s].sa_bits;
    ix->st[s].ld_bits = ix->tab_st[s].ld_bits;
    ix->st[s].t_bits = ix->tab_st[s].t_bits;
    ix->st[s].text_stride = ix->tab_st[s].text_stride;
  }
  ix->device_bytes += ix->tab_bytes;
  ix->tab_state->store(0, std::memory_order_release);
}

// start (or do) the build: allocate here, fill on a side thread unless `sync`
void start_row_tables(sigax_index* ix, bool sync) {
  if (ix->tab_plan == 0 || ix->tab_tried) return;
  ix->tab_tried = true;
  if (!alloc_row_tables(ix)) return;
  if (sync) {
    fill_row_tables(ix, ix->tab_st, &ix->tab_bytes);
    ix->tab_state->store(2);
    publish_tables(ix);
    return;
  }
  ix->tab_state->store(1);
  ix->tab_thread = new std::thread([ix] {
    (void)hipSetDevice(ix->device);
    fill_row_tables(ix, ix->tab_st, &ix->tab_bytes);
    ix->tab_state->store(2, std::memory_order_release);
  });
}

// When are they built?  The build walks the whole index (C3: 1.8 s, 45 GB) and saves ~20 ns per read afterwards: it pays
// on an index that stays open -- a service, bench.py -- and does not in one pass of `siga overlap` over the reads the
// index was made of (BASELINE configs[2]'s read set through the CLI: 7.2 s with the tables, 3.6 s without).  So: small
// indexes (and SIGAX_TABLES_SYNC=1) at once; the others in the background once the index has been asked for as many
// reads as it holds (enqueue()), or at once when the caller says the index is here to stay (sigax_index_prepare).
void build_rowend(sigax_index* ix) {
  ix->tab_state = new std::atomic<int>(0);
  ix->deep_state = new std::atomic<int>(0);
  plan_row_tables(ix);
  if (ix->n_symbols < (1ull << 26) || settings().tables_sync) start_row_tables(ix, true);
}
// the tables in place before this returns (caller holds enqueue_mu)
void row_tables_now(sigax_index* ix) {
  if (ix->tab_thread) {  // a build in flight: wait for it
    ix->tab_thread->join();
    delete ix->tab_thread;
    ix->tab_thread = nullptr;
  }
  publish_tables(ix);
  start_row_tables(ix, true);  // (no-op when they were built, or tried, before)
}


// ------------------------------------------------------------------------------------------------------
// Deep start tables of the block finder (fm_layout.h, sigax_index_prepare_overlap).  Needs the row tables and the
// stretch text (the distinct K-mers are read off them); an accelerator like those: when memory is short, the index has no
// row tables, or a K-mer's walk does not come out at its own rows, there is no table and every chain walks.
// SIGAX_FIND_DEEP=0 never builds them; SIGAX_DEEP_K=k overrides K (tests); SIGAX_DEEP_LOAD=percent sets the load factor.
// ------------------------------------------------------------------------------------------------------
static uint32_t deep_k_for(uint32_t min_overlap) {
  const Settings& cfg = settings();
  if (cfg.find_deep_off) return 0;
  uint32_t k = cfg.deep_k ? (uint32_t)*cfg.deep_k : std::min<uint32_t>(min_overlap, SIGAX_DEEP_KMAX);
  if (k > min_overlap || k > SIGAX_DEEP_KMAX) k = std::min<uint32_t>(min_overlap, SIGAX_DEEP_KMAX);
  if (k < (cfg.deep_k ? 2u : (uint32_t)SIGAX_DEEP_KMIN)) return 0;
  return k;
}
// Tables for K from the strands' row tables `st` (a snapshot taken under enqueue_mu).  `share` = the part of the free
// memory they may take, in per cent.  On success tab[] / slots[] / *bytes are set; on any failure nothing is left allocated.
static bool build_deep_tables(sigax_index* ix, const FmStrand st[2], uint32_t K, unsigned share, void* tab[2], u64 slots[2], u64* bytes) {
  tab[0] = tab[1] = nullptr;
  slots[0] = slots[1] = 0;
  *bytes = 0;
  if (K == 0 || !st[0].sa || !st[1].sa || !st[0].text || !st[1].text || !ix->d_slen[0] || !ix->d_slen[1]) return false;
  const bool verbose = settings().verbose;
  const auto t0 = std::chrono::steady_clock::now();
  const u64 n_stretch = ix->st[0].C[1];
  const std::optional<int>& envl = settings().deep_load;  // SIGAX_DEEP_LOAD
  hipStream_t sb = nullptr;
  u64* d_cnt = nullptr;  // [0] distinct K-mers, [1] errors
  u64* list = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&sb, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&d_cnt, 16);
  bool ok = e == hipSuccess;
  u64 distinct[2] = {0, 0};
  for (int s = 0; s < 2 && ok; ++s) {
    u64 h[2] = {0, 0};
    ok = hipMemsetAsync(d_cnt, 0, 16, sb) == hipSuccess;
    if (!ok) break;
    launch_deep_scan(st[s], ix->d_slen[s], n_stretch, K, d_cnt, nullptr, 0, sb);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h, d_cnt, 16, hipMemcpyDeviceToHost, sb) == hipSuccess &&
         hipStreamSynchronize(sb) == hipSuccess;
    distinct[s] = h[0];
    if (distinct[s] >= (1ull << 32) - 256) ok = false;  // (one launch of k_deep_fill, one lane per K-mer)
  }
  if (ok) {
    // both strands' tables + the larger list must fit `share` per cent of what is free now
    size_t mfree = 0, mtotal = 0;
    (void)hipMemGetInfo(&mfree, &mtotal);
    unsigned load = envl ? (unsigned)std::min(95, std::max(5, *envl)) : 50u;
    for (;;) {
      for (int s = 0; s < 2; ++s) slots[s] = std::max<u64>(64, distinct[s] * 100 / load + 16);
      const u64 need = (slots[0] + slots[1]) * deep_entry_bytes() + std::max(distinct[0], distinct[1]) * 8;
      if (need <= (u64)mfree / 100 * share) break;
      if (envl || load >= 80) { ok = false; break; }
      load += 15;  // 50, 65, 80 per cent: longer probe sequences before no table at all
    }
    if (!ok && verbose) fprintf(stderr, "[sigax] deep start tables (K = %u, %llu + %llu K-mers) do not fit %u %% of the free memory\n", K,
                                distinct[0], distinct[1], share);
  }
  for (int s = 0; s < 2 && ok; ++s) {
    u64 h[2] = {0, 0};
    ok = hipMalloc((void**)&list, std::max<u64>(distinct[s], 1) * 8) == hipSuccess && hipMalloc(&tab[s], slots[s] * deep_entry_bytes()) == hipSuccess &&
         hipMemsetAsync(tab[s], 0, slots[s] * deep_entry_bytes(), sb) == hipSuccess && hipMemsetAsync(d_cnt, 0, 16, sb) == hipSuccess;
    if (!ok) break;
    launch_deep_scan(st[s], ix->d_slen[s], n_stretch, K, d_cnt, list, distinct[s], sb);
    launch_deep_fill(st[s], st[1 - s], ix->wide, ix->d_slen[s], n_stretch, K, list, distinct[s], tab[s], slots[s], d_cnt + 1, sb);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h, d_cnt, 16, hipMemcpyDeviceToHost, sb) == hipSuccess &&
         hipStreamSynchronize(sb) == hipSuccess;
    if (ok && (h[0] != distinct[s] || h[1] != 0)) {
      if (verbose) fprintf(stderr, "[sigax] deep start table of strand %d: %llu K-mers listed of %llu, %llu walks astray: no table\n", s, h[0], distinct[s], h[1]);
      ok = false;
    }
    hipFree(list);
    list = nullptr;
    *bytes += slots[s] * deep_entry_bytes();
  }
  if (list) hipFree(list);
  if (d_cnt) hipFree(d_cnt);
  if (sb) (void)hipStreamDestroy(sb);
  if (!ok) {
    (void)hipGetLastError();
    for (int s = 0; s < 2; ++s) {
      if (tab[s]) hipFree(tab[s]);
      tab[s] = nullptr;
      slots[s] = 0;
    }
    *bytes = 0;
    return false;
  }
  if (verbose)
    fprintf(stderr, "[sigax] deep start tables: K = %u, %llu + %llu distinct K-mers, %.2f GB, %.3f s\n", K, distinct[0], distinct[1], *bytes / 1e9,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return true;
}
// (caller holds enqueue_mu) a finished background build becomes visible to the runs enqueued from now on
void publish_deep(sigax_index* ix) {
  if (!ix->deep_state || ix->deep_state->load(std::memory_order_acquire) != 2) return;
  if (ix->deep_thread) {
    ix->deep_thread->join();
    delete ix->deep_thread;
    ix->deep_thread = nullptr;
  }
  if (ix->deep_new[0] && ix->deep_new[1]) {
    for (int s = 0; s < 2; ++s) {
      ix->d_deep[s] = ix->deep_new[s];
      ix->deep_slots[s] = ix->deep_new_slots[s];
      ix->deep_new[s] = nullptr;
      ix->st[s].deep = ix->d_deep[s];
      ix->st[s].deep_slots = ix->deep_slots[s];
      ix->st[s].deep_k = ix->deep_new_k;
    }
    ix->deep_k = ix->deep_new_k;
    ix->deep_bytes = ix->deep_new_bytes;
    ix->device_bytes += ix->deep_bytes;
  }
  ix->deep_state->store(0, std::memory_order_release);
}
// (caller holds enqueue_mu) the index is being reused and this run's min-overlap has no table: build one beside the runs
void start_deep_tables(sigax_index* ix, uint32_t min_overlap) {
  if (ix->deep_tried || !ix->deep_state || ix->deep_state->load() != 0) return;
  if (ix->deep_k != 0 && ix->deep_k <= min_overlap) return;
  const uint32_t K = deep_k_for(min_overlap);
  if (K == 0 || !ix->st[0].sa || !ix->st[0].text || !ix->st[1].sa || !ix->st[1].text) return;
  ix->deep_tried = true;  // one background attempt per index; sigax_index_prepare_overlap may still replace the table
  if (ix->deep_k != 0) return;  // a table for a larger K is in use by runs in flight: only prepare_overlap swaps tables
  ix->deep_state->store(1);
  FmStrand snap[2] = {ix->st[0], ix->st[1]};
  ix->deep_new_k = K;
  ix->deep_thread = new std::thread([ix, snap, K] {
    (void)hipSetDevice(ix->device);
    (void)build_deep_tables(ix, snap, K, 25, ix->deep_new, ix->deep_new_slots, &ix->deep_new_bytes);
    ix->deep_state->store(2, std::memory_order_release);
  });
}

extern "C" int sigax_index_prepare(sigax_index* ix) {
  if (!ix) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(ix->device));
  std::lock_guard<std::mutex> lock(*ix->enqueue_mu);
  row_tables_now(ix);
  return SIGAX_OK;
}

extern "C" int sigax_index_prepare_overlap(sigax_index* ix, uint32_t min_overlap) {
  if (!ix) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(ix->device));
  std::lock_guard<std::mutex> lock(*ix->enqueue_mu);
  row_tables_now(ix);
  // a background build in flight: let it finish, then see whether its table serves
  if (ix->deep_thread) {
    ix->deep_thread->join();
    delete ix->deep_thread;
    ix->deep_thread = nullptr;
  }
  publish_deep(ix);
  const uint32_t K = deep_k_for(min_overlap);
  if (K == 0 || (ix->deep_k != 0 && ix->deep_k <= min_overlap)) return SIGAX_OK;
  if (ix->d_deep[0]) {
    // a table for a larger K: runs in flight may still read it
    HIP_TRY(hipDeviceSynchronize());
    for (int s = 0; s < 2; ++s) {
      hipFree(ix->d_deep[s]);
      ix->d_deep[s] = nullptr;
      ix->deep_slots[s] = 0;
      ix->st[s].deep = nullptr;
      ix->st[s].deep_slots = 0;
      ix->st[s].deep_k = 0;
    }
    ix->device_bytes -= ix->deep_bytes;
    ix->deep_bytes = 0;
    ix->deep_k = 0;
  }
  FmStrand snap[2] = {ix->st[0], ix->st[1]};
  ix->deep_new_k = K;
  (void)build_deep_tables(ix, snap, K, 45, ix->deep_new, ix->deep_new_slots, &ix->deep_new_bytes);
  ix->deep_state->store(2);
  publish_deep(ix);
  return SIGAX_OK;
}

