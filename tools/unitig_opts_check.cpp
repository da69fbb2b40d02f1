// tools/unitig_opts_check.cpp -- a stand-alone host check of sigax_unitig.cpp: the workspace layout of every level of the rounds calls
// (rounds_work) against the formula include/sigax.h states for the indel call, and the indel call's option checks with their error
// texts.  Meant to be built with the library's sources under the host sanitizers and run on a machine without a GPU: every call here
// returns before it touches a device.  From siga_amd/csrc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined -I../../include \
//         -o unitig_opts_check ../../tools/unitig_opts_check.cpp <the SOURCES of siga_amd/build.py> -fsanitize=address,undefined
// The log of one such run is profiles/indel_host_sanitizer.txt.
#include <cstdio>
#include <cstring>
#include "sigax.h"
int main() {
  unsigned long long checked = 0;
  for (uint64_t n : {0ull, 1ull, 7ull, 4096ull, 1000000ull, (1ull << 31) - 1})
    for (uint64_t ne : {0ull, 5ull, 1ull << 20, 1ull << 32})
      for (int graph = 0; graph < 2; ++graph)
        for (int careful = 0; careful < 2; ++careful) {
          uint64_t b[6] = {0};
          int rc = sigax_unitigs_workspace(n, ne, &b[0]);
          rc |= sigax_unitigs_trim_workspace(n, ne, graph, &b[1]);
          rc |= sigax_unitigs_prune_workspace(n, ne, graph, careful, &b[2]);
          rc |= sigax_unitigs_chimeric_workspace(n, ne, graph, careful, &b[3]);
          rc |= sigax_unitigs_bubble_workspace(n, ne, graph, careful, &b[4]);
          rc |= sigax_unitigs_indel_workspace(n, ne, graph, careful, &b[5]);
          if (rc != SIGAX_OK) { printf("workspace refused n=%llu ne=%llu\n", (unsigned long long)n, (unsigned long long)ne); return 1; }
          for (int k = 1; k < 6; ++k) if (b[k] <= b[k - 1]) { printf("level %d not above level %d\n", k, k - 1); return 1; }
          const uint64_t want = b[4] + 33408 + ((n * 4 + 15) & ~15ull);
          if (b[5] != want) { printf("indel workspace %llu, formula %llu\n", (unsigned long long)b[5], (unsigned long long)want); return 1; }
          ++checked;
        }
  uint64_t bytes;
  if (sigax_unitigs_indel_workspace(1ull << 31, 0, 0, 0, &bytes) == SIGAX_OK || sigax_unitigs_indel_workspace(1, (1ull << 32) + 1, 0, 0, &bytes) == SIGAX_OK ||
      sigax_unitigs_indel_workspace(1, 1, 0, 0, nullptr) == SIGAX_OK) { printf("a limit was not refused\n"); return 1; }
  sigax_indel_opts o;
  memset(&o, 0, sizeof o);
  o.bubble.chimeric.prune.max_rounds = 10;
  o.bubble.chimeric.prune.num_reads = 4;
  o.bubble.max_bubble_span = 40;
  o.max_edits = 2;
  struct { const char* what; sigax_indel_opts v; const char* word; } bad[7];
  for (auto& x : bad) x.v = o;
  bad[0] = {"reserved4[0]", o, "reserved4"}; bad[0].v.reserved4[0] = 1;
  bad[1] = {"reserved4[1]", o, "reserved4"}; bad[1].v.reserved4[1] = 1;
  bad[2] = {"max_edits 32", o, "max_edits"}; bad[2].v.max_edits = 32;
  bad[3] = {"span 0", o, "max_bubble_span"}; bad[3].v.bubble.max_bubble_span = 0;
  bad[4] = {"span 4097", o, "max_bubble_span"}; bad[4].v.bubble.max_bubble_span = 4097;
  bad[5] = {"reserved3", o, "reserved3"}; bad[5].v.bubble.reserved3[1] = 1;
  bad[6] = {"max_rounds 65", o, "max_rounds"}; bad[6].v.bubble.chimeric.prune.max_rounds = 65;
  for (auto& x : bad) {
    const int rc = sigax_unitigs_indel_device(0, nullptr, 0, nullptr, nullptr, nullptr, 0, 20, &x.v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, nullptr, nullptr, 0, nullptr);
    if (rc != SIGAX_E_ARG || !strstr(sigax_last_error(), x.word)) { printf("%s: rc %d, '%s'\n", x.what, rc, sigax_last_error()); return 1; }
    uint64_t nu, st[32]; uint64_t *so, *lo; uint32_t *uf, *rm, *ct; sigax_placement* lay;
    const int rh = sigax_unitigs_indel_host(0, nullptr, 0, nullptr, nullptr, nullptr, 0, 20, &x.v, &nu, &so, &lo, &uf, &lay, nullptr, &rm, &ct, nullptr, st);
    if (rh != SIGAX_E_ARG) { printf("%s: host form rc %d\n", x.what, rh); return 1; }
    ++checked;
  }
  if (sigax_unitigs_indel_device(0, nullptr, 0, nullptr, nullptr, nullptr, 0, 20, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, 0, nullptr) != SIGAX_E_ARG) { printf("NULL options accepted\n"); return 1; }
  // a call with reads and NULL buffers, and one with a workspace one byte short: refused by bufs_ok, before any device call
  char dummy[64] __attribute__((aligned(16)));
  sigax_unitigs_indel_workspace(4, 2, 1, 0, &bytes);
  int rc = sigax_unitigs_indel_device(0, (const sigax_edge*)dummy, 2, dummy, dummy, dummy, 4, 20, &o, dummy, dummy, dummy, (sigax_placement*)dummy, dummy, dummy, dummy,
                                      (sigax_edge*)dummy, dummy, dummy, bytes - 1, nullptr);
  if (rc != SIGAX_E_ARG || !strstr(sigax_last_error(), "sigax_unitigs_indel_workspace")) { printf("short workspace: rc %d '%s'\n", rc, sigax_last_error()); return 1; }
  printf("ok: %llu checks, no sanitizer report\n", checked);
  return 0;
}
