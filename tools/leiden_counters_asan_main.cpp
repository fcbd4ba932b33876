// Stand-alone AddressSanitizer driver of the test entry scamd_leiden_debug_counters_f32 (the community totals, the class and tier
// lists of one local-moving sweep and its apply steps: the kernels bounded by SCAMD_LEIDEN_COUNT_GRID) on the HOST emulation of the
// kernels (tests/emu).  Not part of the test suite; what the entry computes is checked by tests/leiden_counter_cases.py.  Build
// and run (the emulator library from `python tests/emu/build.py --asan`):
//   clang++ -std=c++17 -g -fsanitize=address,undefined -shared-libasan -Iinclude tools/leiden_counters_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -o leiden_counters_asan && ./leiden_counters_asan
// (where the loader does not find the sanitizer's runtime: LD_LIBRARY_PATH=$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so)))
// Every buffer is a heap block of the size include/scanpy_amd.h asks for (the workspace included: the emulator's ASan build also
// poisons the gaps between the buffers carved from it), so a read or write past any of them is reported.  The graph: a ring of
// 4097 vertices (four full 1024-vertex chunks and one vertex) where nine vertices have rows of 97, 385 and 1537 entries -- the
// first rows of the wave, block and giant tier at 16 lanes per vertex -- in the first, second and last chunk; the runs: 64
// communities, singletons and 2049 interleaved communities (more keys than a workgroup's table holds), every vertex listed or
// every other one, with one, two and the default number of workgroups per counter word.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "scanpy_amd.h"

#define CHECK(call)                                                        \
  do {                                                                     \
    const int rc_ = (call);                                                \
    if (rc_ != SCAMD_OK) {                                                 \
      fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, scamd_last_error()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

struct Graph {
  int64_t n, nnz;
  std::vector<int64_t> indptr;
  std::vector<int32_t> indices;
  std::vector<float> w;
};

static Graph ring_with_long_rows(int n) {
  std::vector<std::set<int>> adj((size_t)n);
  for (int v = 0; v < n; ++v) {
    adj[v].insert((v + 1) % n);
    adj[(v + 1) % n].insert(v);
  }
  const int lengths[3] = {97, 385, 1537}, at[3] = {5, 1500, n - 40};
  std::set<int> hubs;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) hubs.insert(at[j] + 3 * i);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int h = at[j] + 3 * i;
      for (int u = 100 + j; (int)adj[h].size() < lengths[i]; u += 2) {  // (ordinary vertices only, so that a hub's row keeps its length)
        if (hubs.count(u) || adj[h].count(u)) continue;
        adj[h].insert(u);
        adj[u].insert(h);
      }
    }
  Graph g;
  g.n = n;
  g.indptr.push_back(0);
  for (int v = 0; v < n; ++v) {
    for (int u : adj[v]) {
      const unsigned a = (unsigned)(u < v ? u : v), b = (unsigned)(u < v ? v : u);
      g.indices.push_back(u);
      g.w.push_back(0.125f + (float)((a * 2654435761u + b * 40503u) % 97u) / 128.0f);  // symmetric, exact in the fixed point
    }
    g.indptr.push_back((int64_t)g.indices.size());
  }
  g.nnz = (int64_t)g.indices.size();
  return g;
}

static int run(const Graph& g, const std::vector<int32_t>& membership, bool every_other, int n_cls, const char* what) {
  const size_t n = (size_t)g.n;
  int block_max = 0;
  CHECK(scamd_leiden_tier_bounds(64, nullptr, nullptr, &block_max));
  const size_t stride = (size_t)(g.nnz / (block_max + 1) + 1);
  std::vector<int32_t> flags(n), decision(n), lists(n * n_cls), tiers(n * n_cls), giant(stride * n_cls), csize0(n), comm1(n), csize1(n), flags1(n);
  std::vector<uint64_t> k0(n), k1(n);
  int64_t want_moved = 0, want_blocked = 0, want_listed = 0;
  for (size_t v = 0; v < n; ++v) {
    flags[v] = every_other ? (int)(v & 1) : 1;
    decision[v] = v % 5 == 0 ? membership[(v * 7 + 1) % n] : (v % 5 == 1 ? -2 : -1);
    if (flags[v]) {
      ++want_listed;
      want_moved += decision[v] >= 0;
      want_blocked += decision[v] == -2;
    }
  }
  int32_t counts[32 + 16 * 32];
  int64_t info[4];
  const size_t ws_bytes = scamd_leiden_workspace_bytes(g.n, g.nnz);
  std::vector<char> ws(ws_bytes);
  CHECK(scamd_leiden_debug_counters_f32(g.indptr.data(), g.indices.data(), g.w.data(), g.n, g.nnz, membership.data(),
                                        every_other ? flags.data() : nullptr, n_cls, 0x51ed27u, decision.data(), lists.data(), tiers.data(),
                                        giant.data(), k0.data(), csize0.data(), comm1.data(), k1.data(), csize1.data(), flags1.data(), counts,
                                        info, ws.data(), ws_bytes, nullptr));
  int64_t listed = 0, long_rows[3] = {0, 0, 0};
  for (int c = 0; c < n_cls; ++c) {
    listed += counts[c];
    for (int t = 0; t < 3; ++t) long_rows[t] += counts[32 + 16 * c + 8 + t];
  }
  printf("%s: listed %lld, long rows %lld / %lld / %lld, moved %lld, blocked %lld\n", what, (long long)listed, (long long)long_rows[0],
         (long long)long_rows[1], (long long)long_rows[2], (long long)info[0], (long long)info[1]);
  if (listed != want_listed || info[0] != want_moved || info[1] != want_blocked) {
    fprintf(stderr, "%s: expected listed %lld, moved %lld, blocked %lld\n", what, (long long)want_listed, (long long)want_moved, (long long)want_blocked);
    return 1;
  }
  return 0;
}

int main() {
  const int n = 4097;
  const Graph g = ring_with_long_rows(n);
  std::vector<int32_t> sixty_four(n), singletons(n), interleaved(n);
  for (int v = 0; v < n; ++v) {
    sixty_four[v] = (int)(((unsigned)v * 2654435761u >> 8) % 64u) * 61 + 7;
    singletons[v] = n - 1 - v;
    interleaved[v] = v % 2049;
  }
  const char* grids[3] = {"1", "2", nullptr};
  for (const char* grid : grids) {
    if (grid) setenv("SCAMD_LEIDEN_COUNT_GRID", grid, 1);
    else unsetenv("SCAMD_LEIDEN_COUNT_GRID");
    printf("SCAMD_LEIDEN_COUNT_GRID=%s\n", grid ? grid : "(default)");
    if (run(g, sixty_four, false, 8, "64 communities, every vertex")) return 1;
    if (run(g, sixty_four, true, 8, "64 communities, every other vertex")) return 1;
    if (run(g, singletons, false, 4, "singletons, every vertex")) return 1;
    if (run(g, interleaved, true, 1, "2049 interleaved communities, every other vertex, one class")) return 1;
  }
  puts("done");
  return 0;
}
