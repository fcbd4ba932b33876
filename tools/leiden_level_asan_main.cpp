// Stand-alone AddressSanitizer driver of the test entry scamd_leiden_debug_level_f32 (one level of a Leiden iteration: the
// refinement and the coarse graph) on the HOST emulation of the kernels (tests/emu).  Not part of the test suite; what the entry
// computes is checked by tests/leiden_level_cases.py.  Build and run (the emulator library from `python tests/emu/build.py --asan`):
//   clang++ -std=c++17 -g -fsanitize=address -shared-libasan -Iinclude tools/leiden_level_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -o leiden_level_asan && ./leiden_level_asan
// Every buffer is a heap block of the size include/scanpy_amd.h asks for (the workspace included: the emulator's ASan build also
// poisons the gaps between the buffers carved from it), so a read or write past any of them is reported.  The graph: a ring
// where every vertex has its eight nearest neighbours, and vertex 0 joined to everybody (a giant-tier row of the propose step,
// a coarse row beyond the wave builder); the runs: pairs as refined groups, whole communities as refined groups (the workgroup
// builders), the same with the split bounds lowered (parts and their merge), and the refinement itself at 64 and 16 lanes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

static Graph ring_with_hub(int n) {
  Graph g;
  g.n = n;
  g.indptr.push_back(0);
  for (int v = 0; v < n; ++v) {
    for (int u = 0; u < n; ++u) {
      const int d = (u - v + n) % n, ring = d == 0 ? 0 : (d <= 4 || d >= n - 4);
      if (u == v || !(ring || v == 0 || u == 0)) continue;
      const int a = u < v ? u : v, b = u < v ? v : u;
      g.indices.push_back(u);
      g.w.push_back(0.125f + (float)((a * 2654435761u + b * 40503u) % 97u) / 128.0f);  // symmetric, exact in the fixed point
    }
    g.indptr.push_back((int64_t)g.indices.size());
  }
  g.nnz = (int64_t)g.indices.size();
  return g;
}

static int run(const Graph& g, const std::vector<int32_t>& membership, const std::vector<int32_t>* refined_in, const char* what) {
  const size_t n = (size_t)g.n, e = (size_t)g.nnz;
  std::vector<int32_t> refined(n), refsize(n), cid(n), cix(e), ccomm(n);
  std::vector<uint64_t> kref(n), eref(n);
  std::vector<int64_t> cptr(n + 1), cwq(e), ck(n);
  int64_t info[8];
  const size_t ws_bytes = scamd_leiden_workspace_bytes(g.n, g.nnz);
  std::vector<char> ws(ws_bytes);
  CHECK(scamd_leiden_debug_level_f32(g.indptr.data(), g.indices.data(), g.w.data(), g.n, g.nnz, membership.data(),
                                     refined_in ? refined_in->data() : nullptr, 1.0, 0.01, 7, refined.data(), kref.data(), eref.data(),
                                     refsize.data(), cid.data(), cptr.data(), cix.data(), cwq.data(), ck.data(), ccomm.data(), info,
                                     ws.data(), ws_bytes, nullptr));
  printf("%s: %lld merges -> %lld coarse vertices, %lld entries; rows by builder: 512-thread %lld, 1024-thread %lld, split %lld\n", what,
         (long long)info[0], (long long)info[1], (long long)info[2], (long long)info[3], (long long)info[4], (long long)info[5]);
  return 0;
}

int main() {
  const int n = 2000, block = 250;
  const Graph g = ring_with_hub(n);
  std::vector<int32_t> membership(n), pairs(n), whole(n);
  for (int v = 0; v < n; ++v) {
    membership[v] = v / block * block + 3;  // a community is named by one of its members
    pairs[v] = v | 1;
    whole[v] = v / block * block;
  }
  if (run(g, membership, &pairs, "pairs")) return 1;
  if (run(g, membership, &whole, "whole communities")) return 1;
  setenv("SCAMD_LEIDEN_AGG_WAVE_WORK", "32", 1);
  setenv("SCAMD_LEIDEN_AGG_SPLIT_CHUNK", "64", 1);
  setenv("SCAMD_LEIDEN_AGG_SPLIT_WORK", "64", 1);
  if (run(g, membership, &whole, "whole communities, split rows")) return 1;
  if (run(g, membership, &pairs, "pairs, split rows")) return 1;
  unsetenv("SCAMD_LEIDEN_AGG_WAVE_WORK");
  unsetenv("SCAMD_LEIDEN_AGG_SPLIT_CHUNK");
  unsetenv("SCAMD_LEIDEN_AGG_SPLIT_WORK");
  setenv("SCAMD_LEIDEN_QUAD", "0", 1);
  if (run(g, membership, nullptr, "refinement, 64 lanes")) return 1;
  setenv("SCAMD_LEIDEN_QUAD", "1", 1);
  if (run(g, membership, nullptr, "refinement, 16 lanes")) return 1;
  puts("done");
  return 0;
}
