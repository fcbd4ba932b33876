// Stand-alone AddressSanitizer driver of the three diffusion-map entry points on the HOST emulation of the kernels
// (tests/emu): scamd_transitions_sym_f32 -> scamd_diffmap_f32 -> scamd_dpt_pseudotime_f32 on a graph read from a file.
// Not part of the test suite.  Build and run (the emulator library from `python tests/emu/build.py --asan`):
//   python -c "import sys; sys.path.insert(0, 'tests'); import diffmap_cases as D; g = D.graph_input('two_blobs'); a = g['a']; \
//     import numpy as np; f = open('graph.bin', 'wb'); np.array([a.shape[0], a.nnz], np.int64).tofile(f); \
//     a.indptr.astype(np.int64).tofile(f); a.indices.astype(np.int32).tofile(f); a.data.astype(np.float32).tofile(f); \
//     g['labels'].astype(np.int32).tofile(f)"
//   clang++ -std=c++17 -g -fsanitize=address -shared-libasan -Iinclude tools/diffmap_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -o diffmap_asan && ./diffmap_asan graph.bin
// Every buffer is a heap block of its exact size (the workspaces included: the emulator's ASan build also poisons the gaps
// between the buffers carved from them), so a read or write past any of them is reported.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scanpy_amd.h"

template <class T>
static std::vector<T> read_vec(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}
#define CHECK(call)                                                        \
  do {                                                                     \
    const int rc_ = (call);                                                \
    if (rc_ != SCAMD_OK) {                                                 \
      fprintf(stderr, "%s: rc=%d: %s\n", #call, rc_, scamd_last_error()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto head = read_vec<int64_t>(f, 2);
  const int64_t n = head[0], nnz = head[1];
  const auto indptr = read_vec<int64_t>(f, n + 1);
  const auto indices = read_vec<int32_t>(f, nnz);
  const auto weights = read_vec<float>(f, nnz);
  const auto labels = read_vec<int32_t>(f, n);
  fclose(f);
  for (int dn = 1; dn >= 0; --dn) {
    std::vector<float> t(nnz);
    std::vector<double> z(n);
    std::vector<char> ws(scamd_transitions_sym_workspace_bytes(n, nnz));
    CHECK(scamd_transitions_sym_f32(indptr.data(), indices.data(), weights.data(), n, nnz, dn, t.data(), z.data(), ws.data(), ws.size(), nullptr));
    for (const int k : {15, 26}) {  // the wide instantiation of the panel kernels and its upper edge
      std::vector<double> evals(k), evecs((size_t)n * k), info(8);
      std::vector<char> ws2(scamd_diffmap_workspace_bytes(n, nnz, k));
      CHECK(scamd_diffmap_f32(indptr.data(), indices.data(), t.data(), n, nnz, k, 0, 2e-6, 60, 64, evals.data(), evecs.data(), info.data(),
                              ws2.data(), ws2.size(), nullptr));
      std::vector<float> e32(evals.begin(), evals.end()), b32(evecs.begin(), evecs.end()), pt(n);
      std::vector<char> ws3(scamd_dpt_pseudotime_workspace_bytes(n));
      CHECK(scamd_dpt_pseudotime_f32(e32.data(), b32.data(), n, k, k, n / 2 - 100, labels.data(), 0, pt.data(), ws3.data(), ws3.size(), nullptr));
      CHECK(scamd_dpt_pseudotime_f32(e32.data(), b32.data(), n, k, k, n / 2 - 100, labels.data(), 1, pt.data(), ws3.data(), ws3.size(), nullptr));
      int n_inf = 0;
      float mx = 0.f;
      for (float v : pt) {
        if (std::isinf(v)) ++n_inf;
        else mx = std::fmax(mx, v);
      }
      printf("density_normalize=%d k=%d: outer %g, applications %g, residual %.2e, lambda_min %.4f; pseudotime max %g, %d inf\n", dn, k,
             info[0], info[1], info[2], info[4], mx, n_inf);
      fflush(stdout);
    }
  }
  return 0;
}
