// Stand-alone AddressSanitizer driver of the Harmony entry points on the HOST emulation of the kernels (tests/emu):
// scamd_harmony_permutation_i32 -> _normalize -> _kmeans -> _init -> _cluster_round (twice) -> _correct, on two cases of the
// table of tests/harmony_cases.py: 157 cells in 2-d, 100 clusters, 11 batch levels of which level 4 has no cell, 19 blocks;
// and 12 cells, 7 clusters, 2 levels in 12 blocks of one cell.  The inputs are generated here (a small LCG), no file is read.
// Not part of the test suite.  Build and run (the emulator library from `python tests/emu/build.py --asan`):
//   RT=$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so))     (the sanitizer's shared runtime, found by rpath)
//   clang++ -std=c++17 -g -fsanitize=address -shared-libasan -Iinclude tools/harmony_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -Wl,-rpath,$RT -o harmony_asan && ./harmony_asan
// Every buffer is a heap block of its exact size (the workspaces included: the emulator's ASan build also poisons the gaps
// between the buffers carved from them), so a read or write past any of them is reported.
#include <cmath>
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

static uint64_t g_state = 0x853c49e6748fea9bull;
static double uniform() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

static int run_case(int64_t n, int d, int K, int B, int empty_level, int64_t n_blocks, int stabilized) {
  std::vector<double> x((size_t)n * d), z((size_t)n * d), n_b(B, 0.0), pr_b(B), theta(B, 2.0), u(K);
  std::vector<int32_t> codes(n), perm(n), labels(n);
  for (int64_t i = 0; i < n; ++i) {
    int b = (int)(uniform() * B);
    if (b == empty_level) b = (b + 1) % B;
    codes[i] = b;
    n_b[b] += 1.0;
    for (int j = 0; j < d; ++j) x[i * d + j] = 4.0 * ((i % 3) - 1) * (j % 2 ? 1 : -1) + uniform() - 0.5 + 0.3 * b;
  }
  for (int b = 0; b < B; ++b) pr_b[b] = n_b[b] / (double)n;
  for (int k = 0; k < K; ++k) u[k] = uniform();
  CHECK(scamd_harmony_permutation_i32(n, 42, 0, perm.data(), nullptr, 0, nullptr));
  CHECK(scamd_harmony_normalize_f64(x.data(), n, d, z.data(), nullptr));
  std::vector<double> cen((size_t)K * d), R((size_t)n * K), E((size_t)B * K), O((size_t)B * K), Y((size_t)K * d), obj(4);
  int sweeps = 0;
  {
    std::vector<char> ws(scamd_harmony_kmeans_workspace_bytes(n, d, K));
    CHECK(scamd_harmony_kmeans_f64(z.data(), n, d, K, u.data(), 25, cen.data(), labels.data(), &sweeps, ws.data(), ws.size(), nullptr));
  }
  {
    std::vector<char> ws(scamd_harmony_state_workspace_bytes(n, d, K, B));
    CHECK(scamd_harmony_init_f64(z.data(), codes.data(), n, d, K, B, 1, cen.data(), pr_b.data(), theta.data(), 0.1, stabilized, R.data(), E.data(),
                                 O.data(), obj.data(), ws.data(), ws.size(), nullptr));
    for (int rnd = 0; rnd < 2; ++rnd) {
      CHECK(scamd_harmony_permutation_i32(n, 42, (uint64_t)rnd, perm.data(), nullptr, 0, nullptr));
      CHECK(scamd_harmony_cluster_round_f64(z.data(), codes.data(), n, d, K, B, 1, perm.data(), n_blocks, pr_b.data(), theta.data(), 0.1, stabilized,
                                            R.data(), E.data(), O.data(), Y.data(), obj.data(), ws.data(), ws.size(), nullptr));
    }
  }
  std::vector<double> z_hat((size_t)n * d), z_norm((size_t)n * d), lam((size_t)B * K);
  {
    std::vector<char> ws(scamd_harmony_correct_workspace_bytes(n, d, K, B));
    CHECK(scamd_harmony_correct_f64(x.data(), codes.data(), n, d, K, B, 1, R.data(), O.data(), E.data(), n_b.data(), stabilized, 0.2, 1e-5, 1.0,
                                    z_hat.data(), z_norm.data(), lam.data(), ws.data(), ws.size(), nullptr));
  }
  double worst = 0.0;
  for (size_t p = 0; p < z_hat.size(); ++p) {
    if (!std::isfinite(z_hat[p])) {
      fprintf(stderr, "z_hat[%zu] is not finite\n", p);
      return 1;
    }
    worst = fmax(worst, fabs(z_hat[p] - x[p]));
  }
  printf("n=%lld d=%d K=%d levels=%d blocks=%lld: %d k-means sweeps, objective %.6f, largest correction %.4f\n", (long long)n, d, K, B,
         (long long)n_blocks, sweeps, obj[0], worst);
  return 0;
}

int main() {
  if (run_case(157, 2, 100, 11, 4, 19, 1)) return 1;
  if (run_case(12, 2, 7, 2, -1, 12, 0)) return 1;
  printf("harmony_asan: clean\n");
  return 0;
}
