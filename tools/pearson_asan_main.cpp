// Stand-alone AddressSanitizer driver of the Pearson-residual entry points on the HOST emulation of the kernels (tests/emu):
// scamd_pp_pearson_gene_var_f32 and scamd_pp_pearson_residuals_f32 on the smallest cases that reach every buffer: (1) 11 cells over
// 2049 genes, float32 out: three column slices, two batches of rows of the residual kernel, rows of 0, 1 and 2049 entries,
// all totals distinct; (2) 4200 cells over 5 genes of which gene 0 is stored in every cell (two chunks of one gene), two
// interleaved batches with their own distinct totals, float64 out; (3) 300 cells with 257 distinct totals (the tail of the sweep);
// (4) n == 0 and g == 0.  The inputs are generated here (a small LCG), no file is read; variance and residuals are compared with
// plain loops on the host.  Not part of the test suite.  Build and run (the emulator library from
// `python tests/emu/build.py --asan`):
//   RT=$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so))     (the sanitizer's shared runtime, found by rpath)
//   clang++ -std=c++17 -g -fsanitize=address,undefined -shared-libasan -Iinclude tools/pearson_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -Wl,-rpath,$RT -o pearson_asan && ./pearson_asan
// Every buffer is a heap block of its exact size, so a read or write past any of them is reported.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
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
static uint32_t next_u32() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33);
}

static double resid(double x, double mu, double inv_theta, double clip) {
  const double r = (x - mu) / std::sqrt(mu + mu * mu * inv_theta);
  return r < -clip ? -clip : (r > clip ? clip : r);
}

// dense: n x g counts (row-major); n_batches interleaved batches (1: no codes).  Runs both entry points and compares.
static int run_case(const char* what, const std::vector<double>& dense, int64_t n, int64_t g, int n_batches, double inv_theta,
                    double clip, int out_is_f64) {
  std::vector<int64_t> indptr(n + 1, 0), t_indptr(g + 1, 0);
  std::vector<int32_t> indices, t_rows;
  std::vector<float> data, t_data;
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = 0; j < g; ++j)
      if (dense[i * g + j] != 0.0) indices.push_back((int32_t)j), data.push_back((float)dense[i * g + j]);
    indptr[i + 1] = (int64_t)indices.size();
  }
  for (int64_t j = 0; j < g; ++j) {
    for (int64_t i = 0; i < n; ++i)
      if (dense[i * g + j] != 0.0) t_rows.push_back((int32_t)i), t_data.push_back((float)dense[i * g + j]);
    t_indptr[j + 1] = (int64_t)t_rows.size();
  }
  const int64_t nnz = (int64_t)data.size();
  std::vector<double> cell_total(n, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < g; ++j) cell_total[i] += dense[i * g + j];
  std::vector<int32_t> codes(n);
  for (int64_t i = 0; i < n; ++i) codes[i] = (int32_t)(i % n_batches);
  const size_t ws_bytes = scamd_pp_pearson_workspace_bytes(g, nnz);
  std::vector<char> ws(std::max<size_t>(ws_bytes, 1), (char)0xAB);
  double worst = 0.0;
  for (int b = 0; b < n_batches; ++b) {
    std::vector<double> gene_sum(g, 0.0);
    std::map<double, double> distinct;
    int64_t n_batch = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (codes[i] != b) continue;
      ++n_batch, distinct[cell_total[i]] += 1.0;
      for (int64_t j = 0; j < g; ++j) gene_sum[j] += dense[i * g + j];
    }
    double total = 0.0;
    for (double s : gene_sum) total += s;
    std::vector<double> tot_u, mult_u;
    for (const auto& kv : distinct) tot_u.push_back(kv.first), mult_u.push_back(kv.second);
    std::vector<double> var(g, -1.0);
    CHECK(scamd_pp_pearson_gene_var_f32(t_indptr.data(), t_rows.data(), t_data.data(), n, g, nnz, gene_sum.data(), cell_total.data(),
                                        total, inv_theta, clip, tot_u.data(), mult_u.data(), (int64_t)tot_u.size(), n_batch,
                                        n_batches > 1 ? codes.data() : nullptr, b, var.data(), ws.data(), ws_bytes, nullptr));
    for (int64_t j = 0; j < g; ++j) {
      double want = 0.0;
      if (gene_sum[j] != 0.0) {
        double mean = 0.0, m2 = 0.0;
        for (int64_t i = 0; i < n; ++i)
          if (codes[i] == b) mean += resid(dense[i * g + j], gene_sum[j] / total * cell_total[i], inv_theta, clip);
        mean /= (double)n_batch;
        for (int64_t i = 0; i < n; ++i)
          if (codes[i] == b) {
            const double d = resid(dense[i * g + j], gene_sum[j] / total * cell_total[i], inv_theta, clip) - mean;
            m2 += d * d;
          }
        want = m2 / (double)n_batch;
      }
      if (std::isnan(want) != std::isnan(var[j])) {
        fprintf(stderr, "%s: batch %d gene %lld: NaN pattern (%g, %g)\n", what, b, (long long)j, var[j], want);
        return 1;
      }
      if (!std::isnan(want)) worst = std::max(worst, std::fabs(var[j] - want) / std::max(std::fabs(want), 1e-300));
    }
  }
  if (worst > 1e-9) {
    fprintf(stderr, "%s: variance off by %g relative\n", what, worst);
    return 1;
  }
  // the residual matrix of all cells
  std::vector<double> gene_sum(g, 0.0);
  double total = 0.0;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < g; ++j) gene_sum[j] += dense[i * g + j], total += dense[i * g + j];
  const size_t item = out_is_f64 ? 8 : 4;
  std::vector<char> out((size_t)n * g * item, (char)0x7f);
  CHECK(scamd_pp_pearson_residuals_f32(indptr.data(), indices.data(), data.data(), n, g, nnz, gene_sum.data(), cell_total.data(), total,
                                       inv_theta, clip, out.data(), out_is_f64, nullptr));
  double worst_r = 0.0;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < g; ++j) {
      const double want = resid(dense[i * g + j], gene_sum[j] / total * cell_total[i], inv_theta, clip);
      const double got = out_is_f64 ? reinterpret_cast<const double*>(out.data())[i * g + j]
                                    : (double)reinterpret_cast<const float*>(out.data())[i * g + j];
      if (std::isnan(want) != std::isnan(got)) {
        fprintf(stderr, "%s: residual (%lld, %lld): NaN pattern (%g, %g)\n", what, (long long)i, (long long)j, got, want);
        return 1;
      }
      if (!std::isnan(want)) worst_r = std::max(worst_r, std::fabs(got - want) / std::max(std::fabs(want), 1.0));
    }
  if (worst_r > (out_is_f64 ? 1e-13 : 1e-6)) {
    fprintf(stderr, "%s: residual off by %g\n", what, worst_r);
    return 1;
  }
  printf("%s: ok (variance %.2e, residual %.2e)\n", what, worst, worst_r);
  return 0;
}

int main() {
  {  // (1) three slices, rows of 0, 1 and g entries
    const int64_t n = 11, g = 2049;
    std::vector<double> d((size_t)n * g, 0.0);
    for (int64_t i = 3; i < n; ++i)
      for (int k = 0; k < 40 + 3 * (int)i; ++k) d[i * g + next_u32() % g] = 1.0 + next_u32() % 5;
    d[1 * g + g - 1] = 4.0;
    for (int64_t j = 0; j < g; ++j) d[2 * g + j] = 1.0 + next_u32() % 3;
    if (run_case("wide", d, n, g, 1, 0.01, std::sqrt((double)n), 0)) return 1;
  }
  {  // (2) one gene in two chunks, two batches
    const int64_t n = 4200, g = 5;
    std::vector<double> d((size_t)n * g, 0.0);
    for (int64_t i = 0; i < n; ++i) {
      d[i * g] = 1.0 + next_u32() % 20;
      if (next_u32() % 7 == 0) d[i * g + 1 + next_u32() % 4] = 1.0 + next_u32() % 3;
    }
    if (run_case("chunks", d, n, g, 2, 0.0, 3.0, 1)) return 1;
  }
  {  // (3) 257 distinct totals
    const int64_t n = 300, g = 4;
    std::vector<double> d((size_t)n * g, 0.0);
    for (int64_t i = 0; i < n; ++i) d[i * g] = 1.0 + (double)(i % 257), d[i * g + 1 + i % 3] = 1.0;
    if (run_case("totals", d, n, g, 1, 1000.0, INFINITY, 1)) return 1;
  }
  {  // (4) nothing to do
    int64_t ip[1] = {0};
    CHECK(scamd_pp_pearson_residuals_f32(ip, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 1.0, 0.01, 3.0, nullptr, 1, nullptr));
    std::vector<char> ws(std::max<size_t>(scamd_pp_pearson_workspace_bytes(0, 0), 1));
    CHECK(scamd_pp_pearson_gene_var_f32(ip, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 1.0, 0.01, 3.0, nullptr, nullptr, 0, 0, nullptr, 0,
                                        nullptr, ws.data(), ws.size(), nullptr));
    printf("empty: ok\n");
  }
  return 0;
}
