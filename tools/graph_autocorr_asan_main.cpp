// Stand-alone AddressSanitizer driver of the graph-autocorrelation entry points on the HOST emulation of the kernels (tests/emu):
// scamd_graph_autocorr_slab_{f32,f64}, scamd_graph_weight_sum_f64, scamd_csr_dense_slab_f32 and scamd_transpose_slab_{f32,f64} on
// (1) a hub graph: 3000 cells, one row of 2500 entries and one other column of 2500, the other rows 0-9 entries (every seventh
// empty), 3 float32 columns read in place at ld = 3: a row shared by many parts, parts that start in empty rows; (2) widths:
// ncols in {1, 63, 64} with n in {2, 63, 65, 1000}, float32 and float64 values and weights, ld = ncols + 2 (the pad is never
// read: it lies inside the block, so the comparison shows a read of it), the last row's slab ending exactly at the end of its
// heap block for ld = ncols; (3) a messy graph: unsorted columns, duplicates, explicit zeros, self-loops, negative weights, an
// entry count that is no multiple of the unroll; (4) the builders: 65 genes of a CSR as two slabs, 5 feature-major rows of 130
// cells; (5) the empty graph.  The inputs are generated here (a small LCG), no file is read; every sum is compared with plain
// loops on the host.  Not part of the test suite.  Build and run (the emulator library from `python tests/emu/build.py --asan`):
//   RT=$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so))     (the sanitizer's shared runtime, found by rpath)
//   clang++ -std=c++17 -g -fsanitize=address -shared-libasan -Iinclude tools/graph_autocorr_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -Wl,-rpath,$RT -o graph_autocorr_asan && ./graph_autocorr_asan
// Every buffer is a heap block of its exact size, so a read or write past any of them is reported.
#include <algorithm>
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
static uint32_t next_u32() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33);
}
static double next_unit() { return (next_u32() % 2000001u) / 1e6 - 1.0; }  // [-1, 1]

struct Graph {
  int64_t n;
  std::vector<int64_t> indptr;
  std::vector<int32_t> indices;
  std::vector<double> w;
};

// kind 0: random rows of 0 .. 9 entries, every seventh row empty; 1: the same with a hub row 5 and a hub column 9; 2: messy
static Graph make_graph(int64_t n, int kind, int hub_len) {
  Graph g;
  g.n = n;
  g.indptr.assign(n + 1, 0);
  for (int64_t r = 0; r < n; ++r) {
    int len = (r % 7 == 3 && n > 2) ? 0 : (int)(next_u32() % 10u);
    if (kind == 1 && r == 5) len = hub_len;
    len = (int)std::min<int64_t>(len, n);
    std::vector<int32_t> cols;
    const int32_t start = (int32_t)(next_u32() % (uint32_t)n);
    for (int j = 0; j < len; ++j) cols.push_back((int32_t)(((int64_t)start + (int64_t)j * std::max<int64_t>(n / std::max(len, 1), 1)) % n));
    if (kind == 1 && r != 5 && r % 7 != 3 && r < hub_len + 50) cols.push_back(9);
    if (kind == 2 && len) {
      cols.push_back(cols[0]);       // a duplicate
      cols.push_back((int32_t)r);    // a self-loop
      std::reverse(cols.begin(), cols.end());
    }
    for (int32_t c : cols) {
      g.indices.push_back(c);
      double w = 0.05 + 0.95 * std::fabs(next_unit());
      if (kind == 2 && g.indices.size() % 4 == 0) w = 0.0;
      if (kind == 2 && g.indices.size() % 5 == 1) w = -w;
      g.w.push_back(w);
    }
    g.indptr[r + 1] = (int64_t)g.indices.size();
  }
  return g;
}

template <typename VT, typename WT>
static int run_case(const char* what, const Graph& g, int ncols, int pad) {
  const int64_t n = g.n, nnz = (int64_t)g.indices.size();
  const int64_t ld = ncols + pad;
  std::vector<VT> slab((size_t)(n * ld - pad));  // the last row ends with its last value: nothing beyond it may be read
  for (int64_t r = 0; r < n; ++r)
    for (int64_t l = 0; l < ld && r * ld + l < (int64_t)slab.size(); ++l) slab[r * ld + l] = l < ncols ? (VT)(next_unit() * 8.0 + 3.0) : (VT)1e30;
  std::vector<WT> w(nnz);
  for (int64_t e = 0; e < nnz; ++e) w[e] = (WT)g.w[e];
  std::vector<double> mean(ncols, -7.0), z2(ncols, -7.0), mor(ncols, -7.0), gea(ncols, -7.0), lo(ncols, -7.0), hi(ncols, -7.0);
  const size_t ws_bytes = scamd_graph_autocorr_workspace_bytes(n, nnz);
  std::vector<unsigned char> ws(ws_bytes, 0xAB);
  double w_sum = -7.0;
  CHECK(scamd_graph_weight_sum_f64(w.data(), sizeof(WT) == 8, nnz, &w_sum, ws.data(), ws_bytes, nullptr));
  if (sizeof(VT) == 8)
    CHECK(scamd_graph_autocorr_slab_f64(g.indptr.data(), g.indices.data(), w.data(), sizeof(WT) == 8, n, nnz, (const double*)slab.data(), ld,
                                        ncols, mean.data(), z2.data(), mor.data(), gea.data(), lo.data(), hi.data(), ws.data(), ws_bytes,
                                        nullptr));
  else
    CHECK(scamd_graph_autocorr_slab_f32(g.indptr.data(), g.indices.data(), w.data(), sizeof(WT) == 8, n, nnz, (const float*)slab.data(), ld,
                                        ncols, mean.data(), z2.data(), mor.data(), gea.data(), lo.data(), hi.data(), ws.data(), ws_bytes,
                                        nullptr));
  double want_w = 0.0;
  for (int64_t e = 0; e < nnz; ++e) want_w += (double)w[e];
  if (!(std::fabs(w_sum - want_w) <= 1e-12 * (1.0 + std::fabs(want_w)))) {
    fprintf(stderr, "%s: W_sum = %.17g, expected %.17g\n", what, w_sum, want_w);
    return 1;
  }
  for (int l = 0; l < ncols; ++l) {
    double s = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t r = 0; r < n; ++r) {
      const double x = (double)slab[r * ld + l];
      s += x;
      mn = std::min(mn, x);
      mx = std::max(mx, x);
    }
    const double mu = s / (double)n;
    double q = 0.0, m = 0.0, c = 0.0, scale = 0.0;
    for (int64_t r = 0; r < n; ++r) q += ((double)slab[r * ld + l] - mu) * ((double)slab[r * ld + l] - mu);
    for (int64_t r = 0; r < n; ++r)
      for (int64_t e = g.indptr[r]; e < g.indptr[r + 1]; ++e) {
        const double xi = (double)slab[r * ld + l], xj = (double)slab[(int64_t)g.indices[e] * ld + l];
        m += (double)w[e] * (xi - mu) * (xj - mu);
        c += (double)w[e] * (xi - xj) * (xi - xj);
        scale += std::fabs((double)w[e]) * 400.0;
      }
    const double tol = 1e-11 * (1.0 + scale);
    if (lo[l] != mn || hi[l] != mx || !(std::fabs(mean[l] - mu) <= 1e-12 * (1.0 + std::fabs(mu))) || !(std::fabs(z2[l] - q) <= 1e-10 * (1.0 + q)) ||
        !(std::fabs(mor[l] - m) <= tol) || !(std::fabs(gea[l] - c) <= tol)) {
      fprintf(stderr, "%s: column %d: mean %.17g / %.17g, z2 %.17g / %.17g, moran %.17g / %.17g, geary %.17g / %.17g, range [%g, %g] / [%g, %g]\n",
              what, l, mean[l], mu, z2[l], q, mor[l], m, gea[l], c, lo[l], hi[l], mn, mx);
      return 1;
    }
  }
  printf("%s: ok (n %lld, nnz %lld, ncols %d, ld %lld, %d entries per part)\n", what, (long long)n, (long long)nnz, ncols, (long long)ld,
         scamd_graph_autocorr_part_entries(nnz));
  return 0;
}

static int run_builders() {
  const int64_t n = 130;
  const int g = 65;
  std::vector<int64_t> indptr(n + 1, 0);
  std::vector<int32_t> indices;
  std::vector<float> data, dense((size_t)n * g, 0.f);
  for (int64_t r = 0; r < n; ++r) {
    for (int c = 0; c < g; ++c)
      if (r % 9 != 4 && (next_u32() % 3u == 0 || r == 1)) {  // row 1 is full, every ninth row empty
        indices.push_back(c);
        data.push_back((float)next_unit());
        dense[(size_t)r * g + c] = data.back();
      }
    indptr[r + 1] = (int64_t)indices.size();
  }
  for (int c0 = 0; c0 < g; c0 += 64) {
    const int b = std::min(64, g - c0);
    std::vector<float> slab((size_t)n * b, -9.f);  // ld = ncols: the block ends with the last value
    CHECK(scamd_csr_dense_slab_f32(indptr.data(), indices.data(), data.data(), n, g, (int64_t)indices.size(), c0, b, slab.data(), b, nullptr));
    for (int64_t r = 0; r < n; ++r)
      for (int l = 0; l < b; ++l)
        if (slab[(size_t)r * b + l] != dense[(size_t)r * g + c0 + l]) {
          fprintf(stderr, "csr slab at %d: [%lld, %d] = %g, expected %g\n", c0, (long long)r, l, slab[(size_t)r * b + l], dense[(size_t)r * g + c0 + l]);
          return 1;
        }
  }
  std::vector<float> rows32(5 * n);
  std::vector<double> rows64(5 * n);
  for (size_t i = 0; i < rows32.size(); ++i) rows64[i] = rows32[i] = (float)next_unit();
  std::vector<float> t32((size_t)n * 5, -9.f);
  std::vector<double> t64((size_t)n * 5, -9.0);
  CHECK(scamd_transpose_slab_f32(rows32.data(), n, n, 5, t32.data(), 5, nullptr));
  CHECK(scamd_transpose_slab_f64(rows64.data(), n, n, 5, t64.data(), 5, nullptr));
  for (int64_t r = 0; r < n; ++r)
    for (int f = 0; f < 5; ++f)
      if (t32[(size_t)r * 5 + f] != rows32[(size_t)f * n + r] || t64[(size_t)r * 5 + f] != rows64[(size_t)f * n + r]) {
        fprintf(stderr, "transpose: [%lld, %d]\n", (long long)r, f);
        return 1;
      }
  printf("builders: ok\n");
  return 0;
}

int main() {
  {
    const Graph hub = make_graph(3000, 1, 2500);
    if (run_case<float, float>("hub, 3 columns in place", hub, 3, 0)) return 1;
    if (run_case<double, double>("hub, 64 float64 columns", hub, 64, 0)) return 1;
  }
  const int64_t ns[] = {2, 63, 65, 1000};
  const int widths[] = {1, 63, 64};
  for (int64_t n : ns)
    for (int m : widths) {
      const Graph g = make_graph(n, 0, 0);
      char what[96];
      snprintf(what, sizeof what, "widths n = %lld, ncols = %d", (long long)n, m);
      if (run_case<float, double>(what, g, m, 2)) return 1;
      if (run_case<double, float>(what, g, m, 0)) return 1;
    }
  {
    const Graph messy = make_graph(203, 2, 0);
    if (run_case<double, double>("messy", messy, 5, 1)) return 1;
    if (run_case<float, float>("messy", messy, 64, 0)) return 1;
  }
  if (run_builders()) return 1;
  {
    Graph empty;
    empty.n = 70;
    empty.indptr.assign(71, 0);
    if (run_case<float, float>("empty graph", empty, 7, 0)) return 1;
  }
  return 0;
}
