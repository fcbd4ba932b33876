// Stand-alone AddressSanitizer driver of the regress_out entry points on the HOST emulation of the kernels (tests/emu):
// scamd_pp_regress_sums_f32 and scamd_pp_regress_resid_f32 on four cases: (1) two numeric keys (3 table rows), 67 rows over 2049
// genes, float32 out: range table and sums table in global memory, three column slices, a row count that is no multiple of the
// batch; (2) 16 numeric keys (17 table rows, 64 threads per row), 70 rows over 300 genes, float64 out, tables in LDS; (3) a
// categorical key with 5 categories (one empty), 4500 rows over 1030 genes of which only every fourth row is stored, float32 out:
// more batches than row blocks (the stride loop and the two copies of the staged codes); (4) n == 0.  The inputs are generated
// here (a small LCG), no file is read; the sums and the residual are compared with plain loops on the host.  Not part of the
// test suite.  Build and run (the emulator library from `python tests/emu/build.py --asan`):
//   RT=$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so))     (the sanitizer's shared runtime, found by rpath)
//   clang++ -std=c++17 -g -fsanitize=address -shared-libasan -Iinclude tools/regress_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -Wl,-rpath,$RT -o regress_asan && ./regress_asan
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

// m table rows; n_cat > 0: a categorical key with m = n_cat categories (category 1 stays empty), else numeric weights in [-1, 1]
// with a first column of ones.  Row r stores per_row entries when r % every == 0, none otherwise.
static int run_case(const char* what, int64_t n, int g, int m, int n_cat, int per_row, int every, int out_is_f64) {
  std::vector<int64_t> indptr(n + 1, 0);
  for (int64_t r = 0; r < n; ++r) indptr[r + 1] = indptr[r] + (r % every == 0 ? std::min(per_row, g) : 0);
  const int64_t nnz = indptr[n];
  std::vector<int32_t> indices(nnz);
  std::vector<float> data(nnz);
  std::vector<double> dense((size_t)n * g, 0.0);
  for (int64_t r = 0; r < n; ++r) {
    const int len = (int)(indptr[r + 1] - indptr[r]);
    const int start = (int)(next_u32() % (uint32_t)g);
    std::vector<int32_t> cols(len);
    for (int j = 0; j < len; ++j) cols[j] = (int32_t)(((int64_t)start + (int64_t)j * (g / std::max(len, 1) > 0 ? g / std::max(len, 1) : 1)) % g);
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    for (int j = 0; j < len; ++j) {
      const int32_t c = j < (int)cols.size() ? cols[j] : -1;
      if (c < 0) {  // (a repeated column: fall back to the first free ones)
        fprintf(stderr, "%s: generator produced a repeated column\n", what);
        return 1;
      }
      indices[indptr[r] + j] = c;
      data[indptr[r] + j] = (float)((int)(next_u32() % 2001u) - 1000) / 8.0f;
      dense[(size_t)r * g + c] = (double)data[indptr[r] + j];
    }
  }
  std::vector<double> w, wbound(m, 0.0);
  std::vector<int32_t> codes;
  if (n_cat) {
    codes.resize(n);
    for (int64_t r = 0; r < n; ++r) {
      int c = (int)(next_u32() % (uint32_t)m);
      if (c == 1 && m > 1) c = 0;
      codes[r] = c;
      wbound[c] += 1.0;
    }
  } else {
    w.resize((size_t)n * m);
    for (int64_t r = 0; r < n; ++r)
      for (int k = 0; k < m; ++k) {
        w[(size_t)r * m + k] = k == 0 ? 1.0 : next_unit();
        wbound[k] += std::fabs(w[(size_t)r * m + k]);
      }
  }
  std::vector<double> sums((size_t)m * g, -1.0);
  std::vector<float> col_min(g, -7.f), col_max(g, -7.f);
  uint32_t flags = 7u;
  const size_t ws_bytes = scamd_pp_regress_workspace_bytes(g, m);
  std::vector<unsigned char> ws(ws_bytes, 0xAB);
  CHECK(scamd_pp_regress_sums_f32(indptr.data(), indices.data(), data.data(), n, g, nnz, n_cat ? nullptr : w.data(),
                                  n_cat ? codes.data() : nullptr, m, wbound.data(), sums.data(), col_min.data(), col_max.data(), &flags,
                                  ws.data(), ws_bytes, nullptr));
  if (flags != 0u) {
    fprintf(stderr, "%s: flags = %u\n", what, flags);
    return 1;
  }
  std::vector<double> want((size_t)m * g, 0.0);
  for (int64_t r = 0; r < n; ++r)
    for (int c = 0; c < g; ++c) {
      const double x = dense[(size_t)r * g + c];
      if (x == 0.0) continue;
      if (n_cat) want[(size_t)codes[r] * g + c] += x;
      else
        for (int k = 0; k < m; ++k) want[(size_t)k * g + c] += w[(size_t)r * m + k] * x;
    }
  for (int k = 0; k < m; ++k)
    for (int c = 0; c < g; ++c) {
      const double err = std::fabs(sums[(size_t)k * g + c] - want[(size_t)k * g + c]);
      if (!(err <= 1e-9 * (wbound[k] * 125.0 + 1.0))) {
        fprintf(stderr, "%s: sums[%d, %d] = %.17g, expected %.17g\n", what, k, c, sums[(size_t)k * g + c], want[(size_t)k * g + c]);
        return 1;
      }
    }
  for (int c = 0; c < g; ++c) {
    double lo = n ? dense[c] : 0.0, hi = lo;
    for (int64_t r = 0; r < n; ++r) {
      lo = std::min(lo, dense[(size_t)r * g + c]);
      hi = std::max(hi, dense[(size_t)r * g + c]);
    }
    if ((double)col_min[c] != lo || (double)col_max[c] != hi) {
      fprintf(stderr, "%s: range of gene %d is [%g, %g], expected [%g, %g]\n", what, c, col_min[c], col_max[c], lo, hi);
      return 1;
    }
  }
  // the table as the front end makes it (means of the ones column / of the categories), every third gene not kept
  std::vector<double> table(sums);
  for (int k = 0; k < m; ++k)
    if (n_cat || k == 0)
      for (int c = 0; c < g; ++c) table[(size_t)k * g + c] /= std::max(n_cat ? wbound[k] : (double)n, 1.0);
  std::vector<uint8_t> keep(g);
  for (int c = 0; c < g; ++c) keep[c] = c % 3 != 0;
  std::vector<unsigned char> out((size_t)n * g * (out_is_f64 ? 8 : 4), 0xCD);
  CHECK(scamd_pp_regress_resid_f32(indptr.data(), indices.data(), data.data(), n, g, nnz, keep.data(), table.data(),
                                   n_cat ? nullptr : w.data(), n_cat ? codes.data() : nullptr, m, out.data(), out_is_f64, nullptr));
  for (int64_t r = 0; r < n; ++r)
    for (int c = 0; c < g; ++c) {
      double fit = 0.0;
      if (keep[c]) {
        if (n_cat) fit = table[(size_t)codes[r] * g + c];
        else
          for (int k = 0; k < m; ++k) fit += w[(size_t)r * m + k] * table[(size_t)k * g + c];
      }
      const double expect = dense[(size_t)r * g + c] - fit;
      const double got = out_is_f64 ? reinterpret_cast<const double*>(out.data())[(size_t)r * g + c]
                                    : (double)reinterpret_cast<const float*>(out.data())[(size_t)r * g + c];
      if (!(std::fabs(got - expect) <= (out_is_f64 ? 1e-10 : 2e-5) * (1.0 + std::fabs(expect)))) {
        fprintf(stderr, "%s: out[%lld, %d] = %.17g, expected %.17g\n", what, (long long)r, c, got, expect);
        return 1;
      }
    }
  printf("%s: ok (%lld x %d, nnz %lld, %d table rows)\n", what, (long long)n, g, (long long)nnz, m);
  return 0;
}

int main() {
  if (run_case("numeric, 2 keys, three slices", 67, 2049, 3, 0, 40, 1, 0)) return 1;
  if (run_case("numeric, 16 keys, 64 threads per row", 70, 300, 17, 0, 300, 1, 1)) return 1;
  if (run_case("categorical, row-block stride", 4500, 1030, 5, 5, 6, 4, 0)) return 1;
  {
    const int64_t indptr0 = 0;
    std::vector<double> sums(3 * 16, -1.0), wbound(3, 1.0), w(1, 1.0), table(3 * 16, 0.0);
    std::vector<float> lo(16, -7.f), hi(16, -7.f);
    std::vector<uint8_t> keep(16, 1);
    uint32_t flags = 7u;
    const size_t ws_bytes = scamd_pp_regress_workspace_bytes(16, 3);
    std::vector<unsigned char> ws(ws_bytes, 0xAB);
    CHECK(scamd_pp_regress_sums_f32(&indptr0, nullptr, nullptr, 0, 16, 0, w.data(), nullptr, 3, wbound.data(), sums.data(), lo.data(),
                                    hi.data(), &flags, ws.data(), ws_bytes, nullptr));
    CHECK(scamd_pp_regress_resid_f32(&indptr0, nullptr, nullptr, 0, 16, 0, keep.data(), table.data(), w.data(), nullptr, 3, nullptr, 0,
                                     nullptr));
    for (double v : sums)
      if (v != 0.0) {
        fprintf(stderr, "n == 0: a sum is %g\n", v);
        return 1;
      }
    printf("n == 0: ok\n");
  }
  return 0;
}
