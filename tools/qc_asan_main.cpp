// Stand-alone AddressSanitizer driver of the quality-control entry points on the HOST emulation of the kernels (tests/emu):
// scamd_pp_qc_sweep_f32 and scamd_pp_qc_top_f32 on three cases: (1) 40 rows over 9000 genes of which four are longer than the
// 8192 staged keys of a workgroup (the selection path; positions 50, 500, 4096; global per-gene table) and, at a wave per row, 60
// rows over 2300 genes with rows beyond the wave's 2048 keys; (2) 32 gene masks on 300 rows over 500 genes (LDS per-gene table);
// (3) n == 0.  The inputs are generated here (a small LCG), no file is read; top(n) and the row totals are compared with a sort
// on the host.  Not part of the test suite.  Build and run (the emulator library from `python tests/emu/build.py --asan`):
//   RT=$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so))     (the sanitizer's shared runtime, found by rpath)
//   clang++ -std=c++17 -g -fsanitize=address -shared-libasan -Iinclude tools/qc_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -Wl,-rpath,$RT -o qc_asan && ./qc_asan
// Every buffer is a heap block of its exact size, so a read or write past any of them is reported.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
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

// lengths[r] stored entries in row r: the first columns of a per-row rotation, counts 0..999 (stored zeros among them)
static int run_case(const char* what, const std::vector<int>& lengths, int g, const std::vector<int32_t>& positions, int n_masks) {
  const int64_t n = (int64_t)lengths.size();
  std::vector<int64_t> indptr(n + 1, 0);
  for (int64_t r = 0; r < n; ++r) indptr[r + 1] = indptr[r] + lengths[r];
  const int64_t nnz = indptr[n];
  std::vector<int32_t> indices(nnz);
  std::vector<float> data(nnz);
  for (int64_t r = 0; r < n; ++r) {
    const int start = (int)(next_u32() % (uint32_t)g);
    std::vector<int32_t> cols(lengths[r]);
    for (int j = 0; j < lengths[r]; ++j) cols[j] = (start + j) % g;
    std::sort(cols.begin(), cols.end());
    for (int j = 0; j < lengths[r]; ++j) {
      indices[indptr[r] + j] = cols[j];
      data[indptr[r] + j] = (float)(next_u32() % 1000u);
    }
  }
  std::vector<uint32_t> gene_mask(g);
  for (int c = 0; c < g; ++c) gene_mask[c] = n_masks ? (next_u32() & next_u32()) | 0x80000000u : 0u;  // mask 31 selects all genes
  std::vector<int32_t> row_nnz(n);
  std::vector<double> row_total(n), row_masked((size_t)n_masks * n), col_sum(g), top((size_t)n * positions.size());
  std::vector<int64_t> col_nnz(g);
  uint32_t flags = 7u;
  CHECK(scamd_pp_qc_sweep_f32(indptr.data(), indices.data(), data.data(), n, g, nnz, n_masks ? gene_mask.data() : nullptr, n_masks,
                              row_nnz.data(), row_total.data(), n_masks ? row_masked.data() : nullptr, col_nnz.data(), col_sum.data(),
                              &flags, nullptr));
  CHECK(scamd_pp_qc_top_f32(indptr.data(), data.data(), n, nnz, positions.data(), (int)positions.size(), top.data(), nullptr));
  if (flags != 0u) {
    fprintf(stderr, "%s: flags = %u\n", what, flags);
    return 1;
  }
  const int nmax = positions.back();
  double all = 0.0, cols_all = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    std::vector<double> v;
    for (int64_t p = indptr[r]; p < indptr[r + 1]; ++p)
      if (data[p] != 0.f) v.push_back((double)data[p]);
    const size_t stored = v.size();
    if (v.size() < (size_t)nmax) v.resize(nmax, 0.0);
    std::sort(v.begin(), v.end(), std::greater<double>());
    double total = 0.0;
    for (double e : v) total += e;
    double acc = 0.0;
    size_t k = 0;
    for (size_t j = 0; j < positions.size(); ++j) {
      for (; k < (size_t)positions[j]; ++k) acc += v[k];
      if (top[r * positions.size() + j] != acc) {
        fprintf(stderr, "%s: row %lld position %d: %.1f, expected %.1f\n", what, (long long)r, positions[j], top[r * positions.size() + j], acc);
        return 1;
      }
    }
    if (row_total[r] != total || (size_t)row_nnz[r] != stored || (n_masks == 32 && row_masked[(size_t)31 * n + r] != total)) {
      fprintf(stderr, "%s: row %lld: total %.1f nnz %d, expected %.1f %zu\n", what, (long long)r, row_total[r], row_nnz[r], total, stored);
      return 1;
    }
    all += total;
  }
  for (int c = 0; c < g; ++c) cols_all += col_sum[c];
  if (all != cols_all) {
    fprintf(stderr, "%s: the per-gene sums add up to %.1f, the per-row totals to %.1f\n", what, cols_all, all);
    return 1;
  }
  printf("%s: n=%lld g=%d nnz=%lld positions=%zu masks=%d: total %.0f\n", what, (long long)n, g, (long long)nnz, positions.size(), n_masks, all);
  return 0;
}

int main() {
  {  // (1) rows beyond the staging capacity: 8192 keys at a workgroup per row, 2048 at a wave per row
    std::vector<int> lengths(40, 300);
    lengths[0] = 0, lengths[5] = 8193, lengths[6] = 9000, lengths[20] = 8192, lengths[21] = 8500, lengths[22] = 8999, lengths[39] = 0;
    if (run_case("long rows, workgroup per row", lengths, 9000, {50, 500, 4096}, 0)) return 1;
    std::vector<int> wave(60, 100);
    wave[0] = 0, wave[7] = 2049, wave[8] = 2300, wave[30] = 2048, wave[31] = 2047, wave[59] = 0;
    if (run_case("long rows, wave per row", wave, 2300, {1, 64, 2048}, 1)) return 1;
  }
  {  // (2) 32 masks
    std::vector<int> lengths(300);
    for (size_t r = 0; r < lengths.size(); ++r) lengths[r] = (int)(next_u32() % 200u);
    lengths[0] = lengths[150] = lengths[299] = 0;
    if (run_case("32 masks", lengths, 500, {50, 100, 200, 500}, 32)) return 1;
  }
  {  // (3) n == 0
    int64_t indptr0 = 0;
    int32_t pos[2] = {1, 2};
    uint32_t flags = 7u;
    std::vector<double> col_sum(16, -1.0);
    std::vector<int64_t> col_nnz(16, -1);
    CHECK(scamd_pp_qc_sweep_f32(&indptr0, nullptr, nullptr, 0, 16, 0, nullptr, 0, nullptr, nullptr, nullptr, col_nnz.data(), col_sum.data(),
                                &flags, nullptr));
    CHECK(scamd_pp_qc_top_f32(&indptr0, nullptr, 0, 0, pos, 2, nullptr, nullptr));
    if (flags != 0u || col_sum[15] != 0.0 || col_nnz[15] != 0) {
      fprintf(stderr, "n == 0: the per-gene outputs and the flag word are not zeroed\n");
      return 1;
    }
    printf("n == 0: ok\n");
  }
  printf("qc_asan: clean\n");
  return 0;
}
