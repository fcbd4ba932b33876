// Stand-alone AddressSanitizer driver of the scrublet entry points on the HOST emulation of the kernels (tests/emu):
// scamd_pp_scrublet_pair_count + scamd_pp_scrublet_pair_fill_f32 and scamd_scrublet_scores_f64 on: (1) 300 short rows over 97 genes
// (8 lanes per row), 700 pairs with self pairs and empty rows; (2) 40 rows of 200-700 entries over 2049 genes (32 lanes per row,
// several chunks per row and the carry across them); (3) rows of up to 3000 entries over 4099 genes (64 lanes per row) paired
// with rows of 3; (4) no pairs at all; then the scores for k = 1, 17, 66 and 256.  The inputs are generated here (a small LCG),
// no file is read; the sums are compared with a two-pointer merge on the host, the counts with a plain loop.  Not part of the
// test suite.  Build and run (the emulator library from `python tests/emu/build.py --asan`):
//   RT=$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so))     (the sanitizer's shared runtime, found by rpath)
//   clang++ -std=c++17 -g -fsanitize=address -shared-libasan -Iinclude tools/scrublet_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -Wl,-rpath,$RT -o scrublet_asan && ./scrublet_asan
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

// row r holds lo + (random below span) entries, every `empty_every`-th row none
static int run_pairs(const char* what, int n, int g, int lo, int span, int empty_every, int n_sim) {
  std::vector<int64_t> indptr(n + 1, 0);
  std::vector<int32_t> indices;
  std::vector<float> data;
  std::vector<uint8_t> used(g);
  for (int r = 0; r < n; ++r) {
    const int len = (empty_every && r % empty_every == 0) ? 0 : std::min(g, lo + (int)(next_u32() % (uint32_t)std::max(span, 1)));
    std::fill(used.begin(), used.end(), 0);
    int have = 0;
    while (have < len) {
      const int c = (int)(next_u32() % (uint32_t)g);
      if (!used[c]) used[c] = 1, ++have;
    }
    for (int c = 0; c < g; ++c)
      if (used[c]) {
        indices.push_back(c);
        data.push_back((float)(1 + next_u32() % 50u));
      }
    indptr[r + 1] = (int64_t)indices.size();
  }
  const int64_t nnz = indptr[n];
  std::vector<int32_t> pairs((size_t)2 * n_sim);
  for (int r = 0; r < n_sim; ++r) {
    pairs[2 * r] = (int32_t)(next_u32() % (uint32_t)n);
    pairs[2 * r + 1] = r % 7 == 0 ? pairs[2 * r] : (int32_t)(next_u32() % (uint32_t)n);
  }
  std::vector<double> row_total(n, 0.0), total_sim(n_sim, -1.0);
  for (int r = 0; r < n; ++r)
    for (int64_t p = indptr[r]; p < indptr[r + 1]; ++p) row_total[r] += data[p];
  std::vector<int64_t> out_indptr(n_sim + 1, -1);
  uint32_t flags = 7u;
  int64_t out_nnz = -1;
  const size_t ws_bytes = scamd_pp_scrublet_workspace_bytes(n_sim);
  std::vector<unsigned char> ws(ws_bytes, 0xAB);
  CHECK(scamd_pp_scrublet_pair_count(indptr.data(), indices.data(), n, g, nnz, pairs.data(), n_sim, row_total.data(), 1, out_indptr.data(),
                                     total_sim.data(), &flags, &out_nnz, ws.data(), ws_bytes, nullptr));
  if (flags != 0u || out_nnz != out_indptr[n_sim]) {
    fprintf(stderr, "%s: count phase: flags = %u, total %lld / %lld\n", what, flags, (long long)out_nnz, (long long)out_indptr[n_sim]);
    return 1;
  }
  std::vector<int32_t> out_indices((size_t)out_nnz, -1);
  std::vector<float> out_data((size_t)out_nnz, -1.f);
  flags = 7u;
  CHECK(scamd_pp_scrublet_pair_fill_f32(indptr.data(), indices.data(), data.data(), n, g, nnz, pairs.data(), n_sim, out_indptr.data(),
                                        out_nnz, out_indices.data(), out_data.data(), &flags, nullptr));
  if (flags != 0u) {
    fprintf(stderr, "%s: fill phase: flags = %u\n", what, flags);
    return 1;
  }
  for (int r = 0; r < n_sim; ++r) {
    const int a = pairs[2 * r], b = pairs[2 * r + 1];
    int64_t pa = indptr[a], pb = indptr[b], at = out_indptr[r];
    while (pa < indptr[a + 1] || pb < indptr[b + 1]) {
      const int ca = pa < indptr[a + 1] ? indices[pa] : g, cb = pb < indptr[b + 1] ? indices[pb] : g;
      const int c = std::min(ca, cb);
      float v = 0.f;
      if (ca == c) v += data[pa++];
      if (cb == c) v += data[pb++];
      if (at >= out_indptr[r + 1] || out_indices[at] != c || out_data[at] != v) {
        fprintf(stderr, "%s: output row %d (%d + %d), entry %lld: expected column %d value %g\n", what, r, a, b,
                (long long)(at - out_indptr[r]), c, v);
        return 1;
      }
      ++at;
    }
    if (at != out_indptr[r + 1] || total_sim[r] != row_total[a] + row_total[b]) {
      fprintf(stderr, "%s: output row %d: length or total\n", what, r);
      return 1;
    }
  }
  printf("%s: ok (%d x %d, nnz %lld, %d pairs, %lld entries out)\n", what, n, g, (long long)nnz, n_sim, (long long)out_nnz);
  return 0;
}

static int run_scores(int n_all, int k, int n_obs) {
  std::vector<int32_t> idx((size_t)n_all * k);
  for (auto& v : idx) v = (int32_t)(next_u32() % (uint32_t)n_all);
  std::vector<int32_t> cnt(n_all, -1);
  std::vector<double> score(n_all, -1.0), err(n_all, -1.0);
  const double rho = 0.05, r = 2.0, se_rho = 0.02;
  CHECK(scamd_scrublet_scores_f64(idx.data(), n_all, k, n_obs, rho, r, se_rho, cnt.data(), score.data(), err.data(), nullptr));
  for (int i = 0; i < n_all; ++i) {
    int want = 0;
    for (int j = 0; j < k; ++j) want += idx[(size_t)i * k + j] >= n_obs;
    const double q = (want + 1.0) / (k + 2.0);
    const double ld = q * rho / r / (1.0 - rho - q * (1.0 - rho - rho / r));
    if (cnt[i] != want || !(std::fabs(score[i] - ld) <= 1e-15 * ld) || !(err[i] > 0.0)) {
      fprintf(stderr, "scores k = %d: row %d: count %d (expected %d), score %.17g (expected %.17g)\n", k, i, cnt[i], want, score[i], ld);
      return 1;
    }
  }
  printf("scores: ok (%d rows, k = %d, %d observed)\n", n_all, k, n_obs);
  return 0;
}

int main() {
  if (run_pairs("short rows, 8 lanes", 300, 97, 0, 30, 5, 700)) return 1;
  if (run_pairs("several chunks, 32 lanes", 40, 2049, 200, 500, 0, 150)) return 1;
  if (run_pairs("long against short, 64 lanes", 12, 4099, 3, 3000, 0, 60)) return 1;
  if (run_pairs("no pairs", 5, 9, 1, 3, 0, 0)) return 1;
  for (int k : {1, 17, 66, 256})
    if (run_scores(1000 + k, k, 333)) return 1;
  return 0;
}
