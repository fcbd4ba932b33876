// Stand-alone AddressSanitizer driver of the aggregation entry points on the HOST emulation of the kernels (tests/emu):
// scamd_aggregate_moments_f32 and scamd_aggregate_median_f32 on (1) 3000 x 9 at 90 %, three groups of which one holds 60 % of the
// rows (its entries span several parts; the LDS table); (2) 2000 x 5 with 500 groups of 4 rows (every run adds to the global
// table; many groups in one part; short median segments); (3) 40 x 4097 at 15 % (two gene windows, 64 lanes per row); (4) a dense
// 300 x 6 matrix, one group of all rows but the first and last ten (code -1), an empty group in front of it (segments beyond
// the in-wave tier); (5) 4200 x 2, one group, column 0 fully stored and negative (a segment beyond the LDS chunk); (6) n = 0,
// g = 0 and n_groups = 0.  The inputs are generated here (a small LCG), no file is read; every output is compared with plain
// loops on the host (counts and medians exactly, sums to 1e-12, m2 to 1e-9 relative).  Not part of the test suite.  Build and run
// (the emulator library from `python tests/emu/build.py --asan`):
//   RT=$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so))     (the sanitizer's shared runtime, found by rpath)
//   clang++ -std=c++17 -g -fsanitize=address -shared-libasan -Iinclude tools/aggregate_asan_main.cpp \
//     -Ltests/emu/_build/asan -lscanpy_amd_emu -Wl,-rpath,tests/emu/_build/asan -Wl,-rpath,$RT -o aggregate_asan && ./aggregate_asan
// Every buffer is a heap block of its exact size, so a read or write past any of them is reported.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scanpy_amd.h"

static uint64_t g_state = 0x853c49e6748fea9bull;
static uint32_t next_u32() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33);
}
static double next_unit() { return (next_u32() % 2000001u) / 1e6 - 1.0; }  // [-1, 1]

// an exact-size heap block (at least one byte, so that the pointer is never NULL)
template <typename T>
struct Block {
  T* p;
  size_t n;
  explicit Block(size_t count) : p(static_cast<T*>(malloc(std::max<size_t>(count * sizeof(T), 1)))), n(count) {}
  Block(const std::vector<T>& v) : Block(v.size()) {
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  }
  ~Block() { free(p); }
  Block(const Block&) = delete;
};

struct Problem {
  int64_t n, g, n_groups;
  std::vector<float> dense;   // [n x g]
  std::vector<char> stored;   // [n x g]
  std::vector<int32_t> codes;
};

static int run(const char* name, const Problem& pr, int mid_in_f32) {
  const int64_t n = pr.n, g = pr.g, ng = pr.n_groups;
  std::vector<int64_t> indptr(n + 1, 0), sizes(ng, 0);
  std::vector<int32_t> indices, order;
  std::vector<float> data;
  for (int64_t r = 0; r < n; ++r) {
    for (int64_t c = 0; c < g; ++c)
      if (pr.stored[r * g + c]) {
        indices.push_back((int32_t)c);
        data.push_back(pr.dense[r * g + c]);
      }
    indptr[r + 1] = (int64_t)indices.size();
  }
  for (int64_t k = 0; k < ng; ++k)
    for (int64_t r = 0; r < n; ++r)
      if (pr.codes[r] == k) {
        order.push_back((int32_t)r);
        ++sizes[k];
      }
  const int64_t nnz = (int64_t)data.size(), cells = ng * g;
  Block<int64_t> b_indptr(indptr), b_sizes(sizes);
  Block<int32_t> b_indices(indices), b_order(order), b_codes(pr.codes);
  Block<float> b_data(data);
  Block<double> sum(cells), m2(cells), median(cells);
  Block<int64_t> nz(cells), neg(cells);
  Block<uint32_t> flags(1);
  const size_t ws_bytes = scamd_aggregate_workspace_bytes(n, g, nnz, ng);
  Block<char> ws(ws_bytes);
  memset(ws.p, 0xAB, std::max<size_t>(ws_bytes, 1));
  int rc = scamd_aggregate_moments_f32(b_indptr.p, nnz ? b_indices.p : nullptr, nnz ? b_data.p : nullptr, n, g, nnz, n ? b_codes.p : nullptr,
                                       order.empty() ? nullptr : b_order.p, (int64_t)order.size(), ng ? b_sizes.p : nullptr, ng,
                                       cells ? sum.p : nullptr, cells ? nz.p : nullptr, cells ? neg.p : nullptr, cells ? m2.p : nullptr,
                                       flags.p, ws.p, ws_bytes, nullptr);
  if (rc != SCAMD_OK || flags.p[0] != 0) {
    fprintf(stderr, "%s: moments rc=%d flags=%u: %s\n", name, rc, flags.p[0], scamd_last_error());
    return 1;
  }
  int64_t info[3] = {-1, -1, -1};
  rc = scamd_aggregate_median_f32(b_indptr.p, nnz ? b_indices.p : nullptr, nnz ? b_data.p : nullptr, n, g, nnz,
                                  order.empty() ? nullptr : b_order.p, (int64_t)order.size(), ng ? b_sizes.p : nullptr, ng,
                                  cells ? nz.p : nullptr, cells ? neg.p : nullptr, mid_in_f32, cells ? median.p : nullptr, info, ws.p,
                                  ws_bytes, nullptr);
  if (rc != SCAMD_OK || info[0] + info[1] + info[2] != cells) {
    fprintf(stderr, "%s: median rc=%d info=%lld %lld %lld: %s\n", name, rc, (long long)info[0], (long long)info[1], (long long)info[2],
            scamd_last_error());
    return 1;
  }
  int bad = 0;
  for (int64_t k = 0; k < ng && !bad; ++k) {
    for (int64_t c = 0; c < g && !bad; ++c) {
      std::vector<float> v;
      for (int64_t r = 0; r < n; ++r)
        if (pr.codes[r] == k) v.push_back(pr.dense[r * g + c]);
      long double s = 0, q = 0;
      int64_t cnt = 0, cneg = 0;
      for (float x : v) {
        s += x;
        cnt += x != 0.f;
        cneg += x < 0.f;
      }
      const long double mean = v.empty() ? 0 : s / (long double)v.size();
      for (float x : v) q += ((long double)x - mean) * ((long double)x - mean);
      std::sort(v.begin(), v.end());
      double med = NAN;
      if (!v.empty()) {
        const float lo = v[(v.size() - 1) / 2], hi = v[v.size() / 2];
        med = v.size() % 2 ? (double)lo : (mid_in_f32 ? (double)((lo + hi) / 2.0f) : ((double)lo + (double)hi) / 2.0);
        if (med == 0.0) med = 0.0;
      }
      const int64_t i = k * g + c;
      const bool ok = nz.p[i] == cnt && neg.p[i] == cneg && fabsl(sum.p[i] - s) <= 1e-12L * (fabsl(s) + 1) &&
                      fabsl(m2.p[i] - q) <= 1e-9L * (q + 1e-30L) + 1e-300L && ((std::isnan(med) && std::isnan(median.p[i])) || med == median.p[i]);
      if (!ok) {
        fprintf(stderr, "%s: pair (%lld, %lld): sum %.17g / %.17Lg, nz %lld / %lld, neg %lld / %lld, m2 %.17g / %.17Lg, median %.17g / %.17g\n",
                name, (long long)k, (long long)c, sum.p[i], s, (long long)nz.p[i], (long long)cnt, (long long)neg.p[i], (long long)cneg,
                m2.p[i], q, median.p[i], med);
        bad = 1;
      }
    }
  }
  printf("%-28s n=%lld g=%lld groups=%lld nnz=%lld  median: %lld by counts, %lld in a wave, %lld by a workgroup  %s\n", name, (long long)n,
         (long long)g, (long long)ng, (long long)nnz, (long long)info[0], (long long)info[1], (long long)info[2], bad ? "FAILED" : "ok");
  return bad;
}

static Problem random_problem(int64_t n, int64_t g, int64_t ng, double density, int group_rule) {
  Problem pr;
  pr.n = n, pr.g = g, pr.n_groups = ng;
  pr.dense.assign(n * g, 0.f);
  pr.stored.assign(n * g, 0);
  pr.codes.assign(n, 0);
  for (int64_t i = 0; i < n * g; ++i) {
    if ((next_u32() % 1000000u) < density * 1e6) {
      pr.stored[i] = 1;
      const uint32_t kind = next_u32() % 20u;
      pr.dense[i] = kind == 0 ? 0.f : (kind == 1 ? -0.f : (float)(next_unit() * 50.0));
    }
  }
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t u = next_u32();
    if (group_rule == 0) pr.codes[r] = (int32_t)(u % 10u < 6u ? 1 : (u % 10u < 8u ? 0 : ng - 1));  // one group holds 60 %
    else pr.codes[r] = ng ? (int32_t)(r % ng) : -1;
  }
  return pr;
}

int main() {
  int bad = 0;
  bad |= run("big group", random_problem(3000, 9, 3, 0.9, 0), 1);
  bad |= run("many groups", random_problem(2000, 5, 500, 0.5, 1), 0);
  bad |= run("two windows", random_problem(40, 4097, 3, 0.15, 1), 1);
  {
    Problem pr = random_problem(300, 6, 2, 1.0, 1);
    std::fill(pr.stored.begin(), pr.stored.end(), 1);
    for (int64_t r = 0; r < 300; ++r) pr.codes[r] = (r < 10 || r >= 290) ? -1 : 1;   // group 0 is empty
    bad |= run("dense, an empty group", pr, 1);
  }
  {
    Problem pr = random_problem(4200, 2, 1, 0.3, 1);
    for (int64_t r = 0; r < 4200; ++r) {
      pr.stored[r * 2] = 1;
      pr.dense[r * 2] = -(float)(1 + next_u32() % 1000u);
    }
    bad |= run("a segment beyond the chunk", pr, 0);
  }
  bad |= run("n = 0", random_problem(0, 5, 0, 0.5, 1), 1);
  bad |= run("g = 0", random_problem(7, 0, 2, 0.5, 1), 1);
  {
    Problem pr = random_problem(7, 5, 0, 0.5, 1);
    std::fill(pr.codes.begin(), pr.codes.end(), -1);
    bad |= run("n_groups = 0", pr, 1);
  }
  if (bad) {
    fprintf(stderr, "FAILED\n");
    return 1;
  }
  printf("all cases ok\n");
  return 0;
}
