// Scrublet on the device: the two passes behind scanpy_amd.pp.scrublet / pp.scrublet_simulate_doublets that the project did not
// own yet (reference: `Scrublet.simulate_doublets` and `_nearest_neighbor_classifier` in
// src/scanpy/preprocessing/_scrublet/core.py).  PCA, projection and the kNN search are the existing entry points.
//
// 1. ROW-PAIR SUMS.  Simulated doublet r is row pairs[r, 0] + row pairs[r, 1] of a canonical CSR matrix (sorted, unique columns):
//    the sorted union of the two column lists, values added where both rows store the column.  Two phases:
//      scamd_pp_scrublet_pair_count     per output row the size of the union and total_sim[r] = row_total[a] + row_total[b], then the
//                                       exclusive scan of the sizes (scan.h) into out_indptr and ONE pinned read-back of the total;
//      scamd_pp_scrublet_pair_fill_f32  the caller allocates out_indices / out_data of that size; every element is written once.
//    One route whatever g is.  G lanes own an output row (G from the mean row length).  Call the rows A and B.  A lane takes
//    element p of A (column c) and finds rank_B(c) = |{columns of B below c}| by binary search, and whether B stores c (a match).
//    THE RANK FORMULA.  The output holds, before that element, the p elements of A before it and the elements of B below c that
//    are not matched; each matched one pairs with exactly one of the p elements of A.  So
//        position(A[p]) = p + rank_B(c) - matches among A[0 .. p)
//    and by symmetry for an unmatched element q of B:  position(B[q]) = q + rank_A(c) - matches among B[0 .. q).
//    The matched element of A carries the sum, the matched element of B is dropped.  "Matches before" is a ballot of the chunk's
//    match bits, the popcount of the lane's lower bits in its group, plus a running carry over the chunks of G elements.  Every
//    position is a pure function of the input: no atomics, two runs give the same bytes.  A pair (i, i) matches everywhere and
//    yields row i doubled.  Nothing is dropped for being zero: a stored zero stays stored, and sums of counts create none.
//    The trip count of the chunk loop is made uniform over the wave (the maximum over its groups -- what the SIMD pays anyway), so
//    every ballot is a collective of a full wave.
//    flags (device word, zeroed by each phase): bit 0 = an output value above 2^24 in magnitude (sums of integer counts are exact
//    in float32 up to there), bit 1 = a pair outside [0, n) or a row pointer outside [0, nnz] (such an output row is empty),
//    bit 2 = an output position outside out_nnz (out_indptr was not made by the count phase for these inputs; nothing is written
//    there).
//
// 2. SCORES.  scamd_scrublet_scores_f64: idx int32 [n_all, k] are the neighbour lists of the concatenated manifold (observed rows
//    first, the layout scamd_knn_l2_f32 returns).  n_sim_neigh[i] = |{j : idx[i, j] >= n_obs}| by ballot + popcount in a lane
//    group per row, then the reference's Bayesian score and its standard error in float64, in the reference's operation order
//    (IEEE division and square root, no contraction): the same bits as numpy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "scan.h"

namespace scamd {

namespace {

constexpr int SB_BLOCK = 256;
constexpr int SB_GRID_CAP = 256 * 32;  // workgroups of a row-wise launch
constexpr float SB_EXACT_MAX = 16777216.0f;  // 2^24

constexpr unsigned SB_FLAG_INEXACT = 1u, SB_FLAG_BAD_PAIR = 2u, SB_FLAG_CAPACITY = 4u;

// number of entries of the sorted list idx[0 .. len) below c
__device__ __forceinline__ int sb_lower_bound(const int32_t* __restrict__ idx, int len, int c) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (idx[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct SbRows {
  int64_t a0, b0;
  int la, lb;
  int a, b;
  bool bad;
};

// the two parent rows of output row r; a row past n_sim or a bad pair is a pair of empty rows
__device__ __forceinline__ SbRows sb_rows(const int64_t* __restrict__ indptr, const int32_t* __restrict__ pairs, int64_t n, int64_t nnz,
                                          int64_t r, bool valid) {
  SbRows w = {0, 0, 0, 0, 0, 0, false};
  if (!valid) return w;
  const int a = pairs[2 * r], b = pairs[2 * r + 1];
  if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n) {
    w.bad = true;
    return w;
  }
  const int64_t a0 = indptr[a], a1 = indptr[a + 1], b0 = indptr[b], b1 = indptr[b + 1];
  if (a0 < 0 || a1 < a0 || a1 > nnz || b0 < 0 || b1 < b0 || b1 > nnz || a1 - a0 > 0x7fffffff || b1 - b0 > 0x7fffffff) {
    w.bad = true;
    return w;
  }
  w.a = a, w.b = b, w.a0 = a0, w.b0 = b0, w.la = (int)(a1 - a0), w.lb = (int)(b1 - b0);
  return w;
}

// ---- phase 1: the size of every union and the totals.  The row loop is uniform over the workgroup; the element loop holds no
// collective (its trip count differs between the groups of a wave), the group sum comes after it.
template <int G, typename TotT>
__global__ __launch_bounds__(SB_BLOCK) void sb_count_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            int64_t n, int64_t nnz, const int32_t* __restrict__ pairs, int64_t n_sim,
                                                            const TotT* __restrict__ row_total, int* __restrict__ counts,
                                                            TotT* __restrict__ total_sim, unsigned int* flags) {
  constexpr int RPB = SB_BLOCK / G;
  const int sub = threadIdx.x % G;
  unsigned int bad = 0u;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < n_sim; base += (int64_t)gridDim.x * RPB) {
    const int64_t r = base + threadIdx.x / G;
    const bool valid = r < n_sim;
    const SbRows w = sb_rows(indptr, pairs, n, nnz, r, valid);
    if (w.bad) bad = SB_FLAG_BAD_PAIR;
    // the shorter row is searched for in the longer one
    const bool swap = w.la > w.lb;
    const int32_t* sa = indices + (swap ? w.b0 : w.a0);
    const int32_t* sb = indices + (swap ? w.a0 : w.b0);
    const int ls = swap ? w.lb : w.la, ll = swap ? w.la : w.lb;
    int m = 0;
    if (w.a == w.b) {
      m = sub == 0 ? ls : 0;  // (i, i): every element matches
    } else {
      for (int p = sub; p < ls; p += G) {
        const int c = sa[p];
        const int pos = sb_lower_bound(sb, ll, c);
        m += (pos < ll && sb[pos] == c) ? 1 : 0;
      }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) m += __shfl_xor(m, o);
    if (valid && sub == 0) {
      counts[r] = w.la + w.lb - m;  // (the union of two rows has at most g < 2^31 columns)
      total_sim[r] = w.bad ? (TotT)0 : row_total[w.a] + row_total[w.b];
    }
  }
  if (bad) atomicOr(flags, bad);
}

// ---- phase 2: the merge.  Per trip a lane takes element t * G + sub of A and of B.
template <int G>
__global__ __launch_bounds__(SB_BLOCK) void sb_fill_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                           const float* __restrict__ data, int64_t n, int64_t nnz,
                                                           const int32_t* __restrict__ pairs, int64_t n_sim,
                                                           const int64_t* __restrict__ out_indptr, int64_t out_nnz,
                                                           int32_t* __restrict__ out_indices, float* __restrict__ out_data,
                                                           unsigned int* flags) {
  constexpr int RPB = SB_BLOCK / G;
  constexpr unsigned long long GROUP = G == 64 ? ~0ull : ((1ull << (G % 64)) - 1ull);
  const int sub = threadIdx.x % G;
  const int shift = (threadIdx.x & 63) - sub;                    // first lane of this group in its wave
  const unsigned long long below = (1ull << sub) - 1ull;         // the lanes of the group before this one
  unsigned int bad = 0u;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < n_sim; base += (int64_t)gridDim.x * RPB) {
    const int64_t r = base + threadIdx.x / G;
    const bool valid = r < n_sim;
    const SbRows w = sb_rows(indptr, pairs, n, nnz, r, valid);
    if (w.bad) bad |= SB_FLAG_BAD_PAIR;
    const int64_t o0 = valid ? out_indptr[r] : 0;
    const int32_t* ia = indices + w.a0;
    const int32_t* ib = indices + w.b0;
    const float* da = data + w.a0;
    const float* db = data + w.b0;
    int trips = (max(w.la, w.lb) + G - 1) / G;
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) trips = max(trips, __shfl_xor(trips, o));  // uniform over the wave
    int carry_a = 0, carry_b = 0;
    for (int t = 0; t < trips; ++t) {
      const int p = t * G + sub;
      const bool act_a = p < w.la, act_b = p < w.lb;
      int ca = 0, cb = 0, pos_a = 0, pos_b = 0;
      float va = 0.f, vb = 0.f;
      bool match_a = false, match_b = false;
      if (act_a) {
        ca = ia[p];
        va = da[p];
        pos_a = sb_lower_bound(ib, w.lb, ca);
        match_a = pos_a < w.lb && ib[pos_a] == ca;
        if (match_a) va += db[pos_a];
      }
      if (act_b) {
        cb = ib[p];
        vb = db[p];
        pos_b = sb_lower_bound(ia, w.la, cb);
        match_b = pos_b < w.la && ia[pos_b] == cb;
      }
      const unsigned long long ma = (__ballot(match_a) >> shift) & GROUP;
      const unsigned long long mb = (__ballot(match_b) >> shift) & GROUP;
      if (act_a) {
        const int64_t at = o0 + p + pos_a - (carry_a + __popcll(ma & below));
        if (at >= 0 && at < out_nnz) {
          out_indices[at] = ca;
          out_data[at] = va;
        } else {
          bad |= SB_FLAG_CAPACITY;
        }
        if (fabsf(va) > SB_EXACT_MAX) bad |= SB_FLAG_INEXACT;
      }
      if (act_b && !match_b) {
        const int64_t at = o0 + p + pos_b - (carry_b + __popcll(mb & below));
        if (at >= 0 && at < out_nnz) {
          out_indices[at] = cb;
          out_data[at] = vb;
        } else {
          bad |= SB_FLAG_CAPACITY;
        }
        if (fabsf(vb) > SB_EXACT_MAX) bad |= SB_FLAG_INEXACT;
      }
      carry_a += __popcll(ma);
      carry_b += __popcll(mb);
    }
  }
  if (bad) atomicOr(flags, bad);
}

// ---- the scores.  k is the same for every row: the chunk loop is uniform over the launch, a row past n_all contributes nothing.
template <int G>
__global__ __launch_bounds__(SB_BLOCK) void sb_scores_kernel(const int32_t* __restrict__ idx, int64_t n_all, int k, int n_obs, double rho,
                                                             double r, double se_rho, int32_t* __restrict__ n_sim_neigh,
                                                             double* __restrict__ score, double* __restrict__ score_err) {
  constexpr int RPB = SB_BLOCK / G;
  constexpr unsigned long long GROUP = G == 64 ? ~0ull : ((1ull << (G % 64)) - 1ull);
  const int sub = threadIdx.x % G;
  const int shift = (threadIdx.x & 63) - sub;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < n_all; base += (int64_t)gridDim.x * RPB) {
    const int64_t row = base + threadIdx.x / G;
    const bool valid = row < n_all;
    int count = 0;
    for (int j0 = 0; j0 < k; j0 += G) {
      const int j = j0 + sub;
      const bool sim = valid && j < k && idx[row * k + j] >= n_obs;
      count += __popcll((__ballot(sim) >> shift) & GROUP);
    }
    if (valid && sub == 0) {
      const double nd = (double)count, nn = (double)k;
      const double q = (nd + 1.0) / (nn + 2.0);
      const double den = 1.0 - rho - q * (1.0 - rho - rho / r);
      const double ld = q * rho / r / den;
      const double se_q = sqrt(q * (1.0 - q) / (nn + 3.0));
      const double t1 = se_q / q * (1.0 - rho), t2 = se_rho / rho * (1.0 - q);
      const double se_ld = q * rho / r / (den * den) * sqrt(t1 * t1 + t2 * t2);
      n_sim_neigh[row] = count;
      score[row] = ld;
      score_err[row] = se_ld;
    }
  }
}

// lanes per output row from the mean length of the input rows (the rule of csrc/preprocess.hip and rg_lanes_per_row)
inline int sb_lanes_per_row(int64_t n, int64_t nnz) {
  const int64_t avg = n > 0 ? nnz / n : 0;
  return avg <= 32 ? 8 : (avg <= 160 ? 16 : (avg <= 512 ? 32 : 64));
}

// lanes per row of the score kernel from the length of the neighbour lists
inline int sb_score_lanes(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : (k <= 32 ? 32 : 64)); }

inline unsigned sb_grid(int64_t rows, int G) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(rows, SB_BLOCK / G), 1), SB_GRID_CAP);
}

struct ScrubletWorkspace {
  int* counts;
  int64_t* block_tmp;
  size_t bytes;
  bool ok;
};

ScrubletWorkspace sb_carve(void* base, size_t cap, int64_t n_sim) {
  Workspace ws(base, cap);
  ScrubletWorkspace r;
  r.counts = ws.take<int>((size_t)std::max<int64_t>(n_sim, 1));
  r.block_tmp = ws.take<int64_t>((size_t)scan_num_blocks(std::max<int64_t>(n_sim, 1)) + 1);
  r.bytes = ws.used();
  r.ok = ws.ok;
  return r;
}

template <int G>
void sb_launch_count(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const int32_t* pairs, int64_t n_sim,
                     const void* row_total, bool f64, int* counts, void* total_sim, unsigned int* flags, hipStream_t stream) {
  if (f64)
    hipLaunchKernelGGL((sb_count_kernel<G, double>), dim3(sb_grid(n_sim, G)), dim3(SB_BLOCK), 0, stream, indptr, indices, n, nnz, pairs,
                       n_sim, static_cast<const double*>(row_total), counts, static_cast<double*>(total_sim), flags);
  else
    hipLaunchKernelGGL((sb_count_kernel<G, float>), dim3(sb_grid(n_sim, G)), dim3(SB_BLOCK), 0, stream, indptr, indices, n, nnz, pairs,
                       n_sim, static_cast<const float*>(row_total), counts, static_cast<float*>(total_sim), flags);
}

template <int G>
void sb_launch_fill(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t nnz, const int32_t* pairs,
                    int64_t n_sim, const int64_t* out_indptr, int64_t out_nnz, int32_t* out_indices, float* out_data,
                    unsigned int* flags, hipStream_t stream) {
  hipLaunchKernelGGL((sb_fill_kernel<G>), dim3(sb_grid(n_sim, G)), dim3(SB_BLOCK), 0, stream, indptr, indices, data, n, nnz, pairs, n_sim,
                     out_indptr, out_nnz, out_indices, out_data, flags);
}

template <int G>
void sb_launch_scores(const int32_t* idx, int64_t n_all, int k, int n_obs, double rho, double r, double se_rho, int32_t* n_sim_neigh,
                      double* score, double* score_err, hipStream_t stream) {
  hipLaunchKernelGGL((sb_scores_kernel<G>), dim3(sb_grid(n_all, G)), dim3(SB_BLOCK), 0, stream, idx, n_all, k, n_obs, rho, r, se_rho,
                     n_sim_neigh, score, score_err);
}

// the checks both phases share; `what` names the entry point
int sb_check_pairs(const char* what, const int64_t* indptr, const int32_t* indices, int64_t n, int64_t g, int64_t nnz,
                   const int32_t* pairs, int64_t n_sim) {
  SCAMD_REQUIRE(indptr && n >= 0 && g >= 0 && nnz >= 0 && n_sim >= 0 && (nnz == 0 || indices) && (n_sim == 0 || pairs), SCAMD_EINVAL,
                "%s: null pointer or negative size", what);
  SCAMD_REQUIRE(n < ((int64_t)1 << 31) && g < ((int64_t)1 << 31) && n_sim < ((int64_t)1 << 31), SCAMD_EUNSUPPORTED,
                "%s: n = %lld, g = %lld, n_sim = %lld: each must be below 2^31", what, (long long)n, (long long)g, (long long)n_sim);
  SCAMD_REQUIRE(n > 0 || n_sim == 0, SCAMD_EINVAL, "%s: %lld pairs of a matrix without rows", what, (long long)n_sim);
  return SCAMD_OK;
}

}  // namespace
}  // namespace scamd

using namespace scamd;

extern "C" size_t scamd_pp_scrublet_workspace_bytes(int64_t n_sim) {
  if (n_sim < 0) return 0;
  return sb_carve(nullptr, 0, n_sim).bytes;
}

extern "C" int scamd_pp_scrublet_pair_count(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t g, int64_t nnz,
                                            const int32_t* pairs, int64_t n_sim, const void* row_total, int row_total_is_f64,
                                            int64_t* out_indptr, void* total_sim, uint32_t* flags, int64_t* out_nnz, void* workspace,
                                            size_t workspace_bytes, scamd_stream_t stream) {
  const int rc = sb_check_pairs("pp_scrublet_pair_count", indptr, indices, n, g, nnz, pairs, n_sim);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(out_indptr && flags && out_nnz && (n_sim == 0 || (row_total && total_sim)), SCAMD_EINVAL,
                "pp_scrublet_pair_count: null pointer");
  const ScrubletWorkspace ws = sb_carve(workspace, workspace_bytes, n_sim);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EINVAL, "pp_scrublet_pair_count: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes);
  SCAMD_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(uint32_t), stream));
  if (n_sim > 0) {
    const bool f64 = row_total_is_f64 != 0;
    switch (sb_lanes_per_row(n, nnz)) {
      case 8: sb_launch_count<8>(indptr, indices, n, nnz, pairs, n_sim, row_total, f64, ws.counts, total_sim, flags, stream); break;
      case 16: sb_launch_count<16>(indptr, indices, n, nnz, pairs, n_sim, row_total, f64, ws.counts, total_sim, flags, stream); break;
      case 32: sb_launch_count<32>(indptr, indices, n, nnz, pairs, n_sim, row_total, f64, ws.counts, total_sim, flags, stream); break;
      default: sb_launch_count<64>(indptr, indices, n, nnz, pairs, n_sim, row_total, f64, ws.counts, total_sim, flags, stream); break;
    }
    SCAMD_LAUNCH_CHECK();
  }
  const int src = exclusive_scan_i32_i64(ws.counts, n_sim, out_indptr, ws.block_tmp, stream);
  if (src != SCAMD_OK) return src;
  SCAMD_READBACK_NOW(out_nnz, out_indptr + n_sim, sizeof(int64_t), stream);
  return SCAMD_OK;
}

extern "C" int scamd_pp_scrublet_pair_fill_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                               int64_t nnz, const int32_t* pairs, int64_t n_sim, const int64_t* out_indptr,
                                               int64_t out_nnz, int32_t* out_indices, float* out_data, uint32_t* flags,
                                               scamd_stream_t stream) {
  const int rc = sb_check_pairs("pp_scrublet_pair_fill", indptr, indices, n, g, nnz, pairs, n_sim);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(out_indptr && flags && out_nnz >= 0 && (nnz == 0 || data) && (out_nnz == 0 || (out_indices && out_data)), SCAMD_EINVAL,
                "pp_scrublet_pair_fill: null pointer or negative size");
  SCAMD_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(uint32_t), stream));
  if (n_sim == 0) return SCAMD_OK;
  switch (sb_lanes_per_row(n, nnz)) {
    case 8: sb_launch_fill<8>(indptr, indices, data, n, nnz, pairs, n_sim, out_indptr, out_nnz, out_indices, out_data, flags, stream); break;
    case 16: sb_launch_fill<16>(indptr, indices, data, n, nnz, pairs, n_sim, out_indptr, out_nnz, out_indices, out_data, flags, stream); break;
    case 32: sb_launch_fill<32>(indptr, indices, data, n, nnz, pairs, n_sim, out_indptr, out_nnz, out_indices, out_data, flags, stream); break;
    default: sb_launch_fill<64>(indptr, indices, data, n, nnz, pairs, n_sim, out_indptr, out_nnz, out_indices, out_data, flags, stream); break;
  }
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

extern "C" int scamd_scrublet_scores_f64(const int32_t* idx, int64_t n_all, int32_t k, int64_t n_obs, double rho, double r, double se_rho,
                                         int32_t* n_sim_neigh, double* score, double* score_err, scamd_stream_t stream) {
  SCAMD_REQUIRE(n_all >= 0 && k >= 1 && n_obs >= 0 && n_obs <= n_all && (n_all == 0 || (idx && n_sim_neigh && score && score_err)),
                SCAMD_EINVAL, "scrublet_scores: null pointer, negative size, k < 1 or n_obs > n_all");
  SCAMD_REQUIRE(n_all < ((int64_t)1 << 31), SCAMD_EUNSUPPORTED, "scrublet_scores: n_all = %lld, must be below 2^31", (long long)n_all);
  if (n_all == 0) return SCAMD_OK;
  const int no = (int)n_obs;
  switch (sb_score_lanes(k)) {
    case 8: sb_launch_scores<8>(idx, n_all, k, no, rho, r, se_rho, n_sim_neigh, score, score_err, stream); break;
    case 16: sb_launch_scores<16>(idx, n_all, k, no, rho, r, se_rho, n_sim_neigh, score, score_err, stream); break;
    case 32: sb_launch_scores<32>(idx, n_all, k, no, rho, r, se_rho, n_sim_neigh, score, score_err, stream); break;
    default: sb_launch_scores<64>(idx, n_all, k, no, rho, r, se_rho, n_sim_neigh, score, score_err, stream); break;
  }
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}
