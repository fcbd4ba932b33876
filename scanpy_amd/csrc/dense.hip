// Dense float64 side of the PCA: top-k eigenpairs of the g x g covariance-like matrix A = X^T X - n mu mu^T.
//
// Replaces, for the Gram route of sc.pp.pca, what sklearn's PCA(svd_solver='arpack') gets from ARPACK
// (sklearn/decomposition/_pca.py:704-793 as called at src/scanpy/preprocessing/_pca/__init__.py:287-308) and what the
// reference's own covariance route gets from `eigh` (src/scanpy/preprocessing/_pca/_dask.py:28-132): round 1 ran this
// part through torch.linalg (rocBLAS GEMMs + ~100 small rocSOLVER kernels, ~10 ms at g = 2000, 6 of them in six
// 128 x 128 `eigh` calls).  Here every piece is a hand-written gfx950 kernel:
//   * tall-skinny GEMMs (g x g x 128, 128 x 128 x g) on the float64 matrix cores, v_mfma_f64_16x16x4_f64: one kernel,
//     C = alpha P^T Q + beta1 D1 + beta2 D2 with P, Q stored k-major, so that both operand fragments are 128-byte
//     coalesced rows (A is symmetric: A Z = A^T Z); 32 x 32 output tile per workgroup, the K range split over its four
//     waves and reduced through LDS in a fixed order (bitwise reproducible);
//   * CholeskyQR of a g x 128 block = Gram matrix (same GEMM) + one-workgroup 128 x 128 Cholesky / triangular inverse in
//     LDS + a panel-times-small product; twice (CholeskyQR2), shifted on a failed pivot;
//   * the 128 x 128 Rayleigh-Ritz eigenproblem by one-sided (Hestenes) Jacobi in ONE workgroup, matrix resident in LDS
//     (133 KB of the 160): 64 disjoint column pairs per step, 16 lanes per pair, round-robin ordering;
//   * Chebyshev-filtered subspace iteration (Zhou & Saad) around them: the filter steps are the GEMM with the
//     three-term recurrence in its epilogue.  The steps (CholeskyQR2, Rayleigh-Ritz, degree rule, filter) are written once over
//     an operator in subspace.h; this file holds the two operators and their drivers.
// Contents, in order: the float64 kernels (GEMM, Cholesky factor, panel x small, Jacobi, residuals, model finalisation);
// `DenseOp` + `dense_topk` (scamd_eigh_topk_f64, scamd_dense_debug_f64); the batched, deflated solve and the dense half of the
// Gram-route PCA (scamd_pca_solve_gram_f64, scamd_pca_csr_f32); the sp_* kernels, `SpectralOp` and the spectral
// initialisation of the UMAP layout (scamd_spectral_embedding_f32); `DiffmapOp` and the diffusion-map entries
// (scamd_transitions_sym_f32, scamd_diffmap_f32, scamd_dpt_pseudotime_f32).
// Algorithmic work at g = 2000, b = 128: 2 g^2 b = 1.0e9 flop per operator application (~13 us at the 78.6 TFLOP/s
// float64 matrix peak), ~11-26 applications; everything else is O(g b^2) or O(b^3).
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace scamd {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int DB_MAX = 128;      // largest block size / Jacobi dimension
constexpr int DB_LD = DB_MAX + 2;  // LDS column stride (doubles): 1040 B, not a multiple of the 256-B bank period
constexpr int DENSE_BATCH_HOST = DB_MAX - 32;  // eigenpairs per batch of the deflated solve (dense_topk_batched)
constexpr int GEMM_KB = 8;       // k-steps (of 4) whose operands a GEMM wave fetches in one batch

__device__ __forceinline__ unsigned int dhash32(unsigned int x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// Cross-lane float64 through DPP (one VALU move per dword, no LDS crossbar round trip as with ds_bpermute):
// CTRL = DPP control word: 0x120 + n = row_ror:n (rotate within a row of 16 lanes), 0xB1 = quad_perm [1,0,3,2],
// 0x4E = quad_perm [2,3,0,1], 0x141 = row_half_mirror (lane i <-> 7 - i within 8).
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// sum over the 16 lanes of a DPP row, result in every lane
__device__ __forceinline__ double row16_sum(double x) {
  x += dpp_f64<0x128>(x);
  x += dpp_f64<0x124>(x);
  x += dpp_f64<0x122>(x);
  x += dpp_f64<0x121>(x);
  return x;
}
// sum over aligned groups of 8 lanes, result in every lane
__device__ __forceinline__ double oct_sum(double x) {
  x += dpp_f64<0xB1>(x);
  x += dpp_f64<0x4E>(x);
  x += dpp_f64<0x141>(x);
  return x;
}

// ---------------------------------------------------------------------------------------------------------------------
// C[M x N] = alpha * sum_k P[k][m] Q[k][n] + beta1 * D1[m][n] + beta2 * D2[m][n]     (float64, MFMA 16x16x4)
// P: [K x ldp], Q: [K x ldq] row-major (k-major).  grid (ceil(M/32), ceil(N/32)), 512 threads: wave w owns the
// w-th eighth of K and the whole 32 x 32 tile (2 x 2 MFMA tiles); the eight partial tiles are summed in a fixed order.
// MFMA operand layout (v_mfma_f64_16x16x4_f64): A fragment lane l = A[i = l & 15][k = l >> 4], B fragment lane l =
// B[k = l >> 4][j = l & 15], accumulator register v of lane l = D[i = (l >> 4) + 4 v][j = l & 15] (NOT the
// 4 (l >> 4) + v of the float32 16x16x4 instruction; pinned by tests/test_gpu_dense.py::test_dgemm_tn).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void dgemm_tn_kernel(const double* __restrict__ P, int64_t ldp,
                                                       const double* __restrict__ Q, int64_t ldq, int M, int N, int K,
                                                       double alpha, const double* __restrict__ D1, int64_t ldd1,
                                                       double beta1, const double* __restrict__ D2, int64_t ldd2,
                                                       double beta2, double* __restrict__ C, int64_t ldc) {
  __shared__ double red[8][32 * 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int kc = ((K + 7) / 8 + 3) / 4 * 4;  // K range of a wave (eight of them), a multiple of 4
  const int kb = wave * kc, ke = min(K, kb + kc);
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[a][b][v] = 0.0;
  const bool mv0 = m0 + l15 < M, mv1 = m0 + 16 + l15 < M;
  const bool nv0 = n0 + l15 < N, nv1 = n0 + 16 + l15 < N;
  // Every load is unconditional, on an address clamped into the matrix; a lane outside the tile or the K range gets its zero
  // where the operand is USED.  The raw operands of GEMM_KB k-steps are fetched together and the next batch is requested before
  // this one is consumed: K / 32 / GEMM_KB memory round trips per wave instead of K / 32 (one load per wait).
  const double* pp0 = P + min(m0 + l15, M - 1);
  const double* pp1 = P + min(m0 + 16 + l15, M - 1);
  const double* qq0 = Q + min(n0 + l15, N - 1);
  const double* qq1 = Q + min(n0 + 16 + l15, N - 1);
  const int nsteps = ke > kb ? (ke - kb + 3) >> 2 : 0;
  double ca0[GEMM_KB], ca1[GEMM_KB], cb0[GEMM_KB], cb1[GEMM_KB];
  double na0[GEMM_KB], na1[GEMM_KB], nb0[GEMM_KB], nb1[GEMM_KB];
  if (nsteps > 0) {
#pragma unroll
    for (int j = 0; j < GEMM_KB; ++j) {
      const int64_t kk = min(kb + 4 * j + kq, K - 1);
      ca0[j] = pp0[kk * ldp];
      ca1[j] = pp1[kk * ldp];
      cb0[j] = qq0[kk * ldq];
      cb1[j] = qq1[kk * ldq];
    }
  }
  for (int s0 = 0; s0 < nsteps; s0 += GEMM_KB) {
    const bool more = s0 + GEMM_KB < nsteps;
    if (more) {
#pragma unroll
      for (int j = 0; j < GEMM_KB; ++j) {
        const int64_t kk = min(kb + 4 * (s0 + GEMM_KB + j) + kq, K - 1);
        na0[j] = pp0[kk * ldp];
        na1[j] = pp1[kk * ldp];
        nb0[j] = qq0[kk * ldq];
        nb1[j] = qq1[kk * ldq];
      }
    }
#pragma unroll
    for (int j = 0; j < GEMM_KB; ++j) {
      if (s0 + j < nsteps) {  // (uniform; a skipped step adds nothing, not a zero: the sums keep their bits)
        const bool kv = kb + 4 * (s0 + j) + kq < ke;
        const double a0 = (kv && mv0) ? ca0[j] : 0.0;
        const double a1 = (kv && mv1) ? ca1[j] : 0.0;
        const double b0 = (kv && nv0) ? cb0[j] : 0.0;
        const double b1 = (kv && nv1) ? cb1[j] : 0.0;
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < GEMM_KB; ++j) {
        ca0[j] = na0[j];
        ca1[j] = na1[j];
        cb0[j] = nb0[j];
        cb1[j] = nb1[j];
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 4; ++v) red[wave][(16 * a + kq + 4 * v) * 32 + 16 * b + l15] = acc[a][b][v];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = threadIdx.x + 512 * j;
    const int r = idx >> 5, c = idx & 31;
    const int m = m0 + r, n = n0 + c;
    if (m < M && n < N) {
      double s = (((red[0][idx] + red[1][idx]) + (red[2][idx] + red[3][idx])) +
                  ((red[4][idx] + red[5][idx]) + (red[6][idx] + red[7][idx])));
      s *= alpha;
      if (D1) s += beta1 * D1[(int64_t)m * ldd1 + n];
      if (D2) s += beta2 * D2[(int64_t)m * ldd2 + n];
      C[(int64_t)m * ldc + n] = s;
    }
  }
}

static int dgemm_tn(hipStream_t s, const double* P, int64_t ldp, const double* Q, int64_t ldq, int M, int N, int K,
                    double alpha, const double* D1, int64_t ldd1, double beta1, const double* D2, int64_t ldd2,
                    double beta2, double* C, int64_t ldc) {
  hipLaunchKernelGGL(dgemm_tn_kernel, dim3((M + 31) / 32, (N + 31) / 32), dim3(512), 0, s, P, ldp, Q, ldq, M, N, K,
                     alpha, D1, ldd1, beta1, D2, ldd2, beta2, C, ldc);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Cholesky of the column-normalised Gram matrix + the factor CholeskyQR applies, one workgroup, matrix in LDS.
//   in : G [b x b] (ld b) = Z^T Z, shift >= 0 (relative, added to the unit diagonal)
//   out: S [b x b] row-major with Z_new = Z S orthonormal: S = D^-1 L^-T, D = sqrt(diag G), L L^T = D^-1 G D^-1 + shift I
//        flag: 1 if a pivot was not positive (S is then garbage)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void chol_factor_kernel(const double* __restrict__ G, int b, double shift,
                                                           double* __restrict__ S, int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) double sm[];  // L [b][DB_LD] (row-major, padded) + dinv[b]
  double* L = sm;
  double* dinv = sm + DB_MAX * DB_LD;
  const int tid = threadIdx.x;
  const int row = tid >> 3, part = tid & 7;  // 128 rows x 8 partial sums
  for (int j = tid; j < b; j += 1024) {
    const double d = G[(int64_t)j * b + j];
    dinv[j] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < b * b; e += 1024) {
    const int i = e / b, j = e - i * b;
    double v = G[(int64_t)i * b + j] * dinv[i] * dinv[j];
    if (i == j) v = (dinv[i] > 0.0 ? 1.0 : 0.0) + shift;
    L[i * DB_LD + j] = v;
  }
  __syncthreads();
  // left-looking Cholesky, column j from the finished columns: L[i][j] = (A[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j];
  // the dot products of all rows i >= j run at once, eight lanes each (reduced through DPP).  A lane reads four elements of
  // either row per wait (index clamped to k < j, the term dropped where it is not part of the sum) and adds them in the order k = part,
  // part + 8, ... as a one-read-per-wait loop would.
  bool bad = false;
  __shared__ double sh_piv[2], sh_root[2];
  for (int j = 0; j < b; ++j) {
    double acc = 0.0;
    const bool mine = row >= j && row < b;
    double ljj = 0.0;
    if (mine) {
      const double* lr = L + row * DB_LD;
      const double* lj = L + j * DB_LD;
      ljj = lr[j];
      for (int k0 = part; k0 < j; k0 += 32) {
        double x[4], y[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int kk = min(k0 + 8 * t, j - 1);  // (inside the finished columns: nothing this step writes is read)
          x[t] = lr[kk];
          y[t] = lj[kk];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (k0 + 8 * t < j) acc = fma(x[t], y[t], acc);
      }
    }
    acc = oct_sum(acc);
    const double v = mine ? ljj - acc : 0.0;
    if (row == j && part == 0) {  // the pivot's owner takes its root once, for everybody
      sh_piv[j & 1] = v;
      sh_root[j & 1] = sqrt(v);
    }
    __syncthreads();
    const double piv = sh_piv[j & 1];
    if (!(piv > 0.0)) {  // uniform: every thread reads the same pivot
      bad = true;
      break;
    }
    const double root = sh_root[j & 1];
    if (mine && part == 0) L[row * DB_LD + j] = (row == j) ? root : v / root;
    __syncthreads();  // column j is final before the next column's dot products read it
  }
  if (tid == 0) *flag = bad ? 1 : 0;  // (written either way: no clear in front of the launch)
  if (bad) return;
  // X = L^-1 (lower triangular), row by row: X[j][c] = (delta_jc - sum_{c <= k < j} L[j][k] X[k][c]) / L[j][j] for all
  // columns c <= j at once (thread group `row` = c, eight lanes split k).  X[k][c] (k > c) lives in the unused UPPER
  // triangle at (c, k); X[c][c] = 1 / L[c][c].
  {
    const int c = row;
    const double xcc = c < b ? 1.0 / L[c * DB_LD + c] : 0.0;
    for (int j = 1; j < b; ++j) {
      double acc = 0.0, pivot = 1.0;
      if (c < j) {
        const double* lj = L + j * DB_LD;
        const double* lc = L + c * DB_LD;
        const double ljc = lj[c], ljj = lj[j];
        for (int k0 = c + 1 + part; k0 < j; k0 += 32) {
          double x[4], y[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int kk = min(k0 + 8 * t, j - 1);  // (never L[c][j], which this step writes)
            x[t] = lj[kk];
            y[t] = lc[kk];
          }
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (k0 + 8 * t < j) acc = fma(x[t], y[t], acc);
        }
        if (part == 0) acc = fma(ljc, xcc, acc);
        pivot = ljj;
      }
      acc = oct_sum(acc);
      if (c < j && part == 0) L[c * DB_LD + j] = -acc / pivot;
      __syncthreads();
    }
  }
  // S[k][n] = X[n][k] * dinv[k] for n >= k, 0 below the diagonal
  for (int e = tid; e < b * b; e += 1024) {
    const int k = e / b, n = e - k * b;
    double v = 0.0;
    if (n == k) v = 1.0 / L[k * DB_LD + k];
    else if (n > k) v = L[k * DB_LD + n];
    S[e] = v * dinv[k];
  }
}

// C[g x bo] = Z[g x b] S[b x bo] (plain FMA: O(g b^2), 1/16 of a GEMM application), and with gridDim.y = 2 a second panel by the
// same S (C1 = Z1 S: the two products of a Rayleigh-Ritz).  S is staged in LDS ONCE per workgroup, row stride W = 4 << cq_shift
// >= bo with zeros beyond bo, by loads issued PANEL_SB at a time with the next batch requested before this one is stored; the k
// loop then reads LDS only (it read S from global memory behind three bounds guards, one L2 round trip per k).  256 threads =
// (256 >> cq_shift) row groups x (1 << cq_shift) column quads, two rows per thread: 16 rows per workgroup at bo = 128, 256 at
// bo = 8 (the spectral caller: 1M rows, where 8 rows per workgroup left 16 of 256 threads with work).  Every output element is
// still fma(z_k, s_k, c) over k = 0 .. b-1 from c = 0.  Needs b <= W (the Z tile is sized for it) and bo <= DB_MAX.
constexpr int PANEL_SB = 8;  // S elements per thread and batch
constexpr int panel_lds_doubles(int b, int cq_shift) {
  return b * (4 << cq_shift) + 2 * (256 >> cq_shift) * (b | 1);
}
__global__ __launch_bounds__(256) void panel_small_kernel(const double* __restrict__ Z0, const double* __restrict__ Z1,
                                                          const double* __restrict__ S, int g, int b, int bo, int cq_shift,
                                                          double* __restrict__ C0, double* __restrict__ C1) {
  extern __shared__ __attribute__((aligned(16))) double sm[];  // S [b][W], then the Z rows [rows][zld]
  const int tid = threadIdx.x;
  const int W = 4 << cq_shift, rpp = 256 >> cq_shift, rows = 2 * rpp;
  const int zld = b | 1;  // odd: the row groups of a wave read different banks
  double* Ss = sm;
  double* Zs = sm + b * W;
  const double* __restrict__ Z = blockIdx.y ? Z1 : Z0;
  double* __restrict__ C = blockIdx.y ? C1 : C0;
  const int m0 = blockIdx.x * rows;
  // the Z rows of this workgroup: contiguous in memory, rows * b <= 2048 elements, one batch
  {
    double zv[8];
    const int zcount = rows * b;
    const int64_t zlast = (int64_t)g * b - 1;
#pragma unroll
    for (int u = 0; u < 8; ++u) zv[u] = Z[min((int64_t)m0 * b + tid + 256 * u, zlast)];
    const int scount = b * W;
    const int wmask = W - 1, wshift = cq_shift + 2;
    double cur[PANEL_SB], nxt[PANEL_SB];
#pragma unroll
    for (int u = 0; u < PANEL_SB; ++u) {
      const int e = tid + 256 * u;
      cur[u] = S[min(e >> wshift, b - 1) * bo + min(e & wmask, bo - 1)];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = tid + 256 * u;
      if (e < zcount) {
        const int r = e / b;
        Zs[r * zld + (e - r * b)] = (m0 + r < g) ? zv[u] : 0.0;
      }
    }
    for (int e0 = 0; e0 < scount; e0 += 256 * PANEL_SB) {
      const bool more = e0 + 256 * PANEL_SB < scount;
      if (more) {
#pragma unroll
        for (int u = 0; u < PANEL_SB; ++u) {
          const int e = e0 + 256 * PANEL_SB + tid + 256 * u;
          nxt[u] = S[min(e >> wshift, b - 1) * bo + min(e & wmask, bo - 1)];
        }
      }
#pragma unroll
      for (int u = 0; u < PANEL_SB; ++u) {
        const int e = e0 + tid + 256 * u;
        if (e < scount) Ss[e] = ((e & wmask) < bo) ? cur[u] : 0.0;
      }
      if (more) {
#pragma unroll
        for (int u = 0; u < PANEL_SB; ++u) cur[u] = nxt[u];
      }
    }
  }
  __syncthreads();
  const int cq = tid & ((1 << cq_shift) - 1), rg = tid >> cq_shift;
  const double* sp = Ss + 4 * cq;
  const double* z0 = Zs + rg * zld;
  const double* z1 = Zs + (rg + rpp) * zld;
  double c0[4] = {0.0, 0.0, 0.0, 0.0}, c1[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
  for (int k = 0; k < b; ++k) {
    const double za = z0[k], zb = z1[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double sv = sp[k * W + j];
      c0[j] = fma(za, sv, c0[j]);
      c1[j] = fma(zb, sv, c1[j]);
    }
  }
  const int n0 = 4 * cq;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (n0 + j < bo) {
      if (m0 + rg < g) C[(int64_t)(m0 + rg) * bo + n0 + j] = c0[j];
      if (m0 + rg + rpp < g) C[(int64_t)(m0 + rg + rpp) * bo + n0 + j] = c1[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Eigen-decomposition of a symmetric b x b matrix (b <= 128) by one-sided Jacobi, one workgroup of 512 threads.
// W = T (columns in LDS); rotations orthogonalise the columns: at convergence W = T Y with Y orthogonal, column i =
// theta_i y_i.  64 disjoint pairs per step (round-robin tournament), 8 lanes per pair.  Output: theta[b] descending by
// |theta| (the sign is recovered from y^T T y = sign * |W_i|), Y [b x b] row-major, column j = eigenvector j.
// ---------------------------------------------------------------------------------------------------------------------
// The sweeps of the kernel below for b in (8 NJ - 8, 8 NJ]: a lane holds its NJ elements of both columns of its pair in
// registers for the whole step -- every LDS read of the step is issued at once, the three dot products and the rotation work on
// registers, the rotated values are written back (a loop over b read two elements per wait, twice per step, 2 x b / 8 serial LDS
// round trips).  Only the last element of a lane can lie beyond b; its terms are left out of the sums, as before.
template <int NJ>
__device__ __forceinline__ int jacobi_sweeps(double* W, float* off_arr, int b, int n2, int tid) {
  // 64 groups of 8 lanes, one column pair each.  The kernel is bound by the instruction THROUGHPUT of its one CU (every
  // lane of a group repeats the rotation's scalar arithmetic): eight lanes per pair instead of sixteen halves the
  // redundant work per SIMD, the rotation is computed with two rsqrt and no division, the reductions run on DPP.
  const int grp = tid >> 3, t8 = tid & 7;
  const int nm1 = n2 - 1;
  const bool last_in = t8 + 8 * (NJ - 1) < b;
  int sweep = 0;
  for (; sweep < 30; ++sweep) {
    float my_off = 0.f;  // (no shared counter inside the step loop: 64 same-address LDS atomics per step serialise)
    // round-robin tournament: player n2-1 stays, the others rotate; group g > 0 plays (step + g, step - g) mod (n2 - 1)
    int p = grp == 0 ? nm1 : grp % nm1;
    int q = grp == 0 ? 0 : (nm1 - grp % nm1) % nm1;
    for (int step = 0; step < nm1; ++step) {
      const bool act = grp < n2 / 2 && p < b && q < b;
      if (act) {
        double* wp = W + p * DB_LD + t8;
        double* wq = W + q * DB_LD + t8;
        double x[NJ], y[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {  // (t8 + 8 j < 8 NJ <= DB_MAX < DB_LD: inside the column)
          x[j] = wp[8 * j];
          y[j] = wq[8 * j];
        }
        double a = 0.0, bb = 0.0, c = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if (j < NJ - 1 || last_in) {
            a = fma(x[j], x[j], a);
            bb = fma(y[j], y[j], bb);
            c = fma(x[j], y[j], c);
          }
        }
        a = oct_sum(a);
        bb = oct_sum(bb);
        c = oct_sum(c);
        const double ab = a * bb;
        if (c * c > 1e-30 * ab) {  // |c| / sqrt(a bb) > 1e-15
          // rotation by theta with tan(2 theta) = 2c / (bb - a): cos(2 theta) = |d| / r, r = hypot(d, 2c)
          const double d = bb - a, tau = 2.0 * c;
          const double inv_r = rsqrt(fma(d, d, tau * tau));
          const double h = fma(0.5 * fabs(d), inv_r, 0.5);  // cos^2 of the smaller angle
          const double inv_cs = rsqrt(h);
          const double cs = h * inv_cs;
          const double sn = (d >= 0.0 ? 0.5 : -0.5) * tau * inv_r * inv_cs;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            if (j < NJ - 1 || last_in) {
              wp[8 * j] = cs * x[j] - sn * y[j];
              wq[8 * j] = sn * x[j] + cs * y[j];
            }
          }
          my_off = fmaxf(my_off, (float)(fabs(c) * rsqrt(ab)));
        }
      }
      if (grp != 0) {
        p = p + 1 == nm1 ? 0 : p + 1;
        q = q + 1 == nm1 ? 0 : q + 1;
      } else {
        q = step + 1;
      }
      __syncthreads();
    }
    if (t8 == 0) off_arr[grp] = my_off;
    __syncthreads();
    float off = 0.f;
    for (int i = 0; i < 64; ++i) off = fmaxf(off, off_arr[i]);
    __syncthreads();  // everybody has the sweep's maximum before the next sweep overwrites the array
    // `off` is the largest |cos| the sweep MET, before its rotations: every pair above 1e-15 was rotated in this very sweep, and
    // Jacobi converges quadratically -- a sweep that met nothing above 1e-8 leaves ~1e-16.  (1e-13 until round 6: one more sweep,
    // 0.15 ms of the solve, whose only work was to see that.)
    if (off < 1e-8f) {
      ++sweep;
      break;
    }
  }
  return sweep;
}

// `symmetrize`: W is loaded as (T + T^T) / 2 (the Rayleigh-Ritz matrix is symmetric up to rounding; a launch of its own did this)
__global__ __launch_bounds__(512) void jacobi_eigh_kernel(const double* __restrict__ T, int b, int symmetrize,
                                                          double* __restrict__ theta, double* __restrict__ Y,
                                                          int* __restrict__ sweeps_out) {
  extern __shared__ __attribute__((aligned(16))) double sm[];  // W [n2][DB_LD] column-major: W[c * DB_LD + i]
  double* W = sm;
  double* nrm = sm + DB_MAX * DB_LD;  // [DB_MAX]
  __shared__ float off_arr[64];  // per group: largest |cos| between two columns it met in the sweep
  __shared__ int rank_of[DB_MAX];
  const int tid = threadIdx.x;
  const int n2 = (b + 1) & ~1;  // even number of players (a padding column of zeros never rotates)
  for (int e0 = tid; e0 < n2 * DB_LD; e0 += 512 * 4) {  // (four elements per wait, clamped addresses)
    double t1[4], t2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + 512 * u;
      const int c = min(e / DB_LD, b - 1), i = min(e % DB_LD, b - 1);
      t1[u] = T[(int64_t)i * b + c];
      t2[u] = T[(int64_t)(symmetrize ? c : i) * b + (symmetrize ? i : c)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + 512 * u;
      const int c = e / DB_LD, i = e - c * DB_LD;
      if (e < n2 * DB_LD) W[e] = (c < b && i < b) ? ((symmetrize && i != c) ? 0.5 * (t1[u] + t2[u]) : t1[u]) : 0.0;
    }
  }
  __syncthreads();
  const int grp = tid >> 3, t8 = tid & 7;
  int sweep = 0;
  // A compile-time element count per lane: the step is straight-line code on registers.  Sixteen instances make the kernel 43 KB
  // of code; a launch runs ONE of them (2-3 KB of loop: 11 elements at b = 82, 1 at the spectral b = 8), so the instruction
  // cache holds what runs.  b > DB_MAX has no instance and no room in LDS: the entry points refuse it before the launch.
  switch ((b + 7) >> 3) {
#define SCAMD_JACOBI_CASE(NJ) case NJ: sweep = jacobi_sweeps<NJ>(W, off_arr, b, n2, tid); break;
    SCAMD_JACOBI_CASE(1) SCAMD_JACOBI_CASE(2) SCAMD_JACOBI_CASE(3) SCAMD_JACOBI_CASE(4)
    SCAMD_JACOBI_CASE(5) SCAMD_JACOBI_CASE(6) SCAMD_JACOBI_CASE(7) SCAMD_JACOBI_CASE(8)
    SCAMD_JACOBI_CASE(9) SCAMD_JACOBI_CASE(10) SCAMD_JACOBI_CASE(11) SCAMD_JACOBI_CASE(12)
    SCAMD_JACOBI_CASE(13) SCAMD_JACOBI_CASE(14) SCAMD_JACOBI_CASE(15) SCAMD_JACOBI_CASE(16)
#undef SCAMD_JACOBI_CASE
    default: break;
  }
  // column norms, ranks (descending norm, ties by index)
  if (tid < n2) {
    double a = 0.0;
#pragma unroll 8
    for (int i = 0; i < b; ++i) a = fma(W[tid * DB_LD + i], W[tid * DB_LD + i], a);
    nrm[tid] = tid < b ? sqrt(a) : -1.0;
  }
  __syncthreads();
  if (tid < b) {
    int r = 0;
    const double me = nrm[tid];
    for (int j = 0; j < b; ++j) r += (nrm[j] > me || (nrm[j] == me && j < tid)) ? 1 : 0;
    rank_of[tid] = r;
  }
  __syncthreads();
  // W_c = T y_c = theta_c y_c at convergence: theta_c = |W_c| (T is positive semi-definite: the Rayleigh-Ritz matrix
  // of a covariance), y_c = W_c / |W_c|
  for (int c = grp; c < b; c += 64) {
    const double nv = nrm[c];
    const double inv = nv > 0.0 ? 1.0 / nv : 0.0;
    const int r = rank_of[c];
    if (t8 == 0) theta[r] = nv;
    for (int i = t8; i < b; i += 8) Y[(int64_t)i * b + r] = W[c * DB_LD + i] * inv;
  }
  if (tid == 0 && sweeps_out) *sweeps_out = sweep;
}

// ---------------------------------------------------------------------------------------------------------------------
// small element-wise / reduction kernels
// ---------------------------------------------------------------------------------------------------------------------
// Z[g x b] <- standard normal, counter-based (Box-Muller on two hashes of (seed, element))
__global__ void randn_kernel(double* __restrict__ z, int64_t count, unsigned int seed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const unsigned int h1 = dhash32((unsigned int)i * 0x9E3779B1u + seed);
  const unsigned int h2 = dhash32(h1 ^ 0x85EBCA77u ^ (unsigned int)(i >> 32));
  const double u1 = ((double)h1 + 0.5) * (1.0 / 4294967296.0), u2 = ((double)h2 + 0.5) * (1.0 / 4294967296.0);
  z[i] = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// y = a x1 + b x2 (element-wise)
__global__ void axpby_kernel(int64_t count, double a, const double* __restrict__ x1, double b,
                             const double* __restrict__ x2, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) y[i] = a * x1[i] + b * x2[i];
}

// Rayleigh quotients t_j = z_j^T (A z_j) of an orthonormal block: out[1] = min_j t_j, out[2] = max_j t_j (one workgroup)
__global__ __launch_bounds__(1024) void rq_minmax_kernel(const double* __restrict__ Z, const double* __restrict__ AZ, int g,
                                                         int b, double* __restrict__ out) {
  __shared__ double part[8][DB_MAX];
  const int c = threadIdx.x & 127, rr = threadIdx.x >> 7;
  double s = 0.0;
  if (c < b) {  // (four independent chains: the loop is a walk of dependent loads otherwise, 76 us at g = 2000)
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int m = rr;
    for (; m + 24 < g; m += 32) {
      s = fma(Z[(int64_t)m * b + c], AZ[(int64_t)m * b + c], s);
      s1 = fma(Z[(int64_t)(m + 8) * b + c], AZ[(int64_t)(m + 8) * b + c], s1);
      s2 = fma(Z[(int64_t)(m + 16) * b + c], AZ[(int64_t)(m + 16) * b + c], s2);
      s3 = fma(Z[(int64_t)(m + 24) * b + c], AZ[(int64_t)(m + 24) * b + c], s3);
    }
    for (; m < g; m += 8) s = fma(Z[(int64_t)m * b + c], AZ[(int64_t)m * b + c], s);
    s = (s + s1) + (s2 + s3);
  }
  part[rr][c] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double mn = INFINITY, mx = -INFINITY;
    for (int j = 0; j < b; ++j) {
      double t = 0.0;
      for (int r = 0; r < 8; ++r) t += part[r][j];
      mn = fmin(mn, t);
      mx = fmax(mx, t);
    }
    out[1] = mn;
    out[2] = mx;
  }
}

// out[0] = max_{j < k} |AV_j - theta_j V_j| / max(theta_0, tiny); one workgroup, fixed order
__global__ __launch_bounds__(1024) void residual_kernel(const double* __restrict__ V, const double* __restrict__ AV,
                                                        const double* __restrict__ theta, int g, int b, int k,
                                                        double* __restrict__ out) {
  __shared__ double part[8][DB_MAX];
  const int c = threadIdx.x & 127, rr = threadIdx.x >> 7;
  double s = 0.0;
  if (c < k) {
    const double th = theta[c];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int m = rr;
    for (; m + 24 < g; m += 32) {  // (four independent chains, see rq_minmax_kernel)
      const double d0 = AV[(int64_t)m * b + c] - th * V[(int64_t)m * b + c];
      const double d1 = AV[(int64_t)(m + 8) * b + c] - th * V[(int64_t)(m + 8) * b + c];
      const double d2 = AV[(int64_t)(m + 16) * b + c] - th * V[(int64_t)(m + 16) * b + c];
      const double d3 = AV[(int64_t)(m + 24) * b + c] - th * V[(int64_t)(m + 24) * b + c];
      s = fma(d0, d0, s);
      s1 = fma(d1, d1, s1);
      s2 = fma(d2, d2, s2);
      s3 = fma(d3, d3, s3);
    }
    for (; m < g; m += 8) {
      const double d = AV[(int64_t)m * b + c] - th * V[(int64_t)m * b + c];
      s = fma(d, d, s);
    }
    s = (s + s1) + (s2 + s3);
  }
  part[rr][c] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double mx = 0.0;
    for (int j = 0; j < k; ++j) {
      double t = 0.0;
      for (int r = 0; r < 8; ++r) t += part[r][j];
      mx = fmax(mx, sqrt(t));
    }
    out[0] = mx / fmax(theta[0], 1e-300);
  }
}

// A[g x g] (float64) = gram_q * inv - n mu mu^T with mu = colsum_q * inv / n (the fixed-point Gram matrix of gram.hip);
// also mean[g] and var[g] (population variance of every column, clamped at 0)
__global__ void cov_from_gram_kernel(const long long* __restrict__ gram, int64_t ld_gram, const long long* __restrict__ colsum,
                                     int g, double inv, double n, int zero_center, double* __restrict__ a,
                                     double* __restrict__ mean, double* __restrict__ var) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)g * g) return;
  const int i = (int)(e / g), j = (int)(e - (int64_t)i * g);
  const double mi = (double)colsum[i] * inv / n, mj = (double)colsum[j] * inv / n;
  // gram is exactly symmetric (integer sums); read the (min, max) entry so that A is symmetric to the bit as well
  const int lo = min(i, j), hi = max(i, j);
  const double gv = (double)gram[(int64_t)lo * ld_gram + hi] * inv;
  a[e] = zero_center ? gv - n * mi * mj : gv;
  if (i == j) {
    mean[i] = mi;
    var[i] = fmax(gv / n - mi * mi, 0.0);
  }
}

// sign convention of sklearn's svd_flip(u_based_decision=False): the largest-|.| loading of a component is positive.
// V [g x b] (first k columns used) -> comp64 [k x g] (row = component), v32 [g x k] float32 for the scores SpMM.
// (k = row stride of v32 = components in all; comp64 / v32 are already offset to this batch's first component)
__global__ __launch_bounds__(256) void finalize_components_kernel(const double* __restrict__ V, int g, int b, int k,
                                                                  double* __restrict__ comp64, float* __restrict__ v32) {
  __shared__ double bv[256];
  __shared__ int bi[256];
  const int c = blockIdx.x;
  double best = -1.0;
  int besti = 0;
  for (int m = threadIdx.x; m < g; m += 256) {
    const double a = fabs(V[(int64_t)m * b + c]);
    if (a > best) {
      best = a;
      besti = m;
    }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = besti;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const double ob = bv[threadIdx.x + o];
      const int oi = bi[threadIdx.x + o];
      if (ob > bv[threadIdx.x] || (ob == bv[threadIdx.x] && oi < bi[threadIdx.x])) {
        bv[threadIdx.x] = ob;
        bi[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  const double sg = V[(int64_t)bi[0] * b + c] < 0.0 ? -1.0 : 1.0;
  for (int m = threadIdx.x; m < g; m += 256) {
    const double v = sg * V[(int64_t)m * b + c];
    comp64[(int64_t)c * g + m] = v;
    if (v32) v32[(int64_t)m * k + c] = (float)v;
  }
}

// shift[c] (float32) = sum_m mean[m] * (double)v32[m][c]  (the projection of the column means: X V - 1 shift^T)
__global__ __launch_bounds__(256) void mean_shift_kernel(const double* __restrict__ mean, const float* __restrict__ v32, int g,
                                                         int k, float* __restrict__ shift, double* __restrict__ proj) {
  __shared__ double part[256];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int m = threadIdx.x; m < g; m += 256) s = fma(mean[m], (double)v32[(int64_t)m * k + c], s);
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += part[i];
    shift[c] = (float)t;
    proj[c] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host orchestration: the steps of the subspace iteration (subspace.h) over the dense operator
// ---------------------------------------------------------------------------------------------------------------------
}  // namespace scamd
#include "subspace.h"
namespace scamd {

struct DenseBuffers {
  double* z[7];  // g x b panels
  SubspaceScratch w;
  double* resid;
};

static void dense_carve(Workspace& ws, int64_t g, int b, DenseBuffers* d) {
  for (int i = 0; i < 7; ++i) d->z[i] = ws.take<double>((size_t)g * b);
  d->w.gm = ws.take<double>((size_t)b * b);
  d->w.smat = ws.take<double>((size_t)b * b);
  d->w.tmat = ws.take<double>((size_t)b * b);
  d->w.ymat = ws.take<double>((size_t)b * b);
  d->w.theta = ws.take<double>((size_t)b + 8);
  d->resid = ws.take<double>(8);
  d->w.flags = ws.take<int>(8);
}

static int dense_block_size(int64_t g, int k) {
  if (g <= DB_MAX) return (int)g;  // the whole space: one Rayleigh-Ritz is the full decomposition
  // k + 32 vectors, rounded up to 16 (round 2: max(k + 64, 2 k) = 128 at k = 50).  The one-workgroup kernels of an outer
  // iteration (Jacobi b^3, Cholesky b^3) dominate the solve; measured at 1M x 2k, k = 50: b = 128 / 112 / 96 -> fit
  // 15.96 / 14.85 / 13.76 ms on the planted matrix (same 11 GEMMs, residual 2e-11 .. 4e-11, loadings equal to 1e-10)
  // and 40.8 / 37.8 / 34.9 ms on the structure-less one (8 / 9 / 10 outer iterations, each cheaper).
  const int b = std::min<int>((k + 32 + 15) / 16 * 16, DB_MAX);
  return (int)std::min<int64_t>(b, g);
}

// what a dense solve reports (info_host of the three entry points); a batched solve sums and maximises over its batches
struct DenseStats {
  int n_outer = 0, n_gemm = 0, block_size = 0, n_chol_retry = 0;
  double residual = 0.0;
};
// info_host[0..3] = the counters, [4..5] = the residual (float64), [6] = scale_bits and [7] = 0 where the entry has one (>= 0)
static void pack_dense_info(int32_t* info_host, const DenseStats& st, int scale_bits) {
  if (!info_host) return;
  info_host[0] = st.n_outer;
  info_host[1] = st.n_gemm;
  info_host[2] = st.block_size;
  info_host[3] = st.n_chol_retry;
  memcpy(info_host + 4, &st.residual, sizeof(double));
  if (scale_bits >= 0) {
    info_host[6] = scale_bits;
    info_host[7] = 0;
  }
}

// the dense operator: the symmetric PSD matrix a [g x g]; every product and Gram matrix is one GEMM on the f64 matrix cores
struct DenseOp {
  hipStream_t s;
  const double* a;
  int64_t lda;
  int g, b;
  DenseBuffers d;
  SubspaceScratch w;
  const char* who = "dense eigensolver";
  int n_gemm = 0, n_chol_retry = 0;
  int64_t rows() const { return g; }
  void carve(Workspace& ws, int block) {
    b = block;
    dense_carve(ws, g, b, &d);
    w = d.w;
  }
  int gram(const double* p, int bp, const double* q, int bq, double* out) {
    return dgemm_tn(s, p, bp, q, bq, bp, bq, g, 1.0, nullptr, 0, 0.0, nullptr, 0, 0.0, out, bq);
  }
  // (the recurrence lives in the GEMM's epilogue)
  int apply(const double* y, const double* yprev, double al, double center, double bcoef, double* out) {
    ++n_gemm;
    if (!yprev) return dgemm_tn(s, a, lda, y, b, g, b, g, 1.0, nullptr, 0, 0.0, nullptr, 0, 0.0, out, b);
    return dgemm_tn(s, a, lda, y, b, g, b, g, al, y, b, -center * al, yprev, b, -bcoef, out, b);
  }
  int deflate(double*) { return SCAMD_OK; }
};

// top-k eigenpairs of the symmetric PSD matrix a [g x g]: theta (device, descending) and v = cx.d.z[3] [g x b]
static int dense_topk(DenseOp& cx, int k, unsigned int seed, double tol, DenseStats& st) {
  const int g = cx.g, b = cx.b;
  DenseBuffers& d = cx.d;
  int rc = prepare_lds_kernels();
  if (rc != SCAMD_OK) return rc;
  HostReadbackScope readback_scope;  // (h_theta below is the destination of a fetch handed out one synchronisation later)
  std::vector<double> h_theta(b);
  double h_resid = INFINITY;
  double *z = d.z[0], *tmp = d.z[1], *az = d.z[2], *v = d.z[3], *av = d.z[4], *y0 = d.z[5], *y1 = d.z[6];
  const int64_t cnt = (int64_t)g * b;
  const unsigned egrid = (unsigned)((cnt + 255) / 256);
  st.block_size = b;
  hipLaunchKernelGGL(randn_kernel, dim3(egrid), dim3(256), 0, cx.s, z, cnt, seed);
  SCAMD_LAUNCH_CHECK();
  if (b == g) {
    // the block is the whole space: one Rayleigh-Ritz on the identity-like basis = a full eigendecomposition
    rc = cholqr2(cx, z, tmp, y0, false, 2);
    if (rc != SCAMD_OK) return rc;
    rc = rayleigh_ritz(cx, y0, az, v, av, h_theta.data());
    if (rc != SCAMD_OK) return rc;
    SCAMD_READBACK_SYNC(cx.s);
    return SCAMD_OK;
  }
  // a filter whose result ends up in z (a copy by a kernel of ours, not a blit of the runtime)
  auto filter_into_z = [&](const double* vv, const double* avv, double c, double top, int m) -> int {
    double* last = nullptr;
    const int rcf = chebyshev_filter(cx, vv, avv, c, top, m, y0, y1, z, &last);
    if (rcf != SCAMD_OK) return rcf;
    if (last != z) {
      hipLaunchKernelGGL(axpby_kernel, dim3(egrid), dim3(256), 0, cx.s, cnt, 1.0, last, 0.0, last, z);
      SCAMD_LAUNCH_CHECK();
    }
    return SCAMD_OK;
  };
  // two power steps (A (A z): the condition number of the block grows by (lambda_1 / lambda_b)^2, well within
  // CholeskyQR2's reach) and one orthonormalisation
  rc = cx.apply(z, nullptr, 1.0, 0.0, 0.0, y1);
  if (rc != SCAMD_OK) return rc;
  rc = cx.apply(y1, nullptr, 1.0, 0.0, 0.0, z);
  if (rc != SCAMD_OK) return rc;
  // (ONE plain round here: the block has been through two power steps, kappa ~ (lambda_1 / lambda_b)^2, and serves for the
  // Rayleigh quotients that bound the first filter and as that filter's start -- orthonormal to ~kappa^2 u is enough for both;
  // the block is orthonormalised properly after the filter; two rounds, as until round 6: pca_fit 9.41 against 9.20 ms, same residual)
  rc = cholqr2(cx, z, tmp, v, false, 1);
  if (rc != SCAMD_OK) return rc;
  // First filter straight on this basis, bounds from its Rayleigh quotients: a Rayleigh-Ritz here would only re-mix
  // the block (the filter does not care) at the price of one more 128 x 128 eigenproblem, the most expensive kernel of
  // the solve.  c = smallest quotient (>= lambda_b is not guaranteed, the filter only needs a cut inside the unwanted
  // part), top = largest quotient (a scaling).
  rc = cx.apply(v, nullptr, 1.0, 0.0, 0.0, av);
  if (rc != SCAMD_OK) return rc;
  hipLaunchKernelGGL(rq_minmax_kernel, dim3(1), dim3(1024), 0, cx.s, v, av, g, b, d.resid);
  SCAMD_LAUNCH_CHECK();
  double h_rq[3] = {0.0, 0.0, 0.0};
  SCAMD_READBACK_NOW(h_rq, d.resid, sizeof(double) * 3, cx.s);
  if (h_rq[2] > h_rq[1] && h_rq[1] > 0.0) {
    // degree of the first filter: 7 (8 until round 6).  On the bench's matrix 8 / 7 / 6 / 5 leave the residual at 4.5e-11 / 4.6e-10 /
    // 4.8e-9 / 5e-8 against the tolerance 2e-8: 8 buys nothing but a block so ill-conditioned that CholeskyQR needs a second
    // shifted round (pca_fit 9.76 / 9.45 / 9.35 ms; 5: a second outer iteration)
    rc = filter_into_z(v, av, h_rq[1], h_rq[2], 7);
    if (rc != SCAMD_OK) return rc;
    rc = cholqr2(cx, z, tmp, y0, true, 2);
    if (rc != SCAMD_OK) return rc;
  } else {  // (the Rayleigh-Ritz below writes v: it works on a copy)
    hipLaunchKernelGGL(axpby_kernel, dim3(egrid), dim3(256), 0, cx.s, cnt, 1.0, v, 0.0, v, y0);
    SCAMD_LAUNCH_CHECK();
  }
  rc = rayleigh_ritz(cx, y0, az, v, av, h_theta.data());
  if (rc != SCAMD_OK) return rc;
  int outer = 0;
  const bool dbg = env_is("SCAMD_DENSE_DEBUG", '1');
  constexpr int MAX_OUTER = 60;
  for (outer = 1;; ++outer) {
    hipLaunchKernelGGL(residual_kernel, dim3(1), dim3(1024), 0, cx.s, v, av, cx.w.theta, g, b, k, d.resid);
    SCAMD_LAUNCH_CHECK();
    SCAMD_READBACK(&h_resid, d.resid, sizeof(double), cx.s);
    SCAMD_READBACK_SYNC(cx.s);  // (also completes the copy of theta)
    if (dbg)
      fprintf(stderr, "[dense] outer %d: residual %.3e, theta[0] %.6e theta[k-1] %.6e theta[b-1] %.6e, gemms %d, chol retries %d\n",
              outer, h_resid, h_theta[0], h_theta[k - 1], h_theta[b - 1], cx.n_gemm, cx.n_chol_retry);
    if (h_resid < tol) break;
    SCAMD_REQUIRE(outer < MAX_OUTER, SCAMD_EUNSUPPORTED,
                  "dense eigensolver: residual %.3e above the tolerance %.3e after %d filtered iterations", h_resid, tol,
                  MAX_OUTER);
    const double c = std::max(h_theta[b - 1], 0.0), top = h_theta[0];
    bool filtered = false;
    if (!(top > c && c > 0.0)) {
      // rank-deficient block (c == 0): a plain power step on the Ritz block
      rc = cx.apply(av, nullptr, 1.0, 0.0, 0.0, z);
      if (rc != SCAMD_OK) return rc;
    } else {
      const int m = chebyshev_degree(c, top, h_theta[k - 1], 16);
      rc = filter_into_z(v, av, c, top, m);
      if (rc != SCAMD_OK) return rc;
      filtered = m >= 8;
    }
    rc = cholqr2(cx, z, tmp, y0, filtered, 2);
    if (rc != SCAMD_OK) return rc;
    rc = rayleigh_ritz(cx, y0, az, v, av, h_theta.data());
    if (rc != SCAMD_OK) return rc;
  }
  st.n_outer += outer;
  st.residual = std::max(st.residual, h_resid);
  return SCAMD_OK;
}

}  // namespace scamd

using namespace scamd;

extern "C" size_t scamd_eigh_topk_workspace_bytes(int64_t g, int k) {
  if (g < 1 || k < 1) return 0;
  Workspace ws(nullptr, 0);
  DenseBuffers d;
  dense_carve(ws, g, dense_block_size(g, k), &d);
  return ws.used();
}

extern "C" int scamd_eigh_topk_f64(const double* a, int64_t g, int64_t lda, int k, uint64_t seed, double tol,
                                   double* lam, double* v, int32_t* info_host, void* workspace, size_t workspace_bytes,
                                   scamd_stream_t stream) {
  SCAMD_REQUIRE(a && lam && v, SCAMD_EINVAL, "eigh_topk: null pointer");
  SCAMD_REQUIRE(g >= 1 && lda >= g && k >= 1 && k <= g, SCAMD_EINVAL, "eigh_topk: bad shape g=%lld k=%d", (long long)g, k);
  SCAMD_REQUIRE(g < ((int64_t)1 << 30), SCAMD_EUNSUPPORTED, "eigh_topk: g too large");
  const int b = dense_block_size(g, k);
  SCAMD_REQUIRE(b == g || k + 32 <= b, SCAMD_EUNSUPPORTED,
                "eigh_topk: k=%d needs a block beyond %d columns (use a full eigendecomposition)", k, DB_MAX);
  SCAMD_REQUIRE(b == g || g >= 2 * b, SCAMD_EUNSUPPORTED, "eigh_topk: g=%lld between %d and %d is served by a full eigh",
                (long long)g, DB_MAX, 2 * DB_MAX);
  DenseOp cx;
  cx.s = stream;
  cx.a = a;
  cx.lda = lda;
  cx.g = (int)g;
  Workspace ws(workspace, workspace_bytes);
  cx.carve(ws, b);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EWORKSPACE, "eigh_topk: workspace %zu < required %zu", workspace_bytes, ws.used());
  DenseStats st;
  int rc = dense_topk(cx, k, eigensolver_seed(seed, 12345u), tol, st);
  if (rc != SCAMD_OK) return rc;
  // lam[k], v [g x k] row-major (column j = eigenvector j), unsigned
  SCAMD_HIP_CHECK(hipMemcpyAsync(lam, cx.w.theta, sizeof(double) * k, hipMemcpyDeviceToDevice, stream));
  SCAMD_HIP_CHECK(hipMemcpy2DAsync(v, sizeof(double) * k, cx.d.z[3], sizeof(double) * b, sizeof(double) * k, (size_t)g,
                                   hipMemcpyDeviceToDevice, stream));
  SCAMD_HIP_CHECK(hipStreamSynchronize(stream));
  st.n_gemm = cx.n_gemm;
  st.n_chol_retry = cx.n_chol_retry;
  pack_dense_info(info_host, st, -1);
  return SCAMD_OK;
}

// debug / test entry: the building blocks on caller buffers.  op 1: C[M x N] = P^T Q (P [K x M], Q [K x N]);
// op 2: S = CholeskyQR factor of G [b x b] (flag_host = pivot failure); op 3: (theta, Y) = eigh(T [b x b]);
// op 4: C[M x N] = Z S (Z [M x kdim], S [kdim x N], kdim and N up to 128): the panel product; op 5: the same for the two
// panels stacked in in0 [2 M x kdim] in ONE launch (out0, out1), as a Rayleigh-Ritz does; op 6: op 3 on (T + T^T) / 2, formed
// while the kernel loads T.
extern "C" int scamd_dense_debug_f64(int op, const double* in0, const double* in1, int m, int n, int kdim, double* out0,
                                     double* out1, int32_t* flag_host, scamd_stream_t stream) {
  SCAMD_REQUIRE(in0 && out0, SCAMD_EINVAL, "dense_debug: null pointer");
  if (op == 1) {
    SCAMD_REQUIRE(in1, SCAMD_EINVAL, "dense_debug: null pointer");
    int rc = dgemm_tn(stream, in0, m, in1, n, m, n, kdim, 1.0, nullptr, 0, 0.0, nullptr, 0, 0.0, out0, n);
    if (rc != SCAMD_OK) return rc;
  } else if (op == 2 || op == 3 || op == 6) {
    const int b = m;
    SCAMD_REQUIRE(b >= 1 && b <= DB_MAX, SCAMD_EINVAL, "dense_debug: b=%d", b);
    int* dflag = nullptr;
    SCAMD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dflag), 2 * sizeof(int)));
    SCAMD_HIP_CHECK(hipMemsetAsync(dflag, 0, 2 * sizeof(int), stream));
    int rc = prepare_lds_kernels();
    if (rc != SCAMD_OK) return rc;
    if (op == 2) {
      hipLaunchKernelGGL(chol_factor_kernel, dim3(1), dim3(1024), CHOL_LDS, stream, in0, b, 0.0, out0, dflag);
    } else {
      SCAMD_REQUIRE(out1, SCAMD_EINVAL, "dense_debug: null pointer");
      hipLaunchKernelGGL(jacobi_eigh_kernel, dim3(1), dim3(512), JAC_LDS, stream, in0, b, op == 6 ? 1 : 0, out0, out1, dflag + 1);
    }
    SCAMD_LAUNCH_CHECK();
    int h[2] = {0, 0};
    SCAMD_HIP_CHECK(hipMemcpyAsync(h, dflag, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    SCAMD_HIP_CHECK(hipStreamSynchronize(stream));
    SCAMD_HIP_CHECK(hipFree(dflag));
    if (flag_host) *flag_host = op == 2 ? h[0] : h[1];
    return SCAMD_OK;
  } else if (op == 4 || op == 5) {  // out0 [m x n] = in0 [m x kdim] in1 [kdim x n]; op 5: and out1 = (in0 + m kdim) in1, same launch
    SCAMD_REQUIRE(in1 && (op == 4 || out1), SCAMD_EINVAL, "dense_debug: null pointer");
    int rc = prepare_lds_kernels();
    if (rc != SCAMD_OK) return rc;
    rc = panel_small(stream, in0, op == 5 ? in0 + (int64_t)m * kdim : nullptr, in1, m, kdim, n, out0, op == 5 ? out1 : nullptr);
    if (rc != SCAMD_OK) return rc;
  } else {
    SCAMD_REQUIRE(false, SCAMD_EINVAL, "dense_debug: op=%d", op);
  }
  SCAMD_HIP_CHECK(hipStreamSynchronize(stream));
  return SCAMD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// sc.pp.pca on a resident CSR matrix in ONE call (SURVEY.md 8(b).3 `pca_csr_f32`): the exact Gram route of
// scanpy_amd/preprocessing/_pca_solver.py without Python -- max|x| -> fixed-point X^T X (gram.hip) -> A = G - n mu mu^T ->
// top-k eigenpairs (above) -> sign convention of sklearn's svd_flip -> scores X V - 1 (mu^T V) (pca.hip) -> variances.
// Single device; a multi-rank run all-reduces the fixed-point Gram matrix between the two halves and therefore uses
// the building blocks (scamd_csr_gram_f32, scamd_eigh_topk_f64, scamd_spmm_csr_f32) instead.
// ---------------------------------------------------------------------------------------------------------------------
namespace scamd {
struct PcaBuffers {
  long long* gram; long long* colsum; float* v32; float* shift;
  void* gram_ws; size_t gram_ws_bytes; void* solve_ws; size_t solve_ws_bytes;
};
// out[0] = sum of var[0..g) in a fixed order (256 strided partial sums in index order, then a fixed tree: one thread walking
// the array took 105 us of dependent loads at g = 2000)
__global__ __launch_bounds__(256) void sum_kernel(const double* __restrict__ x, int g, double* __restrict__ out) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < g; i += 256) s += x[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = part[0];
}
// zero_center: variance[c] = theta[c] / (n - 1) (sklearn PCA: S^2 / (n - 1)); otherwise the variance of the scores of
// the uncentred decomposition, theta[c] / n - (mu^T v_c)^2 (TruncatedSVD); ratio[c] = variance[c] / total
__global__ void variance_kernel(const double* __restrict__ theta, int k, double denom, const double* __restrict__ proj,
                                const double* __restrict__ varsum, double total_scale, double* __restrict__ variance,
                                double* __restrict__ ratio) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  double ev = fmax(theta[c], 0.0) / denom;
  if (proj) ev = fmax(ev - proj[c] * proj[c], 0.0);
  variance[c] = ev;
  const double tot = varsum[0] * total_scale;
  ratio[c] = tot > 0.0 ? ev / tot : 0.0;
}
}  // namespace scamd

// ---- the dense half of the Gram route on its own: (fixed-point Gram matrix, column sums) -> model ------------------------
// What a row-sharded run calls after the all-reduce of the int64 sums, and what scamd_pca_csr_f32 calls on one device: the
// model is therefore bitwise the same for any number of ranks, and no library (torch / rocBLAS) computes any part of it.
namespace scamd {
struct PcaSolveBuffers {
  double* a; double* var; double* varsum; double* proj; double* theta_all; double* deflate; void* dense_ws; size_t dense_ws_bytes;
};
static void pca_solve_carve(Workspace& ws, int64_t g, int k, PcaSolveBuffers* b) {
  b->a = ws.take<double>((size_t)g * g);
  b->var = ws.take<double>((size_t)g);
  b->varsum = ws.take<double>(8);
  b->proj = ws.take<double>((size_t)k + 8);
  b->theta_all = ws.take<double>((size_t)k + 8);
  b->deflate = ws.take<double>(k > DENSE_BATCH_HOST ? (size_t)DENSE_BATCH_HOST * g : 8);
  b->dense_ws_bytes = scamd_eigh_topk_workspace_bytes(g, std::min(k, DENSE_BATCH_HOST));
  b->dense_ws = ws.take<char>(b->dense_ws_bytes);
}
__global__ void copy_theta_kernel(const double* __restrict__ theta, int k, double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < k) out[c] = fmax(theta[c], 0.0);
}
// q[c][m] = theta[c] * p[c][m]  (rows = components of a finished batch: A -= P^T Q deflates them)
__global__ void scale_rows_kernel(const double* __restrict__ p, const double* __restrict__ theta, int kb, int g,
                                  double* __restrict__ q) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (int64_t)kb * g) q[e] = theta[e / g] * p[e];
}
// More components than one block of the subspace iteration holds (k + 32 > DB_MAX): batches of at most DB_MAX - 32, each on
// the matrix DEFLATED by the finished ones, A <- A - V diag(theta) V^T (one rank-kb update on the f64 MFMA): the leading
// eigenpairs of the deflated matrix are the next ones of A, orthogonal to the finished ones to the accuracy they were
// converged to.  Round 6: until then n_comps > 96 ran the same iteration on torch.linalg (rocSOLVER / rocBLAS).
constexpr int DENSE_BATCH = DB_MAX - 32;
static bool dense_in_range(int64_t g, int k) {
  if (g <= DB_MAX) return true;                       // the whole space: one Rayleigh-Ritz
  if (k <= 0 || k > g) return false;
  const int kb = std::min(k, DENSE_BATCH);
  const int bsz = dense_block_size(g, kb);
  return kb + 32 <= bsz && g >= 2 * bsz && (k <= DENSE_BATCH || g >= 2 * k);  // (deflating more than half the space is a full eigh's job)
}
// top-k eigenpairs of cx.a (DESTROYED when k needs more than one batch) -> comp64 [k x g] (sign convention applied),
// v32 [g x k] (may be NULL), theta_all [k] (descending, raw).  `scratch` = kb_max x g doubles for the deflation.
static int dense_topk_batched(DenseOp& cx, double* a_mut, int k, unsigned int dseed, double tol, double* comp64, float* v32,
                              double* theta_all, double* scratch, void* dense_ws, size_t dense_ws_bytes, DenseStats& st) {
  const int g = cx.g;
  for (int k0 = 0; k0 < k;) {
    const int kb = g <= DB_MAX ? k : std::min(k - k0, DENSE_BATCH);
    const int bsz = dense_block_size(g, kb);
    Workspace dws(dense_ws, dense_ws_bytes);
    cx.carve(dws, bsz);
    SCAMD_REQUIRE(dws.ok, SCAMD_EWORKSPACE, "dense eigensolver: workspace");
    int rc = dense_topk(cx, kb, dseed + 0x9E3779B9u * (unsigned int)k0, tol, st);
    if (rc != SCAMD_OK) return rc;
    hipLaunchKernelGGL(finalize_components_kernel, dim3(kb), dim3(256), 0, cx.s, cx.d.z[3], g, bsz, k, comp64 + (int64_t)k0 * g,
                       v32 ? v32 + k0 : (float*)nullptr);
    SCAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(axpby_kernel, dim3((kb + 255) / 256), dim3(256), 0, cx.s, (int64_t)kb, 1.0, cx.w.theta, 0.0, cx.w.theta,
                       theta_all + k0);
    SCAMD_LAUNCH_CHECK();
    k0 += kb;
    if (k0 < k) {  // deflate: A -= P^T (diag(theta) P), P = this batch's components [kb x g]
      const double* pb = comp64 + (int64_t)(k0 - kb) * g;
      hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)(((int64_t)kb * g + 255) / 256)), dim3(256), 0, cx.s, pb,
                         theta_all + (k0 - kb), kb, g, scratch);
      SCAMD_LAUNCH_CHECK();
      rc = dgemm_tn(cx.s, pb, g, scratch, g, g, g, kb, -1.0, a_mut, cx.lda, 1.0, nullptr, 0, 0.0, a_mut, cx.lda);
      if (rc != SCAMD_OK) return rc;
      ++cx.n_gemm;
    }
  }
  st.n_gemm = cx.n_gemm;
  st.n_chol_retry = cx.n_chol_retry;
  return SCAMD_OK;
}
// where pca_solve_gram leaves the model (device): components [k x g], float32 loadings [g x k], shift [k] = mu^T V, variance [k],
// variance_ratio [k], mean [g], eigenvalues [k] (may be NULL)
struct PcaModel {
  double* components; float* v32; float* shift; double* variance; double* variance_ratio; double* mean; double* eigenvalues;
};
// steps 3-5 and 7 of the route; `dseed` is handed to the eigensolver as it is.  No synchronisation: the caller drains.
static int pca_solve_gram(const long long* gram, int64_t ld_gram, const long long* colsum, int64_t n, int64_t g, int scale_bits,
                          int k, int zero_center, unsigned int dseed, double tol, const PcaModel& out, PcaSolveBuffers& b,
                          hipStream_t s, DenseStats& st) {
  // 3. A = G - n mu mu^T, means, column variances
  const double inv = std::ldexp(1.0, -scale_bits);
  hipLaunchKernelGGL(cov_from_gram_kernel, dim3((unsigned)(((int64_t)g * g + 255) / 256)), dim3(256), 0, s, gram, ld_gram,
                     colsum, (int)g, inv, (double)n, zero_center ? 1 : 0, b.a, out.mean, b.var);
  SCAMD_LAUNCH_CHECK();
  // 4. top-k eigenpairs (batches of DENSE_BATCH with deflation when k needs more than one block)
  SCAMD_REQUIRE(dense_in_range(g, k), SCAMD_EUNSUPPORTED, "pca: n_comps=%d / g=%lld outside the device eigensolver's range", k,
                (long long)g);
  DenseOp cx;
  cx.s = s;
  cx.a = b.a;
  cx.lda = g;
  cx.g = (int)g;
  // 5. (inside the batches) sign convention, float32 loadings; then the projected means
  int rc = dense_topk_batched(cx, b.a, k, dseed, tol, out.components, out.v32, b.theta_all, b.deflate, b.dense_ws, b.dense_ws_bytes, st);
  if (rc != SCAMD_OK) return rc;
  hipLaunchKernelGGL(mean_shift_kernel, dim3(k), dim3(256), 0, s, out.mean, out.v32, (int)g, k, out.shift, b.proj);
  SCAMD_LAUNCH_CHECK();
  // 7. explained variance (sklearn: S^2 / (n - 1); ratio against the total variance with the same n / (n - 1) factor;
  //    zero_center = False is TruncatedSVD: the variance of the scores of the uncentred decomposition, lam / n - (mu^T v)^2)
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, b.var, (int)g, b.varsum);
  SCAMD_LAUNCH_CHECK();
  const double denom = zero_center ? (double)(n - 1) : (double)n;
  const double total_scale = zero_center ? (double)n / (double)(n - 1) : 1.0;
  hipLaunchKernelGGL(variance_kernel, dim3((k + 255) / 256), dim3(256), 0, s, b.theta_all, k, denom,
                     zero_center ? (const double*)nullptr : (const double*)b.proj, b.varsum, total_scale, out.variance,
                     out.variance_ratio);
  SCAMD_LAUNCH_CHECK();
  if (out.eigenvalues) {
    hipLaunchKernelGGL(copy_theta_kernel, dim3((k + 255) / 256), dim3(256), 0, s, b.theta_all, k, out.eigenvalues);
    SCAMD_LAUNCH_CHECK();
  }
  return SCAMD_OK;
}
}  // namespace scamd

extern "C" size_t scamd_pca_solve_gram_workspace_bytes(int64_t g, int n_comps) {
  if (g < 1 || n_comps < 1) return 0;
  Workspace ws(nullptr, 0);
  PcaSolveBuffers b;
  pca_solve_carve(ws, g, n_comps, &b);
  return ws.used();
}

extern "C" int scamd_pca_solve_gram_f64(const int64_t* gram, int64_t ld_gram, const int64_t* colsum, int64_t n_total, int64_t g,
                                        int scale_bits, int n_comps, int zero_center, uint64_t seed, double tol,
                                        double* components, float* loadings_f32, float* shift, double* variance,
                                        double* variance_ratio, double* mean, double* eigenvalues, int32_t* info_host,
                                        void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(gram && colsum && components && loadings_f32 && shift && variance && variance_ratio && mean, SCAMD_EINVAL,
                "pca solve: null pointer");
  const int k = n_comps;
  SCAMD_REQUIRE(n_total >= 2 && g >= 1 && ld_gram >= g && k >= 1 && k <= g && scale_bits >= 0 && scale_bits <= 60, SCAMD_EINVAL,
                "pca solve: bad shape n=%lld g=%lld ld=%lld k=%d S=%d", (long long)n_total, (long long)g, (long long)ld_gram, k, scale_bits);
  SCAMD_REQUIRE(g <= 8192, SCAMD_EUNSUPPORTED, "pca solve: the Gram route takes up to 8192 genes (g=%lld)", (long long)g);
  Workspace ws(workspace, workspace_bytes);
  PcaSolveBuffers b;
  pca_solve_carve(ws, g, k, &b);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EWORKSPACE, "pca solve: workspace %zu < required %zu", workspace_bytes, ws.used());
  DenseStats st;
  const PcaModel model{components, loadings_f32, shift, variance, variance_ratio, mean, eigenvalues};
  int rc = pca_solve_gram(reinterpret_cast<const long long*>(gram), ld_gram, reinterpret_cast<const long long*>(colsum), n_total, g,
                          scale_bits, k, zero_center, eigensolver_seed(seed, 12345u), tol, model, b, stream, st);
  if (rc != SCAMD_OK) return rc;
  SCAMD_HIP_CHECK(hipStreamSynchronize(stream));
  pack_dense_info(info_host, st, scale_bits);
  return SCAMD_OK;
}

namespace scamd {
static void pca_carve(Workspace& ws, int64_t n, int64_t g, int k, PcaBuffers* b) {
  const int64_t gp = (g + 127) / 128 * 128;
  b->gram = ws.take<long long>((size_t)gp * gp);
  b->colsum = ws.take<long long>((size_t)gp);
  b->v32 = ws.take<float>((size_t)g * k);
  b->shift = ws.take<float>((size_t)k + 8);
  b->gram_ws_bytes = scamd_csr_gram_workspace_bytes(n, g);
  b->gram_ws = ws.take<char>(b->gram_ws_bytes);
  b->solve_ws_bytes = scamd_pca_solve_gram_workspace_bytes(g, k);
  b->solve_ws = ws.take<char>(b->solve_ws_bytes);
}
}  // namespace scamd

extern "C" size_t scamd_pca_csr_workspace_bytes(int64_t n, int64_t g, int n_comps) {
  if (n < 1 || g < 1 || n_comps < 1) return 0;
  Workspace ws(nullptr, 0);
  PcaBuffers b;
  pca_carve(ws, n, g, n_comps, &b);
  return ws.used();
}

extern "C" int scamd_pca_csr_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                 int64_t nnz, int n_comps, int zero_center, uint64_t seed, double tol, float* scores,
                                 double* components, double* variance, double* variance_ratio, double* mean,
                                 int32_t* info_host, void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && scores && components && variance && variance_ratio && mean, SCAMD_EINVAL, "pca: null pointer");
  SCAMD_REQUIRE(n >= 2 && g >= 1 && nnz >= 0, SCAMD_EINVAL, "pca: bad shape n=%lld g=%lld", (long long)n, (long long)g);
  const int k = n_comps;
  SCAMD_REQUIRE(k >= 1 && k < std::min<int64_t>(n, g), SCAMD_EINVAL,
                "n_components=%d must be strictly less than min(n_samples, n_features)=%lld with svd_solver='arpack'", k,
                (long long)std::min<int64_t>(n, g));
  SCAMD_REQUIRE(g <= 8192, SCAMD_EUNSUPPORTED, "pca: the Gram route takes up to 8192 genes (g=%lld)", (long long)g);
  Workspace ws(workspace, workspace_bytes);
  PcaBuffers b;
  pca_carve(ws, n, g, k, &b);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EWORKSPACE, "pca: workspace %zu < required %zu", workspace_bytes, ws.used());
  hipStream_t s = stream;
  const int64_t gp = (g + 127) / 128 * 128;
  // 1. max |x| -> scale of the fixed-point sums (both sum x_a x_b 2^S and sum x 2^S must stay below 2^62)
  float absmax = 0.f;
  int rc = scamd_csr_gram_f32(indptr, indices, data, n, g, nnz, 0, nullptr, 0, nullptr, &absmax, b.gram_ws, b.gram_ws_bytes, s);
  if (rc != SCAMD_OK) return rc;
  const double am = (double)absmax;
  const double bound = std::max(std::max((double)n * am * am, (double)n * am), 1e-300);
  int scale_bits = std::min((int)std::floor(62.0 - std::log2(bound)), 60);
  SCAMD_REQUIRE(!(am > 0.0) || scale_bits + 2.0 * std::log2(am) >= 24.0, SCAMD_EUNSUPPORTED,
                "pca: fixed-point resolution below float32 for this n and dynamic range (max|x| = %g)", am);
  SCAMD_REQUIRE(scale_bits >= 0, SCAMD_EUNSUPPORTED,
                "pca: n * max|x|^2 = %g exceeds the int64 fixed-point range (2^62): values are not normalised", bound);
  // 2. G = X^T X, column sums (int64, exact)
  rc = scamd_csr_gram_f32(indptr, indices, data, n, g, nnz, scale_bits, reinterpret_cast<int64_t*>(b.gram), gp,
                          reinterpret_cast<int64_t*>(b.colsum), nullptr, b.gram_ws, b.gram_ws_bytes, s);
  if (rc != SCAMD_OK) return rc;
  // 3-5, 7. the dense half (shared with the row-sharded route)
  Workspace sws(b.solve_ws, b.solve_ws_bytes);
  PcaSolveBuffers sb;
  pca_solve_carve(sws, g, k, &sb);
  DenseStats st;
  const PcaModel model{components, b.v32, b.shift, variance, variance_ratio, mean, nullptr};
  rc = pca_solve_gram(b.gram, gp, b.colsum, n, g, scale_bits, k, zero_center, eigensolver_seed(seed, 12345u), tol, model, sb, s, st);
  if (rc != SCAMD_OK) return rc;
  // 6. scores = X V - 1 shift^T
  rc = scamd_spmm_csr_f32(indptr, indices, data, n, g, b.v32, k, zero_center ? b.shift : nullptr, scores, s);
  if (rc != SCAMD_OK) return rc;
  SCAMD_HIP_CHECK(hipStreamSynchronize(s));
  pack_dense_info(info_host, st, scale_bits);
  return SCAMD_OK;
}

// =====================================================================================================================
// Spectral initialisation of the UMAP layout on the device (round 6).  `sc.tl.umap(init_pos='spectral')`
// (src/scanpy/tools/_umap.py:165-215 -> umap-learn `spectral_layout`: the eigenvectors of the normalised Laplacian that
// follow the trivial one, by ARPACK) as ONE call: Chebyshev-filtered subspace iteration on M = (S + I) / 2,
// S = D^-1/2 A D^-1/2, with the known trivial eigenvector sqrt(deg) projected out -- the algorithm of
// scanpy_amd/tools/_umap.py:_top_eigenvectors_below_trivial (which ran on torch.linalg QR / Cholesky / eigh + torch.bmm
// until this round and remains the CPU stand-in of the tests), on the kernels of this file: the block is n x b with
// b = dim + 6 <= 16 columns, S y is the float32 SpMM of pca.hip, every reduction over the n rows is a two-stage sum in a
// fixed order (bitwise reproducible).
// =====================================================================================================================
namespace scamd {
constexpr int SP_MAXB = 16;   // the block of the spectral initialisation (dim + 6 <= 16): the narrow instantiation of the panel kernels
constexpr int SP_WIDEB = 32;  // the block of the diffusion map (n_comps + 6 <= 32): the wide one
constexpr int SP_GRID = 1024;

// deg[v] = sum of the row (float64), one wave per row
__global__ __launch_bounds__(256) void sp_degree_kernel(const int64_t* __restrict__ indptr, const float* __restrict__ w, int64_t n,
                                                        double* __restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n) return;
  double s = 0.0;
  for (int64_t e = indptr[v] + lane; e < indptr[v + 1]; e += 64) s += (double)w[e];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) deg[v] = s;
}
// s[e] = w[e] / sqrt(deg[row] deg[col]) (float32: the SpMM's operand), t0[v] = sqrt(deg[v]) (the trivial eigenvector, unnormalised)
__global__ __launch_bounds__(256) void sp_scale_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                       const float* __restrict__ w, int64_t n, const double* __restrict__ deg,
                                                       float* __restrict__ s, double* __restrict__ t0) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n) return;
  const double dv = deg[v];
  const double dis_v = dv > 0.0 ? 1.0 / sqrt(dv) : 0.0;
  if (lane == 0) t0[v] = sqrt(fmax(dv, 0.0));
  for (int64_t e = indptr[v] + lane; e < indptr[v + 1]; e += 64) {
    const double du = deg[indices[e]];
    const double dis_u = du > 0.0 ? 1.0 / sqrt(du) : 0.0;
    s[e] = (float)((double)w[e] * dis_v * dis_u);
  }
}
// part[blk][i * bq + j] = sum over the block's rows of p[row][i] q[row][j]   (p: n x bp, q: n x bq, both <= W columns).
// 256 threads = 16 x 16 thread positions, each owning the (W / 16)^2 outputs (i + 16 a, j + 16 c); 64 rows at a time staged
// through LDS.  W = 16 is the thread map and summation order the spectral initialisation has always had (its pinned
// iteration counts depend on it); W = 32 (the diffusion map's block, up to 32 columns) gives a thread 2 x 2 outputs: 4
// accumulators (8 VGPRs) fed by 2 + 2 LDS reads per row -- by this count nowhere near the register budget; neither the
// registers nor the LDS traffic of the wide instantiation were measured (the step is O(n b^2) beside the SpMM).  LDS, W = 32: 2 x 64 x 33
// doubles = 33 KB.  The row stride of W + 1 doubles is odd, so the staging writes of a wave (consecutive e: consecutive
// columns, then the next row) fall on consecutive banks but for the one-double pad per row; in the product loop the four
// i of a wave read one address each (broadcast) and its 16 j read 16 consecutive doubles: no bank is asked twice.
template <int W>
__global__ __launch_bounds__(256) void sp_tall_gram_kernel(const double* __restrict__ p, int bp, const double* __restrict__ q,
                                                           int bq, int64_t n, double* __restrict__ part) {
  constexpr int R = W / 16;
  __shared__ double sp[64][W + 1], sq[64][W + 1];
  const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int64_t rows_per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
  double acc[R][R];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int c = 0; c < R; ++c) acc[a][c] = 0.0;
  for (int64_t base = r0; base < r1; base += 64) {
    const int cnt = (int)(r1 - base < 64 ? r1 - base : 64);
    for (int e = threadIdx.x; e < 64 * W; e += 256) {
      const int r = e / W, c = e % W;
      sp[r][c] = (r < cnt && c < bp) ? p[(base + r) * bp + c] : 0.0;
      sq[r][c] = (r < cnt && c < bq) ? q[(base + r) * bq + c] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < 64; ++r) {
#pragma unroll
      for (int a = 0; a < R; ++a)
#pragma unroll
        for (int c = 0; c < R; ++c) acc[a][c] = fma(sp[r][i + 16 * a], sq[r][j + 16 * c], acc[a][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int c = 0; c < R; ++c)
      if (i + 16 * a < bp && j + 16 * c < bq) part[(int64_t)blockIdx.x * (bp * bq) + (i + 16 * a) * bq + j + 16 * c] = acc[a][c];
}
// out[e] = sum over the blocks in index order
__global__ void sp_reduce_kernel(const double* __restrict__ part, int nblk, int cnt, double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * cnt + e];
  out[e] = s;
}
// y[row][j] -= t0[row] * c[j] / |t0|^2   (c = t0^T y, nrm2[0] = t0^T t0)
__global__ void sp_deflate_kernel(double* __restrict__ y, const double* __restrict__ t0, const double* __restrict__ c,
                                  const double* __restrict__ nrm2, int64_t n, int b) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * b) return;
  const int64_t row = e / b;
  const int j = (int)(e - row * b);
  const double d = nrm2[0];
  if (d > 0.0) y[e] -= t0[row] * (c[j] / d);
}
__global__ void sp_to_f32_kernel(const double* __restrict__ y, int64_t count, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < count) out[e] = (float)y[e];
}
// out = a * (M y - center y) - bcoef * yprev with M y = (sgn S y + y) / 2; a = 1, center = 0, bcoef = 0: out = M y.
// sgn = 1: the upper end of S's spectrum (multiplying by 1.0 is exact); sgn = -1: its lower end (the diffusion map's guard)
__global__ void sp_cheb_kernel(int64_t count, const float* __restrict__ sy, const double* __restrict__ y,
                               const double* __restrict__ yprev, double sgn, double a, double center, double bcoef,
                               double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const double yy = y[e];
  const double my = 0.5 * (sgn * (double)sy[e] + yy);
  double r = a * (my - center * yy);
  if (bcoef != 0.0) r -= bcoef * yprev[e];
  out[e] = r;
}
// part[blk][j] = sum over the block's rows of (mv[row][j] - theta[j] v[row][j])^2, j < dim <= W
// (256 / W row lanes x W columns; W = 16: the map the spectral initialisation has always had)
template <int W>
__global__ __launch_bounds__(256) void sp_resid_kernel(const double* __restrict__ v, const double* __restrict__ mv,
                                                       const double* __restrict__ theta, int64_t n, int b, int dim,
                                                       double* __restrict__ part) {
  constexpr int RL = 256 / W;
  __shared__ double red[256];
  const int j = threadIdx.x % W, rl = threadIdx.x / W;
  const int64_t rows_per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
  double acc = 0.0;
  if (j < dim) {
    const double th = theta[j];
    for (int64_t r = r0 + rl; r < r1; r += RL) {
      const double d = mv[r * b + j] - th * v[r * b + j];
      acc = fma(d, d, acc);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (rl == 0) {
    double s = 0.0;
    for (int k = 0; k < RL; ++k) s += red[k * W + j];
    if (j < dim) part[(int64_t)blockIdx.x * dim + j] = s;
  }
}
// out[row][j] = v[row][j], j < dim (row stride b -> dim)
__global__ void sp_take_kernel(const double* __restrict__ v, int64_t n, int b, int dim, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * dim) return;
  const int64_t row = e / dim;
  out[e] = v[row * b + (e - row * dim)];
}

struct SpectralBuffers {
  double* deg; double* t0; float* s; double* pan[7]; float* y32; float* sy32; double* part;
  SubspaceScratch w; double* cvec; double* nrm2; double* rnorm;
};
// b <= SP_MAXB: the sizes the spectral initialisation has always carved; beyond it the small matrices hold SP_WIDEB columns
static void spectral_carve(Workspace& ws, int64_t n, int64_t nnz, int b, SpectralBuffers* sb) {
  const int maxb = b <= SP_MAXB ? SP_MAXB : SP_WIDEB;
  sb->deg = ws.take<double>((size_t)n);
  sb->t0 = ws.take<double>((size_t)n);
  sb->s = ws.take<float>((size_t)std::max<int64_t>(nnz, 1));
  for (int i = 0; i < 7; ++i) sb->pan[i] = ws.take<double>((size_t)n * b);
  sb->y32 = ws.take<float>((size_t)n * b);
  sb->sy32 = ws.take<float>((size_t)n * b);
  sb->part = ws.take<double>((size_t)SP_GRID * maxb * maxb);
  sb->w.gm = ws.take<double>(maxb * maxb);
  sb->w.smat = ws.take<double>(maxb * maxb);
  sb->w.tmat = ws.take<double>(maxb * maxb);
  sb->w.ymat = ws.take<double>(maxb * maxb);
  sb->w.theta = ws.take<double>(maxb);
  sb->cvec = ws.take<double>(maxb);
  sb->nrm2 = ws.take<double>(8);
  sb->rnorm = ws.take<double>(maxb);
  sb->w.flags = ws.take<int>(8);
}

// the spectral operator: M = (S + I) / 2 on n x b panels, S = D^-1/2 A D^-1/2 as the float32 SpMM of pca.hip; every reduction
// over the n rows is a two-stage sum in a fixed order.  b <= SP_MAXB runs the narrow instantiation of the panel kernels,
// b <= SP_WIDEB the wide one.
struct SpectralOp {
  hipStream_t s;
  const int64_t* indptr;
  const int32_t* indices;
  const float* sval;  // the entries of S (float32) on the pattern of indptr / indices
  int64_t n;
  int b, dim;
  double sgn = 1.0;  // M = (sgn S + I) / 2
  SpectralBuffers sb;
  SubspaceScratch w;
  const char* who = "spectral init";
  int n_apply = 0, n_chol_retry = 0;
  int64_t rows() const { return n; }
  int grid_rows() const { return (int)std::min<int64_t>(SP_GRID, (n + 63) / 64); }
  unsigned egrid() const { return (unsigned)((n * b + 255) / 256); }
  // out[bp x bq] = p^T q over the n rows
  int gram(const double* p, int bp, const double* q, int bq, double* out) {
    const int g = grid_rows();
    if (bp <= SP_MAXB && bq <= SP_MAXB)
      hipLaunchKernelGGL(sp_tall_gram_kernel<SP_MAXB>, dim3(g), dim3(256), 0, s, p, bp, q, bq, n, sb.part);
    else
      hipLaunchKernelGGL(sp_tall_gram_kernel<SP_WIDEB>, dim3(g), dim3(256), 0, s, p, bp, q, bq, n, sb.part);
    SCAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_reduce_kernel, dim3((unsigned)((bp * bq + 255) / 256)), dim3(256), 0, s, sb.part, g, bp * bq, out);
    SCAMD_LAUNCH_CHECK();
    return SCAMD_OK;
  }
  // rnorm[j] = |mv_j - theta_j v_j|^2, j < dim
  int residuals(const double* v, const double* mv) {
    const int g = grid_rows();
    if (b <= SP_MAXB)
      hipLaunchKernelGGL(sp_resid_kernel<SP_MAXB>, dim3(g), dim3(256), 0, s, v, mv, (const double*)w.theta, n, b, dim, sb.part);
    else
      hipLaunchKernelGGL(sp_resid_kernel<SP_WIDEB>, dim3(g), dim3(256), 0, s, v, mv, (const double*)w.theta, n, b, dim, sb.part);
    SCAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)sb.part, g, dim, sb.rnorm);
    SCAMD_LAUNCH_CHECK();
    return SCAMD_OK;
  }
  // y <- y - t0 (t0^T y) / |t0|^2
  int deflate(double* y) {
    int rc = gram(sb.t0, 1, y, b, sb.cvec);
    if (rc != SCAMD_OK) return rc;
    hipLaunchKernelGGL(sp_deflate_kernel, dim3(egrid()), dim3(256), 0, s, y, sb.t0, sb.cvec, sb.nrm2, n, b);
    SCAMD_LAUNCH_CHECK();
    return SCAMD_OK;
  }
  // out = a (M y - center y) - bcoef yprev
  int apply(const double* y, const double* yprev, double a, double center, double bcoef, double* out) {
    const int64_t cnt = n * b;
    hipLaunchKernelGGL(sp_to_f32_kernel, dim3(egrid()), dim3(256), 0, s, y, cnt, sb.y32);
    SCAMD_LAUNCH_CHECK();
    int rc = scamd_spmm_csr_f32(indptr, indices, sval, n, n, sb.y32, b, nullptr, sb.sy32, s);
    if (rc != SCAMD_OK) return rc;
    hipLaunchKernelGGL(sp_cheb_kernel, dim3(egrid()), dim3(256), 0, s, cnt, (const float*)sb.sy32, y, yprev, sgn, a, center, bcoef, out);
    SCAMD_LAUNCH_CHECK();
    ++n_apply;
    return SCAMD_OK;
  }
};
// the diffusion map's operator: M = (sgn T_sym + I) / 2 with T_sym handed in as it is stored -- the same panels, SpMM and
// reductions, and NO deflation: the stationary eigenvector is part of the answer (column 0 of `sc.tl.diffmap`)
struct DiffmapOp : SpectralOp {
  int deflate(double*) { return SCAMD_OK; }
};

struct SubspaceRun {
  int outer = 0;
  double resid = INFINITY;
};
// The outer iteration over a graph operator (SpectralOp, DiffmapOp): random start block, then Rayleigh-Ritz, residual of the
// cx.dim wanted Ritz pairs (|M| = 1: absolute = relative), Chebyshev filter of [0, smallest Ritz value], deflation, CholeskyQR2
// until the residual is below tol or max_outer is reached.  Leaves the Ritz vectors in pan[3], M times them in pan[4], the
// Ritz values of M in h_theta [b] (descending) and on the device in w.theta.  The caller owns a HostReadbackScope and ends with
// a SCAMD_READBACK_SYNC after its own last launch: a loop that ends by max_outer leaves the last theta queued.
template <class Op>
static int graph_subspace_iteration(Op& cx, unsigned int seed, double tol, int max_outer, int max_degree, double* h_theta,
                                    SubspaceRun* run) {
  SpectralBuffers& sb = cx.sb;
  hipStream_t s = cx.s;
  const int64_t n = cx.n;
  const int b = cx.b, dim = cx.dim;
  double *z = sb.pan[0], *tmp = sb.pan[1], *mz = sb.pan[2], *v = sb.pan[3], *mv = sb.pan[4], *y0 = sb.pan[5], *y1 = sb.pan[6];
  const int64_t cnt = n * b;
  hipLaunchKernelGGL(randn_kernel, dim3(cx.egrid()), dim3(256), 0, s, z, cnt, seed);
  SCAMD_LAUNCH_CHECK();
  int rc = cx.deflate(z);
  if (rc != SCAMD_OK) return rc;
  rc = cholqr2(cx, z, tmp, y0, false, 2);
  if (rc != SCAMD_OK) return rc;
  rc = rayleigh_ritz(cx, y0, mz, v, mv, h_theta);
  if (rc != SCAMD_OK) return rc;
  double resid = INFINITY;
  int outer = 0;
  for (outer = 1; outer <= max_outer; ++outer) {
    rc = cx.residuals(v, mv);
    if (rc != SCAMD_OK) return rc;
    double h_r[SP_WIDEB];
    SCAMD_READBACK(h_r, sb.rnorm, sizeof(double) * dim, s);
    SCAMD_READBACK_SYNC(s);  // (also completes the copy of theta)
    resid = 0.0;
    for (int j = 0; j < dim; ++j) resid = std::max(resid, std::sqrt(std::max(h_r[j], 0.0)));
    if (resid < tol) break;
    const double c = h_theta[b - 1];
    double* blk = nullptr;  // the block that is orthonormalised next
    if (!(c > 0.0 && c < 1.0)) {
      // a degenerate block: one plain step, on a COPY (mv is an output of the Rayleigh-Ritz that follows)
      rc = cx.deflate(mv);
      if (rc != SCAMD_OK) return rc;
      hipLaunchKernelGGL(axpby_kernel, dim3(cx.egrid()), dim3(256), 0, s, cnt, 1.0, (const double*)mv, 0.0, (const double*)mv, y0);
      SCAMD_LAUNCH_CHECK();
      blk = y0;
    } else {
      // the degree: as high as the amplification spread inside the wanted set allows; the spectrum's upper end is 1
      const int m = chebyshev_degree(c, 1.0, h_theta[dim - 1], max_degree);
      rc = chebyshev_filter(cx, v, mv, c, 1.0, m, y0, y1, z, &blk);
      if (rc != SCAMD_OK) return rc;
      rc = cx.deflate(blk);
      if (rc != SCAMD_OK) return rc;
    }
    double* zq = blk == y0 ? y1 : y0;  // (tmp never joins the filter's rotation)
    rc = cholqr2(cx, blk, tmp, zq, false, 2);
    if (rc != SCAMD_OK) return rc;
    rc = rayleigh_ritz(cx, zq, mz, v, mv, h_theta);
    if (rc != SCAMD_OK) return rc;
  }
  run->outer = std::min(outer, max_outer);
  run->resid = resid;
  return SCAMD_OK;
}
}  // namespace scamd

extern "C" size_t scamd_spectral_embedding_workspace_bytes(int64_t n, int64_t nnz, int dim) {
  if (n < 1 || nnz < 0 || dim < 1 || dim + 6 > SP_MAXB) return 0;
  Workspace ws(nullptr, 0);
  SpectralBuffers sb;
  spectral_carve(ws, n, nnz, dim + 6, &sb);
  return ws.used();
}

extern "C" int scamd_spectral_embedding_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                            int64_t nnz, int dim, uint64_t seed, double tol, int max_outer, int max_degree,
                                            double* out, double* info_host, void* workspace, size_t workspace_bytes,
                                            scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && indices && weights && out, SCAMD_EINVAL, "spectral init: null pointer");
  SCAMD_REQUIRE(dim >= 1 && dim + 6 <= SP_MAXB, SCAMD_EUNSUPPORTED, "spectral init: %d components (at most %d)", dim, SP_MAXB - 6);
  SCAMD_REQUIRE(n > dim + 6 && n < ((int64_t)1 << 31) && nnz >= 1, SCAMD_EINVAL, "spectral init: bad shape n=%lld nnz=%lld",
                (long long)n, (long long)nnz);
  SpectralOp cx;
  cx.s = stream;
  cx.indptr = indptr;
  cx.indices = indices;
  cx.n = n;
  cx.dim = dim;
  cx.b = dim + 6;
  const int b = cx.b;
  Workspace ws(workspace, workspace_bytes);
  spectral_carve(ws, n, nnz, b, &cx.sb);
  cx.w = cx.sb.w;
  cx.sval = cx.sb.s;
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EWORKSPACE, "spectral init: workspace %zu < required %zu", workspace_bytes, ws.used());
  int rc = prepare_lds_kernels();
  if (rc != SCAMD_OK) return rc;
  HostReadbackScope readback_scope;  // (h_theta is the destination of a fetch handed out one synchronisation later)
  double h_theta[SP_MAXB];
  SpectralBuffers& sb = cx.sb;
  hipStream_t s = stream;
  // the operator: degrees, S = D^-1/2 A D^-1/2 in float32, the trivial eigenvector sqrt(deg)
  hipLaunchKernelGGL(sp_degree_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, indptr, weights, n, sb.deg);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_scale_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, indptr, indices, weights, n,
                     (const double*)sb.deg, sb.s, sb.t0);
  SCAMD_LAUNCH_CHECK();
  rc = cx.gram(sb.t0, 1, sb.t0, 1, sb.nrm2);
  if (rc != SCAMD_OK) return rc;
  SubspaceRun run;
  rc = graph_subspace_iteration(cx, eigensolver_seed(seed, 0x5bd1e995u), tol, max_outer, max_degree, h_theta, &run);
  if (rc != SCAMD_OK) return rc;
  hipLaunchKernelGGL(sp_take_kernel, dim3((unsigned)((n * dim + 255) / 256)), dim3(256), 0, s, (const double*)sb.pan[3], n, b, dim, out);
  SCAMD_LAUNCH_CHECK();
  SCAMD_READBACK_SYNC(s);
  if (info_host) {
    info_host[0] = (double)run.outer;
    info_host[1] = (double)cx.n_apply;
    info_host[2] = run.resid;
    info_host[3] = run.resid < tol ? 1.0 : 0.0;
    for (int j = 0; j < dim && j < 4; ++j) info_host[4 + j] = 2.0 * h_theta[j] - 1.0;  // eigenvalues of S
  }
  return SCAMD_OK;
}

// =====================================================================================================================
// Diffusion maps and diffusion pseudotime: `sc.tl.diffmap` / `sc.tl.dpt` (src/scanpy/neighbors/__init__.py:791-953).
//   * scamd_transitions_sym_f32: the density-normalised, symmetrised transition matrix T_sym of `compute_transitions` on the
//     pattern of the graph (float64 sums one wave per row, every entry rounded to float32 once);
//   * scamd_diffmap_f32: the n_comps leading eigenpairs of T_sym (`compute_eigen`: ARPACK on one host thread) by the
//     Chebyshev-filtered subspace iteration above on M = (T_sym + I) / 2, block b = n_comps + 6 <= 32 columns, nothing deflated:
//     the stationary eigenvector is column 0 of the answer.  Sign rule: the entry of largest magnitude of every column is
//     positive (lowest row on ties), applied here so that runs and machines agree.
//     ARPACK is asked for the largest MAGNITUDES, the filter finds the largest ALGEBRAIC values; they differ only when T_sym has
//     an eigenvalue below -lambda[n_comps - 1].  A second, cheap run of the same iteration on (I - T_sym) / 2 (block of 8, one
//     wanted pair, tol 1e-3) estimates lambda_min, and the entry refuses (SCAMD_EUNSUPPORTED) when -lambda_min >=
//     lambda[n_comps - 1].  A Ritz value approaches its eigenvalue from inside the spectrum, so the estimate bounds lambda_min
//     from ABOVE: the guard can prove a conflict, never the absence of one.
//   * scamd_dpt_pseudotime_f32: one row of the DPT distance matrix (`_get_dpt_row`), on request divided by its largest finite
//     entry (`_set_pseudotime`), float64 accumulation, the maximum by a two-stage reduction.
// =====================================================================================================================
namespace scamd {
constexpr int DM_GUARD_B = 8;      // block of the lambda_min run
constexpr double DM_GUARD_TOL = 1e-3;
constexpr int DPT_GRID = 1024;
constexpr int DPT_MAXC = 128;      // most diffusion components a pseudotime takes

// flag[0] |= 1 when a row stores nothing
__global__ void dm_empty_rows_kernel(const int64_t* __restrict__ indptr, int64_t n, int* __restrict__ flag) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n && indptr[v + 1] <= indptr[v]) atomicOr(flag, 1);
}
// ksum[v] = sum over the row of K_vu = w_vu / (dens_v dens_u) (float64, the lane-strided order of sp_degree_kernel)
__global__ __launch_bounds__(256) void dm_kernel_sum_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const float* __restrict__ w, int64_t n, const double* __restrict__ dens,
                                                            double* __restrict__ ksum) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n) return;
  const double dv = dens[v];
  double s = 0.0;
  for (int64_t e = indptr[v] + lane; e < indptr[v + 1]; e += 64) s += (double)w[e] / (dv * dens[indices[e]]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) ksum[v] = s;
}
// z[v] = sqrt(ksum[v]), t[e] = float(K_vu / (z_v z_u)); dens == nullptr: K = w (no density normalisation, ksum = the degrees).
// flag[0] |= 1 for a row whose sums are not positive and finite (an empty row, non-positive weights)
__global__ __launch_bounds__(256) void dm_transitions_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                             const float* __restrict__ w, int64_t n, const double* __restrict__ dens,
                                                             const double* __restrict__ ksum, float* __restrict__ t,
                                                             double* __restrict__ z, int* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n) return;
  const double kv = ksum[v], dv = dens ? dens[v] : 1.0;
  const double zv = sqrt(kv);
  if (lane == 0) {
    z[v] = zv;
    if (!(kv > 0.0 && kv < INFINITY && dv > 0.0)) atomicOr(flag, 1);
  }
  for (int64_t e = indptr[v] + lane; e < indptr[v + 1]; e += 64) {
    const int u = indices[e];
    const double k = dens ? (double)w[e] / (dv * dens[u]) : (double)w[e];
    t[e] = (float)(k / (zv * sqrt(ksum[u])));
  }
}

// part_v / part_i [blk][j] = the entry of largest magnitude of column j (< dim) over the block's rows and its row, the lowest
// row on ties; -1: the block has no row
__global__ __launch_bounds__(256) void dm_colmax_kernel(const double* __restrict__ v, int64_t n, int b, int dim,
                                                        double* __restrict__ part_v, int* __restrict__ part_i) {
  constexpr int W = SP_WIDEB, RL = 256 / W;
  __shared__ double rv[256];
  __shared__ int ri[256];
  const int j = threadIdx.x % W, rl = threadIdx.x / W;
  const int64_t rows_per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
  double best = 0.0;
  int bi = -1;
  if (j < dim) {
    for (int64_t r = r0 + rl; r < r1; r += RL) {  // (rows ascend: `>` keeps the lowest)
      const double x = v[r * b + j];
      if (bi < 0 || fabs(x) > fabs(best)) {
        best = x;
        bi = (int)r;
      }
    }
  }
  rv[threadIdx.x] = best;
  ri[threadIdx.x] = bi;
  __syncthreads();
  if (rl == 0 && j < dim) {
    for (int k = 1; k < RL; ++k) {
      const double x = rv[k * W + j];
      const int i = ri[k * W + j];
      if (i >= 0 && (bi < 0 || fabs(x) > fabs(best) || (fabs(x) == fabs(best) && i < bi))) {
        best = x;
        bi = i;
      }
    }
    part_v[(int64_t)blockIdx.x * dim + j] = best;
    part_i[(int64_t)blockIdx.x * dim + j] = bi;
  }
}
// sign[j] = -1 if the entry of largest magnitude of column j is negative, else 1 (blocks in index order = rows ascending);
// evals[j] = 2 theta[j] - 1: the eigenvalue of T_sym behind the Ritz value of M
__global__ void dm_sign_kernel(const double* __restrict__ part_v, const int* __restrict__ part_i, int nblk, int dim,
                               const double* __restrict__ theta, double* __restrict__ sign, double* __restrict__ evals) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= dim) return;
  double best = 0.0;
  bool have = false;
  for (int blk = 0; blk < nblk; ++blk) {
    if (part_i[(int64_t)blk * dim + j] < 0) continue;
    const double x = part_v[(int64_t)blk * dim + j];
    if (!have || fabs(x) > fabs(best)) {
      best = x;
      have = true;
    }
  }
  sign[j] = best < 0.0 ? -1.0 : 1.0;
  evals[j] = 2.0 * theta[j] - 1.0;
}
// out[row][j] = sign[j] v[row][j], j < dim (row stride b -> dim)
__global__ void dm_take_kernel(const double* __restrict__ v, const double* __restrict__ sign, int64_t n, int b, int dim,
                               double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * dim) return;
  const int64_t row = e / dim;
  const int j = (int)(e - row * dim);
  out[e] = sign[j] * v[row * b + j];
}

struct DiffmapBuffers {
  SpectralBuffers sb;
  int* part_i;
  double* sign;
};
static void diffmap_carve(Workspace& ws, int64_t n, int b, DiffmapBuffers* db) {
  spectral_carve(ws, n, 0, std::max(b, DM_GUARD_B), &db->sb);  // (T_sym is the caller's: sb.s stays unused)
  db->part_i = ws.take<int>((size_t)SP_GRID * SP_WIDEB);
  db->sign = ws.take<double>(SP_WIDEB);
}

// d[v] = sqrt(sum_j wgt_j (basis[iroot][j] - basis[v][j])^2), wgt_j = (lambda_j / (1 - lambda_j))^2 for lambda_j < 0.9994, else
// 1 (float64, j ascending); +inf outside the root's component (labels != nullptr); part[blk] = largest finite d of the block
__global__ __launch_bounds__(256) void dpt_row_kernel(const float* __restrict__ evals, const float* __restrict__ basis, int64_t n,
                                                      int n_dcs, int64_t ld, int64_t iroot, const int32_t* __restrict__ labels,
                                                      double* __restrict__ d, double* __restrict__ part) {
  __shared__ double wgt[DPT_MAXC], root[DPT_MAXC], red[256];
  for (int j = threadIdx.x; j < n_dcs; j += 256) {
    const double lam = (double)evals[j];
    const double q = lam / (1.0 - lam);
    wgt[j] = lam < 0.9994 ? q * q : 1.0;
    root[j] = (double)basis[iroot * ld + j];
  }
  __syncthreads();
  const int root_label = labels ? labels[iroot] : 0;
  const int64_t rows_per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
  double mx = 0.0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
    double acc = 0.0;
    for (int j = 0; j < n_dcs; ++j) {
      const double df = root[j] - (double)basis[r * ld + j];
      acc = fma(wgt[j] * df, df, acc);
    }
    double val = sqrt(acc);
    if (labels && labels[r] != root_label) val = INFINITY;
    d[r] = val;
    if (val < INFINITY && val > mx) mx = val;
  }
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
// part[nblk] = max over part[0 .. nblk)
__global__ __launch_bounds__(256) void dpt_max_kernel(double* __restrict__ part, int nblk) {
  __shared__ double red[256];
  double mx = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) mx = fmax(mx, part[i]);
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[nblk] = red[0];
}
// out[v] = float(d[v] / max), or float(d[v]) with mx == nullptr: rounded to float32 once
__global__ void dpt_scale_kernel(const double* __restrict__ d, const double* __restrict__ mx, int64_t n, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) out[v] = mx ? (float)(d[v] / mx[0]) : (float)d[v];
}
struct DptBuffers {
  double* d; double* part;
};
static void dpt_carve(Workspace& ws, int64_t n, DptBuffers* b) {
  b->d = ws.take<double>((size_t)n);
  b->part = ws.take<double>(DPT_GRID + 1);
}
}  // namespace scamd

extern "C" size_t scamd_transitions_sym_workspace_bytes(int64_t n, int64_t nnz) {
  if (n < 1 || nnz < 0) return 0;
  Workspace ws(nullptr, 0);
  ws.take<double>((size_t)n);
  ws.take<double>((size_t)n);
  ws.take<int>(8);
  return ws.used();
}

extern "C" int scamd_transitions_sym_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                         int64_t nnz, int density_normalize, float* t_sym, double* z, void* workspace,
                                         size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && indices && weights && t_sym && z, SCAMD_EINVAL, "transitions: null pointer");
  SCAMD_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && nnz >= 1, SCAMD_EINVAL, "transitions: bad shape n=%lld nnz=%lld", (long long)n,
                (long long)nnz);
  Workspace ws(workspace, workspace_bytes);
  double* dens = ws.take<double>((size_t)n);
  double* ksum = ws.take<double>((size_t)n);
  int* flag = ws.take<int>(8);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EWORKSPACE, "transitions: workspace %zu < required %zu", workspace_bytes, ws.used());
  hipStream_t s = stream;
  HostReadbackScope readback_scope;
  const unsigned grid = (unsigned)((n + 3) / 4);
  SCAMD_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), s));
  // dens = the column sums of the symmetric graph = its row sums
  hipLaunchKernelGGL(sp_degree_kernel, dim3(grid), dim3(256), 0, s, indptr, weights, n, dens);
  SCAMD_LAUNCH_CHECK();
  if (density_normalize) {
    hipLaunchKernelGGL(dm_kernel_sum_kernel, dim3(grid), dim3(256), 0, s, indptr, indices, weights, n, (const double*)dens, ksum);
    SCAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(dm_transitions_kernel, dim3(grid), dim3(256), 0, s, indptr, indices, weights, n,
                     density_normalize ? (const double*)dens : (const double*)nullptr,
                     density_normalize ? (const double*)ksum : (const double*)dens, t_sym, z, flag);
  SCAMD_LAUNCH_CHECK();
  int bad = 0;
  SCAMD_READBACK_NOW(&bad, flag, sizeof(int), s);
  SCAMD_REQUIRE(!bad, SCAMD_EUNSUPPORTED, "transitions: a row of the graph has no positive weight (empty row?)");
  return SCAMD_OK;
}

extern "C" size_t scamd_diffmap_workspace_bytes(int64_t n, int64_t nnz, int n_comps) {
  if (n < 1 || nnz < 0 || n_comps < 1 || n_comps + 6 > SP_WIDEB) return 0;
  Workspace ws(nullptr, 0);
  DiffmapBuffers db;
  diffmap_carve(ws, n, n_comps + 6, &db);
  return ws.used();
}

extern "C" int scamd_diffmap_f32(const int64_t* indptr, const int32_t* indices, const float* t_sym, int64_t n, int64_t nnz,
                                 int n_comps, uint64_t seed, double tol, int max_outer, int max_degree, double* evals,
                                 double* evecs, double* info_host, void* workspace, size_t workspace_bytes,
                                 scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && indices && t_sym && evals && evecs, SCAMD_EINVAL, "diffmap: null pointer");
  SCAMD_REQUIRE(n_comps >= 1 && n_comps + 6 <= SP_WIDEB, SCAMD_EUNSUPPORTED, "diffmap: %d components (1 to %d)", n_comps,
                SP_WIDEB - 6);
  SCAMD_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && nnz >= 1, SCAMD_EINVAL, "diffmap: bad shape n=%lld nnz=%lld", (long long)n,
                (long long)nnz);
  const int b = n_comps + 6;
  SCAMD_REQUIRE(n > std::max(b, DM_GUARD_B), SCAMD_EUNSUPPORTED, "diffmap: %lld cells, a block of %d columns needs more",
                (long long)n, std::max(b, DM_GUARD_B));
  DiffmapOp cx;
  cx.s = stream;
  cx.indptr = indptr;
  cx.indices = indices;
  cx.sval = t_sym;
  cx.n = n;
  cx.dim = n_comps;
  cx.b = b;
  cx.who = "diffmap";
  Workspace ws(workspace, workspace_bytes);
  DiffmapBuffers db;
  diffmap_carve(ws, n, b, &db);
  cx.sb = db.sb;
  cx.w = db.sb.w;
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EWORKSPACE, "diffmap: workspace %zu < required %zu", workspace_bytes, ws.used());
  int rc = prepare_lds_kernels();
  if (rc != SCAMD_OK) return rc;
  HostReadbackScope readback_scope;
  hipStream_t s = stream;
  int* empty_flag = cx.w.flags + 4;
  SCAMD_HIP_CHECK(hipMemsetAsync(empty_flag, 0, sizeof(int), s));
  hipLaunchKernelGGL(dm_empty_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, indptr, n, empty_flag);
  SCAMD_LAUNCH_CHECK();
  int has_empty = 0;
  SCAMD_READBACK_NOW(&has_empty, empty_flag, sizeof(int), s);
  SCAMD_REQUIRE(!has_empty, SCAMD_EUNSUPPORTED, "diffmap: the transition matrix has an empty row");
  // the n_comps largest eigenvalues of T_sym
  double h_theta[SP_WIDEB];
  SubspaceRun run;
  rc = graph_subspace_iteration(cx, eigensolver_seed(seed, 0x2545f491u), tol, max_outer, max_degree, h_theta, &run);
  if (rc != SCAMD_OK) return rc;
  const int g = cx.grid_rows();
  const double* v = db.sb.pan[3];
  hipLaunchKernelGGL(dm_colmax_kernel, dim3(g), dim3(256), 0, s, v, n, b, n_comps, db.sb.part, db.part_i);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(dm_sign_kernel, dim3(1), dim3(SP_WIDEB), 0, s, (const double*)db.sb.part, (const int*)db.part_i, g, n_comps,
                     (const double*)cx.w.theta, db.sign, evals);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(dm_take_kernel, dim3((unsigned)((n * n_comps + 255) / 256)), dim3(256), 0, s, v, (const double*)db.sign, n, b,
                     n_comps, evecs);
  SCAMD_LAUNCH_CHECK();
  SCAMD_READBACK_SYNC(s);  // (the last theta of a run that ended by max_outer)
  // the guard: the largest Ritz value of (I - T_sym) / 2 on a small block bounds lambda_min from above
  DiffmapOp gx = cx;
  gx.sgn = -1.0;
  gx.b = DM_GUARD_B;
  gx.dim = 1;
  gx.who = "diffmap guard";
  gx.n_apply = 0;
  gx.n_chol_retry = 0;
  double g_theta[SP_WIDEB];
  SubspaceRun grun;
  rc = graph_subspace_iteration(gx, eigensolver_seed(seed, 0x9e3779b9u), DM_GUARD_TOL, max_outer, max_degree, g_theta, &grun);
  if (rc != SCAMD_OK) return rc;
  SCAMD_READBACK_SYNC(s);
  const double lam_last = 2.0 * h_theta[n_comps - 1] - 1.0, lam_min = 1.0 - 2.0 * g_theta[0];
  const bool conflict = -lam_min >= lam_last;
  if (info_host) {
    info_host[0] = (double)run.outer;
    info_host[1] = (double)cx.n_apply;
    info_host[2] = run.resid;  // of the Ritz pairs of M = (T_sym + I) / 2: half the residual of the pairs of T_sym
    info_host[3] = run.resid < tol ? 1.0 : 0.0;
    info_host[4] = lam_min;
    info_host[5] = (double)gx.n_apply;
    info_host[6] = conflict ? 1.0 : 0.0;
    info_host[7] = (double)(cx.n_chol_retry + gx.n_chol_retry);
  }
  SCAMD_REQUIRE(!conflict, SCAMD_EUNSUPPORTED,
                "diffmap: T_sym has an eigenvalue <= %.6f, of larger magnitude than the last requested one (%.6f): the largest-"
                "magnitude and the largest-algebraic eigenpairs differ",
                lam_min, lam_last);
  return SCAMD_OK;
}

extern "C" size_t scamd_dpt_pseudotime_workspace_bytes(int64_t n) {
  if (n < 1) return 0;
  Workspace ws(nullptr, 0);
  DptBuffers b;
  dpt_carve(ws, n, &b);
  return ws.used();
}

extern "C" int scamd_dpt_pseudotime_f32(const float* evals, const float* basis, int64_t n, int n_dcs, int64_t ld, int64_t iroot,
                                        const int32_t* labels, int scale, float* out, void* workspace, size_t workspace_bytes,
                                        scamd_stream_t stream) {
  SCAMD_REQUIRE(evals && basis && out, SCAMD_EINVAL, "dpt: null pointer");
  SCAMD_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && n_dcs >= 1 && n_dcs <= DPT_MAXC && ld >= n_dcs && iroot >= 0 && iroot < n,
                SCAMD_EINVAL, "dpt: bad shape n=%lld n_dcs=%d ld=%lld iroot=%lld (at most %d components)", (long long)n, n_dcs,
                (long long)ld, (long long)iroot, DPT_MAXC);
  Workspace ws(workspace, workspace_bytes);
  DptBuffers b;
  dpt_carve(ws, n, &b);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EWORKSPACE, "dpt: workspace %zu < required %zu", workspace_bytes, ws.used());
  hipStream_t s = stream;
  const int g = (int)std::min<int64_t>(DPT_GRID, (n + 255) / 256);
  hipLaunchKernelGGL(dpt_row_kernel, dim3(g), dim3(256), 0, s, evals, basis, n, n_dcs, ld, iroot, labels, b.d, b.part);
  SCAMD_LAUNCH_CHECK();
  if (scale) {
    hipLaunchKernelGGL(dpt_max_kernel, dim3(1), dim3(256), 0, s, b.part, g);
    SCAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(dpt_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)b.d,
                     scale ? (const double*)(b.part + g) : (const double*)nullptr, n, out);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}
