// Chebyshev-filtered subspace iteration (Zhou & Saad), its steps written ONCE over an operator: CholeskyQR2 with shifted rounds,
// Rayleigh-Ritz by the one-workgroup Jacobi, the degree rule and the filter.  Two operators use them (dense.hip): the dense
// float64 matrix of the PCA (`DenseOp`: Gram matrices and products on the f64 MFMA GEMM) and the normalised graph of the
// spectral initialisation (`SpectralOp`: float32 SpMM, two-stage tall Gram sums, the trivial eigenvector projected out);
// `DiffmapOp` is the latter on a stored transition matrix with nothing projected out.
// The outer iterations stay with the two drivers (dense_topk; graph_subspace_iteration for both graph operators): their
// prologues, residuals, stop rules and degenerate-block steps differ, and a shared loop would need a hook for each.
//
// Included by dense.hip AFTER the kernels these steps launch (chol_factor_kernel, panel_small_kernel, jacobi_eigh_kernel,
// axpby_kernel); it is not a stand-alone header.
//
// An operator `Op` has
//   int64_t rows() const        rows of a panel (panels are rows x b, row-major)
//   int b                       block width
//   hipStream_t s
//   SubspaceScratch w           the b x b matrices, the Ritz values and the flag words (device)
//   const char* who             the caller's name in error texts
//   int n_chol_retry            failed Cholesky attempts so far
//   int gram(p, bp, q, bq, out)                       out [bp x bq] = p^T q
//   int apply(y, yprev, a, center, bcoef, out)        out = a (A y - center y) - bcoef yprev: one step of the three-term
//                                                     recurrence; yprev == nullptr: out = A y
//   int deflate(y)                                    projects the known eigenvectors out of y (nothing for the dense operator)
#pragma once

namespace scamd {

struct SubspaceScratch {
  double* gm; double* smat; double* tmat; double* ymat;  // Gram matrix, CholeskyQR factor, projected operator, its eigenvectors
  double* theta;                                         // Ritz values, descending
  int* flags;                                            // [0] failed pivot (chol_factor_kernel), [1] Jacobi sweeps
};

static constexpr size_t CHOL_LDS = (size_t)(DB_MAX * DB_LD + DB_MAX) * sizeof(double);
static constexpr size_t JAC_LDS = (size_t)(DB_MAX * DB_LD + DB_MAX) * sizeof(double);
static constexpr size_t PANEL_LDS_MAX = (size_t)panel_lds_doubles(DB_MAX, 5) * sizeof(double);

// the LDS-resident kernels take more dynamic LDS than the default limit: once per entry, before the first launch
static int prepare_lds_kernels() {
  SCAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(chol_factor_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)CHOL_LDS));
  SCAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(jacobi_eigh_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)JAC_LDS));
  SCAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(panel_small_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)PANEL_LDS_MAX));
  return SCAMD_OK;
}

// seed of the start block's generator from the caller's 64-bit seed; `salt` keeps the entry points apart
static unsigned int eigensolver_seed(uint64_t seed, unsigned int salt) {
  return (unsigned int)(seed ^ (seed >> 32)) * 0x9E3779B1u + salt;
}

// c0 [rows x bo] = z0 [rows x b] small [b x bo]; with z1: also c1 = z1 small, in the same launch (after prepare_lds_kernels)
static int panel_small(hipStream_t s, const double* z0, const double* z1, const double* small, int64_t rows, int b, int bo,
                       double* c0, double* c1) {
  int cq_shift = 0;
  while ((4 << cq_shift) < bo) ++cq_shift;  // column quads per row group, a power of two
  SCAMD_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31) && b >= 1 && bo >= 1 && bo <= DB_MAX && b <= (4 << cq_shift), SCAMD_EINVAL,
                "panel product: bad shape rows=%lld b=%d bo=%d", (long long)rows, b, bo);
  const int rows_per = 2 * (256 >> cq_shift);
  hipLaunchKernelGGL(panel_small_kernel, dim3((unsigned)((rows + rows_per - 1) / rows_per), z1 ? 2 : 1), dim3(256),
                     (size_t)panel_lds_doubles(b, cq_shift) * sizeof(double), s, z0, z1, small, (int)rows, b, bo, cq_shift, c0, c1);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}
template <class Op>
static int panel_times_small(Op& op, const double* z, const double* small, double* out) {
  return panel_small(op.s, z, nullptr, small, op.rows(), op.b, op.b, out, nullptr);
}

// zout = orthonormal basis of span(zin) by CholeskyQR2: `plain_rounds` rounds of (Gram matrix, Cholesky factor, block times
// factor).  A failed pivot (the block is a Chebyshev-filtered one: kappa 1e9 and beyond, up to numerical rank deficiency) inserts
// a SHIFTED round (Fukaya et al. 2020: factor G + s I, s ~ 11 (rows b + b (b + 1)) u |Y|^2; every such round divides kappa by
// ~1 / sqrt(s) ~ 3e3) and starts the count of plain rounds again; directions that were lost to rounding come back as
// orthonormal noise, as they do from a Householder QR.  zin and tmp are overwritten; zin, tmp, zout are distinct panels, and
// the last plain round writes zout.
// filtered = the block comes out of a Chebyshev filter of full degree: its plain first round fails (kappa 1e16 and beyond: the
// solve of the bench spent two Cholesky launches and their read-backs on finding that out), so the first round is shifted at once.
// (chol_factor_kernel writes its flag either way: nothing clears it.  The flag's read-back resets the read-back queue, so no
// split fetch may be pending here: CholeskyQR comes BEFORE the Rayleigh-Ritz of an iteration, never between it and its sync.)
template <class Op>
static int cholqr2(Op& op, double* zin, double* tmp, double* zout, bool filtered, int plain_rounds) {
  const int b = op.b;
  double* cur = zin;
  double* other = tmp;
  int plain_ok = 0, shifted_rounds = 0;
  const double s0 = 11.0 * ((double)op.rows() * b + (double)b * (b + 1)) * 2.220446049250313e-16 * b;
  while (plain_ok < plain_rounds) {
    int rc = op.gram(cur, b, cur, b, op.w.gm);
    if (rc != SCAMD_OK) return rc;
    double shift = (filtered && plain_ok == 0 && shifted_rounds == 0) ? s0 : 0.0;
    for (int attempt = shift > 0.0 ? 1 : 0;; ++attempt) {
      int bad = 0;
      hipLaunchKernelGGL(chol_factor_kernel, dim3(1), dim3(1024), CHOL_LDS, op.s, op.w.gm, b, shift, op.w.smat, op.w.flags);
      SCAMD_LAUNCH_CHECK();
      SCAMD_READBACK_NOW(&bad, op.w.flags, sizeof(int), op.s);
      if (!bad) break;
      SCAMD_REQUIRE(attempt < 4 && shifted_rounds < 8, SCAMD_EUNSUPPORTED,
                    "%s: CholeskyQR gave up on the block (%d shifted rounds, attempt %d)", op.who, shifted_rounds, attempt);
      shift = shift == 0.0 ? s0 : shift * 1e3;
      ++op.n_chol_retry;
    }
    const bool was_shifted = shift > 0.0;
    double* dst = (!was_shifted && plain_ok == plain_rounds - 1) ? zout : other;
    rc = panel_times_small(op, cur, op.w.smat, dst);
    if (rc != SCAMD_OK) return rc;
    if (dst == other) std::swap(cur, other);
    if (was_shifted) {
      plain_ok = 0;
      ++shifted_rounds;
    } else {
      ++plain_ok;
    }
  }
  return SCAMD_OK;
}

// Rayleigh-Ritz on the orthonormal block z: az = A z, T = z^T az = Y diag(theta) Y^T, v = z Y, av = az Y.  theta is queued for
// the host (h_theta [b]) and handed out by the caller's next SCAMD_READBACK_SYNC.
template <class Op>
static int rayleigh_ritz(Op& op, const double* z, double* az, double* v, double* av, double* h_theta) {
  const int b = op.b;
  int rc = op.apply(z, nullptr, 1.0, 0.0, 0.0, az);
  if (rc != SCAMD_OK) return rc;
  rc = op.gram(z, b, az, b, op.w.tmat);
  if (rc != SCAMD_OK) return rc;
  // (T is symmetrised as the Jacobi kernel loads it; v and av come out of one launch)
  hipLaunchKernelGGL(jacobi_eigh_kernel, dim3(1), dim3(512), JAC_LDS, op.s, op.w.tmat, b, 1, op.w.theta, op.w.ymat, op.w.flags + 1);
  SCAMD_LAUNCH_CHECK();
  rc = panel_small(op.s, z, az, op.w.ymat, op.rows(), b, b, v, av);
  if (rc != SCAMD_OK) return rc;
  SCAMD_READBACK(h_theta, op.w.theta, sizeof(double) * b, op.s);
  return SCAMD_OK;
}

// Degree of a filter that damps [0, c] on a spectrum reaching up to `top`, theta_k = the smallest wanted Ritz value.  The filter
// grows like cosh(m acosh x), x = (lambda - center) / e, so the LARGEST wanted eigenvalue is amplified
// exp(m (acosh x_1 - acosh x_k)) times more than the smallest wanted one.  Beyond ~1e9 every column is the leading eigenvector
// plus rounding noise and the k-th pair never converges (seen with k = 40 on a matrix with 29 separated eigenvalues above a
// bulk: residual stuck at 1e-7, a Cholesky retry every iteration).  Hence floor(20.7 / spread), inside [4, max_degree].
static int chebyshev_degree(double c, double top, double theta_k, int max_degree) {
  const double e = 0.5 * c, center = 0.5 * c;
  const double x1 = (top - center) / e, xk = std::max((theta_k - center) / e, 1.0);
  const double spread = std::acosh(x1) - std::acosh(xk);
  return spread > 0.0 ? std::max(4, std::min(max_degree, (int)std::floor(20.7 / spread))) : max_degree;
}

// One Chebyshev filter of degree m on the block (vv, avv = A vv), damping [0, c] and scaled to ~1 at `top`.  The iterates
// rotate through the panels y0, y1 and z; *result = the one that holds the last.  vv / avv are left intact.
template <class Op>
static int chebyshev_filter(Op& op, const double* vv, const double* avv, double c, double top, int m, double* y0, double* y1, double* z,
                            double** result) {
  const int64_t cnt = op.rows() * op.b;
  const double e = 0.5 * c, center = 0.5 * c;
  double sigma = e / (top - center);
  const double sigma1 = sigma;
  // y = (avv - center vv) sigma1 / e
  hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, op.s, cnt, sigma1 / e, avv, -center * sigma1 / e,
                     vv, y0);
  SCAMD_LAUNCH_CHECK();
  const double* yprev = vv;
  double* ycur = y0;
  double* ynew = y1;
  for (int it = 2; it <= m; ++it) {
    const double sigma2 = 1.0 / (2.0 / sigma1 - sigma);
    const int rc = op.apply(ycur, yprev, 2.0 * sigma2 / e, center, sigma * sigma2, ynew);
    if (rc != SCAMD_OK) return rc;
    double* old = (yprev == vv) ? z : const_cast<double*>(yprev);  // vv is never written: z joins the rotation
    yprev = ycur;
    ycur = ynew;
    ynew = old;
    sigma = sigma2;
  }
  *result = ycur;
  return SCAMD_OK;
}

}  // namespace scamd
