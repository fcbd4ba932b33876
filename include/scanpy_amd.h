/*
 * scanpy_amd.h -- C ABI of libscanpy_amd.so (MI355X / gfx950 kernels for the
 * sc.pp.pca -> sc.pp.neighbors -> sc.tl.leiden path).
 *
 * The reference (scverse/scanpy) is pure Python and has no FFI of its own; the entry
 * points below are the native boundary a binding for that path would call.  Each one
 * cites the reference code whose arithmetic it replaces (paths relative to the scanpy
 * source tree).  Conventions:
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - the caller owns all buffers (inputs, outputs, workspace); the library allocates
 *     nothing that outlives a call and never frees caller memory;
 *   - `stream` is a hipStream_t; work is enqueued on it.  Calls that must report a
 *     data-dependent size (`*_host` outputs) synchronise that stream before returning;
 *   - return value: 0 on success, a negative SCAMD_E* code otherwise, with a
 *     human-readable message available from scamd_last_error() (thread-local);
 *   - no C++ exceptions cross the boundary; one host thread per device.
 *   - row-major everywhere; CSR = (indptr int64[n+1], indices int32[nnz], data f32[nnz]).
 */
#ifndef SCANPY_AMD_H
#define SCANPY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* scamd_stream_t; /* == hipStream_t */

#define SCAMD_OK 0
#define SCAMD_EINVAL (-1)     /* bad argument */
#define SCAMD_EWORKSPACE (-2) /* workspace too small */
#define SCAMD_EHIP (-3)       /* HIP runtime error */
#define SCAMD_EUNSUPPORTED (-4)
#define SCAMD_ECAPACITY (-5)  /* caller-provided output capacity too small */
#define SCAMD_EINTERNAL (-6)  /* internal invariant violated (reported, never hidden) */

#define SCAMD_ABI_VERSION 1

int scamd_abi_version(void);
const char* scamd_last_error(void);
/* Number of HIP devices visible (0 on a CPU-only host); never fails. */
int scamd_device_count(void);

/* ------------------------------------------------------------------------------------------
 * kNN -- exact brute-force Euclidean k-nearest-neighbours of a row range of X against all of X.
 * Replaces sklearn KNeighborsTransformer(algorithm='brute') as called at
 * src/scanpy/neighbors/__init__.py:754-768 (reference `transformer='sklearn'` path) together with
 * the self-column handling of src/scanpy/neighbors/_common.py:74-98 and the in-place diagonal
 * zeroing at neighbors/__init__.py:644.
 *
 *   x        [n, d] float32, row stride ld_x (elements)
 *   queries  rows q_begin .. q_begin+n_query-1 of x (a rank's row shard; the whole matrix on 1 GPU)
 *   k        columns to return.  Column 0 is the query itself with distance exactly 0, columns
 *            1..k-1 its k-1 nearest OTHER rows ordered by (distance, index) -- i.e. what the
 *            reference feeds to the connectivity step for n_neighbors = k.
 *   out_idx  [n_query, k] int32   (-1 where fewer than k-1 other rows exist)
 *   out_dist [n_query, k] float64 Euclidean distance, sqrt of the float64 sum of squared
 *            float64 differences of the float32 inputs (+inf for missing entries)
 *   n_fallback_host  (optional, host) number of queries whose candidate list could not be
 *            certified by the float32 MFMA pass and were recomputed by the float64 scan.
 *   cert_scale  1.0 normally; >1 widens the certification margin (tests use a huge value to force
 *            every query through the float64 fallback scan).
 * Exactness: pass 1 (FP32 MFMA, ||c||^2 - 2 q.c) keeps KP > k candidates per query; pass 2 re-ranks
 * them in float64; a query is accepted only if its k-th exact distance is provably below every
 * rejected candidate given the float32 rounding bound, otherwise pass 3 rescans it in float64.
 * Ties, however many rows share the k-th distance, are broken by the lower row index in every pass.
 * ---------------------------------------------------------------------------------------- */
size_t scamd_knn_workspace_bytes(int64_t n, int d, int64_t n_query, int k);
int scamd_knn_l2_f32(const float* x, int64_t n, int d, int64_t ld_x,
                     int64_t q_begin, int64_t n_query, int k,
                     int32_t* out_idx, double* out_dist,
                     double cert_scale, int64_t* n_fallback_host,
                     void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Approximate variant -- BASELINE.json configs[4] ("IVF-tiled approximate kNN"); the reference's own default above 8192
 * cells is approximate as well (pynndescent, src/scanpy/neighbors/__init__.py:734-739, 769-781).  Same arguments and
 * output conventions as scamd_knn_l2_f32, plus
 *   nprobe   every query sees the rows of the nprobe cells of the k-means quantiser nearest (centroid distance) to its
 *            own cell -- ~2048 rows per cell, at most 1024 cells.  Inside the probed cells the search IS the exact one
 *            (same kernels, float64 re-rank, certificate): a list is the true nearest neighbours among the probed rows,
 *            OR BETTER -- a query whose certificate fails (n_fallback_host counts them) is scanned in float64 over every
 *            cell within its bound, probed or not, and comes back with its exact list over all rows.  So at every rank the
 *            distance is at most that of the best list of the probed rows, at most n_fallback_host lists differ from that
 *            list, and recall < 1 comes from unprobed cells only (tests/knn_cell_cases.py: check_promise).  nprobe <= 0: the
 *            exact search; nprobe >= the cell count: every cell is probed, the exact lists.
 * Answered exactly as well: n < 4096, k > 24, d > 64 (shapes outside the register-list kernel).  Workspace:
 * scamd_knn_workspace_bytes (one figure for both entry points). */
int scamd_knn_l2_ivf_f32(const float* x, int64_t n, int d, int64_t ld_x,
                         int64_t q_begin, int64_t n_query, int k, int nprobe,
                         int32_t* out_idx, double* out_dist, int64_t* n_fallback_host,
                         void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Duration (ms, HIP events on `stream`) of the FP32-MFMA selection kernel of the calling thread's most
 * recent scamd_knn_l2_f32 call; -1 if none.  Used by bench.py for the roofline figure. */
float scamd_knn_last_select_ms(void);
/* (query, candidate) pairs that call's selection kernel evaluated: n_query * n for the brute-force sweep, fewer when
 * the cell-pruned search (n >= 65536) could skip far cells (the threshold pre-pass not included); -1 if none.
 * Useful flop = 2 * d * pairs. */
double scamd_knn_last_select_pairs(void);
/* Pairs the same kernel evaluated in its threshold pre-pass (the own cell of every block, scored once more only to seed
 * the list thresholds): executed by the kernel, NOT useful work -- kept out of the roofline's algorithmic flop. */
double scamd_knn_last_select_prepass_pairs(void);
/* Scoring engine of that call's selection kernel: 0 = float32 MFMA (v_mfma_f32_32x32x2_f32, 2 (d + 2) flop per pair),
 * 1 = 3 x bf16 (v_mfma_f32_32x32x16_bf16 on the hi / lo split of the coordinates: 3 * 2 * 64 flop per pair; 32 < d <= 50,
 * SCAMD_KNN_B3=0 disables it); -1 if none.  Either way pass 2 certifies the result in float64. */
int scamd_knn_last_select_engine(void);
/* Queries of that call that the bf16 engine's certificate rejected and the float32 engine re-did (second tier of the
 * pruned search; 0 when the count stayed below SCAMD_KNN_TIER2_MIN, default 256, or the float32 engine ran anyway).
 * `n_fallback_host` of scamd_knn_l2_f32 counts what went to the float64 scan after that. */
int scamd_knn_last_second_tier_queries(void);
/* cells probed by this thread's last search: 0 = it was answered EXACTLY -- also when scamd_knn_l2_ivf_f32 was asked for a
 * shape its register-list kernel does not take (k > 24, d > 64, n < 4096); the Python layer tells the user. */
int scamd_knn_last_nprobe(void);
/* 1 if this thread's last pruned sweep ran with the coarse first stage (hi.hi product first, the other two products only for
 * sub-tiles with a coarse survivor: chosen when the cell bounds prune little; same lists either way). */
int scamd_knn_last_coarse(void);
/* The certificate's error-bound factors of an engine (0 = float32, 1 = 3 x bf16), in units of u = 2^-24:
 *   |score_engine - score_exact| <= u * (cert_k * (||c||^2 + 2 ||q|| ||c||) + cert_k2 * 2 ||q|| ||c||) (+ key_slack * u * |tau|
 * for the slot bits of the list keys).  Read by the test that measures the bound (tests/test_gpu_knn_certificate.py). */
void scamd_knn_cert_factors(int engine, double* cert_k, double* cert_k2, double* key_slack);
/* Test entry: raw scores ||c||^2 - 2 q.c (centred frame) of the bf16 engine for queries [q0, q0 + nq) x candidates
 * [c0, c0 + nc) of x [n, d <= 50] (both counts multiples of 32), through the select kernel's own image packing, operand
 * construction and MFMA chain.  out_scores [nq, nc] float32; out_mu [128] (the column means the image was centred with) and
 * out_cmax [1] (largest ||x - mu||^2) may be NULL.  Not part of the search; measures the engine's arithmetic error. */
size_t scamd_knn_debug_b3_scores_workspace_bytes(int64_t n);
int scamd_knn_debug_b3_scores_f32(const float* x, int64_t n, int d, int64_t ld_x, int64_t q0, int nq, int64_t c0, int nc,
                                  float* out_scores, float* out_mu, float* out_cmax, void* workspace,
                                  size_t workspace_bytes, scamd_stream_t stream);
/* Test entry: the cell tables a pruned or approximate search used (tests/knn_cell_cases.py).  `workspace` is the workspace
 * of a scamd_knn_l2_f32 / scamd_knn_l2_ivf_f32 call that has just returned SCAMD_OK, the shape arguments, nprobe (0 for the
 * exact entry) and the SCAMD_KNN_* environment are that call's.  The tables are located by the call's own plan and copied out
 * device to device; no kernel of the search runs.  SCAMD_EINVAL when that plan has no cells (brute force, or a shape the
 * approximate entry answers exactly), before anything is read.  Sizes come from the host-only companion
 * scamd_knn_debug_cell_tables_sizes: the cell count nc and the upper bound n_img_max of the image rows.
 *   out_labels [n] the quantiser's cell of every row, out_row_cell [n] = out_cell_map[out_labels[i]] (small cells are folded
 *   into their nearest big cell), out_cell_map [nc], out_cent [nc, d], out_radius [nc], out_tile0 / out_ntiles [nc] (tiles of
 *   64 image rows), out_order / out_lb2 [nc, nc] (row a: the cells in a's sweep order and their squared lower bounds),
 *   out_perm [n_img_max] of which the first *n_img_rows_host entries are written (image row -> row of x, -1 = padding). */
int scamd_knn_debug_cell_tables_sizes(int64_t n, int d, int64_t n_query, int k, int nprobe, int* n_cells, int64_t* n_img_max);
int scamd_knn_debug_cell_tables(int64_t n, int d, int64_t n_query, int k, int nprobe, const void* workspace,
                                size_t workspace_bytes, int32_t* out_labels, int32_t* out_row_cell, int32_t* out_cell_map,
                                float* out_cent, float* out_radius, int32_t* out_tile0, int32_t* out_ntiles, int32_t* out_order,
                                float* out_lb2, int32_t* out_perm, int64_t* n_img_rows_host, scamd_stream_t stream);
/* TEST ENTRY: the tables only the exact pruned search builds (nprobe <= 0; SCAMD_EINVAL after a call of the approximate
 * mode), read from the same workspace in the same way, copies only.  The exact sweep follows max(ball bound, projection
 * bound) between cells: out_reach [nc, nc], reach[p][o] = max over the members x of p of (x - c_p).(c_o - c_p) for the cells
 * o of p's short list and +inf elsewhere; out_list_len [nc], the short list of p being the first out_list_len[p] entries of
 * p's ball row (out_order above); out_sweep_order / out_sweep_lb2 [nc, nc], the rows the sweep followed, under the
 * conventions of out_order / out_lb2. */
int scamd_knn_debug_sweep_tables(int64_t n, int d, int64_t n_query, int k, int nprobe, const void* workspace,
                                 size_t workspace_bytes, float* out_reach, int32_t* out_list_len, int32_t* out_sweep_order,
                                 float* out_sweep_lb2, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fuzzy simplicial set -- umap connectivities from a kNN result.
 * Replaces umap.umap_.fuzzy_simplicial_set(..., set_op_mix_ratio=1, local_connectivity=1) as called
 * at src/scanpy/neighbors/_connectivity.py:103-138 (smooth_knn_dist + compute_membership_strengths
 * + W + W^T - W o W^T, zeros eliminated, CSR with sorted column indices).
 *
 *   knn_idx  [n, k] int32, column 0 = the row itself; knn_dist [n, k] float32
 *   out_indptr [n+1] int64; out_indices/out_data: capacity `cap` entries (2*n*(k-1) always suffices)
 *   out_sigma, out_rho [n] float32 (optional, may be NULL)
 *   nnz_host  (host) number of stored entries written
 * ---------------------------------------------------------------------------------------- */
size_t scamd_fuzzy_workspace_bytes(int64_t n, int k);
int scamd_fuzzy_simplicial_set_f32(const int32_t* knn_idx, const float* knn_dist, int64_t n, int k,
                                   int64_t* out_indptr, int32_t* out_indices, float* out_data,
                                   int64_t cap, float* out_sigma, float* out_rho, int64_t* nnz_host,
                                   void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Row-sharded fuzzy simplicial set (one process per GPU, rows [row_begin, row_begin + n_local) of n_total; knn_idx holds
 * GLOBAL row ids).  weights: sigma / rho / membership strengths of the local rows -- w [n_local, k] (0 = absent: the self
 * column, padding), out_count[i] = entries of row i with w > 0; sum_all_dev = device double holding the sum of ALL
 * n_total * k distances (the caller all-reduces it; used only for the rows without a positive distance, as in
 * umap.smooth_knn_dist).  merge_rows: the symmetrisation C = W + W^T - W o W^T of the local rows given their in-edges
 * (in_indptr [n_local + 1], in_src ascending within a row, in_w: the (j, i, w_ji) triples the other ranks sent for
 * these rows); bit-identical to the rows scamd_fuzzy_simplicial_set_f32 produces on one device.  cap >= nnz of the
 * local rows (<= n_local * (k - 1) + number of in-edges). */
int scamd_fuzzy_weights_f32(const int32_t* knn_idx, const float* knn_dist, int64_t n_local, int k, int64_t row_begin,
                            int64_t n_total, const double* sum_all_dev, float* w, float* out_sigma, float* out_rho,
                            int32_t* out_count, scamd_stream_t stream);
size_t scamd_fuzzy_merge_workspace_bytes(int64_t n_local, int64_t cap);
int scamd_fuzzy_merge_rows_f32(const int32_t* knn_idx, const float* w, int64_t n_local, int k, const int64_t* in_indptr,
                               const int32_t* in_src, const float* in_w, int64_t* out_indptr, int32_t* out_indices,
                               float* out_data, int64_t cap, int64_t* nnz_host, void* workspace, size_t workspace_bytes,
                               scamd_stream_t stream);
/* method='gauss' on the kNN pattern (src/scanpy/neighbors/_connectivity.py:21-100, CSR branch): sigma_i^2 = median of the
 * squared distances to the row's neighbours, w_ij = sqrt(2 s_i s_j / (s_i^2 + s_j^2)) exp(-d_ij^2 / (s_i^2 + s_j^2)),
 * w_ji := w_ij where i is not among j's neighbours.  Same in/out conventions and workspace size as the fuzzy set. */
int scamd_gauss_connectivities_f32(const int32_t* knn_idx, const float* knn_dist, int64_t n, int k, int64_t* out_indptr,
                                   int32_t* out_indices, float* out_data, int64_t cap, int64_t* nnz_host,
                                   void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* method='jaccard' (PhenoGraph weights, _connectivity.py:141-186): |N(i) & N(j)| / (2 (k-1) - |N(i) & N(j)|) on the kNN
 * pattern without the self columns, symmetrised by averaging. */
int scamd_jaccard_connectivities_f32(const int32_t* knn_idx, int64_t n, int k, int64_t* out_indptr,
                                     int32_t* out_indices, float* out_data, int64_t cap, int64_t* nnz_host,
                                     void* workspace, size_t workspace_bytes, scamd_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * PCA building blocks on a CSR float32 matrix (n rows = cells, g columns = genes).
 * Together they replace sklearn PCA(svd_solver='arpack')._fit_truncated on sparse input
 * (sklearn/decomposition/_pca.py:704-793 as called at src/scanpy/preprocessing/_pca/__init__.py:
 * 287-308): mean_variance_axis, the implicitly centred operator X - 1 mu^T
 * (sklearn/utils/sparsefuncs.py:718-742; in-repo restatement _pca/_compat.py:43-56) applied to
 * blocks of vectors, and the Gram-matrix alternative of _pca/_kernels.py:14-58.
 * ---------------------------------------------------------------------------------------- */
/* per-row sum and sum of squares in float64 (fixed summation order).  Applied to the CSC copy
 * (rows = genes) it yields the column statistics of mean_variance_axis. */
int scamd_csr_row_stats_f32(const int64_t* indptr, const float* data, int64_t n_rows,
                            double* row_sum, double* row_sumsq, scamd_stream_t stream);
/* Deterministic (stable) CSR -> CSC: t_indptr int64[g+1], t_indices int32[nnz] (row ids, ascending
 * within a column), t_data f32[nnz]. */
size_t scamd_csr_transpose_workspace_bytes(int64_t n, int64_t g, int64_t nnz);
int scamd_csr_transpose_f32(const int64_t* indptr, const int32_t* indices, const float* data,
                            int64_t n, int64_t g, int64_t nnz,
                            int64_t* t_indptr, int32_t* t_indices, float* t_data,
                            void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Y[n, l] (float32) = A[n, g] * B[g, l] - 1 * shift[l]^T   (shift may be NULL).
 * A is CSR; B row-major float32 with leading dimension l; 1 <= l <= 256 (scamd_spmm_csr_f32; the float64-accumulating variant takes l <= 128). */
int scamd_spmm_csr_f32(const int64_t* indptr, const int32_t* indices, const float* data,
                       int64_t n, int64_t g, const float* b, int l, const float* shift,
                       float* y, scamd_stream_t stream);
/* W[n_rows, l] (float64) = A * B with float64 accumulation of float32 products in a fixed order
 * (A = the CSC copy viewed as a g x n CSR, B = Y[n, l] float32: W = X^T Y); optional rank-1
 * correction W -= scale[n_rows] * colsum[l]^T (scale = column means, colsum = 1^T Y; both float64,
 * both NULL to skip). */
size_t scamd_spmm_f64acc_workspace_bytes(int64_t n_rows, int64_t nnz, int l);
int scamd_spmm_csr_f32_f64acc(const int64_t* indptr, const int32_t* indices, const float* data,
                              int64_t n_rows, int64_t nnz, const float* b, int l,
                              const double* scale, const double* colsum, double* w,
                              void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Exact Gram matrix and column sums of a CSR float32 matrix in 64-bit fixed point (the covariance route of
 * src/scanpy/preprocessing/_pca/_kernels.py:14-58 + _pca/_dask.py:28-132, and the engine of the default PCA solve):
 *   gram[i * ld_gram + j] = round-to-nearest-per-product sum_r x_ri * x_rj * 2^scale_bits   (int64, symmetric,
 *                           [g_pad x ld_gram], g_pad = g rounded up to 128, padding rows/columns zero)
 *   colsum[j]             = sum_r round(x_rj * 2^scale_bits)                                 (int64 [g_pad])
 * Integer accumulation is order independent: the result is bitwise reproducible and additive over row shards
 * (ranks all-reduce the int64 arrays).  Two-phase use: call with gram == NULL and absmax_host != NULL to get
 * max|x| (host float) and derive scale_bits <= 62 - log2(n_total * absmax^2); then call with the outputs. */
size_t scamd_csr_gram_workspace_bytes(int64_t n, int64_t g);
int scamd_csr_gram_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                       int64_t nnz, int scale_bits, int64_t* gram, int64_t ld_gram, int64_t* colsum,
                       float* absmax_host, void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Top-k eigenpairs of a symmetric POSITIVE SEMI-DEFINITE float64 matrix a [g x g] (leading dimension lda), the dense half
 * of the Gram-route PCA: what sklearn's PCA(svd_solver='arpack') obtains from ARPACK on the implicitly centred matrix
 * (sklearn/decomposition/_pca.py:704-793, called at src/scanpy/preprocessing/_pca/__init__.py:287-308) and the reference's
 * covariance route from `eigh` (src/scanpy/preprocessing/_pca/_dask.py:28-132).  Chebyshev-filtered subspace iteration on a
 * block of <= 128 vectors; hand-written float64 MFMA GEMMs, CholeskyQR2, one-workgroup Jacobi (csrc/dense.hip).
 *   lam [k] descending; v [g x k] row-major, column j = unit eigenvector j (sign unspecified)
 *   tol: Ritz residual |A v - lam v| / lam_0 of the k pairs (2e-8 reproduces ARPACK-level loadings)
 *   info_host (optional, 6 ints): outer iterations, operator applications, block size, Cholesky retries, then the final
 *             residual as a float64 in [4..5]
 * Supported: g <= 128 (full decomposition) or g >= 256 with k <= 96; SCAMD_EUNSUPPORTED otherwise or when the block turns
 * out numerically rank deficient / the iteration does not converge (callers then use a full eigendecomposition). */
size_t scamd_eigh_topk_workspace_bytes(int64_t g, int k);
int scamd_eigh_topk_f64(const double* a, int64_t g, int64_t lda, int k, uint64_t seed, double tol, double* lam, double* v,
                        int32_t* info_host, void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Building blocks of the above on caller buffers (tests): op 1: out0[m x n] = in0^T in1 with in0 [kdim x m], in1 [kdim x n];
 * op 2: out0[m x m] = CholeskyQR factor S of the Gram matrix in0 [m x m] (Z S orthonormal when in0 = Z^T Z), *flag_host =
 * 1 on a non-positive pivot; op 3: out0[m] = eigenvalues (descending), out1[m x m] = eigenvectors (columns) of the
 * symmetric PSD in0 [m x m], *flag_host = Jacobi sweeps.  m <= 128 for ops 2 and 3; op 4: out0[m x n] = in0 [m x kdim]
 * in1 [kdim x n], the panel product (kdim, n <= 128, kdim <= n rounded up to a power of two that is at least 4); op 5: the same
 * for two panels stacked in in0 [2 m x kdim] in one launch (out0, out1 [m x n]); op 6: op 3 on (in0 + in0^T) / 2, formed on load. */
int scamd_dense_debug_f64(int op, const double* in0, const double* in1, int m, int n, int kdim, double* out0, double* out1,
                          int32_t* flag_host, scamd_stream_t stream);
/* sc.pp.pca(svd_solver='arpack' accuracy) on a resident CSR float32 matrix in ONE call (the `pca_csr_f32` entry of the
 * boundary: src/scanpy/preprocessing/_pca/__init__.py:53-384 without its AnnData handling): max|x| -> exact fixed-point
 * Gram matrix -> top-n_comps eigenpairs -> sklearn's sign convention (svd_flip, u_based_decision=False) -> scores.
 *   scores [n x n_comps] float32 = X V - 1 (mu^T V) (zero_center) or X V
 *   components [n_comps x g] float64 (rows = components_), variance / variance_ratio [n_comps] (explained_variance_,
 *   explained_variance_ratio_ of sklearn PCA, or of TruncatedSVD when zero_center = 0), mean [g] float64
 *   info_host (optional, 8 ints): as scamd_eigh_topk_f64, then [6] = scale_bits of the fixed-point Gram matrix
 * Single device, g <= 8192, n_comps <= 96; a row-sharded run all-reduces the int64 Gram matrix between
 * scamd_csr_gram_f32 and scamd_eigh_topk_f64 instead. */
size_t scamd_pca_csr_workspace_bytes(int64_t n, int64_t g, int n_comps);
int scamd_pca_csr_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g, int64_t nnz,
                      int n_comps, int zero_center, uint64_t seed, double tol, float* scores, double* components,
                      double* variance, double* variance_ratio, double* mean, int32_t* info_host, void* workspace,
                      size_t workspace_bytes, scamd_stream_t stream);
/* The dense half of the above on its own -- what a ROW-SHARDED run calls after the all-reduce of the int64 sums (and what
 * scamd_pca_csr_f32 itself calls), so that the model is bitwise the same for any number of ranks and no library computes
 * any part of it (replaces the covariance-eigh arithmetic of src/scanpy/preprocessing/_pca/_kernels.py:14-58 and
 * _pca/_dask.py:28-132, sklearn's svd_flip and explained-variance bookkeeping, sklearn/decomposition/_pca.py:704-793):
 *   gram [g x g] int64 fixed point (2^scale_bits X^T X summed over ALL n_total rows, row stride ld_gram; only the upper
 *   triangle is read), colsum [g] int64 (2^scale_bits column sums)  ->  components [n_comps x g] float64 (sign convention
 *   applied), loadings_f32 [g x n_comps] float32 (= the B operand of scamd_spmm_csr_f32 for the scores), shift [n_comps]
 *   float32 (mu^T V: its `shift` operand), variance / variance_ratio [n_comps], mean [g], eigenvalues [n_comps] (of
 *   X^T X - n mu mu^T, clamped at 0: singular values squared; may be NULL).  info_host (optional, 8 ints) as scamd_pca_csr_f32.
 * Same range as scamd_eigh_topk_f64 (SCAMD_EUNSUPPORTED outside). */
size_t scamd_pca_solve_gram_workspace_bytes(int64_t g, int n_comps);
int scamd_pca_solve_gram_f64(const int64_t* gram, int64_t ld_gram, const int64_t* colsum, int64_t n_total, int64_t g,
                             int scale_bits, int n_comps, int zero_center, uint64_t seed, double tol, double* components,
                             float* loadings_f32, float* shift, double* variance, double* variance_ratio, double* mean,
                             double* eigenvalues, int32_t* info_host, void* workspace, size_t workspace_bytes,
                             scamd_stream_t stream);
/* Spectral initialisation of the UMAP layout: the `dim` eigenvectors of the symmetric normalised adjacency
 * S = D^-1/2 A D^-1/2 that follow the trivial one (= the smallest non-trivial ones of the normalised Laplacian) -- what
 * `sc.tl.umap(init_pos='spectral')` gets from umap-learn's `spectral_layout` (src/scanpy/tools/_umap.py:165-215; ARPACK
 * there, Chebyshev-filtered subspace iteration on (S + I) / 2 here, float32 SpMM operand, float64 everywhere else).
 *   indptr / indices / weights: the symmetric fuzzy graph (device CSR, n x n); dim <= 10; n > dim + 6
 *   out [n x dim] float64 (device): unit-norm, mutually orthogonal, orthogonal to sqrt(deg)
 *   info_host (optional, 8 doubles): outer iterations, operator applications, residual of the wanted Ritz pairs,
 *             1 if it is below `tol` (2e-6 is what the float32 operand allows), then up to four eigenvalues of S
 *   max_outer / max_degree: bounds of the iteration (60 / 64 in the Python layer)
 * SCAMD_EUNSUPPORTED when the block cannot be orthonormalised (the caller falls back to a random layout, as umap-learn does
 * when its eigensolver fails). */
size_t scamd_spectral_embedding_workspace_bytes(int64_t n, int64_t nnz, int dim);
int scamd_spectral_embedding_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                 int64_t nnz, int dim, uint64_t seed, double tol, int max_outer, int max_degree,
                                 double* out, double* info_host, void* workspace, size_t workspace_bytes,
                                 scamd_stream_t stream);
/* The symmetrised transition matrix of diffusion maps, `Neighbors.compute_transitions`
 * (src/scanpy/neighbors/__init__.py:805-827): dens = column sums of the symmetric graph, K_ij = A_ij / (dens_i dens_j)
 * (density_normalize != 0; K = A otherwise), z_i = sqrt(sum_j K_ij), T_sym_ij = K_ij / (z_i z_j).
 *   indptr / indices / weights: the symmetric graph (device CSR, n x n, positive weights)
 *   t_sym [nnz] float32 (device): T_sym on the same pattern, every entry computed in float64 and rounded once
 *   z [n] float64 (device): the reference's `Z` is diag(1 / z)
 * Sums are float64 in a fixed order (one wave per row).  SCAMD_EUNSUPPORTED when a row has no positive weight. */
size_t scamd_transitions_sym_workspace_bytes(int64_t n, int64_t nnz);
int scamd_transitions_sym_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                              int64_t nnz, int density_normalize, float* t_sym, double* z, void* workspace,
                              size_t workspace_bytes, scamd_stream_t stream);
/* The n_comps leading eigenpairs of T_sym, `Neighbors.compute_eigen(sort='decrease')`
 * (src/scanpy/neighbors/__init__.py:864-895: scipy `eigsh(which='LM')`, ARPACK on one host thread): Chebyshev-filtered
 * subspace iteration on (T_sym + I) / 2 with a block of n_comps + 6 <= 32 columns, float32 SpMM operand, float64 elsewhere,
 * bitwise reproducible.
 *   indptr / indices / t_sym: T_sym (device CSR, n x n, no empty row); 1 <= n_comps <= 26; n > max(n_comps + 6, 8)
 *   evals [n_comps] float64 (device), descending; evecs [n x n_comps] float64 (device): unit norm, mutually orthogonal,
 *   column 0 the stationary one (z / |z|); in every column the entry of largest magnitude is positive (lowest row on ties)
 *   info_host (optional, 8 doubles): outer iterations, operator applications, residual of the wanted Ritz pairs of
 *             (T_sym + I) / 2 (half that of the pairs of T_sym), 1 if it is below `tol` (2e-6 is what the float32 operand
 *             allows), the estimate of lambda_min, operator applications of its run, 1 if the guard refused, failed Cholesky
 *             attempts
 *   max_outer / max_degree: bounds of the iteration (60 / 64 in the Python layer)
 * Largest magnitude against largest algebraic value: the filter finds the largest algebraic eigenvalues, ARPACK is asked for
 * the largest magnitudes; a second run on (I - T_sym) / 2 (block of 8, one pair, tol 1e-3) estimates lambda_min, and the
 * entry returns SCAMD_EUNSUPPORTED (info_host filled, [6] = 1) when -lambda_min >= evals[n_comps - 1].  A Ritz value bounds
 * lambda_min from ABOVE: the guard can prove a conflict, never the absence of one.
 * SCAMD_EUNSUPPORTED also for n_comps > 26, n too small for the block, an empty row, and a block that cannot be
 * orthonormalised. */
size_t scamd_diffmap_workspace_bytes(int64_t n, int64_t nnz, int n_comps);
int scamd_diffmap_f32(const int64_t* indptr, const int32_t* indices, const float* t_sym, int64_t n, int64_t nnz,
                      int n_comps, uint64_t seed, double tol, int max_outer, int max_degree, double* evals,
                      double* evecs, double* info_host, void* workspace, size_t workspace_bytes,
                      scamd_stream_t stream);
/* Diffusion pseudotime from one root: `_get_dpt_row(iroot)` followed by `_set_pseudotime`
 * (src/scanpy/neighbors/__init__.py:920-953): d_v = sqrt(sum_j w_j (basis[iroot][j] - basis[v][j])^2) with
 * w_j = (lambda_j / (1 - lambda_j))^2 for lambda_j < 0.9994 and 1 otherwise, +inf outside the root's connected component,
 * divided by the largest finite entry when scale != 0 (the pseudotime) and left as it is when scale == 0 (the row of
 * `distances_dpt`).  Float64 accumulation (j ascending), the maximum by a two-stage reduction, the result rounded to
 * float32 once.
 *   evals [n_dcs] float32, basis [n x ld] float32 (ld >= n_dcs, n_dcs <= 128), labels [n] int32 component ids or NULL (one
 *   component) -- all on the device; out [n] float32 (device) */
size_t scamd_dpt_pseudotime_workspace_bytes(int64_t n);
int scamd_dpt_pseudotime_f32(const float* evals, const float* basis, int64_t n, int n_dcs, int64_t ld, int64_t iroot,
                             const int32_t* labels, int scale, float* out, void* workspace, size_t workspace_bytes,
                             scamd_stream_t stream);
/* colsum[l] (float64) = 1^T Y for Y [n, l] float32, fixed summation order. */
size_t scamd_colsum_workspace_bytes(int l);
int scamd_colsum_f32_f64(const float* y, int64_t n, int l, double* colsum,
                         void* workspace, size_t workspace_bytes, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Leiden community detection on a symmetric weighted CSR graph.
 * Replaces leidenalg.find_partition(g, RBConfigurationVertexPartition, weights, n_iterations,
 * resolution_parameter, seed) / igraph Graph.community_leiden(objective_function='modularity')
 * as called at src/scanpy/tools/_leiden.py:167-196 (graph built by
 * src/scanpy/_utils/__init__.py:278-304).  Objective:
 *   Q = 1/(2m) sum_ij (A_ij - resolution * k_i k_j / (2m)) delta(c_i, c_j).
 *   membership [n] int32: consecutive ids, renumbered by decreasing community size
 *   modularity_host, n_communities_host: host outputs
 *   n_iterations < 0: iterate until an iteration changes nothing.
 * ---------------------------------------------------------------------------------------- */
size_t scamd_leiden_workspace_bytes(int64_t n, int64_t nnz);
int scamd_leiden_csr_f32(const int64_t* indptr, const int32_t* indices, const float* weights,
                         int64_t n, int64_t nnz, double resolution, int n_iterations,
                         double beta, uint64_t seed,
                         int32_t* membership, double* modularity_host, int32_t* n_communities_host,
                         void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* The same optimiser started from a given partition instead of singletons -- `initial_membership` of
 * leidenalg.find_partition / igraph community_leiden, which the reference passes through `**clustering_args`
 * (src/scanpy/tools/_leiden.py:66, 174-196).  initial_membership [n] int32 on the device, ids in [0, n) (SCAMD_EINVAL
 * otherwise); n_iterations = 0 returns it renumbered (by decreasing size) with its modularity. */
int scamd_leiden_csr_init_f32(const int64_t* indptr, const int32_t* indices, const float* weights,
                              int64_t n, int64_t nnz, double resolution, int n_iterations,
                              double beta, uint64_t seed, const int32_t* initial_membership,
                              int32_t* membership, double* modularity_host, int32_t* n_communities_host,
                              void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* ... with the objective named: 0 = modularity (the two entry points above), 1 = CPM -- igraph's
 * community_leiden(objective_function='CPM') as reached from sc.tl.leiden(flavor='igraph', objective_function='CPM')
 * (src/scanpy/tools/_leiden.py:188-196): every vertex weighs 1, the resolution is not divided by 2m.
 * initial_membership may be NULL.  With objective 1 *modularity_host is the resolution-1 modularity of the returned
 * partition (the reference stores part.modularity, :219), not the CPM quality the run maximised. */
int scamd_leiden_csr_ex_f32(const int64_t* indptr, const int32_t* indices, const float* weights,
                            int64_t n, int64_t nnz, double resolution, int n_iterations,
                            double beta, uint64_t seed, int objective, const int32_t* initial_membership,
                            int32_t* membership, double* modularity_host, int32_t* n_communities_host,
                            void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* ... CPM with the caller's vertex weights -- igraph `community_leiden(objective_function='CPM', node_weights=...)`, which
 * `sc.tl.leiden(flavor='igraph', objective_function='CPM', node_weights=...)` reaches through **clustering_args
 * (src/scanpy/tools/_leiden.py:66, 188-196): a community pays resolution * (sum of its members' weights)^2.
 * node_weights: device pointer, n floats in [0, 1e6] (SCAMD_EINVAL otherwise; held in fixed point, 16 fractional bits) or
 * NULL (every vertex weighs 1: scamd_leiden_csr_ex_f32).  objective 0 (modularity: the vertex weights are the strengths)
 * takes NULL only (SCAMD_EUNSUPPORTED). */
int scamd_leiden_csr_nw_f32(const int64_t* indptr, const int32_t* indices, const float* weights,
                            int64_t n, int64_t nnz, double resolution, int n_iterations,
                            double beta, uint64_t seed, int objective, const float* node_weights,
                            const int32_t* initial_membership, int32_t* membership, double* modularity_host,
                            int32_t* n_communities_host, void* workspace, size_t workspace_bytes,
                            scamd_stream_t stream);
/* Statistics of the last scamd_leiden_csr_* call on this thread, out[0 .. min(n, 20)); scamd_leiden_stat_name gives the key of
 * every slot.  Diagnostics only (bench.py, tools/, the two warnings).
 *   iterations, launches, host_round_trips: outer iterations run, kernel launches, blocking host round trips;
 *   polish_full_sweeps / polish_rounds / polish_moves: of the final polish (n_iterations < 0: strictly monotone single-vertex
 *       moves until a sweep over ALL vertices finds no improving one -- the node optimality a stable partition of leidenalg /
 *       igraph has, src/scanpy/tools/_leiden.py:166-196 with n_iterations=-1); polish_skipped_proven: 1 if the last iteration
 *       itself had proven node optimality; polish_splits: communities the polish split off (a departing vertex had cut them in
 *       two); polish_ended_by_round_cap: 1 if a polish pass stopped at its round cap (node optimality then unproven;
 *       `tl.leiden` warns);
 *   levels_first_iteration; lm_sweeps: local-moving sweeps of the levels that run as separate kernels,
 *       lm_sweep_algorithmic_MB: their algorithmic traffic (active rows x (12 B per entry + 16 B per vertex): SURVEY.md 8(d)'s
 *       per-sweep figure over the rows a sweep visits);
 *   ended_by_iteration_cap: 1 if the cap on the outer iterations (iteration_cap; 32 unless SCAMD_LEIDEN_ITER_CAP says
 *       otherwise) ended an n_iterations < 0 run instead of convergence -- `tl.leiden` turns it into a UserWarning;
 *   device_fills: launches of the multi-region clear kernel;
 *   levels_reused / quiet_reuse_iterations: levels that took their coarse graph from the stored hierarchy / iterations that
 *       ran on it to its end without a move; overflow_pass_vertices / hub_pass_vertices: rows too long for the main tier of
 *       a 16- / 32-lane decide launch / rows longer than the wave table (block and giant tier together; see
 *       scamd_leiden_tier_bounds);
 *   out[14], which has no key: walks of the level-0 graph for a quality (after a polish pass that moved something, of a given
 *       start partition, for the modularity report of a CPM run).  A run from singletons needs none for its iterations: their
 *       quality is taken from the last level of each. */
void scamd_leiden_last_stats(int32_t* out, int n);
/* Key of statistics slot `slot` (a static string); NULL for slot 14, which has none, and outside [0, 20). */
const char* scamd_leiden_stat_name(int slot);
/* The longest rows the tiers of a Leiden decide step take when its main tier gives a vertex `lanes` (16, 32 or 64) lanes: up
 * to *main_max entries the main tier, up to *wave_max a wave per row, up to *block_max a 256-thread workgroup per row inside
 * the same launch, longer ones the 1024-thread launch of their own.  Read-only, no device needed; SCAMD_EINVAL for another
 * `lanes`.  Read by the tests that build rows at these lengths (tests/leiden_tier_cases.py). */
int scamd_leiden_tier_bounds(int lanes, int* main_max, int* wave_max, int* block_max);
/* Test entry: the component split the polish applies after its moves -- every connected component (over the stored
 * entries) of a community of `membership` (ids in [0, n), device, rewritten in place) becomes a community of its own, id =
 * its smallest vertex; *n_split_host = components - communities (0: membership untouched).  Workspace:
 * scamd_leiden_workspace_bytes. */
int scamd_leiden_debug_split_f32(const int64_t* indptr, const int32_t* indices, const float* weights,
                                 int64_t n, int64_t nnz, int32_t* membership, int32_t* n_split_host,
                                 void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Test entry: ONE level of a Leiden iteration on a given partition, by the functions the run itself calls -- the refinement
 * of `membership` (ids in [0, n), device) at `resolution`, `beta` and `seed` as scamd_leiden_csr_f32 takes them, then the
 * coarse graph under the refined partition.  refined_in != NULL (device, [n]: the id of a refined group is one of its members,
 * every group lies inside one community): the refinement is skipped and the coarse graph is built under refined_in.
 * Device outputs, the caller's: refined, Kref, Eref, refsize [n] (the sums and the size of a group at its representative: total
 * vertex weight, weight to the rest of its community -- zero when refined_in is given -- and members; zero elsewhere);
 * cid [n] (vertex -> coarse vertex), coarse_indptr [n + 1], coarse_indices / coarse_wq [nnz] (weights in units of 2^-32),
 * coarse_k [n] (strengths), coarse_comm [n] (the community of a coarse vertex, named by its smallest coarse vertex): the first
 * n_coarse + 1 / coarse nnz / n_coarse elements are written.  info_host [8]: merges, n_coarse, coarse nnz, rows built by
 * the 512-thread builder, by the 1024-thread builder, by the split path, 1 if nothing merged (n_coarse == n: no graph is
 * built and nothing from cid on is written), 0.  The SCAMD_LEIDEN_QUAD, SCAMD_LEIDEN_AGG_* and SCAMD_LEIDEN_HUB_TRY_PROBES
 * switches apply as in a run.  Workspace: scamd_leiden_workspace_bytes. */
int scamd_leiden_debug_level_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                 int64_t nnz, const int32_t* membership, const int32_t* refined_in, double resolution,
                                 double beta, uint64_t seed, int32_t* refined, uint64_t* Kref, uint64_t* Eref,
                                 int32_t* refsize, int32_t* cid, int64_t* coarse_indptr, int32_t* coarse_indices,
                                 int64_t* coarse_wq, int64_t* coarse_k, int32_t* coarse_comm, int64_t* info_host,
                                 void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Test entry: the counters of one local-moving sweep on a given partition, by the functions and kernels the run itself uses:
 * the community totals of `membership` (ids in [0, n), device), the class lists of a sweep with `n_cls` classes (a power of two,
 * at most 32 for n <= 4096 and 8 beyond) and class hash salt `salt` over the vertices whose word in flags_in (device, [n]) is
 * not zero -- flags_in == NULL: every vertex -- and one apply step per non-empty class with the caller's decisions (device, [n]:
 * decision[v] >= 0 the community v moves to, -2 "blocked": v stays and is flagged again, anything else: v stays).
 * Device outputs, the caller's: lists and tier_lists [n_cls * n] (class c at [c * n ..]: the vertices of the class; the list
 * positions of its rows of the wave tier upwards from [c * n], of the block tier downwards from [c * n + n - 1]), giant_lists
 * [n_cls * S], S = nnz / (block_max + 1) + 1 (scamd_leiden_tier_bounds), class c at [c * S ..]; Ktot_before / csize_before [n]:
 * total vertex weight (strengths in units of 2^-32) and members per community; comm_after, Ktot_after, csize_after,
 * flags_after [n]: the state after the apply steps.  counts_host [544]: [c] the length of class list c, [32 + 16 c + 8 / 9 /
 * 10] the rows of its wave / block / giant tier.  info_host [4]: moved, blocked, S, lanes per vertex of the level's main tier.
 * SCAMD_LEIDEN_COUNT_GRID and SCAMD_LEIDEN_QUAD apply as in a run.  Workspace: scamd_leiden_workspace_bytes. */
int scamd_leiden_debug_counters_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                    int64_t nnz, const int32_t* membership, const int32_t* flags_in, int n_cls, uint32_t salt,
                                    const int32_t* decision, int32_t* lists, int32_t* tier_lists, int32_t* giant_lists,
                                    uint64_t* Ktot_before, int32_t* csize_before, int32_t* comm_after, uint64_t* Ktot_after,
                                    int32_t* csize_after, int32_t* flags_after, int32_t* counts_host, int64_t* info_host,
                                    void* workspace, size_t workspace_bytes, scamd_stream_t stream);
/* Modularity of a given membership (replaces igraph Graph.modularity as used by
 * src/scanpy/metrics/_metrics.py:202-214). */
int scamd_modularity_csr_f32(const int64_t* indptr, const int32_t* indices, const float* weights,
                             int64_t n, int64_t nnz, const int32_t* membership, double resolution,
                             double* modularity_host, void* workspace, size_t workspace_bytes,
                             scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Graph autocorrelation: the device half of metrics.morans_i and metrics.gearys_c (reference: `_morans_i_mtx` / `_morans_i_vec_w`,
 * metrics/_morans_i.py:134-181, and `_gearys_c_mtx` / `_gearys_c_vec_W`, metrics/_gearys_c.py:145-244, which walk every stored
 * graph entry once per feature on the CPU; csrc/graph_autocorr.hip).  Graph: square CSR on the device, indptr
 * int64 [n + 1], indices int32, weights float32 or float64 (weights_is_f64); it need not be symmetric, sorted or free of
 * duplicates, and explicit zeros, self-loops and negative weights are ordinary entries.  A column id outside [0, n) takes no
 * part.  1 <= n < 2^31 (SCAMD_EUNSUPPORTED beyond).  All arithmetic is float64; no atomics: every sum is added in a fixed order
 * that depends on n and nnz alone, so two calls give the same bits and a feature's result does not depend on its slab or lane.
 * Arguments are checked before any HIP call and a rejected call writes nothing.
 *
 * scamd_graph_autocorr_slab_{f32,f64}: slab = the values, cell-major: slab[j * ld + l] is feature l of cell j, l < ncols <= 64,
 *   ld >= ncols (a dense cell-major array is read in place).  Outputs float64 [ncols] (device), per feature: mean = sum / n,
 *   z2 = sum_i (x_i - mean)^2, moran = sum_ij w_ij z_i z_j, geary = sum_ij w_ij (x_i - x_j)^2 (from the differences as
 *   written: exactly 0 for a feature constant on every connected component), min, max (NaN ignored).  A feature is constant
 *   exactly when min == max; a feature with a non-finite value has a non-finite mean and leaves the others alone.  The caller
 *   divides: I = n / W_sum * moran / z2, C = (n - 1) / (2 W_sum) * geary / z2.  Workspace: scamd_graph_autocorr_workspace_bytes.
 * scamd_graph_autocorr_part_entries: the stored entries one wave of the edge sweep takes at that nnz (the sweep is split by
 *   entries, not rows: a longer row is shared by several waves).
 * scamd_graph_weight_sum_f64: out[0] (device) = W_sum, the float64 sum of all stored weights in a fixed order (replaces
 *   `g.data.sum()`).  Workspace: the same function (8 KiB are used).
 * scamd_csr_dense_slab_f32: columns [c0, c0 + ncols) of a canonical cell-major CSR float32 (sorted, unique columns) as a slab,
 *   implicit zeros written as 0 (replaces `.toarray()` of a block of genes); every element slab[i * ld + l], l < ncols, is written.
 * scamd_transpose_slab_{f32,f64}: feature-major dense rows vals[f * ldv + j] (f < ncols, j < n) -> slab[j * ld + f]
 *   (replaces the `.T` copy of a block of features).
 * ---------------------------------------------------------------------------------------- */
size_t scamd_graph_autocorr_workspace_bytes(int64_t n, int64_t nnz);
int scamd_graph_autocorr_part_entries(int64_t nnz);
int scamd_graph_autocorr_slab_f32(const int64_t* indptr, const int32_t* indices, const void* weights, int weights_is_f64,
                                  int64_t n, int64_t nnz, const float* slab, int64_t ld, int32_t ncols, double* out_mean,
                                  double* out_z2, double* out_moran, double* out_geary, double* out_min, double* out_max,
                                  void* workspace, size_t workspace_bytes, scamd_stream_t stream);
int scamd_graph_autocorr_slab_f64(const int64_t* indptr, const int32_t* indices, const void* weights, int weights_is_f64,
                                  int64_t n, int64_t nnz, const double* slab, int64_t ld, int32_t ncols, double* out_mean,
                                  double* out_z2, double* out_moran, double* out_geary, double* out_min, double* out_max,
                                  void* workspace, size_t workspace_bytes, scamd_stream_t stream);
int scamd_graph_weight_sum_f64(const void* weights, int weights_is_f64, int64_t nnz, double* out, void* workspace,
                               size_t workspace_bytes, scamd_stream_t stream);
int scamd_csr_dense_slab_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                             int64_t nnz, int64_t c0, int32_t ncols, float* slab, int64_t ld, scamd_stream_t stream);
int scamd_transpose_slab_f32(const float* vals, int64_t ldv, int64_t n, int32_t ncols, float* slab, int64_t ld,
                             scamd_stream_t stream);
int scamd_transpose_slab_f64(const double* vals, int64_t ldv, int64_t n, int32_t ncols, double* slab, int64_t ld,
                             scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Upstream normalisation chain: normalize_total -> log1p -> highly_variable_genes -> scale on a
 * CSR float32 matrix resident on the device.  One HBM-bound sweep each; no workspace (the caller owns every output).
 * A dense matrix is passed as a CSR with the full pattern (indptr[i] = i*g, indices = column ids).
 * nnz = number of stored entries (= indptr[n]); the row-wise kernels size their lanes-per-row from nnz / n.
 * ---------------------------------------------------------------------------------------- */
/* out[r] = float(sum_j x_rj accumulated in float64): the CSR branch of _normalize_csr
 * (src/scanpy/preprocessing/_normalization.py:40-46).  col_skip != NULL: entries of columns with col_skip[c] != 0
 * are left out (second pass of exclude_highly_expressed, :60-65). */
int scamd_pp_row_sums_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t nnz,
                          const int32_t* col_skip, float* out, scamd_stream_t stream);
/* out[r] = #{stored x_rj > 0}: `stats.sum(data > 0, axis=1)` of filter_cells(min_genes= / max_genes=)
 * (src/scanpy/preprocessing/_simple.py:170-172); the per-gene counterpart of filter_genes is npos of
 * scamd_pp_col_stats_f32 */
int scamd_pp_row_count_positive_f32(const int64_t* indptr, const float* data, int64_t n, int64_t nnz, int32_t* out,
                                    scamd_stream_t stream);
/* col_counts[c] = #{r : x_rc > max_fraction * row_total[r]}  (_normalization.py:47-58); col_counts [g] is zeroed here */
int scamd_pp_count_high_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                            int64_t nnz, const float* row_total, float max_fraction, int32_t* col_counts,
                            scamd_stream_t stream);
/* x_rj /= factor[r] in float32, factor == 0 treated as 1: axis_mul_or_truediv(x, counts_per_cell, op=truediv,
 * allow_divide_by_zero=False, axis=0) (src/scanpy/_utils/__init__.py:623-659, called at _normalization.py:121-123) */
int scamd_pp_row_divide_f32(const int64_t* indptr, float* data, int64_t n, int64_t nnz, const float* factor,
                            scamd_stream_t stream);
/* data[i] = log1p(data[i]) (/ log(base) when base > 0; base == 0 means natural log): log1p_array / log1p_sparse
 * (src/scanpy/preprocessing/_simple.py:359-379) */
int scamd_pp_log1p_f32(float* data, int64_t count, double base, scamd_stream_t stream);
/* Per-gene sum[c], sumsq[c] (float64) and npos[c] = #{stored x_rc > 0} over the rows with row_mask[r] != 0
 * (row_mask == NULL: all rows); outputs [g] are zeroed here.  transform 0: x as stored; 1: expm1(x * tscale) in
 * float32 (flavor 'seurat' works in counts space, _highly_variable_genes.py:402-410).  Feeds
 * fast_array_utils.stats.mean_var(x, axis=0, correction=1) (_highly_variable_genes.py:413, _scale.py:189) and
 * filter_genes(min_cells=1) (_highly_variable_genes.py:387-395).  Float64 atomics: sums agree with a sequential
 * float64 sum to ~1e-15 relative, not bitwise. */
int scamd_pp_col_stats_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                           int64_t nnz, const uint8_t* row_mask, int transform, double tscale, double* sum,
                           double* sumsq, uint64_t* npos /* may be NULL */, scamd_stream_t stream);
/* The same sweep with every value clipped from above at clip[gene] (float64) before it is summed: `clip_square_sum` of
 * flavor='seurat_v3' (src/scanpy/preprocessing/_highly_variable_genes.py:75-115: sum and sum of squares of
 * min(x, sigma_hat * sqrt(n) + mu) per gene). */
int scamd_pp_col_stats_clip_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                int64_t nnz, const uint8_t* row_mask, const double* clip, double* sum, double* sumsq,
                                scamd_stream_t stream);
/* zero_center=False: x_rc = min(max_value, x_rc / std[c]) on the masked rows, sparsity kept: scale_and_clip_csr
 * (src/scanpy/preprocessing/_scale.py:280-295) */
int scamd_pp_scale_csr_f32(const int64_t* indptr, const int32_t* indices, float* data, int64_t n, int64_t nnz,
                           const double* std_, double max_value, int has_max, const uint8_t* row_mask,
                           scamd_stream_t stream);
/* zero_center=True: dense out[r*g + c] = clip((x_rc - mean[c]) / std[c], +-max_value) for masked rows, x_rc for the
 * others; out is float64 (sparse input: the reference's `x -= mean` yields a float64 matrix) or float32
 * (out_is_f64 == 0, float32 dense input): scale_array (_scale.py:189-216) + clip_array (:53-69) */
int scamd_pp_scale_dense_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                             int64_t nnz, const double* mean, const double* std_, double max_value, int has_max,
                             const uint8_t* row_mask, void* out, int out_is_f64, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Quality-control metrics: the device half of pp.calculate_qc_metrics (reference: `describe_obs`, `describe_var`,
 * `top_segment_proportions` and `top_segment_proportions_sparse_csr` in src/scanpy/preprocessing/_qc.py; csrc/qc.hip,
 * DESIGN.md 3.10).  Input as for the normalisation chain: CSR float32 on the device, a dense matrix as the full pattern.
 * A stored 0.0 / -0.0 is no entry (the reference calls eliminate_zeros; the matrix is not rewritten).  Values are assumed
 * finite.  No workspace: the caller owns every output.  Arguments are checked before any HIP call and a rejected call
 * writes nothing; n = 0 and g = 0 are legal.
 *
 * scamd_pp_qc_sweep_f32: one sweep.  Per row: row_nnz [n] = stored non-zeros, row_total [n] = their sum in float64 and,
 *   for n_masks > 0, row_masked [n_masks x n] (mask-major: row_masked[k * n + r]) = the sum over the genes c with bit k of
 *   gene_mask[c] set (gene_mask uint32 [g]; n_masks <= 32, SCAMD_EUNSUPPORTED beyond).  Per gene (col_nnz and col_sum both
 *   given, or both NULL): col_nnz [g] = stored non-zeros, col_sum [g] = their sum in float64; zeroed here.  flags [1]:
 *   bit 0 = a negative value was seen; zeroed here.  `indices` is read only when a mask or the per-gene outputs are asked
 *   for.  The per-row outputs are bitwise reproducible; the per-gene sums are float64 atomics: bitwise reproducible on
 *   integer-valued matrices (partial sums below 2^53), ~1e-15 relative otherwise.
 * scamd_pp_qc_top_f32: top [n x n_positions] (row-major), top[r, j] = top(positions[j]) of row r under THE RULE: take the
 *   stored non-zero values of the row, pad them with zeros up to n_max = positions[last] elements; top(p) is the sum, in
 *   float64, of the p largest elements of that multiset.  The result does not depend on how ties are broken and is
 *   bitwise reproducible; on integer-valued rows with totals below 2^53 it is exact.  positions_host: HOST pointer,
 *   1 <= positions[0] < positions[1] < ... (SCAMD_EINVAL otherwise); n_positions <= 16 and positions[last] <= 4096
 *   (SCAMD_EUNSUPPORTED beyond).  Rows of any length are handled.
 * ---------------------------------------------------------------------------------------- */
int scamd_pp_qc_sweep_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                          int64_t nnz, const uint32_t* gene_mask /* may be NULL */, int n_masks, int32_t* row_nnz,
                          double* row_total, double* row_masked /* may be NULL */, int64_t* col_nnz /* may be NULL */,
                          double* col_sum /* may be NULL */, uint32_t* flags, scamd_stream_t stream);
int scamd_pp_qc_top_f32(const int64_t* indptr, const float* data, int64_t n, int64_t nnz, const int32_t* positions_host,
                        int n_positions, double* top, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Regressing out observation annotations: the device half of pp.regress_out (reference: `regress_out`,
 * `numpy_regress_out`, `_create_regressor_categorical`, `_regress_out_chunk` in src/scanpy/preprocessing/_simple.py:468-681;
 * csrc/regress.hip).  Input as for the normalisation chain: canonical CSR float32 on the device (no column
 * twice in a row), a dense matrix as the full pattern; an implicit zero is the value 0.  Both branches of the reference are
 * one model, out[i, j] = x_ij - sum_k W[i, k] * T[k, j], with m table rows:
 *   numeric keys (w given, codes NULL):     w float64 [n x m] row-major, m <= 17 (the ones and 16 keys);
 *   a categorical key (codes given, w NULL): codes int32 [n], 0 <= code < m <= 65536; W is the one-hot of the code.
 * Exactly one of w / codes (SCAMD_EINVAL otherwise); more rows than that: SCAMD_EUNSUPPORTED.  g < 2^31.  Arguments are
 * checked before any HIP call and a rejected call writes nothing; n = 0 and g = 0 are legal.
 *
 * scamd_pp_regress_sums_f32: sums [m x g] (row-major, float64) = W^T X; col_min / col_max [g] = the smallest / largest
 *   value of every gene over all n cells, implicit zeros included (both 0 for n = 0); flags [1]: bit 0 = a stored value
 *   was not finite (such values take part in nothing), bit 1 = a code outside [0, m) (such rows take part in nothing);
 *   zeroed here.  wbound float64 [m] (device): wbound[k] >= sum_i |W[i, k]| -- n for a column of ones, the number of cells
 *   of category k.  Every term is rounded once to 64-bit fixed point at the scale 2^62 / (2^ew 2^ea), 2^ew > wbound[k],
 *   2^ea > max_i |x_ij|, and added with integer atomics: the result does not depend on the order of addition and is
 *   bitwise reproducible.  |sums[k, j] - exact| <= (n 2^-61 + 2^-52) wbound[k] max_i |x_ij|.  A wbound that is too small
 *   makes the sums of that row meaningless (nothing else).  Workspace: scamd_pp_regress_workspace_bytes(g, m).
 * scamd_pp_regress_resid_f32: out [n x g] row-major, float64 (out_is_f64 != 0) or float32:
 *   out[i, j] = x_ij - sum_k W[i, k] table[k, j] computed in float64 (k ascending) and rounded once, for the genes with
 *   keep[j] != 0; x_ij for the others.  table float64 [m x g].  One pass; every element is written exactly once.
 * ---------------------------------------------------------------------------------------- */
size_t scamd_pp_regress_workspace_bytes(int64_t g, int32_t m);
int scamd_pp_regress_sums_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                              int64_t nnz, const double* w /* or NULL */, const int32_t* codes /* or NULL */, int32_t m,
                              const double* wbound, double* sums, float* col_min, float* col_max, uint32_t* flags,
                              void* workspace, size_t workspace_bytes, scamd_stream_t stream);
int scamd_pp_regress_resid_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                               int64_t nnz, const uint8_t* keep, const double* table, const double* w /* or NULL */,
                               const int32_t* codes /* or NULL */, int32_t m, void* out, int out_is_f64,
                               scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Scrublet: the device passes of pp.scrublet / pp.scrublet_simulate_doublets that are not PCA, projection or kNN (reference:
 * `Scrublet.simulate_doublets`, `_nearest_neighbor_classifier` in src/scanpy/preprocessing/_scrublet/core.py; csrc/scrublet.hip,
 * DESIGN.md 3.12).  Arguments are checked before any HIP call and a rejected call writes nothing.
 *
 * ROW-PAIR SUMS, a two-phase protocol.  Input: canonical CSR float32 on the device (sorted, unique columns; n, g, n_sim < 2^31,
 * SCAMD_EUNSUPPORTED beyond), pairs int32 [n_sim x 2] with values in [0, n).  Output row r is row pairs[r, 0] + row pairs[r, 1]:
 * the sorted union of their columns, values added where both store the column (the float32 sum), nothing dropped for being
 * zero.  A pair (i, i) gives row i doubled.  No atomics: the output is a pure function of the input, bit for bit.
 *   1. scamd_pp_scrublet_pair_count: out_indptr int64 [n_sim + 1] (device) = the exclusive scan of the output row lengths;
 *      *out_nnz (HOST) = out_indptr[n_sim], by one pinned read-back (the call synchronises the stream); total_sim [n_sim] =
 *      row_total[a] + row_total[b], float64 (row_total_is_f64 != 0) or float32 like row_total [n].
 *      Workspace: scamd_pp_scrublet_workspace_bytes(n_sim).
 *   2. scamd_pp_scrublet_pair_fill_f32: the caller allocates out_indices int32 / out_data float32 [out_nnz] and passes the
 *      out_indptr of phase 1; every element is written exactly once.
 * flags [1] (device, zeroed by each phase): bit 0 = an output value above 2^24 in magnitude (sums of integer counts are exact in
 * float32 up to there; phase 2), bit 1 = a pair outside [0, n) or a row pointer outside [0, nnz]: that output row is empty,
 * bit 2 = an output position outside [0, out_nnz): out_indptr does not belong to these inputs, nothing is written there.
 * n_sim = 0 is legal (out_indptr[0] = 0).
 *
 * scamd_scrublet_scores_f64: idx int32 [n_all x k] = the neighbour lists of the concatenated manifold, observed rows first (the
 * layout scamd_knn_l2_f32 writes; the self column counts).  n_sim_neigh[i] = |{j : idx[i, j] >= n_obs}|; with nd that count,
 * N = k:  q = (nd + 1) / (N + 2),  score = q rho / r / (1 - rho - q (1 - rho - rho / r)),
 * se_q = sqrt(q (1 - q) / (N + 3)),  score_err = q rho / r / (1 - rho - q (1 - rho - rho / r))^2 *
 * sqrt((se_q / q (1 - rho))^2 + (se_rho / rho (1 - q))^2): float64, in the reference's operation order (the bits numpy gives).
 * 0 <= n_obs <= n_all < 2^31, k >= 1.
 * ---------------------------------------------------------------------------------------- */
size_t scamd_pp_scrublet_workspace_bytes(int64_t n_sim);
int scamd_pp_scrublet_pair_count(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t g, int64_t nnz,
                                 const int32_t* pairs, int64_t n_sim, const void* row_total, int row_total_is_f64,
                                 int64_t* out_indptr, void* total_sim, uint32_t* flags, int64_t* out_nnz /* host */,
                                 void* workspace, size_t workspace_bytes, scamd_stream_t stream);
int scamd_pp_scrublet_pair_fill_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                    int64_t nnz, const int32_t* pairs, int64_t n_sim, const int64_t* out_indptr, int64_t out_nnz,
                                    int32_t* out_indices, float* out_data, uint32_t* flags, scamd_stream_t stream);
int scamd_scrublet_scores_f64(const int32_t* idx, int64_t n_all, int32_t k, int64_t n_obs, double rho, double r, double se_rho,
                              int32_t* n_sim_neigh, double* score, double* score_err, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Marker genes: the device half of tl.rank_genes_groups (reference: `_RankGenes` in
 * src/scanpy/tools/_rank_genes_groups.py -- `_aggregate_group_stats`, `_ranks`, `_tiecorrect`, `wilcoxon`; csrc/rank_genes.hip,
 * DESIGN.md 3.8).  Input: the CSC copy of the cells x genes matrix as scamd_csr_transpose_f32 writes it (t_indptr int64[g + 1],
 * t_indices int32 = row ids ascending within a column, t_data f32) and codes int32[n]: the group of every cell,
 * 0 <= code < n_groups, or -1 for a cell that does not take part.  n_groups (the remainder group of reference='rest'
 * included) <= SCAMD_RANK_GENES_MAX_GROUPS, SCAMD_EUNSUPPORTED beyond.  A stored 0.0 / -0.0 counts as a zero everywhere
 * (the reference calls eliminate_zeros); values are assumed finite.  One gene = one workgroup; every accumulation is an
 * integer one, so all outputs are bitwise reproducible.  n = 0, g = 0 and empty columns are legal.  Outputs [n_groups x g]
 * are group-major: out[k * g + j].
 *
 * scamd_rank_genes_group_stats_f32: sum / sumsq (float64) and nnz (stored non-zeros) per (group, gene).  transform 0: x as
 *   stored; 1: expm1(x * tscale) as a float32 value, correctly rounded (the float32 product, expm1 evaluated in float64,
 *   rounded once).  Sums are 64-bit fixed point with a scale PER GENE:
 *   with L_j the column's stored entries and absmax_j its max |value| after the transform,
 *   sb = floor(62 - log2(L_j * absmax_j)) fractional bits for the sum and floor(62 - log2(L_j * absmax_j^2)) for the squares;
 *   every value is rounded once.  Hence |sum - exact| <= L_j * 2^-sb / 2 <= L_j^2 * absmax_j * 2^-62 (squares: absmax_j^2)
 *   before the one rounding of the result to float64.  The workspace is not used (NULL is accepted).
 * scamd_rank_genes_wilcoxon_f32: twice the rank sums.  group_sizes int64[n_groups] (device): cells per code.
 *   reference = -1 ('rest'): ranks are over all participating cells (average ranks, the implicit zeros one tie block);
 *     ranksum2[k, j] = 2 * sum of the ranks of group k; tie_term (NULL or [g]) = sum over the blocks of equal values of
 *     t^3 - t, the zero block included.
 *   reference = r: group k != r is ranked inside k u r: ranksum2[k, j] = n_k (n_k + 1) + 2 U with
 *     2 U = sum_{a in k} (2 #{x in r: x < a} + #{x in r: x = a}); tie_term (NULL or [n_groups x g]) = sum over the values v
 *     of k u r of (t_k(v) + t_r(v))^3 - (t_k(v) + t_r(v)).  Row r of both outputs is written as 0.
 *   The tie term is summed in integers and converted once: exact below 2^53.  n <= 2^21 (a block of all cells cubed stays
 *   below 2^63), SCAMD_EUNSUPPORTED beyond.
 * scamd_rank_genes_chunk_entries: stored entries of a column that one LDS chunk holds for that group count (0: unsupported
 *   count); a longer column is sorted chunk by chunk into the workspace and costs O(L * chunks * log chunk) searches.
 * ---------------------------------------------------------------------------------------- */
#define SCAMD_RANK_GENES_MAX_GROUPS 2000
size_t scamd_rank_genes_workspace_bytes(int64_t n, int64_t g, int64_t nnz, int n_groups);
int scamd_rank_genes_chunk_entries(int n_groups);
int scamd_rank_genes_group_stats_f32(const int64_t* t_indptr, const int32_t* t_indices, const float* t_data, int64_t n,
                                     int64_t g, const int32_t* codes, int n_groups, int transform, double tscale,
                                     double* sum, double* sumsq, int64_t* nnz, void* workspace, size_t workspace_bytes,
                                     scamd_stream_t stream);
int scamd_rank_genes_wilcoxon_f32(const int64_t* t_indptr, const int32_t* t_indices, const float* t_data, int64_t n,
                                  int64_t g, const int32_t* codes, int n_groups, const int64_t* group_sizes,
                                  int reference /* -1 = rest */, int64_t* ranksum2, double* tie_term /* may be NULL */,
                                  void* workspace, size_t workspace_bytes, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Harmony batch correction (`sc.pp.harmony_integrate`; src/scanpy/preprocessing/_harmony/core.py), csrc/harmony.hip.
 * All arithmetic is float64.  z_norm / x [n x d], R [n x K], O / E / lambda_kb [n_levels x K], centroids / y_norm [K x d],
 * codes int32[n] with 0 <= code < n_levels, pr_b / theta / n_b float64[n_levels] (cells of a level / n, the penalty
 * weight after the tau discount, cells of a level).  Limits (SCAMD_EUNSUPPORTED beyond, nothing written): d <= 128,
 * K <= 256, n_levels <= 1024, n < 2^31, n_covariates == 1 (several batch variables need the general-design ridge solve).
 * Every sum over cells is rounded once per term (or per fixed chunk of cells) to 64-bit fixed point and added in
 * integers: all outputs are bitwise reproducible.
 *
 * scamd_harmony_permutation_i32: perm = a keyed bijection on [0, n) (6-round Feistel network with cycle walking) of
 *   (seed, round); element i is computed on its own.
 * scamd_harmony_normalize_f64: rows of x divided by max(their Euclidean norm, 1e-12).
 * scamd_harmony_kmeans_f64: k-means++ seeding by D^2 sampling driven by K uniforms in [0, 1) (host array): centre 0 is cell
 *   floor(u_0 n), centre c the first cell whose running sum of D^2 exceeds u_c * total; then at most max_iter Lloyd sweeps
 *   (ties to the lowest centre, an empty centre stays), stopping after the sweep that changes no label.
 *   *n_iter_host = sweeps run.  Synchronises the stream.
 * scamd_harmony_init_f64: R = exp(-2/sigma (1 - z_norm . y_norm)) with rows divided by max(sum, 1e-12) (y_norm = the
 *   normalised centroids), O[b, k] = sum of R[i, k] over the cells of level b, E = pr_b (x) column sums of R,
 *   objective[4] = total, k-means error, entropy term, diversity term.  stabilized != 0: the harmony2 penalty
 *   (denominator O + E + 1), else harmony1 (O + 1).
 * scamd_harmony_cluster_round_f64: one clustering iteration: y_norm = rows of R^T z_norm normalised; the cells
 *   perm[0..n) cut into n_blocks blocks (the first n % n_blocks hold one cell more) processed one after another -- take
 *   the block's rows out of O and E, penalty theta_b (log(E + 1) - log(O [+ E] + 1)) of each cell's level, row-max-shifted
 *   softmax with the sum clamped at 1e-12, put the new rows back; then the objective as above.  R, E, O in/out.
 * scamd_harmony_correct_f64: lambda_kb (harmony2, dynamic_lambda != 0: alpha E, 1e30 where O / n_b <
 *   batch_prune_threshold or n_b = 0, a negative threshold prunes nothing; harmony1: ridge_lambda; 1e30 where O + lambda
 *   = 0), the closed-form single-variable ridge correction z_hat = x - sum_k R[:, k] W_k[code], z_norm = its normalised
 *   rows.  lambda_kb_out may be NULL.
 * init and cluster_round share scamd_harmony_state_workspace_bytes.
 * ---------------------------------------------------------------------------------------- */
#define SCAMD_HARMONY_MAX_D 128
#define SCAMD_HARMONY_MAX_K 256
#define SCAMD_HARMONY_MAX_LEVELS 1024
size_t scamd_harmony_permutation_workspace_bytes(int64_t n);
int scamd_harmony_permutation_i32(int64_t n, uint64_t seed, uint64_t round, int32_t* perm, void* workspace,
                                  size_t workspace_bytes, scamd_stream_t stream);
int scamd_harmony_normalize_f64(const double* x, int64_t n, int d, double* z_norm, scamd_stream_t stream);
size_t scamd_harmony_kmeans_workspace_bytes(int64_t n, int d, int K);
int scamd_harmony_kmeans_f64(const double* z_norm, int64_t n, int d, int K, const double* uniforms_host, int max_iter,
                             double* centroids, int32_t* labels, int* n_iter_host, void* workspace,
                             size_t workspace_bytes, scamd_stream_t stream);
size_t scamd_harmony_state_workspace_bytes(int64_t n, int d, int K, int n_levels);
int scamd_harmony_init_f64(const double* z_norm, const int32_t* codes, int64_t n, int d, int K, int n_levels,
                           int n_covariates, const double* centroids, const double* pr_b, const double* theta,
                           double sigma, int stabilized, double* R, double* E, double* O, double* objective,
                           void* workspace, size_t workspace_bytes, scamd_stream_t stream);
int scamd_harmony_cluster_round_f64(const double* z_norm, const int32_t* codes, int64_t n, int d, int K, int n_levels,
                                    int n_covariates, const int32_t* perm, int64_t n_blocks, const double* pr_b,
                                    const double* theta, double sigma, int stabilized, double* R, double* E, double* O,
                                    double* y_norm, double* objective, void* workspace, size_t workspace_bytes,
                                    scamd_stream_t stream);
size_t scamd_harmony_correct_workspace_bytes(int64_t n, int d, int K, int n_levels);
int scamd_harmony_correct_f64(const double* x, const int32_t* codes, int64_t n, int d, int K, int n_levels,
                              int n_covariates, const double* R, const double* O, const double* E, const double* n_b,
                              int dynamic_lambda, double alpha, double batch_prune_threshold, double ridge_lambda,
                              double* z_hat, double* z_norm, double* lambda_kb_out /* may be NULL */, void* workspace,
                              size_t workspace_bytes, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * UMAP layout: the SGD of umap-learn's optimize_layout_euclidean, which
 * simplicial_set_embedding runs for sc.tl.umap (src/scanpy/tools/_umap.py:196-216), in a synchronous, race-free
 * gather formulation (csrc/umap.hip).  Input: CSR of the pruned symmetric fuzzy graph (indptr [n+1], indices [nnz]),
 * epochs_per_sample [nnz] (umap_.make_epochs_per_sample: n_epochs * w / max w inverted; <= 0: never sampled),
 * y [n x dim] float32 row-major = the initial embedding scaled to [0, 10], overwritten with the result.
 * a, b: curve parameters (find_ab_params); gamma, initial_alpha, negative_sample_rate as in the reference call;
 * seed drives the counter-based negative sampling.  Deterministic: same inputs -> bitwise the same embedding.
 * ---------------------------------------------------------------------------------------- */
size_t scamd_umap_workspace_bytes(int64_t n, int64_t nnz, int dim);
int scamd_umap_optimize_f32(const int64_t* indptr, const int32_t* indices, const float* epochs_per_sample, int64_t n,
                            int64_t nnz, int dim, int n_epochs, double a, double b, double gamma,
                            double initial_alpha, double negative_sample_rate, uint64_t seed, float* y,
                            void* workspace, size_t workspace_bytes, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Collapsing cells into groups: the device half of get.aggregate (reference: `aggregate`, `Aggregate.{sum, count_nonzero,
 * mean_var, median}` in src/scanpy/get/_aggregated.py, the sweeps of src/scanpy/get/_kernels.py and sklearn's
 * csc_median_axis_0; csrc/aggregate.hip).  Input as for the normalisation chain: canonical CSR float32 on the
 * device, a dense matrix as the full pattern; an implicit zero is the value 0, and so is a stored +-0.0.
 *   codes int32 [n]: the group of every row, 0 <= code < n_groups, or -1 for a row that takes no part (the host folds the mask
 *     and missing categories into -1);
 *   order int32 [n_order]: the rows that take part, sorted by group (a counting sort of codes; any order inside a group);
 *   group_sizes int64 [n_groups] (device): the rows of every group; a group may have size 0; their sum is n_order.
 * Outputs are group-major [n_groups x g], out[k * g + j], with 64-bit offsets; n_groups <= n is the only bound on the number
 * of groups.  n, g < 2^31.  Arguments are checked before any HIP call and a rejected call writes nothing; n = 0, g = 0,
 * n_order = 0 and n_groups = 0 are legal.
 *
 * scamd_aggregate_moments_f32: per (group, gene) sum (float64), count_nonzero and count_negative (int64) and, when m2 is not
 *   NULL, m2 (float64) = the sum over ALL cells of the group of (x - mean)^2 with mean = sum / size, implicit zeros included
 *   (the deviations are taken from the final mean in sweeps of their own; sumsq - sum^2 / n is never formed; 0 for an empty
 *   group).  flags [1], zeroed here: bit 0 = a stored value of a row that takes part was not finite (such values take part in
 *   nothing), bit 1 = a code outside [-1, n_groups) (such rows take part in nothing), bit 2 = order, codes, group_sizes or a
 *   column index contradict each other (such rows / entries take part in nothing; nothing is written out of bounds).
 *   Every value is rounded once to 64-bit fixed point and added in integers (no float atomics): every output is bitwise
 *   reproducible and independent of the order of rows, lanes, waves and workgroups.  With size the rows of the group and
 *   amax the largest finite |x| of the gene over the rows that take part:
 *     |sum - exact| <= (size 2^-61 + 2^-53) size amax        (integers of magnitude <= 2^24: exact)
 *     |m2 - exact|  <= size^2 D^2 2^-60 + 2^-50 m2 + size ((size 2^-61 + 2^-52) amax)^2,
 *                      D = max |x - mean| over the stored non-zero values of the pair, D <= 2 amax
 *   A column that is constant and fully stored within a group has m2 == 0.0 exactly.
 * scamd_aggregate_median_f32: median [n_groups x g] (float64) = the exact median of the `size` values of every pair, from
 *   count_nonzero / count_negative as the moments wrote them.  An even size gives (lo + hi) / 2: the sum formed in float32
 *   and halved when mid_in_f32 != 0 (numpy's and sklearn's arithmetic on float32 data), in float64 otherwise (integer data).
 *   A zero result is +0.0; a group of size 0 gives NaN.  g <= 40944 (the transpose), SCAMD_EUNSUPPORTED beyond.
 *   info_host (host, may be NULL) int64 [3]: pairs decided from the counts alone, pairs searched by one wave, by a workgroup.
 * The sizing rules, for the tests that straddle them (host only, no device needed):
 *   scamd_aggregate_part_entries(nnz): stored entries of one part of the sweep (the split is by entries, not rows or groups);
 *   scamd_aggregate_lanes_per_row(n, nnz): lanes that share a row (8, 16, 32 or 64, from the mean row length);
 *   scamd_aggregate_tier_bounds: genes of one LDS window; entries from which a run (one group inside one part) is summed in
 *     LDS (a shorter one adds to the global table directly); the longest segment the in-wave median takes; the longest whose
 *     keys a workgroup stages in LDS (a longer one is read from global memory in every radix pass).
 *   scamd_aggregate_workspace_bytes(n, g, nnz, n_groups): serves both entry points (SCAMD_EWORKSPACE below it).
 * ---------------------------------------------------------------------------------------- */
size_t scamd_aggregate_workspace_bytes(int64_t n, int64_t g, int64_t nnz, int64_t n_groups);
int scamd_aggregate_part_entries(int64_t nnz);
int scamd_aggregate_lanes_per_row(int64_t n, int64_t nnz);
int scamd_aggregate_tier_bounds(int* gene_window, int* lds_min_run, int* median_wave_max, int* median_chunk);
int scamd_aggregate_moments_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                int64_t nnz, const int32_t* codes, const int32_t* order, int64_t n_order,
                                const int64_t* group_sizes, int64_t n_groups, double* sum, int64_t* count_nonzero,
                                int64_t* count_negative, double* m2 /* may be NULL */, uint32_t* flags, void* workspace,
                                size_t workspace_bytes, scamd_stream_t stream);
int scamd_aggregate_median_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                               int64_t nnz, const int32_t* order, int64_t n_order, const int64_t* group_sizes,
                               int64_t n_groups, const int64_t* count_nonzero, const int64_t* count_negative,
                               int mid_in_f32, double* median, int64_t* info_host /* may be NULL */, void* workspace,
                               size_t workspace_bytes, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Analytic Pearson residuals (Lause et al. 2021): the device half of scanpy_amd.experimental.pp (reference:
 * `_calculate_res_sparse` of src/scanpy/experimental/pp/_highly_variable_genes.py, `_pearson_residuals` of _normalization.py;
 * csrc/pearson.hip).
 *   mu_ij = (gene_sum[j] / total) * cell_total[i],  r_ij = clip((x_ij - mu_ij) / sqrt(mu_ij + mu_ij^2 * inv_theta), +-clip),
 * all float64.  inv_theta = 1 / theta >= 0 (0: Poisson), clip >= 0 (infinity: none); SCAMD_EINVAL otherwise.  A NaN (a cell with
 * total 0) is kept, nothing is special-cased.  All arguments are checked before any launch.
 * scamd_pp_pearson_gene_var_f32: var_out [g] float64 = the population variance (divisor n_batch) of every gene's residuals, an
 *   unstored entry counting as x = 0.  Input: the CSC copy of the cells x genes matrix as scamd_csr_transpose_f32 writes it
 *   (t_indptr int64 [g + 1], t_rows int32, t_data float32; n_rows < 2^31 rows), cell_total float64 [n_rows], the DISTINCT cell
 *   totals tot_u float64 [n_u] with their multiplicities mult_u float64 [n_u] (sum = n_batch; n_u <= n_batch <= n_rows,
 *   SCAMD_EINVAL otherwise).  batch_codes (int32 [n_rows], may be NULL) and batch_id keep the stored entries of the rows with that
 *   code only; gene_sum, total, tot_u, mult_u and n_batch are then that batch's.  A gene with gene_sum 0 gets 0.  Sums over the
 *   totals: float64 in a fixed order; sums over the stored entries: 128-bit fixed point, so two runs and any order of the rows give
 *   the same bits; the error bound is stated in csrc/pearson.hip.  Workspace: scamd_pp_pearson_workspace_bytes(g, nnz)
 *   (SCAMD_EWORKSPACE below it).
 * scamd_pp_pearson_residuals_f32: out [n x g] row-major, float64 (out_is_f64 != 0) or float32, every cell written once, from the
 *   canonical CSR matrix (column indices ascending in every row); float64 arithmetic, rounded once on store.
 * scamd_pp_pearson_limits: the stored entries of one gene per workgroup, the totals per pass of a workgroup, the columns of a
 *   slice and the rows of a batch of the residual kernel (read-only, no device needed).
 * ---------------------------------------------------------------------------------------- */
int scamd_pp_pearson_limits(int32_t* chunk_entries, int32_t* totals_block, int32_t* slice_columns, int32_t* batch_rows);
size_t scamd_pp_pearson_workspace_bytes(int64_t g, int64_t nnz);
int scamd_pp_pearson_gene_var_f32(const int64_t* t_indptr, const int32_t* t_rows, const float* t_data, int64_t n_rows, int64_t g,
                                  int64_t nnz, const double* gene_sum, const double* cell_total, double total, double inv_theta,
                                  double clip, const double* tot_u, const double* mult_u, int64_t n_u, int64_t n_batch,
                                  const int32_t* batch_codes /* may be NULL */, int32_t batch_id, double* var_out, void* workspace,
                                  size_t workspace_bytes, scamd_stream_t stream);
int scamd_pp_pearson_residuals_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                   int64_t nnz, const double* gene_sum, const double* cell_total, double total, double inv_theta,
                                   double clip, void* out, int out_is_f64, scamd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Host-side byte codecs of the on-disk readers (csrc/hostio.cpp).  No device work: callable on a
 * host without a GPU, from many threads at once.  They replace what the reference gets from h5py's bundled filters
 * when it reads `.h5ad` / 10x `.h5` files (src/scanpy/readwrite.py:15-29, 235-243; `compression='lzf'` is one of
 * the two codecs its writer offers, :657-667).
 * scamd_lzf_decompress: liblzf stream -> dst; returns the number of bytes produced (>= 0) or a negative SCAMD_E* code
 *   (malformed stream, or dst_cap too small).
 * scamd_unshuffle: inverse of the HDF5 shuffle filter -- src = elem_size byte planes of n_elem bytes, dst = elements.
 * ---------------------------------------------------------------------------------------- */
int64_t scamd_lzf_decompress(const void* src, size_t src_len, void* dst, size_t dst_cap);
int scamd_unshuffle(const void* src, void* dst, size_t n_elem, int elem_size);

/* ------------------------------------------------------------------------------------------
 * Self tests / micro benchmarks (device).  scamd_selftest_mfma_layout checks the
 * v_mfma_f32_32x32x2_f32 operand/result lane mapping the kNN kernel relies on; returns 0 if OK.
 * ---------------------------------------------------------------------------------------- */
int scamd_selftest_mfma_layout(scamd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCANPY_AMD_H */
