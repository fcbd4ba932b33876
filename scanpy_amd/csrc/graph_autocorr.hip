// Graph autocorrelation: the device passes behind scanpy_amd.metrics.morans_i and gearys_c (reference: `_morans_i_mtx`,
// `_gearys_c_mtx` and their per-vector loops in metrics/_morans_i.py:134-181 and metrics/_gearys_c.py:145-244, which walk every stored
// graph entry once PER FEATURE).  With W a square CSR graph (any stored pattern), x a feature over the n cells, z = x - mean(x):
//   I = n / W_sum * sum_ij w_ij z_i z_j / sum_i z_i^2        C = (n - 1) / (2 W_sum) * sum_ij w_ij (x_i - x_j)^2 / sum_i z_i^2
// The kernels give the two numerators, sum z^2, the mean, the minimum and the maximum of up to 64 features per call; the two
// divisions are the caller's.  All arithmetic is float64; values and weights are float32 or float64 and converted at the load.
//
// THE SLAB.  The values sit cell-major, S[n][ld]: row j holds the (up to) GA_SLAB = 64 features of cell j next to each other,
// so one graph entry (i, j, w) costs ONE coalesced wave-wide load of S[j][0 .. 64) -- lane l owns feature l and adds
// w * z_i * z_j and w * (x_i - x_j)^2 to two float64 registers.  Geary's numerator is taken from the differences as written:
// the expanded form sum x^2 (r + c) - 2 sum w x_i x_j cancels, and loses the exact 0 of a signal that is constant on every
// connected component.  A dense cell-major array (obsm['X_pca']) is read in place through (pointer, ld, ncols); a cell-major
// CSR is densified 64 columns at a time (ga_csr_slab_kernel), feature-major dense rows are transposed through LDS
// (ga_transpose_kernel).
//
// THE WORK SPLIT is by stored entries, not by rows: a symmetrised kNN graph has hub rows of thousands of entries, and a
// row-per-wave split runs as long as its most loaded wave.  One wave = one PART = a fixed range of ga_part_entries(nnz)
// consecutive entries; it finds its first row by a binary search in indptr and walks on from there, so a long row is shared by
// several parts.  x_i and z_i are reloaded when the row changes.  The entry loop is unrolled by GA_UNROLL = 4: four entries'
// column ids and weights are broadcast from a 64-entry batch, then four independent row gathers are issued before the first use
// (60 VGPRs, 8 waves per SIMD; eight gathers need 100 VGPRs, halve the waves and measured 1.69 against 1.54 ms).
//
// NO ATOMICS.  Every part writes its [2][64] partial sums to the workspace; ga_reduce_kernel adds them in a fixed order (groups of
// 64 parts, then the groups) that depends on the number of parts alone.  The column pass (sum -> mean, min, max, then sum z^2) and the weight sum use the
// same scheme: fixed chunks, fixed order.  Hence two runs give the same bits, and a feature's result does not depend on which
// slab or which lane it sat in.  A feature is constant exactly when min == max (fl(sum / n) need not equal the constant, so
// sum z^2 == 0 is NOT the test); a non-finite value makes the feature's sum non-finite and leaves the other lanes alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"

namespace scamd {

namespace {

constexpr int GA_BLOCK = 256;
constexpr int GA_SLAB = 64;                   // features per slab: one per lane
constexpr int GA_WAVES = GA_BLOCK / GA_SLAB;  // parts per workgroup
constexpr int GA_UNROLL = 4;                  // neighbour rows in flight per wave (8: SCAMD_AUTOCORR_UNROLL)
constexpr int GA_PART_MIN = 256;              // entries per part: ceil(nnz / GA_PART_TARGET) within [GA_PART_MIN, GA_PART_MAX]
constexpr int GA_PART_MAX = 4096;
constexpr int GA_PART_TARGET = 8192;          // parts aimed at: 32 waves for each of 256 CUs
constexpr int GA_REDUCE_GROUP = 64;           // parts per workgroup of the first level of the reduction over the parts
constexpr int GA_REDUCE_UNROLL = 8;           // partial sums requested back to back by a thread of a reduction
constexpr int GA_COL_CHUNKS = 1024;           // row chunks of the column pass, at most
constexpr int GA_COL_CHUNK_ROWS = 256;        // rows per chunk, at least
constexpr int GA_WSUM_CHUNKS = 1024;          // chunks of the weight sum, at most
constexpr int GA_WSUM_CHUNK_MIN = 4096;       // entries per chunk, at least

inline int ga_part_entries(int64_t nnz) {
  const int64_t per = (nnz + GA_PART_TARGET - 1) / GA_PART_TARGET;
  return (int)std::min<int64_t>(std::max<int64_t>(per, GA_PART_MIN), GA_PART_MAX);
}
inline int64_t ga_parts(int64_t nnz) {
  const int64_t pe = ga_part_entries(nnz);
  return (nnz + pe - 1) / pe;
}
inline int64_t ga_col_chunk_rows(int64_t n) {
  return std::max<int64_t>((n + GA_COL_CHUNKS - 1) / GA_COL_CHUNKS, GA_COL_CHUNK_ROWS);
}
inline int64_t ga_col_chunks(int64_t n) {
  const int64_t rows = ga_col_chunk_rows(n);
  return std::max<int64_t>((n + rows - 1) / rows, 1);
}
inline int64_t ga_wsum_chunk(int64_t nnz) {
  return std::max<int64_t>((nnz + GA_WSUM_CHUNKS - 1) / GA_WSUM_CHUNKS, GA_WSUM_CHUNK_MIN);
}

// ---- the column pass.  A workgroup owns rows [chunk * rows, (chunk + 1) * rows): wave q takes the rows q, q + 4, ... of it in
// order, lane l column l; the four waves' results are combined in wave order.  PASS 0: sum, min, max; PASS 1: sum (x - mean)^2.
// part [chunks][3][64] (PASS 1: plane 0 only).
template <typename VT, int PASS>
__global__ __launch_bounds__(GA_BLOCK) void ga_col_chunk_kernel(const VT* __restrict__ S, int64_t ld, int ncols, int64_t n,
                                                                int64_t rows, const double* __restrict__ mean,
                                                                double* __restrict__ part) {
  __shared__ double s_acc[3][GA_WAVES][GA_SLAB];
  const int lane = threadIdx.x & (GA_SLAB - 1), q = threadIdx.x >> 6;
  const bool active = lane < ncols;
  const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = std::min<int64_t>(r0 + rows, n);
  double sum = 0.0, lo = INFINITY, hi = -INFINITY;
  const double mu = (PASS == 1 && active) ? mean[lane] : 0.0;
  if (active) {
    for (int64_t r = r0 + q; r < r1; r += GA_WAVES) {
      const double x = (double)S[r * ld + lane];
      if (PASS == 0) {
        sum += x;
        lo = fmin(lo, x);
        hi = fmax(hi, x);
      } else {
        const double z = x - mu;
        sum += z * z;
      }
    }
  }
  s_acc[0][q][lane] = sum;
  if (PASS == 0) {
    s_acc[1][q][lane] = lo;
    s_acc[2][q][lane] = hi;
  }
  __syncthreads();
  if (q == 0) {
    double* o = part + (int64_t)blockIdx.x * 3 * GA_SLAB;
    double t = s_acc[0][0][lane];
#pragma unroll
    for (int k = 1; k < GA_WAVES; ++k) t += s_acc[0][k][lane];
    o[lane] = t;
    if (PASS == 0) {
      double a = s_acc[1][0][lane], b = s_acc[2][0][lane];
#pragma unroll
      for (int k = 1; k < GA_WAVES; ++k) {
        a = fmin(a, s_acc[1][k][lane]);
        b = fmax(b, s_acc[2][k][lane]);
      }
      o[GA_SLAB + lane] = a;
      o[2 * GA_SLAB + lane] = b;
    }
  }
}

// one workgroup: the chunks in order, four interleaved runs per column combined in run order.  PASS 0 -> mean (sum / n), min, max;
// PASS 1 -> sum z^2.
template <int PASS>
__global__ __launch_bounds__(GA_BLOCK) void ga_col_reduce_kernel(const double* __restrict__ part, int64_t chunks, int ncols, int64_t n,
                                                                 double* __restrict__ out_mean, double* __restrict__ out_min,
                                                                 double* __restrict__ out_max, double* __restrict__ out_z2) {
  __shared__ double s_acc[3][GA_WAVES][GA_SLAB];
  const int lane = threadIdx.x & (GA_SLAB - 1), q = threadIdx.x >> 6;
  double sum = 0.0, lo = INFINITY, hi = -INFINITY;
  // (GA_REDUCE_UNROLL chunks are requested before the first is added: one workgroup cannot hide a load's latency otherwise; a
  // chunk past the end is the last one again and adds 0)
  for (int64_t c = q; c < chunks; c += GA_WAVES * GA_REDUCE_UNROLL) {
    double a[GA_REDUCE_UNROLL], b[GA_REDUCE_UNROLL], d[GA_REDUCE_UNROLL];
#pragma unroll
    for (int k = 0; k < GA_REDUCE_UNROLL; ++k) {
      const int64_t at = c + (int64_t)k * GA_WAVES;
      const double* p = part + std::min<int64_t>(at, chunks - 1) * 3 * GA_SLAB;
      a[k] = p[lane];
      b[k] = PASS == 0 ? p[GA_SLAB + lane] : 0.0;
      d[k] = PASS == 0 ? p[2 * GA_SLAB + lane] : 0.0;
      if (at >= chunks) a[k] = 0.0;  // (its minimum and maximum are one chunk's again: harmless)
    }
#pragma unroll
    for (int k = 0; k < GA_REDUCE_UNROLL; ++k) {
      sum += a[k];
      if (PASS == 0) {
        lo = fmin(lo, b[k]);
        hi = fmax(hi, d[k]);
      }
    }
  }
  s_acc[0][q][lane] = sum;
  s_acc[1][q][lane] = lo;
  s_acc[2][q][lane] = hi;
  __syncthreads();
  if (q == 0 && lane < ncols) {
    double t = s_acc[0][0][lane], a = s_acc[1][0][lane], b = s_acc[2][0][lane];
#pragma unroll
    for (int k = 1; k < GA_WAVES; ++k) {
      t += s_acc[0][k][lane];
      a = fmin(a, s_acc[1][k][lane]);
      b = fmax(b, s_acc[2][k][lane]);
    }
    if (PASS == 0) {
      out_mean[lane] = t / (double)n;
      out_min[lane] = a;
      out_max[lane] = b;
    } else {
      out_z2[lane] = t;
    }
  }
}

// a wave-uniform copy of lane t's weight (two 32-bit broadcasts for a float64 weight)
__device__ __forceinline__ double ga_bcast(float v, int t) {
  return (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t));
}
__device__ __forceinline__ double ga_bcast(double v, int t) {
  union {
    double d;
    int i[2];
  } u;
  u.d = v;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], t);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], t);
  return u.d;
}

// ---- the edge sweep: one wave per part.  partial [parts][2][64]: plane 0 Moran's numerator, plane 1 Geary's.
// The part's (column id, weight) pairs are loaded 64 at a time, one per lane, and broadcast with readlane (the first version read
// them with wave-uniform scalar loads: five dependent waits per four entries, 2.4 ms for 23.8 M entries whatever the slab width,
// profiles/graph_autocorr_timing.log); the next 64 are requested before the current ones are used.  GA_UNROLL row gathers are
// issued back to back and consumed in order.  The row after the current one -- its end and its own values -- is requested when a
// row is entered, so that a row change costs no wait unless empty rows lie between.
template <typename VT, typename WT, int UNROLL>
__global__ __launch_bounds__(GA_BLOCK) void ga_sweep_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const WT* __restrict__ weights, int64_t n, int64_t nnz, int part_entries,
                                                            int64_t parts, const VT* __restrict__ S, int64_t ld, int ncols,
                                                            const double* __restrict__ mean, double* __restrict__ partial) {
  const int lane = threadIdx.x & (GA_SLAB - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t part = (int64_t)blockIdx.x * GA_WAVES + wave;
  if (part >= parts) return;  // (whole waves: the padding of the last workgroup)
  // a lane at or beyond ncols is masked by reading column 0 again: valid memory, no divergent load, and its sums are never read
  const int lane_c = lane < ncols ? lane : 0;
  const int64_t e0 = part * part_entries, e1 = std::min<int64_t>(e0 + part_entries, nnz);
  int32_t ci = indices[std::min<int64_t>(e0 + lane, e1 - 1)];
  WT cv = weights[std::min<int64_t>(e0 + lane, e1 - 1)];
  // the last row r with indptr[r] <= e0: its successor starts beyond e0 (e0 < nnz = indptr[n]), so it holds entry e0
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (indptr[mid] <= e0) lo = mid;
    else hi = mid - 1;
  }
  int64_t r = lo, row_end = indptr[r + 1];
  const double mu = mean[lane_c];
  double xi = (double)S[r * ld + lane_c], zi = xi - mu;
  int64_t rn = std::min<int64_t>(r + 1, n - 1), row_end_n = indptr[rn + 1];  // the row after r, requested ahead
  double xin = (double)S[rn * ld + lane_c];
  double mor = 0.0, gea = 0.0;
  for (int64_t base = e0; base < e1; base += GA_SLAB) {
    const int64_t en = std::min<int64_t>(base + GA_SLAB + lane, e1 - 1);  // (past the part's end: its last entry again, never used)
    const int32_t ci_n = indices[en];
    const WT cv_n = weights[en];
    const int cnt = (int)std::min<int64_t>(GA_SLAB, e1 - base);
    for (int u = 0; u < cnt; u += UNROLL) {
      // An entry that takes no part -- beyond the batch's end, or a column id outside the graph -- reads row 0 with weight 0
      // (0 * NaN could only come from a value of this very column, whose result is NaN whatever is added here).
      int64_t j[UNROLL];
      double w[UNROLL], xj[UNROLL];
#pragma unroll
      for (int t = 0; t < UNROLL; ++t) {
        const int tt = std::min(u + t, cnt - 1);
        const int32_t col = __builtin_amdgcn_readlane(ci, tt);
        const double wt = ga_bcast(cv, tt);
        const bool ok = u + t < cnt && (uint32_t)col < (uint64_t)n;
        j[t] = ok ? col : 0;
        w[t] = ok ? wt : 0.0;
      }
#pragma unroll
      for (int t = 0; t < UNROLL; ++t) xj[t] = (double)S[j[t] * ld + lane_c];
      const int64_t e = base + u;
      if (std::min<int64_t>(e + UNROLL, e1) <= row_end) {  // all in the current row
#pragma unroll
        for (int t = 0; t < UNROLL; ++t) {
          const double zj = xj[t] - mu, d = xi - xj[t];
          mor += w[t] * (zi * zj);
          gea += w[t] * (d * d);
        }
      } else {
#pragma unroll
        for (int t = 0; t < UNROLL; ++t) {
          if (e + t < e1 && e + t >= row_end && r + 1 < n) {
            r = rn;
            row_end = row_end_n;
            xi = xin;
            if (e + t >= row_end && r + 1 < n) {
              do {  // (empty rows are stepped over; r stays inside the graph whatever indptr holds)
                ++r;
                row_end = indptr[r + 1];
              } while (e + t >= row_end && r + 1 < n);
              xi = (double)S[r * ld + lane_c];
            }
            zi = xi - mu;
            rn = std::min<int64_t>(r + 1, n - 1);
            row_end_n = indptr[rn + 1];
            xin = (double)S[rn * ld + lane_c];
          }
          const double zj = xj[t] - mu, d = xi - xj[t];
          mor += w[t] * (zi * zj);
          gea += w[t] * (d * d);
        }
      }
    }
    ci = ci_n;
    cv = cv_n;
  }
  double* o = partial + part * 2 * GA_SLAB;
  o[lane] = mor;
  o[GA_SLAB + lane] = gea;
}

// thread (q, l) adds the items first, first + 4, ... (< end) of column l in order, both planes; GA_REDUCE_UNROLL items are requested
// before the first is added (an item past the end is the last one again and adds 0)
__device__ __forceinline__ void ga_ordered_sum(const double* __restrict__ items, int64_t first, int64_t end, int lane, double& s0,
                                               double& s1) {
  for (int64_t p = first; p < end; p += GA_WAVES * GA_REDUCE_UNROLL) {
    double a[GA_REDUCE_UNROLL], b[GA_REDUCE_UNROLL];
#pragma unroll
    for (int k = 0; k < GA_REDUCE_UNROLL; ++k) {
      const int64_t at = p + (int64_t)k * GA_WAVES;
      const double* o = items + std::min<int64_t>(at, end - 1) * 2 * GA_SLAB;
      a[k] = o[lane];
      b[k] = o[GA_SLAB + lane];
      if (at >= end) a[k] = 0.0, b[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < GA_REDUCE_UNROLL; ++k) {
      s0 += a[k];
      s1 += b[k];
    }
  }
}

// the reduction over the parts, two levels, no atomics: workgroup b adds the parts [b * GA_REDUCE_GROUP, (b + 1) * GA_REDUCE_GROUP)
// (wave q the parts q, q + 4, ... of them in order, then the four waves in wave order) into group b; one workgroup adds the
// groups the same way.  The order is a function of the number of parts alone.  (One workgroup over all 8192 parts of a 1M-cell
// graph took 2 ms, five times the sweep: 2048 dependent trips of one exposed load each.)
template <bool FINAL>
__global__ __launch_bounds__(GA_BLOCK) void ga_reduce_kernel(const double* __restrict__ items, int64_t count, int ncols,
                                                             double* __restrict__ groups, double* __restrict__ out_moran,
                                                             double* __restrict__ out_geary) {
  __shared__ double s_acc[2][GA_WAVES][GA_SLAB];
  const int lane = threadIdx.x & (GA_SLAB - 1), q = threadIdx.x >> 6;
  const int64_t begin = FINAL ? 0 : (int64_t)blockIdx.x * GA_REDUCE_GROUP;
  const int64_t end = FINAL ? count : std::min<int64_t>(begin + GA_REDUCE_GROUP, count);
  double mor = 0.0, gea = 0.0;
  ga_ordered_sum(items, begin + q, end, lane, mor, gea);
  s_acc[0][q][lane] = mor;
  s_acc[1][q][lane] = gea;
  __syncthreads();
  if (q == 0) {
    double a = s_acc[0][0][lane], b = s_acc[1][0][lane];
#pragma unroll
    for (int k = 1; k < GA_WAVES; ++k) {
      a += s_acc[0][k][lane];
      b += s_acc[1][k][lane];
    }
    if (FINAL) {
      if (lane < ncols) {
        out_moran[lane] = a;
        out_geary[lane] = b;
      }
    } else {
      groups[(int64_t)blockIdx.x * 2 * GA_SLAB + lane] = a;
      groups[(int64_t)blockIdx.x * 2 * GA_SLAB + GA_SLAB + lane] = b;
    }
  }
}

// ---- the weight sum: chunk c = entries [c * chunk, (c + 1) * chunk); thread t adds t, t + 256, ... of it in order, then a
// fixed tree over the workgroup; the last kernel adds the chunk sums the same way.
__device__ __forceinline__ double ga_block_tree(double v, double* s_red) {
  s_red[threadIdx.x] = v;
  __syncthreads();
  for (int half = GA_BLOCK / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) s_red[threadIdx.x] += s_red[threadIdx.x + half];
    __syncthreads();
  }
  return s_red[0];
}

template <typename WT>
__global__ __launch_bounds__(GA_BLOCK) void ga_wsum_chunk_kernel(const WT* __restrict__ w, int64_t nnz, int64_t chunk,
                                                                 double* __restrict__ part) {
  __shared__ double s_red[GA_BLOCK];
  const int64_t b = (int64_t)blockIdx.x * chunk, e = std::min<int64_t>(b + chunk, nnz);
  double acc = 0.0;
  for (int64_t p = b + threadIdx.x; p < e; p += GA_BLOCK) acc += (double)w[p];
  const double t = ga_block_tree(acc, s_red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(GA_BLOCK) void ga_wsum_final_kernel(const double* __restrict__ part, int64_t chunks, double* __restrict__ out) {
  __shared__ double s_red[GA_BLOCK];
  double acc = 0.0;
  for (int64_t p = threadIdx.x; p < chunks; p += GA_BLOCK) acc += part[p];
  const double t = ga_block_tree(acc, s_red);
  if (threadIdx.x == 0) out[0] = t;
}

// ---- slab builder (a): columns [c0, c0 + ncols) of a canonical cell-major CSR (sorted, unique columns) as a dense slab, implicit
// zeros written as 0.  One wave per row and trip: the row's first entry at or beyond c0 by a binary search (wave-uniform), the
// entries of the range scattered into the wave's LDS row, the row written with one coalesced store.  The row loop is uniform
// over the workgroup.
__global__ __launch_bounds__(GA_BLOCK) void ga_csr_slab_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                               const float* __restrict__ data, int64_t n, int c0, int ncols,
                                                               float* __restrict__ slab, int64_t ld) {
  __shared__ float s_row[GA_WAVES][GA_SLAB];
  const int lane = threadIdx.x & (GA_SLAB - 1), q = threadIdx.x >> 6;
  for (int64_t base = (int64_t)blockIdx.x * GA_WAVES; base < n; base += (int64_t)gridDim.x * GA_WAVES) {
    const int64_t r = base + q;
    s_row[q][lane] = 0.f;
    __syncthreads();
    if (r < n) {
      int64_t lo = indptr[r];
      const int64_t end = indptr[r + 1];
      int64_t hi = end;
      while (lo < hi) {  // the first entry with column >= c0
        const int64_t mid = (lo + hi) >> 1;
        if (indices[mid] < c0) lo = mid + 1;
        else hi = mid;
      }
      const int64_t p = lo + lane;  // (unique columns: at most ncols <= 64 entries fall into the range)
      if (p < end) {
        const int c = indices[p] - c0;
        if ((unsigned)c < (unsigned)ncols) s_row[q][c] = data[p];
      }
    }
    __syncthreads();
    if (r < n && lane < ncols) slab[r * ld + lane] = s_row[q][lane];
    __syncthreads();
  }
}

// ---- slab builder (b): feature-major dense rows vals[f][0 .. n) (row stride ldv) -> slab[cell][f], 64 x 64 tiles through LDS
template <typename VT>
__global__ __launch_bounds__(GA_BLOCK) void ga_transpose_kernel(const VT* __restrict__ vals, int64_t ldv, int64_t n, int ncols,
                                                                VT* __restrict__ slab, int64_t ld) {
  __shared__ VT s_tile[GA_SLAB][GA_SLAB + 1];
  const int lane = threadIdx.x & (GA_SLAB - 1), q = threadIdx.x >> 6;
  for (int64_t cell0 = (int64_t)blockIdx.x * GA_SLAB; cell0 < n; cell0 += (int64_t)gridDim.x * GA_SLAB) {
    for (int f = q; f < ncols; f += GA_WAVES)
      if (cell0 + lane < n) s_tile[f][lane] = vals[(int64_t)f * ldv + cell0 + lane];
    __syncthreads();
    for (int c = q; c < GA_SLAB; c += GA_WAVES)
      if (cell0 + c < n && lane < ncols) slab[(cell0 + c) * ld + lane] = s_tile[lane][c];
    __syncthreads();
  }
}

struct AutocorrWorkspace {
  double *col_part, *partial, *groups;
  size_t bytes;
  bool ok;
};

AutocorrWorkspace ga_carve(void* base, size_t cap, int64_t n, int64_t nnz) {
  Workspace ws(base, cap);
  AutocorrWorkspace r;
  r.col_part = ws.take<double>((size_t)ga_col_chunks(n) * 3 * GA_SLAB);
  r.partial = ws.take<double>((size_t)std::max<int64_t>(std::max<int64_t>(ga_parts(nnz), 1) * 2 * GA_SLAB, GA_WSUM_CHUNKS));
  r.groups = ws.take<double>((size_t)std::max<int64_t>(ceil_div(ga_parts(nnz), GA_REDUCE_GROUP), 1) * 2 * GA_SLAB);
  r.bytes = ws.used();
  r.ok = ws.ok;
  return r;
}

template <typename VT, typename WT>
void ga_launch_sweep(const int64_t* indptr, const int32_t* indices, const void* weights, int64_t n, int64_t nnz, const VT* S,
                     int64_t ld, int ncols, const double* mean, double* partial, hipStream_t stream) {
  const int64_t parts = ga_parts(nnz);
  const dim3 grid((unsigned)ceil_div(parts, GA_WAVES)), block(GA_BLOCK);
  // SCAMD_AUTOCORR_UNROLL=4 / 8: the other instantiation, for measurements; the sums do not depend on it
  if (env_int("SCAMD_AUTOCORR_UNROLL", GA_UNROLL) == 4)
    hipLaunchKernelGGL((ga_sweep_kernel<VT, WT, 4>), grid, block, 0, stream, indptr, indices, static_cast<const WT*>(weights), n, nnz,
                       ga_part_entries(nnz), parts, S, ld, ncols, mean, partial);
  else
    hipLaunchKernelGGL((ga_sweep_kernel<VT, WT, 8>), grid, block, 0, stream, indptr, indices, static_cast<const WT*>(weights), n, nnz,
                       ga_part_entries(nnz), parts, S, ld, ncols, mean, partial);
}

template <typename VT>
int ga_slab(const char* what, const int64_t* indptr, const int32_t* indices, const void* weights, int weights_is_f64, int64_t n,
            int64_t nnz, const VT* S, int64_t ld, int ncols, double* out_mean, double* out_z2, double* out_moran, double* out_geary,
            double* out_min, double* out_max, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  SCAMD_REQUIRE(indptr && n >= 1 && nnz >= 0 && (nnz == 0 || (indices && weights)) && S && out_mean && out_z2 && out_moran &&
                    out_geary && out_min && out_max,
                SCAMD_EINVAL, "%s: null pointer, n < 1 or negative nnz", what);
  SCAMD_REQUIRE(n < ((int64_t)1 << 31), SCAMD_EUNSUPPORTED, "%s: n = %lld cells, fewer than 2^31 are offered", what, (long long)n);
  SCAMD_REQUIRE(ncols >= 1 && ncols <= GA_SLAB && ld >= ncols, SCAMD_EINVAL, "%s: ncols = %d (1 .. %d), ld = %lld (>= ncols)", what,
                ncols, GA_SLAB, (long long)ld);
  const AutocorrWorkspace ws = ga_carve(workspace, workspace_bytes, n, nnz);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, ws.bytes);
  const int64_t rows = ga_col_chunk_rows(n), chunks = ga_col_chunks(n);
  hipLaunchKernelGGL((ga_col_chunk_kernel<VT, 0>), dim3((unsigned)chunks), dim3(GA_BLOCK), 0, stream, S, ld, ncols, n, rows,
                     (const double*)nullptr, ws.col_part);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((ga_col_reduce_kernel<0>), dim3(1), dim3(GA_BLOCK), 0, stream, ws.col_part, chunks, ncols, n, out_mean, out_min,
                     out_max, out_z2);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((ga_col_chunk_kernel<VT, 1>), dim3((unsigned)chunks), dim3(GA_BLOCK), 0, stream, S, ld, ncols, n, rows,
                     (const double*)out_mean, ws.col_part);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((ga_col_reduce_kernel<1>), dim3(1), dim3(GA_BLOCK), 0, stream, ws.col_part, chunks, ncols, n, out_mean, out_min,
                     out_max, out_z2);
  SCAMD_LAUNCH_CHECK();
  if (nnz > 0) {
    if (weights_is_f64) ga_launch_sweep<VT, double>(indptr, indices, weights, n, nnz, S, ld, ncols, out_mean, ws.partial, stream);
    else ga_launch_sweep<VT, float>(indptr, indices, weights, n, nnz, S, ld, ncols, out_mean, ws.partial, stream);
    SCAMD_LAUNCH_CHECK();
  }
  const int64_t groups = ceil_div(ga_parts(nnz), GA_REDUCE_GROUP);
  if (groups > 0) {
    hipLaunchKernelGGL((ga_reduce_kernel<false>), dim3((unsigned)groups), dim3(GA_BLOCK), 0, stream, ws.partial, ga_parts(nnz), ncols,
                       ws.groups, out_moran, out_geary);
    SCAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((ga_reduce_kernel<true>), dim3(1), dim3(GA_BLOCK), 0, stream, ws.groups, groups, ncols, ws.groups, out_moran,
                     out_geary);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

template <typename VT>
int ga_transpose(const char* what, const VT* vals, int64_t ldv, int64_t n, int ncols, VT* slab, int64_t ld, hipStream_t stream) {
  SCAMD_REQUIRE(n >= 0 && ncols >= 0 && ncols <= GA_SLAB && ld >= ncols && ldv >= n && (n == 0 || ncols == 0 || (vals && slab)),
                SCAMD_EINVAL, "%s: null pointer, ncols outside 0 .. %d, ld < ncols or ldv < n", what, GA_SLAB);
  if (n == 0 || ncols == 0) return SCAMD_OK;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, GA_SLAB), 65536);
  hipLaunchKernelGGL((ga_transpose_kernel<VT>), dim3(grid), dim3(GA_BLOCK), 0, stream, vals, ldv, n, ncols, slab, ld);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

}  // namespace
}  // namespace scamd

using namespace scamd;

extern "C" size_t scamd_graph_autocorr_workspace_bytes(int64_t n, int64_t nnz) {
  if (n < 0 || nnz < 0) return 0;
  return ga_carve(nullptr, 0, n, nnz).bytes;
}

extern "C" int scamd_graph_autocorr_part_entries(int64_t nnz) { return nnz < 0 ? 0 : ga_part_entries(nnz); }

extern "C" int scamd_graph_autocorr_slab_f32(const int64_t* indptr, const int32_t* indices, const void* weights, int weights_is_f64,
                                             int64_t n, int64_t nnz, const float* slab, int64_t ld, int32_t ncols, double* out_mean,
                                             double* out_z2, double* out_moran, double* out_geary, double* out_min, double* out_max,
                                             void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  return ga_slab<float>("graph_autocorr_slab_f32", indptr, indices, weights, weights_is_f64, n, nnz, slab, ld, ncols, out_mean, out_z2,
                        out_moran, out_geary, out_min, out_max, workspace, workspace_bytes, stream);
}

extern "C" int scamd_graph_autocorr_slab_f64(const int64_t* indptr, const int32_t* indices, const void* weights, int weights_is_f64,
                                             int64_t n, int64_t nnz, const double* slab, int64_t ld, int32_t ncols, double* out_mean,
                                             double* out_z2, double* out_moran, double* out_geary, double* out_min, double* out_max,
                                             void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  return ga_slab<double>("graph_autocorr_slab_f64", indptr, indices, weights, weights_is_f64, n, nnz, slab, ld, ncols, out_mean,
                         out_z2, out_moran, out_geary, out_min, out_max, workspace, workspace_bytes, stream);
}

extern "C" int scamd_graph_weight_sum_f64(const void* weights, int weights_is_f64, int64_t nnz, double* out, void* workspace,
                                          size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(nnz >= 0 && out && (nnz == 0 || weights), SCAMD_EINVAL, "graph_weight_sum: null pointer or negative nnz");
  const size_t need = sizeof(double) * GA_WSUM_CHUNKS;
  SCAMD_REQUIRE(workspace && workspace_bytes >= need, SCAMD_EINVAL, "graph_weight_sum: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  double* part = static_cast<double*>(workspace);
  const int64_t chunk = ga_wsum_chunk(nnz), chunks = (nnz + chunk - 1) / chunk;
  if (chunks > 0) {
    if (weights_is_f64)
      hipLaunchKernelGGL((ga_wsum_chunk_kernel<double>), dim3((unsigned)chunks), dim3(GA_BLOCK), 0, stream,
                         static_cast<const double*>(weights), nnz, chunk, part);
    else
      hipLaunchKernelGGL((ga_wsum_chunk_kernel<float>), dim3((unsigned)chunks), dim3(GA_BLOCK), 0, stream,
                         static_cast<const float*>(weights), nnz, chunk, part);
    SCAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ga_wsum_final_kernel, dim3(1), dim3(GA_BLOCK), 0, stream, part, chunks, out);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

extern "C" int scamd_csr_dense_slab_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                        int64_t nnz, int64_t c0, int32_t ncols, float* slab, int64_t ld, scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && n >= 0 && g >= 0 && nnz >= 0 && g < ((int64_t)1 << 31) && (nnz == 0 || (indices && data)) && (n == 0 || slab),
                SCAMD_EINVAL, "csr_dense_slab: null pointer or negative size");
  SCAMD_REQUIRE(ncols >= 1 && ncols <= GA_SLAB && ld >= ncols && c0 >= 0 && c0 + ncols <= g, SCAMD_EINVAL,
                "csr_dense_slab: columns [%lld, %lld + %d) of %lld, ld = %lld", (long long)c0, (long long)c0, ncols, (long long)g,
                (long long)ld);
  if (n == 0) return SCAMD_OK;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, GA_WAVES), 65536);
  hipLaunchKernelGGL(ga_csr_slab_kernel, dim3(grid), dim3(GA_BLOCK), 0, stream, indptr, indices, data, n, (int)c0, (int)ncols, slab, ld);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

extern "C" int scamd_transpose_slab_f32(const float* vals, int64_t ldv, int64_t n, int32_t ncols, float* slab, int64_t ld,
                                        scamd_stream_t stream) {
  return ga_transpose<float>("transpose_slab_f32", vals, ldv, n, ncols, slab, ld, stream);
}

extern "C" int scamd_transpose_slab_f64(const double* vals, int64_t ldv, int64_t n, int32_t ncols, double* slab, int64_t ld,
                                        scamd_stream_t stream) {
  return ga_transpose<double>("transpose_slab_f64", vals, ldv, n, ncols, slab, ld, stream);
}
