// Regressing out observation annotations from a CSR float32 matrix: the device passes behind scanpy_amd.pp.regress_out
// (reference: `regress_out`, `numpy_regress_out`, `_regress_out_chunk` in src/scanpy/preprocessing/_simple.py:468-681).
//
// Both branches of the reference are ONE model, out[i, j] = x_ij - sum_k W[i, k] * T[k, j]:
//   numeric keys     W[i, :] = [1, Q[i, :]] with Q an orthonormal basis of the centred regressors (made on the host, m = r + 1 <= 17
//                    columns), T = [mean; Q^T X]: the residual of the least-squares fit on span[1, keys...];
//   categorical key  W[i, :] = one-hot of codes[i], T = the per-gene mean of every category: row codes[i] of T is looked up.
// The matrix must be canonical CSR (no column twice in a row); an implicit zero is the value 0.
//
// 1. scamd_pp_regress_sums_f32: S = W^T X (float64, m x g), per gene the minimum and maximum over all n cells and a flag
//    "a stored value was not finite" (such values take no part in anything).  Two sweeps of the matrix:
//    rg_range_kernel   per gene the largest and smallest stored value as order-preserving keys (integer atomicMax / atomicMin) and
//                      the number of stored entries (a gene with fewer than n of them also holds the value 0);
//    rg_sums_kernel    every term w * x is rounded ONCE to 64-bit fixed point and added with integer atomics -- in a table in LDS
//                      per workgroup where m * g * 8 B fit RG_LDS_TABLE_BYTES, then globally -- so that S does not depend on the
//                      order in which lanes, waves and workgroups run: two calls give the same bits.  There are no float atomics.
//    THE SCALE.  For table row k and gene j: |sum_i W[i,k] x_ij| <= wbound[k] * amax_j with wbound[k] >= sum_i |W[i,k]| (given by
//    the caller: n for the column of ones, <= sqrt(n) for a unit column of Q, the size of category k) and amax_j = max_i |x_ij|
//    (from the range sweep).  With wbound[k] < 2^ew and amax_j < 2^ea (frexp) the term is scaled by 2^(62 - ew - ea): the sum stays
//    below 2^62 in magnitude and every term is off by at most half a unit, 2^(ew + ea - 63).
//    THE BOUND.  |S[k,j] - exact| <= nnz_j * 2^(ew + ea - 63) + wbound[k] * amax_j * 2^-52
//                                 <= (n * 2^-61 + 2^-52) * wbound[k] * amax_j
//    (2^ew <= 2 wbound, 2^ea <= 2 amax; the second term is the float64 rounding of the products w * x and of the conversion).
//    For the residual, which multiplies S[k,j] by |W[i,k]| <= 1 (numeric: after division by 1 for Q, by n for the mean) this is
//    n^1.5 * 2^-61 * amax_j per key: 4.3e-10 * amax_j at n = 10^6, 1.5e-13 * amax_j at n = 5000.
//
// 2. scamd_pp_regress_resid_f32: the dense row-major output, float32 or float64; every element is computed in float64 and
//    rounded once.  One pass, no read-modify-write: a workgroup owns a slice of CS = 4 * TPR columns and walks down the rows, a
//    batch of 4 * RG_BLOCK / TPR consecutive rows at a time.  The stored entries of the batch that fall into the slice are
//    scattered into zeroed row buffers in LDS; then every thread takes the four neighbouring columns it owns from the buffers,
//    subtracts the fit (fma, k ascending) and writes them with one 16-byte store (float32; two for float64): full-width
//    coalesced stores, n * g * sizeof(out) bytes.  Numeric: the slice of T (m x CS float64, <= 34 KiB) is staged in LDS once per
//    workgroup, with zero columns for the genes that are not kept (x - 0 is x), and the batch's rows of W -- one contiguous run of
//    w -- once per batch.  Categorical: T can be megabytes; the cell's own row of it is read through L2.
//    Every workgroup scans the whole rows for the entries of its slice: the matrix is read ceil(g / CS) times, which is 1-2 times
//    for a matrix of highly variable genes and 30 times at 30 000 genes, where the kernel loses to the fill + scatter scheme of
//    scale_dense; at 1M x 2000 it takes 0.52-0.74 of that scheme's time and reaches a third to a half of the store roofline,
//    bound by the latency of its two load phases per batch, not by the stores (profiles/regress_out_timing.log).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"

namespace scamd {

namespace {

constexpr int RG_BLOCK = 256;
constexpr int RG_MAX_W = 17;                 // numeric: the column of ones and up to 16 keys
constexpr int RG_MAX_CATEGORIES = 65536;
constexpr int RG_GRID_CAP = 256 * 32;        // workgroups of a row-wise launch
constexpr int RG_LDS_GRID_CAP = 512;         // workgroups of a sweep with its table in LDS (one flush each)
constexpr int RG_RANGE_LDS_GENES = 2048;     // the range table (12 B per gene) lives in LDS up to this many genes
constexpr int RG_LDS_TABLE_BYTES = 48 * 1024;  // the fixed-point table of the sums lives in LDS up to this size
constexpr int RG_BATCH_PASSES = 4;        // rows per thread and batch of the residual kernel
constexpr int RG_RESID_GRID = 2048;          // workgroups of the residual kernel (row blocks x column slices), about

constexpr unsigned RG_KEY_NONE_MAX = 0u;           // below the key of every finite value
constexpr unsigned RG_KEY_NONE_MIN = 0xffffffffu;  // above it

__device__ __forceinline__ bool rg_finite(unsigned bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
// float bits -> unsigned key with the order of the values (negative: all bits flipped, else the sign bit set)
__device__ __forceinline__ unsigned rg_key(unsigned bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float rg_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}
__device__ __forceinline__ void rg_fix_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// ---- sweep 1: per gene the largest / smallest stored value (keys) and the number of stored entries.  LDS: the table of the
// workgroup in LDS (g <= RG_RANGE_LDS_GENES), flushed once.  The row loop is uniform over the workgroup.
template <int G, bool LDS>
__global__ __launch_bounds__(RG_BLOCK) void rg_range_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const float* __restrict__ data, int64_t n, int g, unsigned int* kmax,
                                                            unsigned int* kmin, unsigned long long* cnt, unsigned int* flags) {
  extern __shared__ __attribute__((aligned(16))) double rg_smem[];
  unsigned int* s_max = reinterpret_cast<unsigned int*>(rg_smem);
  unsigned int* s_min = s_max + g;
  unsigned int* s_cnt = s_min + g;
  if (LDS) {
    for (int c = threadIdx.x; c < g; c += RG_BLOCK) {
      s_max[c] = RG_KEY_NONE_MAX;
      s_min[c] = RG_KEY_NONE_MIN;
      s_cnt[c] = 0u;
    }
    __syncthreads();
  }
  unsigned int* tmax = LDS ? s_max : kmax;
  unsigned int* tmin = LDS ? s_min : kmin;
  constexpr int RPB = RG_BLOCK / G;
  const int sub = threadIdx.x % G;
  unsigned int bad = 0u;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < n; base += (int64_t)gridDim.x * RPB) {
    const int64_t r = base + threadIdx.x / G;
    const bool valid = r < n;
    const int64_t b = valid ? indptr[r] : 0, e = valid ? indptr[r + 1] : 0;
    for (int64_t p = b + sub; p < e; p += G) {
      const unsigned bits = __float_as_uint(data[p]);
      if (!rg_finite(bits)) {
        bad = 1u;
        continue;
      }
      const int c = indices[p];
      const unsigned key = rg_key(bits);
      // the tables only grow / shrink: a stale value read here costs a needless atomic, never a missed one
      if (key > tmax[c]) atomicMax(&tmax[c], key);
      if (key < tmin[c]) atomicMin(&tmin[c], key);
      if (LDS) atomicAdd(&s_cnt[c], 1u);
      else atomicAdd(&cnt[c], 1ull);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int c = threadIdx.x; c < g; c += RG_BLOCK) {
      if (s_cnt[c]) {
        atomicMax(&kmax[c], s_max[c]);
        atomicMin(&kmin[c], s_min[c]);
        atomicAdd(&cnt[c], (unsigned long long)s_cnt[c]);
      }
    }
  }
  if (bad) atomicOr(flags, 1u);
}

// per gene: minimum and maximum over all n cells (an implicit zero is a value), the power of two above max |x|; per table row:
// the power of two above wbound.  sx * sw = 2^(62 - ea - ew) is the fixed-point scale, ix * iw its inverse.
__global__ __launch_bounds__(RG_BLOCK) void rg_scale_kernel(int64_t n, int g, int m, const unsigned int* __restrict__ kmax,
                                                            const unsigned int* __restrict__ kmin,
                                                            const unsigned long long* __restrict__ cnt,
                                                            const double* __restrict__ wbound, float* __restrict__ col_min,
                                                            float* __restrict__ col_max, double* __restrict__ sx,
                                                            double* __restrict__ ix, double* __restrict__ sw,
                                                            double* __restrict__ iw) {
  const int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
  if (i < g) {
    float lo = 0.f, hi = 0.f;
    const unsigned long long c = cnt[i];
    if (c) {
      lo = rg_value(kmin[i]);
      hi = rg_value(kmax[i]);
      if ((int64_t)c < n) {
        lo = lo < 0.f ? lo : 0.f;
        hi = hi > 0.f ? hi : 0.f;
      }
    }
    col_min[i] = lo;
    col_max[i] = hi;
    const double amax = fmax(fabs((double)lo), fabs((double)hi));
    int ea = 0;
    if (amax > 0.0) {
      frexp(amax, &ea);  // amax < 2^ea
      sx[i] = ldexp(1.0, -ea);
      ix[i] = ldexp(1.0, ea);
    } else {
      sx[i] = 0.0;
      ix[i] = 0.0;
    }
  }
  if (i < m) {
    const double wb = wbound[i];
    int ew = 0;
    if (wb > 0.0 && wb < 1e300) {
      frexp(wb, &ew);  // wb < 2^ew
      sw[i] = ldexp(1.0, 62 - ew);
      iw[i] = ldexp(1.0, ew - 62);
    } else {
      sw[i] = 0.0;
      iw[i] = 0.0;
    }
  }
}

// ---- sweep 2: fix[k, c] += round(W[r, k] * x * 2^(62 - ew_k - ea_c)).  codes == nullptr: numeric, k = 0 .. m - 1; else the one
// row k = codes[r] with weight 1.  LDS: the table of the workgroup in LDS (m * g * 8 B <= RG_LDS_TABLE_BYTES), flushed once.
template <int G, bool LDS>
__global__ __launch_bounds__(RG_BLOCK) void rg_sums_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                           const float* __restrict__ data, int64_t n, int g, int m,
                                                           const double* __restrict__ w, const int32_t* __restrict__ codes,
                                                           const double* __restrict__ sx, const double* __restrict__ sw,
                                                           long long* fix, unsigned int* flags) {
  extern __shared__ __attribute__((aligned(16))) double rg_smem[];
  long long* s_fix = reinterpret_cast<long long*>(rg_smem);
  const int cells = m * g;  // (LDS only: at most RG_LDS_TABLE_BYTES / 8)
  if (LDS) {
    for (int c = threadIdx.x; c < cells; c += RG_BLOCK) s_fix[c] = 0;
    __syncthreads();
  }
  long long* tab = LDS ? s_fix : fix;
  constexpr int RPB = RG_BLOCK / G;
  const int sub = threadIdx.x % G;
  const int nk = codes ? 1 : m;
  unsigned int bad = 0u;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < n; base += (int64_t)gridDim.x * RPB) {
    const int64_t r = base + threadIdx.x / G;
    const bool valid = r < n;
    int64_t b = valid ? indptr[r] : 0, e = valid ? indptr[r + 1] : 0;
    int row0 = 0;
    double ws[RG_MAX_W];
    if (codes) {
      row0 = valid ? codes[r] : 0;
      if ((unsigned)row0 >= (unsigned)m) {  // no such category: the row takes no part, the caller is told
        if (valid) bad = 2u;
        row0 = 0;
        e = b;
      }
      ws[0] = sw[row0];
    } else {
#pragma unroll
      for (int k = 0; k < RG_MAX_W; ++k) ws[k] = (valid && k < m) ? w[r * m + k] * sw[k] : 0.0;
    }
    long long* trow = tab + (int64_t)row0 * g;
    for (int64_t p = b + sub; p < e; p += G) {
      const unsigned bits = __float_as_uint(data[p]);
      if (!rg_finite(bits)) continue;
      const int c = indices[p];
      const double x = (double)__uint_as_float(bits), s = sx[c];
#pragma unroll
      for (int k = 0; k < RG_MAX_W; ++k) {
        if (k < nk) {
          const long long v = llrint((ws[k] * x) * s);
          if (v) rg_fix_add(&trow[(int64_t)k * g + c], v);
        }
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += RG_BLOCK)
      if (s_fix[c]) rg_fix_add(&fix[c], s_fix[c]);
  }
  if (bad) atomicOr(flags, bad);
}

__global__ __launch_bounds__(RG_BLOCK) void rg_convert_kernel(int g, int64_t cells, const long long* __restrict__ fix,
                                                              const double* __restrict__ ix, const double* __restrict__ iw,
                                                              double* __restrict__ sums) {
  for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * RG_BLOCK)
    sums[i] = ((double)fix[i] * ix[i % g]) * iw[i / g];
}

__device__ __forceinline__ void rg_store4(float* o, const double* v) {
  *reinterpret_cast<float4*>(o) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ void rg_store4(double* o, const double* v) {
  *reinterpret_cast<double2*>(o) = make_double2(v[0], v[1]);
  *reinterpret_cast<double2*>(o + 2) = make_double2(v[2], v[3]);
}

// ---- the residual.  TPR threads per row own CS = 4 * TPR columns: 256 / 128 / 64 threads for m <= 4 / 8 / 17 table rows, which
// keeps the staged slice of T at or below 34 KiB.  blockIdx.x = row block * slices + slice.  A workgroup takes a batch of
// R = RG_BATCH_PASSES * RPB consecutive rows between two barriers: their stored entries are one contiguous run of the CSR
// arrays, read by all 256 threads with coalesced loads whatever the row lengths (the row of an entry is found among the R + 1
// staged row pointers) and scattered into R zeroed row buffers in LDS; then every thread takes its four columns of
// RG_BATCH_PASSES rows, clears what it read (the next batch finds the buffers zeroed) and writes.  All loops are uniform over
// the workgroup (rows past n are empty rows that write nothing).
template <typename OutT, int TPR, bool CAT>
__global__ __launch_bounds__(RG_BLOCK) void rg_resid_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const float* __restrict__ data, int64_t n, int g, int m, int slices,
                                                            const uint8_t* __restrict__ keep, const double* __restrict__ table,
                                                            const double* __restrict__ w, const int32_t* __restrict__ codes,
                                                            OutT* __restrict__ out) {
  constexpr int CS = TPR * 4, RPB = RG_BLOCK / TPR, R = RG_BATCH_PASSES * RPB;
  extern __shared__ __attribute__((aligned(16))) double rg_smem[];  // numeric: T[:, c0 : c0 + CS], row stride CS
  __shared__ __attribute__((aligned(16))) float s_x[R * CS];       // R row buffers of CS values (16 KiB)
  __shared__ int64_t s_ptr[R + 1];
  // numeric: W[r0 : r0 + R, :], one contiguous run of w; categorical: the codes.  Two copies, by the parity of the trip: they
  // are read in step 3, which no barrier separates from step 1 of the next trip
  __shared__ double s_w2[2][CAT ? 1 : R * RG_MAX_W];
  __shared__ int s_code2[2][CAT ? R : 1];
  const int slice = (int)(blockIdx.x % (unsigned)slices);
  const int64_t row_block = blockIdx.x / (unsigned)slices, row_blocks = gridDim.x / (unsigned)slices;
  const int c0 = slice * CS;
  const int ncols = min(CS, g - c0);
  if (!CAT) {
    for (int i = threadIdx.x; i < m * CS; i += RG_BLOCK) {
      const int k = i / CS, c = i % CS;
      rg_smem[i] = (c < ncols && keep[c0 + c] != 0) ? table[(int64_t)k * g + c0 + c] : 0.0;  // (keep == 0: x - 0 is x)
    }
  }
  const int slot = threadIdx.x / TPR, t = threadIdx.x % TPR;
  const int cq = 4 * t;  // first of this thread's four columns, inside the slice
  bool kq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) kq[q] = cq + q < ncols && keep[c0 + cq + q] != 0;
#pragma unroll
  for (int j = 0; j < RG_BATCH_PASSES; ++j)
    *reinterpret_cast<float4*>(s_x + (j * RPB + slot) * CS + cq) = make_float4(0.f, 0.f, 0.f, 0.f);
  int trip = 0;
  for (int64_t r0 = row_block * R; r0 < n; r0 += row_blocks * R, trip ^= 1) {
    double* s_w = s_w2[trip];
    int* s_code = s_code2[trip];
    // ---- 1. the batch's row pointers and its rows of W (or its codes): independent loads, one latency
    if (threadIdx.x <= R) s_ptr[threadIdx.x] = indptr[min(r0 + threadIdx.x, n)];
    if (CAT) {
      if (threadIdx.x < R) s_code[threadIdx.x] = r0 + threadIdx.x < n ? codes[r0 + threadIdx.x] : -1;
    } else {
      const int64_t w_end = n * m;
      for (int i = threadIdx.x; i < R * m; i += RG_BLOCK) {
        const int64_t at = r0 * m + i;
        s_w[i] = at < w_end ? w[at] : 0.0;
      }
    }
    __syncthreads();  // (the first trip: also the staged slice of T and the zeroed buffers)
    // ---- 2. the batch's entries, two per thread and trip, every load issued before the first use
    const int64_t pb = s_ptr[0], pe = s_ptr[R];
    for (int64_t p = pb + threadIdx.x; p < pe; p += 2 * RG_BLOCK) {
      const bool two = p + RG_BLOCK < pe;
      const int64_t p2 = two ? p + RG_BLOCK : p;
      const int ca = indices[p] - c0, cb = indices[p2] - c0;
      const float va = data[p], vb = data[p2];
      int ra = 0, rb = 0;
#pragma unroll
      for (int j = 1; j < R; ++j) {
        const int64_t bound = s_ptr[j];
        ra += p >= bound ? 1 : 0;
        rb += p2 >= bound ? 1 : 0;
      }
      if ((unsigned)ca < (unsigned)ncols) s_x[ra * CS + ca] = va;
      if (two && (unsigned)cb < (unsigned)ncols) s_x[rb * CS + cb] = vb;
    }
    __syncthreads();
    // ---- 3. four columns of RG_BATCH_PASSES rows per thread
    if (cq < ncols) {
      const bool whole = cq + 4 <= ncols;
      double fit[RG_BATCH_PASSES][4];
      float4 xv[RG_BATCH_PASSES];
#pragma unroll
      for (int j = 0; j < RG_BATCH_PASSES; ++j) {
        float4* xp = reinterpret_cast<float4*>(s_x + (j * RPB + slot) * CS + cq);
        xv[j] = *xp;
        *xp = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < 4; ++q) fit[j][q] = 0.0;
      }
      if (CAT) {
#pragma unroll
        for (int j = 0; j < RG_BATCH_PASSES; ++j) {
          const int code = s_code[j * RPB + slot];
          // (a row past n, or no such category: nothing is subtracted; the sums pass has raised its flag)
          const double* trow = table + (int64_t)((unsigned)code < (unsigned)m ? code : 0) * g + c0 + cq;
          const bool on = (unsigned)code < (unsigned)m;
          if (whole) {
#pragma unroll
            for (int q = 0; q < 4; ++q) fit[j][q] = trow[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) fit[j][q] = (on && kq[q]) ? fit[j][q] : 0.0;
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (cq + q < ncols && on && kq[q]) fit[j][q] = trow[q];
          }
        }
      } else {
        for (int k = 0; k < m; ++k) {
          const double* tl = rg_smem + k * CS + cq;
          const double t0 = tl[0], t1 = tl[1], t2 = tl[2], t3 = tl[3];
#pragma unroll
          for (int j = 0; j < RG_BATCH_PASSES; ++j) {
            const double wk = s_w[(j * RPB + slot) * m + k];
            fit[j][0] = fma(wk, t0, fit[j][0]);
            fit[j][1] = fma(wk, t1, fit[j][1]);
            fit[j][2] = fma(wk, t2, fit[j][2]);
            fit[j][3] = fma(wk, t3, fit[j][3]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < RG_BATCH_PASSES; ++j) {
        const int64_t r = r0 + j * RPB + slot;
        if (r < n) {
          const double x[4] = {(double)xv[j].x, (double)xv[j].y, (double)xv[j].z, (double)xv[j].w};
          double v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = x[q] - fit[j][q];  // (a gene that is not kept has fit 0)
          OutT* o = out + r * (int64_t)g + c0 + cq;
          if (whole && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
            rg_store4(o, v);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (cq + q < ncols) o[q] = (OutT)v[q];
          }
        }
      }
    }
  }
}

// lanes per row of the sweeps from the mean row length (the rule of csrc/preprocess.hip)
inline int rg_lanes_per_row(int64_t n, int64_t nnz) {
  const int64_t avg = n > 0 ? nnz / n : 0;
  return avg <= 32 ? 8 : (avg <= 160 ? 16 : (avg <= 512 ? 32 : 64));
}

// threads per row of the residual kernel from the number of table rows it stages (categorical: none, 256)
inline int rg_resid_threads(int m, bool cat) { return (cat || m <= 4) ? 256 : (m <= 8 ? 128 : 64); }

inline unsigned rg_sweep_grid(int64_t n, int G, bool lds) {
  constexpr int64_t one = 1;
  if (lds) return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n, (RG_BLOCK / G) * 16), one), RG_LDS_GRID_CAP);
  return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n, RG_BLOCK / G), one), RG_GRID_CAP);
}

struct RegressWorkspace {
  long long* fix;
  unsigned int *kmax, *kmin;
  unsigned long long* cnt;
  double *sx, *ix, *sw, *iw;
  size_t bytes;
  bool ok;
};

RegressWorkspace rg_carve(void* base, size_t cap, int64_t g, int m) {
  Workspace ws(base, cap);
  RegressWorkspace r;
  r.fix = ws.take<long long>((size_t)m * (size_t)g);
  r.kmax = ws.take<unsigned int>((size_t)g);
  r.kmin = ws.take<unsigned int>((size_t)g);
  r.cnt = ws.take<unsigned long long>((size_t)g);
  r.sx = ws.take<double>((size_t)g);
  r.ix = ws.take<double>((size_t)g);
  r.sw = ws.take<double>((size_t)m);
  r.iw = ws.take<double>((size_t)m);
  r.bytes = ws.used();
  r.ok = ws.ok;
  return r;
}

template <int G>
void rg_launch_range(bool lds, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int g,
                     const RegressWorkspace& ws, unsigned int* flags, hipStream_t stream) {
  if (lds)
    hipLaunchKernelGGL((rg_range_kernel<G, true>), dim3(rg_sweep_grid(n, G, true)), dim3(RG_BLOCK), (size_t)g * 12 + 16, stream,
                       indptr, indices, data, n, g, ws.kmax, ws.kmin, ws.cnt, flags);
  else
    hipLaunchKernelGGL((rg_range_kernel<G, false>), dim3(rg_sweep_grid(n, G, false)), dim3(RG_BLOCK), 0, stream, indptr, indices,
                       data, n, g, ws.kmax, ws.kmin, ws.cnt, flags);
}

template <int G>
void rg_launch_sums(bool lds, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int g, int m,
                    const double* w, const int32_t* codes, const RegressWorkspace& ws, unsigned int* flags, hipStream_t stream) {
  if (lds)
    hipLaunchKernelGGL((rg_sums_kernel<G, true>), dim3(rg_sweep_grid(n, G, true)), dim3(RG_BLOCK), (size_t)m * g * 8 + 16, stream,
                       indptr, indices, data, n, g, m, w, codes, ws.sx, ws.sw, ws.fix, flags);
  else
    hipLaunchKernelGGL((rg_sums_kernel<G, false>), dim3(rg_sweep_grid(n, G, false)), dim3(RG_BLOCK), 0, stream, indptr, indices,
                       data, n, g, m, w, codes, ws.sx, ws.sw, ws.fix, flags);
}

template <typename OutT, int TPR>
void rg_launch_resid(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int g, int m,
                     const uint8_t* keep, const double* table, const double* w, const int32_t* codes, OutT* out,
                     hipStream_t stream) {
  constexpr int CS = TPR * 4, R = RG_BATCH_PASSES * (RG_BLOCK / TPR);
  const int slices = ceil_div(g, CS);
  const int64_t row_blocks =
      std::min<int64_t>(std::max<int64_t>(ceil_div(n, R), 1), std::max<int64_t>(RG_RESID_GRID / slices, 1));
  const unsigned grid = (unsigned)(row_blocks * slices);
  if (codes)
    hipLaunchKernelGGL((rg_resid_kernel<OutT, TPR, true>), dim3(grid), dim3(RG_BLOCK), 0, stream, indptr, indices, data, n, g, m,
                       slices, keep, table, w, codes, out);
  else
    hipLaunchKernelGGL((rg_resid_kernel<OutT, TPR, false>), dim3(grid), dim3(RG_BLOCK), (size_t)m * CS * 8, stream, indptr,
                       indices, data, n, g, m, slices, keep, table, w, codes, out);
}

template <typename OutT>
void rg_dispatch_resid(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int g, int m,
                       const uint8_t* keep, const double* table, const double* w, const int32_t* codes, OutT* out,
                       hipStream_t stream) {
  switch (rg_resid_threads(m, codes != nullptr)) {
    case 256: rg_launch_resid<OutT, 256>(indptr, indices, data, n, g, m, keep, table, w, codes, out, stream); break;
    case 128: rg_launch_resid<OutT, 128>(indptr, indices, data, n, g, m, keep, table, w, codes, out, stream); break;
    default: rg_launch_resid<OutT, 64>(indptr, indices, data, n, g, m, keep, table, w, codes, out, stream); break;
  }
}

// the checks both entry points share; `what` names the entry point
int rg_check_model(const char* what, const double* w, const int32_t* codes, int m) {
  SCAMD_REQUIRE((w == nullptr) != (codes == nullptr), SCAMD_EINVAL, "%s: exactly one of w (numeric keys) and codes (a categorical key)",
                what);
  SCAMD_REQUIRE(m >= 1, SCAMD_EINVAL, "%s: m = %d table rows", what, m);
  SCAMD_REQUIRE(codes || m <= RG_MAX_W, SCAMD_EUNSUPPORTED, "%s: %d numeric columns, at most %d (the ones and 16 keys)", what, m,
                RG_MAX_W);
  SCAMD_REQUIRE(w || m <= RG_MAX_CATEGORIES, SCAMD_EUNSUPPORTED, "%s: %d categories, at most %d", what, m, RG_MAX_CATEGORIES);
  return SCAMD_OK;
}

}  // namespace
}  // namespace scamd

using namespace scamd;

extern "C" size_t scamd_pp_regress_workspace_bytes(int64_t g, int32_t m) {
  if (g < 0 || m < 0) return 0;
  return rg_carve(nullptr, 0, g, m).bytes;
}

extern "C" int scamd_pp_regress_sums_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                         int64_t nnz, const double* w, const int32_t* codes, int32_t m, const double* wbound,
                                         double* sums, float* col_min, float* col_max, uint32_t* flags, void* workspace,
                                         size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && n >= 0 && g >= 0 && nnz >= 0 && g < ((int64_t)1 << 31) && flags && (nnz == 0 || (data && indices)) &&
                    wbound && (g == 0 || (sums && col_min && col_max)),
                SCAMD_EINVAL, "pp_regress_sums: null pointer or negative size");
  const int rc = rg_check_model("pp_regress_sums", w, codes, m);
  if (rc != SCAMD_OK) return rc;
  const RegressWorkspace ws = rg_carve(workspace, workspace_bytes, g, m);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EINVAL, "pp_regress_sums: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes);
  SCAMD_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(uint32_t), stream));
  if (g == 0) return SCAMD_OK;
  const int gi = (int)g;
  const int64_t cells = (int64_t)m * g;
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.fix, 0, sizeof(long long) * (size_t)cells, stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.kmax, 0x00, sizeof(unsigned int) * (size_t)g, stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.kmin, 0xff, sizeof(unsigned int) * (size_t)g, stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.cnt, 0, sizeof(unsigned long long) * (size_t)g, stream));
  const int G = rg_lanes_per_row(n, nnz);
  const bool range_lds = g <= RG_RANGE_LDS_GENES;
  const bool sums_lds = cells * 8 <= RG_LDS_TABLE_BYTES;
  if (n > 0) {
    switch (G) {
      case 8: rg_launch_range<8>(range_lds, indptr, indices, data, n, gi, ws, flags, stream); break;
      case 16: rg_launch_range<16>(range_lds, indptr, indices, data, n, gi, ws, flags, stream); break;
      case 32: rg_launch_range<32>(range_lds, indptr, indices, data, n, gi, ws, flags, stream); break;
      default: rg_launch_range<64>(range_lds, indptr, indices, data, n, gi, ws, flags, stream); break;
    }
    SCAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rg_scale_kernel, dim3(ceil_div(std::max<int64_t>(g, m), RG_BLOCK)), dim3(RG_BLOCK), 0, stream, n, gi, m, ws.kmax,
                     ws.kmin, ws.cnt, wbound, col_min, col_max, ws.sx, ws.ix, ws.sw, ws.iw);
  SCAMD_LAUNCH_CHECK();
  if (n > 0) {
    switch (G) {
      case 8: rg_launch_sums<8>(sums_lds, indptr, indices, data, n, gi, m, w, codes, ws, flags, stream); break;
      case 16: rg_launch_sums<16>(sums_lds, indptr, indices, data, n, gi, m, w, codes, ws, flags, stream); break;
      case 32: rg_launch_sums<32>(sums_lds, indptr, indices, data, n, gi, m, w, codes, ws, flags, stream); break;
      default: rg_launch_sums<64>(sums_lds, indptr, indices, data, n, gi, m, w, codes, ws, flags, stream); break;
    }
    SCAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rg_convert_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(cells, RG_BLOCK), RG_GRID_CAP)), dim3(RG_BLOCK), 0,
                     stream, gi, cells, ws.fix, ws.ix, ws.iw, sums);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

extern "C" int scamd_pp_regress_resid_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                          int64_t nnz, const uint8_t* keep, const double* table, const double* w,
                                          const int32_t* codes, int32_t m, void* out, int out_is_f64, scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && n >= 0 && g >= 0 && nnz >= 0 && g < ((int64_t)1 << 31) && (nnz == 0 || (data && indices)) &&
                    (g == 0 || (keep && table)) && (n == 0 || g == 0 || out),
                SCAMD_EINVAL, "pp_regress_resid: null pointer or negative size");
  const int rc = rg_check_model("pp_regress_resid", w, codes, m);
  if (rc != SCAMD_OK) return rc;
  if (n == 0 || g == 0) return SCAMD_OK;
  if (out_is_f64)
    rg_dispatch_resid<double>(indptr, indices, data, n, (int)g, m, keep, table, w, codes, static_cast<double*>(out), stream);
  else
    rg_dispatch_resid<float>(indptr, indices, data, n, (int)g, m, keep, table, w, codes, static_cast<float*>(out), stream);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}
