// Quality-control metrics on a CSR float32 matrix: the device passes behind scanpy_amd.pp.calculate_qc_metrics
// (reference: `describe_obs`, `describe_var`, `top_segment_proportions` in src/scanpy/preprocessing/_qc.py).
//
// A stored 0.0 / -0.0 is no entry anywhere in this file (the reference calls eliminate_zeros first): the kernels skip it
// by its bit pattern, the caller's matrix is never rewritten.
//
// 1. qc_sweep_kernel: ONE sweep over indptr / indices / data (8 B per stored entry, 4 B when neither a gene mask nor the
//    per-gene outputs are asked for) gives, per row, the non-zero count (int32), the total (float64) and up to 32 masked
//    totals (float64; bit k of gene_mask[c] = gene c belongs to mask k), and, per gene, the non-zero count and the sum over
//    cells.  The per-row sums are lane-local float64 sums reduced by a fixed shuffle tree: bitwise reproducible.  The
//    per-gene table lives in LDS up to QC_LDS_GENES genes (12 B per gene and workgroup, flushed once); beyond -- every raw
//    count matrix -- the adds go to global memory (one float64 and one 64-bit integer atomic per entry).  Float64 atomics
//    add in arrival order: the per-gene sums are bitwise reproducible on integer-valued matrices (every partial sum below
//    2^53 is exact) and agree to ~1e-15 relative otherwise.  A flag word records "a negative value was seen".
//
// 2. qc_top_kernel: top(n) for up to QC_MAX_POSITIONS sorted positions n_1 < ... < n_k = n_max <= QC_MAX_TOP.
//    THE RULE.  For one row: take the stored non-zero values, pad them with zeros up to n_max elements; top(n) is the sum
//    of the n largest elements of that multiset.  (This is what the reference's CSR routine computes; on non-negative data
//    it is the share of counts in the top n genes times the row total.)  top(n) does not depend on how ties are broken --
//    with t the n-th largest value, c the number of elements above t and S their sum, top(n) = S + (n - c) t -- so the
//    result is exact for whatever order equal values end up in.
//    THE ALGORITHM.  T = 64 or 256 threads work on a row (256 / T rows per workgroup at a time).  The non-zero values of
//    the row are compacted into LDS as order-preserving 32-bit keys (sign and exponent order as the floats do, subnormals
//    included); a row whose non-zeros fit its QC_TOP_KEYS * T / 256 staged keys is sorted whole (bitonic network, padded to
//    the next power of two), and top(n) is a prefix sum of the sorted row in float64 -- no selection at all.  A longer row
//    first runs a SELECTION over its values in global memory: the key of the n_max-th largest value is built bit by bit
//    (32 counting passes), the values above it are gathered into LDS and the list is filled up to n_max with copies of that
//    value; then it is sorted and summed like a short row.  With m < n_max non-zeros the n_max - m zeros of the padding rank
//    between the positive and the negative values: top(n) = prefix(n) for n <= k+ (the positive values), prefix(k+) up to
//    k+ + (n_max - m), prefix(n - (n_max - m)) beyond.  All control flow is uniform over the workgroup.
//    Bytes: 4 B per stored entry read once (33 more reads of a row beyond the staging capacity, served by L2), 8 B per
//    (row, position) written.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"

namespace scamd {

namespace {

constexpr int QC_BLOCK = 256;
constexpr int QC_LDS_GENES = 4096;      // per-gene tables up to this many genes live in LDS (48 KB per workgroup)
constexpr int QC_GRID_CAP = 256 * 32;   // workgroups of a row-wise launch
constexpr int QC_LDS_GRID_CAP = 512;    // workgroups of the sweep with the LDS table (g flush atomics each)
constexpr int QC_MAX_MASKS = 32;
constexpr int QC_MAX_POSITIONS = 16;
constexpr int QC_MAX_TOP = 4096;
constexpr int QC_TOP_KEYS = 8192;       // staged keys per workgroup (32 KB): 8192 per row at T = 256, 2048 at T = 64

__device__ __forceinline__ bool qc_nonzero(unsigned bits) { return (bits & 0x7fffffffu) != 0u; }
// float bits -> unsigned key with the order of the values (negative: all bits flipped, else the sign bit set)
__device__ __forceinline__ unsigned qc_key(unsigned bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ double qc_value(unsigned key) {
  return (double)__uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}
constexpr unsigned QC_KEY_ZERO = 0x80000000u;  // key of +0.0: keys above it are the positive values

template <int G>
__device__ __forceinline__ double qc_group_sum(double v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// COLS: 0 no per-gene outputs, 1 table in LDS, 2 global atomics.  MK: masked totals kept per lane (0, 4 or 32).
// The row loop is uniform over the workgroup (rows past n are empty rows that write nothing): every lane takes part in
// every shuffle and reaches the barrier of the LDS flush together with the others.
template <int G, int MK, int COLS>
__global__ __launch_bounds__(QC_BLOCK) void qc_sweep_kernel(const int64_t* __restrict__ indptr,
                                                            const int32_t* __restrict__ indices,
                                                            const float* __restrict__ data, int64_t n, int g,
                                                            const uint32_t* __restrict__ gene_mask, int n_masks,
                                                            int32_t* __restrict__ row_nnz, double* __restrict__ row_total,
                                                            double* __restrict__ row_masked,
                                                            unsigned long long* __restrict__ col_nnz,
                                                            double* __restrict__ col_sum, unsigned int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) double qc_smem[];
  double* s_sum = qc_smem;
  unsigned int* s_cnt = reinterpret_cast<unsigned int*>(qc_smem + g);
  if (COLS == 1) {
    for (int c = threadIdx.x; c < g; c += QC_BLOCK) {
      s_sum[c] = 0.0;
      s_cnt[c] = 0u;
    }
    __syncthreads();
  }
  constexpr int RPB = QC_BLOCK / G;
  const int sub = threadIdx.x % G;
  unsigned int neg = 0u;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < n; base += (int64_t)gridDim.x * RPB) {
    const int64_t r = base + threadIdx.x / G;
    const bool valid = r < n;
    const int64_t b = valid ? indptr[r] : 0, e = valid ? indptr[r + 1] : 0;
    int cnt = 0;
    double tot = 0.0;
    double mk[MK > 0 ? MK : 1];
#pragma unroll
    for (int k = 0; k < (MK > 0 ? MK : 1); ++k) mk[k] = 0.0;
#pragma unroll 2
    for (int64_t p = b + sub; p < e; p += G) {
      const unsigned bits = __float_as_uint(data[p]);
      if (!qc_nonzero(bits)) continue;
      neg |= bits >> 31;
      const double dv = (double)__uint_as_float(bits);
      ++cnt;
      tot += dv;
      if (MK > 0 || COLS > 0) {
        const int c = indices[p];
        if (MK > 0) {
          const uint32_t m = gene_mask[c];
#pragma unroll
          for (int k = 0; k < MK; ++k) mk[k] += ((m >> k) & 1u) ? dv : 0.0;
        }
        if (COLS == 1) {
          atomicAdd(&s_sum[c], dv);
          atomicAdd(&s_cnt[c], 1u);
        } else if (COLS == 2) {
          atomicAdd(&col_sum[c], dv);
          atomicAdd(&col_nnz[c], 1ull);
        }
      }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    tot = qc_group_sum<G>(tot);
#pragma unroll
    for (int k = 0; k < MK; ++k) mk[k] = qc_group_sum<G>(mk[k]);
    if (valid && sub == 0) {
      row_nnz[r] = cnt;
      row_total[r] = tot;
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < n_masks) row_masked[(int64_t)k * n + r] = mk[k];
    }
  }
  if (COLS == 1) {
    __syncthreads();
    for (int c = threadIdx.x; c < g; c += QC_BLOCK) {
      if (s_cnt[c]) {
        atomicAdd(&col_sum[c], s_sum[c]);
        atomicAdd(&col_nnz[c], (unsigned long long)s_cnt[c]);
      }
    }
  }
  if (neg) atomicOr(flags, 1u);
}

struct QcPositions {
  int n;
  int p[QC_MAX_POSITIONS];
};

// T threads per row, R = QC_BLOCK / T rows per workgroup at a time, CAP staged keys per row.
template <int T>
__global__ __launch_bounds__(QC_BLOCK) void qc_top_kernel(const int64_t* __restrict__ indptr, const float* __restrict__ data,
                                                          int64_t n, QcPositions pos, double* __restrict__ out) {
  constexpr int R = QC_BLOCK / T, CAP = QC_TOP_KEYS / R, WPR = T / 64;
  __shared__ unsigned int s_keys[QC_TOP_KEYS];
  __shared__ double s_seg[QC_BLOCK / 64][QC_MAX_POSITIONS];
  __shared__ int s_cnt[QC_BLOCK / 64];
  __shared__ int s_acc[QC_BLOCK / 64];
  __shared__ int s_pad, s_long;
  const int slot = threadIdx.x / T, t = threadIdx.x % T;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  unsigned int* keys = s_keys + slot * CAP;
  const int nmax = pos.p[pos.n - 1];
  for (int64_t base = (int64_t)blockIdx.x * R; base < n; base += (int64_t)gridDim.x * R) {
    const int64_t r = base + slot;
    const bool valid = r < n;
    const int64_t b = valid ? indptr[r] : 0, e = valid ? indptr[r + 1] : 0;
    if (threadIdx.x < R) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
      s_pad = 0;
      s_long = 0;
    }
    __syncthreads();
    // ---- the non-zero values of the row as keys, in arrival order (the sort removes the order)
    for (int64_t p = b + t; p < e; p += T) {
      const unsigned bits = __float_as_uint(data[p]);
      if (qc_nonzero(bits)) {
        const int i = atomicAdd(&s_cnt[slot], 1);
        if (i < CAP) keys[i] = qc_key(bits);
      }
    }
    __syncthreads();
    int m = s_cnt[slot];
    const bool lng = m > CAP;
    if (lng && t == 0) s_long = 1;
    __syncthreads();
    if (s_long) {
      // ---- selection for the rows beyond the staging capacity (CAP >= nmax): prefix = the largest key x with
      // #{key >= x} >= nmax, i.e. the key of the nmax-th largest value; rows that fit only keep the barriers company
      unsigned prefix = 0u;
      for (int bit = 31; bit >= 0; --bit) {
        if (t == 0) s_acc[slot] = 0;
        __syncthreads();
        const unsigned cand = prefix | (1u << bit);
        int c = 0;
        if (lng)
          for (int64_t p = b + t; p < e; p += T) {
            const unsigned bits = __float_as_uint(data[p]);
            c += (qc_nonzero(bits) && qc_key(bits) >= cand) ? 1 : 0;
          }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0 && c) atomicAdd(&s_acc[slot], c);
        __syncthreads();
        if (s_acc[slot] >= nmax) prefix = cand;
        __syncthreads();
      }
      if (lng && t == 0) s_cnt[slot] = 0;
      __syncthreads();
      if (lng)
        for (int64_t p = b + t; p < e; p += T) {
          const unsigned bits = __float_as_uint(data[p]);
          if (qc_nonzero(bits) && qc_key(bits) > prefix) {  // fewer than nmax of them, by the choice of prefix
            const int i = atomicAdd(&s_cnt[slot], 1);
            if (i < CAP) keys[i] = qc_key(bits);
          }
        }
      __syncthreads();
      if (lng) {
        const int c = min(s_cnt[slot], nmax);
        for (int i = c + t; i < nmax; i += T) keys[i] = prefix;
        m = nmax;
      }
      __syncthreads();
    }
    // ---- bitonic sort, descending, of the row padded to a power of two with the lowest key
    int psz = 1;
    while (psz < m) psz <<= 1;
    if (m == 0) psz = 0;
    if (t == 0) atomicMax(&s_pad, psz);
    for (int i = m + t; i < psz; i += T) keys[i] = 0u;
    __syncthreads();
    const int pmax = s_pad;
    for (int k = 2; k <= pmax; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        if (k <= psz)
          for (int i = t; i < psz; i += T) {
            const int q = i ^ j;
            if (q > i) {
              const unsigned a = keys[i], c = keys[q];
              const bool desc = (i & k) == 0;
              if (desc ? a < c : a > c) {
                keys[i] = c;
                keys[q] = a;
              }
            }
          }
        __syncthreads();
      }
    }
    // ---- top(n) = prefix sums of the sorted row; the zeros of the padding rank between positive and negative values
    int lo = 0, hi = m;  // kpos = #{keys > QC_KEY_ZERO}: first index whose key is not above it
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] > QC_KEY_ZERO) lo = mid + 1;
      else hi = mid;
    }
    const int kpos = lo, zeros = max(nmax - m, 0);
    int q0 = 0;
    for (int j = 0; j < pos.n; ++j) {
      const int p = pos.p[j];
      const int q1 = p <= kpos ? p : (p <= kpos + zeros ? kpos : p - zeros);
      double s = 0.0;
      for (int i = q0 + t; i < q1; i += T) s += qc_value(keys[i]);
      s = qc_group_sum<64>(s);
      if (lane == 0) s_seg[wave][j] = s;
      q0 = q1;
    }
    __syncthreads();
    if (valid && t == 0) {
      double cum = 0.0;
      for (int j = 0; j < pos.n; ++j) {
        for (int w = 0; w < WPR; ++w) cum += s_seg[slot * WPR + w][j];
        out[r * pos.n + j] = cum;
      }
    }
  }
}

// lanes per row of the sweep from the mean row length (the rule of csrc/preprocess.hip)
inline int qc_lanes_per_row(int64_t n, int64_t nnz) {
  const int64_t avg = n > 0 ? nnz / n : 0;
  return avg <= 32 ? 8 : (avg <= 160 ? 16 : (avg <= 512 ? 32 : 64));
}

// threads per row of the top-n kernel: a wave per row while rows are short and n_max fits the wave's 2048 staged keys
inline int qc_top_threads(int64_t n, int64_t nnz, int nmax) {
  const int64_t avg = n > 0 ? nnz / n : 0;
  return (avg <= 256 && nmax <= QC_TOP_KEYS / 4) ? 64 : 256;
}

template <int G, int MK>
int qc_launch_sweep(int cols, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int g,
                    const uint32_t* gene_mask, int n_masks, int32_t* row_nnz, double* row_total, double* row_masked,
                    unsigned long long* col_nnz, double* col_sum, unsigned int* flags, hipStream_t stream) {
  constexpr int RPB = QC_BLOCK / G;
  const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n, RPB), 1), QC_GRID_CAP);
  if (cols == 1) {
    const size_t lds = (size_t)g * (8 + 4) + 16;
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n, RPB * 16), 1), QC_LDS_GRID_CAP);
    hipLaunchKernelGGL((qc_sweep_kernel<G, MK, 1>), dim3(blocks), dim3(QC_BLOCK), lds, stream, indptr, indices, data, n, g,
                       gene_mask, n_masks, row_nnz, row_total, row_masked, col_nnz, col_sum, flags);
  } else if (cols == 2) {
    hipLaunchKernelGGL((qc_sweep_kernel<G, MK, 2>), dim3(grid), dim3(QC_BLOCK), 0, stream, indptr, indices, data, n, g,
                       gene_mask, n_masks, row_nnz, row_total, row_masked, col_nnz, col_sum, flags);
  } else {
    hipLaunchKernelGGL((qc_sweep_kernel<G, MK, 0>), dim3(grid), dim3(QC_BLOCK), 0, stream, indptr, indices, data, n, g,
                       gene_mask, n_masks, row_nnz, row_total, row_masked, col_nnz, col_sum, flags);
  }
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

template <int G>
int qc_launch_sweep_masks(int mk, int cols, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int g,
                          const uint32_t* gene_mask, int n_masks, int32_t* row_nnz, double* row_total, double* row_masked,
                          unsigned long long* col_nnz, double* col_sum, unsigned int* flags, hipStream_t stream) {
  switch (mk) {
    case 0: return qc_launch_sweep<G, 0>(cols, indptr, indices, data, n, g, gene_mask, n_masks, row_nnz, row_total, row_masked, col_nnz, col_sum, flags, stream);
    case 4: return qc_launch_sweep<G, 4>(cols, indptr, indices, data, n, g, gene_mask, n_masks, row_nnz, row_total, row_masked, col_nnz, col_sum, flags, stream);
    default: return qc_launch_sweep<G, QC_MAX_MASKS>(cols, indptr, indices, data, n, g, gene_mask, n_masks, row_nnz, row_total, row_masked, col_nnz, col_sum, flags, stream);
  }
}

}  // namespace
}  // namespace scamd

using namespace scamd;

extern "C" int scamd_pp_qc_sweep_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                     int64_t nnz, const uint32_t* gene_mask, int n_masks, int32_t* row_nnz,
                                     double* row_total, double* row_masked, int64_t* col_nnz, double* col_sum,
                                     uint32_t* flags, scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && n >= 0 && g >= 0 && nnz >= 0 && g < ((int64_t)1 << 31) && n_masks >= 0 && flags &&
                    (nnz == 0 || data) && (n == 0 || (row_nnz && row_total)),
                SCAMD_EINVAL, "pp_qc_sweep: null pointer or negative size");
  SCAMD_REQUIRE(n_masks <= QC_MAX_MASKS, SCAMD_EUNSUPPORTED, "pp_qc_sweep: %d masks, at most %d", n_masks, QC_MAX_MASKS);
  SCAMD_REQUIRE((col_nnz == nullptr) == (col_sum == nullptr), SCAMD_EINVAL, "pp_qc_sweep: col_nnz and col_sum go together");
  const bool want_cols = col_nnz != nullptr && g > 0;
  SCAMD_REQUIRE(n_masks == 0 || ((g == 0 || gene_mask) && (n == 0 || row_masked)), SCAMD_EINVAL,
                "pp_qc_sweep: masks need gene_mask and row_masked");
  SCAMD_REQUIRE(nnz == 0 || indices || (n_masks == 0 && !want_cols), SCAMD_EINVAL,
                "pp_qc_sweep: masks and per-gene outputs need indices");
  SCAMD_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(uint32_t), stream));
  if (want_cols) {
    SCAMD_HIP_CHECK(hipMemsetAsync(col_nnz, 0, sizeof(int64_t) * (size_t)g, stream));
    SCAMD_HIP_CHECK(hipMemsetAsync(col_sum, 0, sizeof(double) * (size_t)g, stream));
  }
  if (n == 0) return SCAMD_OK;
  const int cols = !want_cols ? 0 : (g <= QC_LDS_GENES ? 1 : 2);
  const int mk = n_masks == 0 ? 0 : (n_masks <= 4 ? 4 : QC_MAX_MASKS);
  unsigned long long* cn = reinterpret_cast<unsigned long long*>(col_nnz);
  switch (qc_lanes_per_row(n, nnz)) {
    case 8: return qc_launch_sweep_masks<8>(mk, cols, indptr, indices, data, n, (int)g, gene_mask, n_masks, row_nnz, row_total, row_masked, cn, col_sum, flags, stream);
    case 16: return qc_launch_sweep_masks<16>(mk, cols, indptr, indices, data, n, (int)g, gene_mask, n_masks, row_nnz, row_total, row_masked, cn, col_sum, flags, stream);
    case 32: return qc_launch_sweep_masks<32>(mk, cols, indptr, indices, data, n, (int)g, gene_mask, n_masks, row_nnz, row_total, row_masked, cn, col_sum, flags, stream);
    default: return qc_launch_sweep_masks<64>(mk, cols, indptr, indices, data, n, (int)g, gene_mask, n_masks, row_nnz, row_total, row_masked, cn, col_sum, flags, stream);
  }
}

extern "C" int scamd_pp_qc_top_f32(const int64_t* indptr, const float* data, int64_t n, int64_t nnz,
                                   const int32_t* positions_host, int n_positions, double* top, scamd_stream_t stream) {
  SCAMD_REQUIRE(indptr && n >= 0 && nnz >= 0 && positions_host && n_positions >= 1 && (nnz == 0 || data) && (n == 0 || top),
                SCAMD_EINVAL, "pp_qc_top: null pointer, negative size or no position");
  SCAMD_REQUIRE(n_positions <= QC_MAX_POSITIONS, SCAMD_EUNSUPPORTED, "pp_qc_top: %d positions, at most %d", n_positions,
                QC_MAX_POSITIONS);
  QcPositions pos;
  pos.n = n_positions;
  for (int j = 0; j < QC_MAX_POSITIONS; ++j) pos.p[j] = 0;
  for (int j = 0; j < n_positions; ++j) {
    SCAMD_REQUIRE(positions_host[j] >= 1 && (j == 0 || positions_host[j] > positions_host[j - 1]), SCAMD_EINVAL,
                  "pp_qc_top: positions must be >= 1 and strictly increasing (position %d is %d)", j, positions_host[j]);
    pos.p[j] = positions_host[j];
  }
  SCAMD_REQUIRE(pos.p[n_positions - 1] <= QC_MAX_TOP, SCAMD_EUNSUPPORTED, "pp_qc_top: position %d, at most %d",
                pos.p[n_positions - 1], QC_MAX_TOP);
  if (n == 0) return SCAMD_OK;
  if (qc_top_threads(n, nnz, pos.p[n_positions - 1]) == 64) {
    const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n, QC_BLOCK / 64), 1), QC_GRID_CAP);
    hipLaunchKernelGGL((qc_top_kernel<64>), dim3(grid), dim3(QC_BLOCK), 0, stream, indptr, data, n, pos, top);
  } else {
    const unsigned grid = (unsigned)std::min<int64_t>(n, QC_GRID_CAP);
    hipLaunchKernelGGL((qc_top_kernel<256>), dim3(grid), dim3(QC_BLOCK), 0, stream, indptr, data, n, pos, top);
  }
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}
