// Collapsing cells into groups (`sc.get.aggregate`): per (group, gene) the sum, the number of non-zero and of negative values,
// the centred second moment and the exact median of a CSR float32 matrix, read as it sits on the device (reference:
// src/scanpy/get/_aggregated.py and get/_kernels.py).  Outputs are group-major [n_groups x g].
//
// THE ORDER.  The caller hands in `order`: the rows that take part, sorted by group (a counting sort of `codes`; any order
// inside a group).  Two scans give goff [n_groups + 1] (the slots of every group, from group_sizes) and pos [n_order + 1] (the
// stored entries in front of every slot): the matrix in group order is one stream of pos[n_order] entries in which every group
// is one contiguous run.  Nothing is copied for the moments; the rows are read in place through `order`.
//
// THE SPLIT.  The stream is cut into parts of scamd_aggregate_part_entries(nnz) ENTRIES, not rows or groups: one workgroup per
// part and per window of AG_WINDOW genes.  A group holding half the cells is shared by half the workgroups; 10^4 groups of 100
// cells are walked by the few workgroups whose parts they fall into.  Inside its part a workgroup takes one run (the entries of
// one group) at a time: a run of at least AG_LDS_MIN_RUN entries is accumulated in a table in LDS (16 B per gene of the window)
// that is flushed ONCE with integer adds into the global fixed-point table; a shorter run adds to the global table directly
// (clearing and flushing a window would cost more than its entries).  All loops are uniform over the workgroup.
//
// THE SCALE.  Every value is rounded ONCE to 64-bit fixed point and added with integer atomics (LDS or global): no float
// atomics, and no output depends on the order of rows, lanes, waves or workgroups -- two calls give the same bits, and so does a
// permutation of the rows.  With size_k < 2^es the size of the group and amax_j < 2^ea the largest finite |x| of gene j over the
// rows that take part (the range sweep; exponents read off the float bits), x is scaled by 2^(62 - es - ea): the sum stays below
// 2^62 and every term is off by at most half a unit, 2^(es + ea - 63).
//   |sum[k, j] - exact| <= stored_kj 2^(es + ea - 63) + |sum| 2^-53 <= (size_k 2^-61 + 2^-53) size_k amax_j
// (2^es <= 2 size_k, 2^ea <= 2 amax_j).  Integers of magnitude <= 2^24 are multiples of the unit: their sums are exact.
//
// THE SECOND MOMENT is centred: m2[k, j] = sum over all size_k cells of (x - mean)^2 with mean = sum / size_k the FINAL mean.
// Two more sweeps, run only when m2 is asked for: the largest |x - mean| of the stored non-zero values, D_kj < 2^ed (float32,
// rounded up), then (x - mean)^2 in float64, rounded once at the scale 2^(62 - es - 2 ed) and added in integers; the cells that
// store nothing (or a zero) are the closed form (size_k - count_nonzero) mean^2.  With D_kj <= 2 amax_j:
//   |m2[k, j] - exact| <= size_k^2 D_kj^2 2^-60 + 2^-50 m2 + size_k ((size_k 2^-61 + 2^-52) amax_j)^2
// (the first term: half a unit per stored entry, at most size_k^2 amax_j^2 2^-58; the second: the float64 roundings of x - mean,
// its square, the zero block and the last addition; the third: the squares are taken about the computed mean, which is off by
// the error of the sum over size_k and one rounding, and sum (x - m)^2 = sum (x - mean)^2 + size_k (m - mean)^2).  `sumsq - sum^2 / n` is never formed.  A column that is constant and fully stored within a group has
// mean == x exactly (its fixed-point sum is exact), every deviation is 0 and m2 == 0.0.
//
// THE MEDIAN is exact, implicit zeros included.  With n_neg negative and n_zero = size - count_nonzero zero values the element of
// rank r is the r-th negative value, 0, or stored value r - (size - stored) in ascending order.  A pair whose two middle ranks
// fall into the zero block is decided from the two counts alone (on count data: nearly every pair; where they decide every
// pair nothing else runs).  For the others the rows are gathered into group order and transposed (scamd_csr_transpose_f32:
// slot ids ascend within a column, so a (group, gene) pair is one contiguous segment), and the segment is searched by its length:
//   <= AG_MED_WAVE_MAX entries   one wave, one key per lane, ranks by 64 shuffles;
//   <= AG_MED_CHUNK              one workgroup, the keys staged in LDS, radix select (4 passes of 8 order-preserving key bits);
//   longer                       the same radix select reading the segment from global memory in every pass.
// No step is quadratic in the length beyond the 64 lanes of the first tier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"

namespace scamd {

namespace {

constexpr int AG_BLOCK = 256;
constexpr int AG_WINDOW = 4096;        // genes of one LDS table (16 B each: 64 KiB)
constexpr int AG_PART_MIN = 2048;      // stored entries of one part: nnz / AG_PART_TARGET, within these bounds
constexpr int AG_PART_MAX = 32768;
constexpr int AG_PART_TARGET = 8192;
constexpr int AG_LDS_MIN_RUN = 512;    // a run of fewer entries adds to the global table directly
constexpr int AG_SCAN_ITEMS = 8;       // consecutive items per thread of a scan tile
constexpr int AG_SCAN_TILE = AG_BLOCK * AG_SCAN_ITEMS;
constexpr int AG_MED_WAVE_MAX = 64;    // segment entries the in-wave tier takes
constexpr int AG_MED_CHUNK = 4096;     // segment entries whose keys are staged in LDS
constexpr int AG_GRID_CAP = 256 * 32;

constexpr unsigned AG_FLAG_NONFINITE = 1u;  // a stored value of a row that takes part was not finite
constexpr unsigned AG_FLAG_CODE = 2u;       // a code outside [-1, n_groups)
constexpr unsigned AG_FLAG_ORDER = 4u;      // order / group_sizes / codes / a column index contradict each other

__device__ __forceinline__ bool ag_finite(unsigned bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
// float bits -> unsigned key with the order of the values
__device__ __forceinline__ unsigned ag_key(unsigned bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float ag_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key); }
// the non-negative float f < 2^e for e = this (subnormals and 0: -126; infinity stands for "below 2^129")
__device__ __forceinline__ int ag_exp_above(unsigned bits) { return (int)((bits >> 23) & 0xffu) - 126; }
// size < 2^e (size >= 1)
__device__ __forceinline__ int ag_size_exp(int64_t size) { return 64 - __clzll((long long)size); }

// number of elements of the ascending a[0, len) that are <= v / < v
__device__ __forceinline__ int64_t ag_upper(const int64_t* __restrict__ a, int64_t len, int64_t v) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t ag_lower(const int64_t* __restrict__ a, int64_t len, int64_t v) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// first p in [lo, hi) with a[p] >= v (a ascending there)
__device__ __forceinline__ int64_t ag_lower32(const int32_t* __restrict__ a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- the two scans.  Items: ROWS ? the stored entries of the row in slot i (0 beyond n_order and for a row id outside [0, n))
// : group_sizes[i] (negative: 0).  out[i] = the sum of the items in front of i, i = 0 .. count.  Three launches: the sums of the
// tiles, their scan by one workgroup, the tiles again.
template <bool ROWS>
__device__ __forceinline__ int64_t ag_item(const int64_t* __restrict__ sizes, const int32_t* __restrict__ order, int64_t n_order,
                                           const int64_t* __restrict__ indptr, int64_t n, int64_t i) {
  if (ROWS) {
    if (i >= n_order) return 0;
    const int64_t r = order[i];
    if (r < 0 || r >= n) return 0;
    const int64_t len = indptr[r + 1] - indptr[r];
    return len > 0 ? len : 0;
  }
  const int64_t s = sizes[i];
  return s > 0 ? s : 0;
}

// exclusive prefix of v over the threads of the workgroup, *total = the sum; every thread calls it
__device__ __forceinline__ int64_t ag_block_scan(int64_t v, int64_t* s_buf, int64_t* total) {
  const int t = threadIdx.x;
  s_buf[t] = v;
  __syncthreads();
  for (int d = 1; d < AG_BLOCK; d <<= 1) {
    const int64_t add = t >= d ? s_buf[t - d] : 0;
    __syncthreads();
    s_buf[t] += add;
    __syncthreads();
  }
  const int64_t incl = s_buf[t];
  *total = s_buf[AG_BLOCK - 1];
  __syncthreads();
  return incl - v;
}

template <bool ROWS>
__global__ __launch_bounds__(AG_BLOCK) void ag_tile_sums_kernel(const int64_t* __restrict__ sizes, const int32_t* __restrict__ order,
                                                                int64_t n_order, const int64_t* __restrict__ indptr, int64_t n,
                                                                int64_t count, int64_t* __restrict__ tiles) {
  __shared__ int64_t s_buf[AG_BLOCK];
  const int64_t first = (int64_t)blockIdx.x * AG_SCAN_TILE + (int64_t)threadIdx.x * AG_SCAN_ITEMS;
  int64_t sum = 0;
  for (int q = 0; q < AG_SCAN_ITEMS; ++q)
    if (first + q < count) sum += ag_item<ROWS>(sizes, order, n_order, indptr, n, first + q);
  int64_t total;
  ag_block_scan(sum, s_buf, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// tiles[t] becomes the sum of the tiles in front of t; out[count] = the sum of all
__global__ __launch_bounds__(AG_BLOCK) void ag_tile_offsets_kernel(int64_t n_tiles, int64_t count, int64_t* __restrict__ tiles,
                                                                   int64_t* __restrict__ out) {
  __shared__ int64_t s_buf[AG_BLOCK];
  int64_t carry = 0;
  for (int64_t base = 0; base < n_tiles; base += AG_BLOCK) {
    const int64_t t = base + threadIdx.x;
    const int64_t v = t < n_tiles ? tiles[t] : 0;
    int64_t total;
    const int64_t ex = ag_block_scan(v, s_buf, &total);
    if (t < n_tiles) tiles[t] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) out[count] = carry;
}

template <bool ROWS>
__global__ __launch_bounds__(AG_BLOCK) void ag_tile_scan_kernel(const int64_t* __restrict__ sizes, const int32_t* __restrict__ order,
                                                                int64_t n_order, const int64_t* __restrict__ indptr, int64_t n,
                                                                int64_t count, const int64_t* __restrict__ tiles,
                                                                int64_t* __restrict__ out) {
  __shared__ int64_t s_buf[AG_BLOCK];
  const int64_t first = (int64_t)blockIdx.x * AG_SCAN_TILE + (int64_t)threadIdx.x * AG_SCAN_ITEMS;
  int64_t v[AG_SCAN_ITEMS];
  int64_t sum = 0;
#pragma unroll
  for (int q = 0; q < AG_SCAN_ITEMS; ++q) {
    v[q] = first + q < count ? ag_item<ROWS>(sizes, order, n_order, indptr, n, first + q) : 0;
    sum += v[q];
  }
  int64_t total;
  int64_t run = tiles[blockIdx.x] + ag_block_scan(sum, s_buf, &total);
#pragma unroll
  for (int q = 0; q < AG_SCAN_ITEMS; ++q) {
    if (first + q < count) out[first + q] = run;
    run += v[q];
  }
}

// ---- the range sweep: per gene the largest finite |x| over the rows that take part, as float bits (integer atomicMax).
// 2^lanes_log2 lanes share a row.
__global__ __launch_bounds__(AG_BLOCK) void ag_range_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const float* __restrict__ data, int64_t n, int g, int64_t nnz,
                                                            const int32_t* __restrict__ codes, int64_t n_groups, int lanes_log2,
                                                            unsigned int* amax, unsigned int* flags) {
  const int lanes = 1 << lanes_log2, rpb = AG_BLOCK >> lanes_log2;
  const int sub = threadIdx.x & (lanes - 1);
  unsigned int bad = 0u;
  for (int64_t base = (int64_t)blockIdx.x * rpb; base < n; base += (int64_t)gridDim.x * rpb) {
    const int64_t r = base + (threadIdx.x >> lanes_log2);
    if (r >= n) continue;
    const int code = codes[r];
    if (code < 0 || code >= n_groups) {
      if (code != -1) bad |= AG_FLAG_CODE;
      continue;
    }
    const int64_t b = indptr[r], e = min(indptr[r + 1], nnz);
    for (int64_t p = b + sub; p < e; p += lanes) {
      const unsigned bits = __float_as_uint(data[p]);
      if (!ag_finite(bits)) {
        bad |= AG_FLAG_NONFINITE;
        continue;
      }
      const int c = indices[p];
      if ((unsigned)c >= (unsigned)g) {
        bad |= AG_FLAG_ORDER;
        continue;
      }
      const unsigned a = bits & 0x7fffffffu;
      // the table only grows: a stale value read here costs a needless atomic, never a missed one
      if (a > amax[c]) atomicMax(&amax[c], a);
    }
  }
  if (bad) atomicOr(flags, bad);
}

// ---- the sweep over the matrix in group order.  MODE 0: fix += round(x 2^(62 - es - ea)), aux += 1 | negative << 32;
// MODE 1: dmax = max |x - mean| as float bits, rounded up; MODE 2: fix += round((x - mean)^2 2^(62 - es - 2 ed)).
// blockIdx.x = part * n_windows + window.  A stored +-0.0 takes part in nothing (it is one of the zeros).
template <int MODE>
__global__ __launch_bounds__(AG_BLOCK) void ag_sweep_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const float* __restrict__ data, int64_t n, int g, int64_t nnz,
                                                            const int32_t* __restrict__ codes, const int32_t* __restrict__ order,
                                                            int64_t n_order, const int64_t* __restrict__ pos,
                                                            const int64_t* __restrict__ goff, const int64_t* __restrict__ group_sizes,
                                                            int64_t n_groups, int part_entries, int n_windows, int lanes_log2,
                                                            const unsigned int* __restrict__ amax, const double* __restrict__ sum,
                                                            long long* fix, unsigned long long* aux, unsigned int* dmax,
                                                            unsigned int* flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long ag_smem[];
  const int64_t part = blockIdx.x / (unsigned)n_windows;
  const int c0 = (int)(blockIdx.x % (unsigned)n_windows) * AG_WINDOW;
  const int wn = min(AG_WINDOW, g - c0);
  long long* s_fix = reinterpret_cast<long long*>(ag_smem);         // MODE 0, 2: [wn]
  unsigned long long* s_aux = ag_smem + wn;                         // MODE 0: [wn]
  unsigned int* s_dmax = reinterpret_cast<unsigned int*>(ag_smem);  // MODE 1: [wn]
  const int64_t total = pos[n_order];
  const int64_t p0 = part * part_entries;
  if (p0 >= total) return;
  const int64_t p1 = min(p0 + part_entries, total);
  const int lanes = 1 << lanes_log2, rpb = AG_BLOCK >> lanes_log2;
  const int sub = threadIdx.x & (lanes - 1), slot_in_step = threadIdx.x >> lanes_log2;
  // the slots whose rows reach into [p0, p1): the last slot starting at or before p0 (an empty row never holds p0) .. the
  // first slot starting at or after p1
  int64_t i = ag_upper(pos, n_order + 1, p0) - 1;
  const int64_t i_end = ag_lower(pos, n_order + 1, p1);
  int64_t k = ag_upper(goff, n_groups + 1, i) - 1;
  unsigned int bad = 0u;
  while (i < i_end) {
    while (k < n_groups && goff[k + 1] <= i) ++k;  // (groups without rows)
    if (k >= n_groups) {  // more slots than the sizes add up to
      bad |= AG_FLAG_ORDER;
      break;
    }
    const int64_t ie = min(i_end, goff[k + 1]);
    const int64_t run = min(pos[ie], p1) - max(pos[i], p0);
    const bool lds = run >= AG_LDS_MIN_RUN;
    const int64_t size = group_sizes[k];
    const int es = ag_size_exp(size);
    const double size_d = (double)size;
    if (lds) {
      for (int c = threadIdx.x; c < wn; c += AG_BLOCK) {
        if (MODE == 1) s_dmax[c] = 0u;
        else s_fix[c] = 0;
        if (MODE == 0) s_aux[c] = 0ull;
      }
      __syncthreads();
    }
    const int64_t cell0 = k * (int64_t)g;
    for (int64_t base = i; base < ie; base += rpb) {
      const int64_t slot = base + slot_in_step;
      if (slot >= ie) continue;
      const int64_t r = order[slot];
      if (r < 0 || r >= n || (int64_t)codes[r] != k) {
        bad |= AG_FLAG_ORDER;
        continue;
      }
      const int64_t pb = pos[slot], src = indptr[r];
      const int64_t lo = max(pb, p0), hi = min(pos[slot + 1], p1);
      for (int64_t p = lo + sub; p < hi; p += lanes) {
        const int64_t q = src + (p - pb);
        if (q >= nnz) break;
        const unsigned bits = __float_as_uint(data[q]);
        if (!ag_finite(bits)) {
          bad |= AG_FLAG_NONFINITE;
          continue;
        }
        const int c = indices[q];
        const int cw = c - c0;
        if ((unsigned)cw >= (unsigned)wn) {
          if ((unsigned)c >= (unsigned)g) bad |= AG_FLAG_ORDER;
          continue;
        }
        const float xf = __uint_as_float(bits);
        if (xf == 0.f) continue;
        const double x = (double)xf;
        if (MODE == 0) {
          const long long v = llrint(ldexp(x, 62 - es - ag_exp_above(amax[c])));
          const unsigned long long one = 1ull | ((bits >> 31) ? (1ull << 32) : 0ull);
          if (lds) {
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(&s_fix[cw]), (unsigned long long)v);
            atomicAdd(&s_aux[cw], one);
          } else {
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(&fix[cell0 + c]), (unsigned long long)v);
            atomicAdd(&aux[cell0 + c], one);
          }
        } else {
          const double d = x - sum[cell0 + c] / size_d;
          if (MODE == 1) {
            const double ad = fabs(d);
            float f = (float)ad;
            if ((double)f < ad) f = __uint_as_float(__float_as_uint(f) + 1u);  // rounded up (at most to infinity)
            const unsigned fb = __float_as_uint(f);
            if (lds) {
              if (fb > s_dmax[cw]) atomicMax(&s_dmax[cw], fb);
            } else {
              if (fb > dmax[cell0 + c]) atomicMax(&dmax[cell0 + c], fb);
            }
          } else {
            const unsigned db = dmax[cell0 + c];
            const long long v = db ? llrint(ldexp(d * d, 62 - es - 2 * ag_exp_above(db))) : 0;
            if (v) {
              if (lds) atomicAdd(reinterpret_cast<unsigned long long*>(&s_fix[cw]), (unsigned long long)v);
              else atomicAdd(reinterpret_cast<unsigned long long*>(&fix[cell0 + c]), (unsigned long long)v);
            }
          }
        }
      }
    }
    if (lds) {
      __syncthreads();
      for (int c = threadIdx.x; c < wn; c += AG_BLOCK) {
        if (MODE == 1) {
          if (s_dmax[c]) atomicMax(&dmax[cell0 + c0 + c], s_dmax[c]);
        } else {
          if (s_fix[c]) atomicAdd(reinterpret_cast<unsigned long long*>(&fix[cell0 + c0 + c]), (unsigned long long)s_fix[c]);
          if (MODE == 0 && s_aux[c]) atomicAdd(&aux[cell0 + c0 + c], s_aux[c]);
        }
      }
      __syncthreads();
    }
    i = ie;
  }
  if (bad) atomicOr(flags, bad);
}

// the fixed-point tables of MODE 0 as float64 sums and int64 counts
__global__ __launch_bounds__(AG_BLOCK) void ag_convert_sums_kernel(int g, int64_t cells, const int64_t* __restrict__ group_sizes,
                                                                   const unsigned int* __restrict__ amax,
                                                                   const long long* __restrict__ fix,
                                                                   const unsigned long long* __restrict__ aux,
                                                                   double* __restrict__ sum, int64_t* __restrict__ count_nonzero,
                                                                   int64_t* __restrict__ count_negative) {
  for (int64_t i = (int64_t)blockIdx.x * AG_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * AG_BLOCK) {
    const int64_t size = group_sizes[i / g];
    const long long f = fix[i];
    sum[i] = f ? ldexp((double)f, ag_size_exp(size > 0 ? size : 1) + ag_exp_above(amax[i % g]) - 62) : 0.0;
    const unsigned long long a = aux[i];
    count_nonzero[i] = (int64_t)(a & 0xffffffffull);
    count_negative[i] = (int64_t)(a >> 32);
  }
}

// m2 = the fixed-point sum of the stored deviations squared + the zero block in closed form
__global__ __launch_bounds__(AG_BLOCK) void ag_convert_m2_kernel(int g, int64_t cells, const int64_t* __restrict__ group_sizes,
                                                                 const unsigned int* __restrict__ dmax,
                                                                 const long long* __restrict__ fix, const double* __restrict__ sum,
                                                                 const int64_t* __restrict__ count_nonzero, double* __restrict__ m2) {
  for (int64_t i = (int64_t)blockIdx.x * AG_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * AG_BLOCK) {
    const int64_t size = group_sizes[i / g];
    if (size <= 0) {
      m2[i] = 0.0;
      continue;
    }
    const long long f = fix[i];
    const double stored = f ? ldexp((double)f, ag_size_exp(size) + 2 * ag_exp_above(dmax[i]) - 62) : 0.0;
    const double mean = sum[i] / (double)size;
    m2[i] = stored + (double)(size - count_nonzero[i]) * (mean * mean);
  }
}

// ---- the median
// the rows in group order as a CSR of their own: row `slot` = row order[slot], at pos[slot]
__global__ __launch_bounds__(AG_BLOCK) void ag_gather_rows_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                                  const float* __restrict__ data, int64_t n, int64_t nnz,
                                                                  const int32_t* __restrict__ order, int64_t n_order,
                                                                  const int64_t* __restrict__ pos, int lanes_log2,
                                                                  int32_t* __restrict__ p_indices, float* __restrict__ p_data) {
  const int lanes = 1 << lanes_log2, rpb = AG_BLOCK >> lanes_log2;
  const int sub = threadIdx.x & (lanes - 1);
  for (int64_t base = (int64_t)blockIdx.x * rpb; base < n_order; base += (int64_t)gridDim.x * rpb) {
    const int64_t slot = base + (threadIdx.x >> lanes_log2);
    if (slot >= n_order) continue;
    const int64_t r = order[slot];
    if (r < 0 || r >= n) continue;  // (its length in pos is 0)
    const int64_t pb = pos[slot], len = pos[slot + 1] - pb, src = indptr[r];
    for (int64_t t = sub; t < len && src + t < nnz; t += lanes) {
      p_indices[pb + t] = indices[src + t];
      p_data[pb + t] = data[src + t];
    }
  }
}

struct AgPair {
  int64_t first, len;         // the segment in the transposed arrays
  int64_t size, neg, zeros;   // cells of the group; negative values; zeros, stored ones included
};

__device__ __forceinline__ AgPair ag_pair(int64_t i, int64_t g, const int64_t* __restrict__ goff, const int64_t* __restrict__ t_indptr,
                                          const int32_t* __restrict__ t_indices, const int64_t* __restrict__ group_sizes,
                                          const int64_t* __restrict__ count_nonzero, const int64_t* __restrict__ count_negative,
                                          bool with_segment) {
  AgPair pr;
  const int64_t k = i / g, j = i % g;
  pr.size = group_sizes[k];
  pr.neg = count_negative[i];
  pr.zeros = pr.size - count_nonzero[i];
  pr.first = 0;
  pr.len = 0;
  if (with_segment) {
    const int64_t b = t_indptr[j], e = t_indptr[j + 1];
    pr.first = ag_lower32(t_indices, b, e, goff[k]);
    pr.len = ag_lower32(t_indices, pr.first, e, goff[k + 1]) - pr.first;
  }
  return pr;
}
__device__ __forceinline__ bool ag_in_zero_block(const AgPair& pr, int64_t r) { return r >= pr.neg && r - pr.neg < pr.zeros; }
// rank r of the group's values -> rank among the stored entries of the segment (the stored zeros sort between the signs)
__device__ __forceinline__ int64_t ag_stored_rank(const AgPair& pr, int64_t r) {
  const int64_t rs = r < pr.neg ? r : r - (pr.size - pr.len);
  return rs < 0 ? 0 : (rs >= pr.len ? pr.len - 1 : rs);
}
__device__ __forceinline__ double ag_middle(float lo, float hi, bool odd, int mid_in_f32) {
  double m;
  if (odd) m = (double)lo;
  else if (mid_in_f32) m = (double)((lo + hi) / 2.0f);
  else m = ((double)lo + (double)hi) / 2.0;
  return m == 0.0 ? 0.0 : m;  // (never -0.0)
}

// every pair that the two counts decide: its median, and the number of pairs they do not decide.  On count data nothing is
// left, and neither the gather nor the transpose runs.
__global__ __launch_bounds__(AG_BLOCK) void ag_median_decide_kernel(int64_t g, int64_t cells, const int64_t* __restrict__ group_sizes,
                                                                    const int64_t* __restrict__ count_nonzero,
                                                                    const int64_t* __restrict__ count_negative,
                                                                    double* __restrict__ median, unsigned long long* counters) {
  unsigned long long open = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * AG_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * AG_BLOCK) {
    const AgPair pr = ag_pair(i, g, nullptr, nullptr, nullptr, group_sizes, count_nonzero, count_negative, false);
    if (pr.size <= 0) median[i] = __longlong_as_double(0x7ff8000000000000ll);
    else if (ag_in_zero_block(pr, (pr.size - 1) / 2) && ag_in_zero_block(pr, pr.size / 2)) median[i] = 0.0;
    else ++open;
  }
  if (open) atomicAdd(&counters[0], open);
}

// every pair: decided from the counts, or put on the work list -- short segments from the front, the others from the back
__global__ __launch_bounds__(AG_BLOCK) void ag_median_classify_kernel(int64_t g, int64_t cells, const int64_t* __restrict__ goff,
                                                                      const int64_t* __restrict__ t_indptr,
                                                                      const int32_t* __restrict__ t_indices,
                                                                      const int64_t* __restrict__ group_sizes,
                                                                      const int64_t* __restrict__ count_nonzero,
                                                                      const int64_t* __restrict__ count_negative,
                                                                      double* __restrict__ median, int64_t* __restrict__ list,
                                                                      unsigned long long* counters) {
  for (int64_t i = (int64_t)blockIdx.x * AG_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * AG_BLOCK) {
    AgPair pr = ag_pair(i, g, goff, t_indptr, t_indices, group_sizes, count_nonzero, count_negative, false);
    if (pr.size <= 0) {
      median[i] = __longlong_as_double(0x7ff8000000000000ll);
      continue;
    }
    if (ag_in_zero_block(pr, (pr.size - 1) / 2) && ag_in_zero_block(pr, pr.size / 2)) {
      median[i] = 0.0;
      continue;
    }
    pr = ag_pair(i, g, goff, t_indptr, t_indices, group_sizes, count_nonzero, count_negative, true);
    if (pr.len <= 0) {  // the counts promise values the matrix does not hold
      median[i] = __longlong_as_double(0x7ff8000000000000ll);
    } else if (pr.len <= AG_MED_WAVE_MAX) {
      list[atomicAdd(&counters[0], 1ull)] = i;
    } else {
      list[cells - 1 - (int64_t)atomicAdd(&counters[1], 1ull)] = i;
    }
  }
}

// one wave per pair, one key per lane; every lane counts the keys in front of its own
__global__ __launch_bounds__(AG_BLOCK) void ag_median_wave_kernel(int64_t g, int64_t n_items, const int64_t* __restrict__ list,
                                                                  const int64_t* __restrict__ goff, const int64_t* __restrict__ t_indptr,
                                                                  const int32_t* __restrict__ t_indices, const float* __restrict__ t_data,
                                                                  const int64_t* __restrict__ group_sizes,
                                                                  const int64_t* __restrict__ count_nonzero,
                                                                  const int64_t* __restrict__ count_negative, int mid_in_f32,
                                                                  double* __restrict__ median) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * (AG_BLOCK / 64) + (threadIdx.x >> 6);
  if (item >= n_items) return;  // (the whole wave)
  const int64_t i = list[item];
  const AgPair pr = ag_pair(i, g, goff, t_indptr, t_indices, group_sizes, count_nonzero, count_negative, true);
  const int len = (int)min(pr.len, (int64_t)AG_MED_WAVE_MAX);
  const unsigned key = lane < len ? ag_key(__float_as_uint(t_data[pr.first + lane])) : 0xffffffffu;
  int rank = 0;
  for (int m = 0; m < 64; ++m) {
    const unsigned other = __shfl(key, m);
    rank += (m < len && (other < key || (other == key && m < lane))) ? 1 : 0;
  }
  const int64_t r_lo = (pr.size - 1) / 2, r_hi = pr.size / 2;
  const bool z_lo = ag_in_zero_block(pr, r_lo), z_hi = ag_in_zero_block(pr, r_hi);
  unsigned v_lo = (lane < len && !z_lo && rank == (int)ag_stored_rank(pr, r_lo)) ? key : 0u;
  unsigned v_hi = (lane < len && !z_hi && rank == (int)ag_stored_rank(pr, r_hi)) ? key : 0u;
  for (int d = 32; d > 0; d >>= 1) {
    v_lo |= __shfl_xor(v_lo, d);
    v_hi |= __shfl_xor(v_hi, d);
  }
  if (lane == 0) median[i] = ag_middle(z_lo ? 0.f : ag_value(v_lo), z_hi ? 0.f : ag_value(v_hi), r_lo == r_hi, mid_in_f32);
}

// one workgroup per pair: radix select, 8 key bits per pass from the top; the keys of a segment of at most AG_MED_CHUNK entries
// are staged in LDS, a longer one is read from global memory in every pass
__global__ __launch_bounds__(AG_BLOCK) void ag_median_block_kernel(int64_t g, int64_t cells, const int64_t* __restrict__ list,
                                                                   const int64_t* __restrict__ goff, const int64_t* __restrict__ t_indptr,
                                                                   const int32_t* __restrict__ t_indices, const float* __restrict__ t_data,
                                                                   const int64_t* __restrict__ group_sizes,
                                                                   const int64_t* __restrict__ count_nonzero,
                                                                   const int64_t* __restrict__ count_negative, int mid_in_f32,
                                                                   double* __restrict__ median) {
  __shared__ unsigned int s_hist[256];
  __shared__ unsigned int s_keys[AG_MED_CHUNK];
  __shared__ unsigned int s_pick[2];  // the chosen bin, the rank inside it
  const int64_t i = list[cells - 1 - (int64_t)blockIdx.x];
  const AgPair pr = ag_pair(i, g, goff, t_indptr, t_indices, group_sizes, count_nonzero, count_negative, true);
  const bool staged = pr.len <= AG_MED_CHUNK;
  const float* seg = t_data + pr.first;
  if (staged)
    for (int64_t e = threadIdx.x; e < pr.len; e += AG_BLOCK) s_keys[e] = ag_key(__float_as_uint(seg[e]));
  const int64_t r_lo = (pr.size - 1) / 2, r_hi = pr.size / 2;
  const bool z[2] = {ag_in_zero_block(pr, r_lo), ag_in_zero_block(pr, r_hi)};
  const int64_t rs[2] = {ag_stored_rank(pr, r_lo), ag_stored_rank(pr, r_hi)};
  float val[2] = {0.f, 0.f};
  for (int which = 0; which < 2; ++which) {
    if (z[which]) continue;
    if (which == 1 && !z[0] && rs[1] == rs[0]) {
      val[1] = val[0];
      continue;
    }
    unsigned prefix = 0u, mask = 0u;
    unsigned rem = (unsigned)rs[which];  // (a segment holds fewer than 2^31 entries)
    for (int shift = 24; shift >= 0; shift -= 8) {
      s_hist[threadIdx.x] = 0u;
      __syncthreads();  // (the first pass: also the staged keys)
      for (int64_t e = threadIdx.x; e < pr.len; e += AG_BLOCK) {
        const unsigned key = staged ? s_keys[e] : ag_key(__float_as_uint(seg[e]));
        if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 0xffu], 1u);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        unsigned bin = 0u, left = rem;
        while (bin < 255u && left >= s_hist[bin]) left -= s_hist[bin++];
        s_pick[0] = bin;
        s_pick[1] = left;
      }
      __syncthreads();
      prefix |= s_pick[0] << shift;
      mask |= 0xffu << shift;
      rem = s_pick[1];
      __syncthreads();  // (s_pick and s_hist are rewritten by the next pass)
    }
    val[which] = ag_value(prefix);
  }
  if (threadIdx.x == 0) median[i] = ag_middle(val[0], val[1], r_lo == r_hi, mid_in_f32);
}

// ---- host side
inline int ag_part_entries(int64_t nnz) {
  const int64_t per = (nnz + AG_PART_TARGET - 1) / AG_PART_TARGET;
  return (int)std::min<int64_t>(std::max<int64_t>(per, AG_PART_MIN), AG_PART_MAX);
}

// lanes per row from the mean row length (the rule of csrc/preprocess.hip and csrc/regress.hip)
inline int ag_lanes_per_row(int64_t n, int64_t nnz) {
  const int64_t avg = n > 0 ? nnz / n : 0;
  return avg <= 32 ? 8 : (avg <= 160 ? 16 : (avg <= 512 ? 32 : 64));
}
inline int ag_log2(int lanes) { return lanes == 8 ? 3 : (lanes == 16 ? 4 : (lanes == 32 ? 5 : 6)); }

inline unsigned ag_row_grid(int64_t n, int lanes) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n, AG_BLOCK / lanes), 1), AG_GRID_CAP);
}
inline unsigned ag_cell_grid(int64_t cells) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(cells, AG_BLOCK), 1), AG_GRID_CAP);
}

struct AgWorkspace {
  int64_t *goff, *pos, *tiles;
  // the moments
  long long* fix;
  unsigned long long* aux;  // MODE 0: the packed counts; afterwards, as 32-bit words, the largest deviations
  unsigned int* amax;
  // the median
  int32_t* p_indices;
  float* p_data;
  int64_t* t_indptr;
  int32_t* t_indices;
  float* t_data;
  int64_t* list;
  unsigned long long* counters;
  char* transpose_ws;
  size_t transpose_bytes;
  size_t bytes;
  bool ok;
};

AgWorkspace ag_carve(void* base, size_t cap, int64_t n, int64_t g, int64_t nnz, int64_t n_groups, bool median) {
  Workspace ws(base, cap);
  AgWorkspace r = {};
  const size_t cells = (size_t)n_groups * (size_t)g;
  r.goff = ws.take<int64_t>((size_t)n_groups + 1);
  r.pos = ws.take<int64_t>((size_t)n + 1);
  r.tiles = ws.take<int64_t>((size_t)(n / AG_SCAN_TILE) + 2);
  if (!median) {
    r.fix = ws.take<long long>(cells);
    r.aux = ws.take<unsigned long long>(cells);
    r.amax = ws.take<unsigned int>((size_t)g);
  } else {
    r.p_indices = ws.take<int32_t>((size_t)nnz);
    r.p_data = ws.take<float>((size_t)nnz);
    r.t_indptr = ws.take<int64_t>((size_t)g + 1);
    r.t_indices = ws.take<int32_t>((size_t)nnz);
    r.t_data = ws.take<float>((size_t)nnz);
    r.list = ws.take<int64_t>(cells);
    r.counters = ws.take<unsigned long long>(2);
    r.transpose_bytes = scamd_csr_transpose_workspace_bytes(n, g, nnz);
    r.transpose_ws = ws.take<char>(r.transpose_bytes);
  }
  r.bytes = ws.used();
  r.ok = ws.ok;
  return r;
}

template <bool ROWS>
int ag_scan(const int64_t* sizes, const int32_t* order, int64_t n_order, const int64_t* indptr, int64_t n, int64_t count,
            int64_t* tiles, int64_t* out, hipStream_t stream) {
  const int64_t n_tiles = (count + AG_SCAN_TILE - 1) / AG_SCAN_TILE;
  if (n_tiles > 0) {
    hipLaunchKernelGGL((ag_tile_sums_kernel<ROWS>), dim3((unsigned)n_tiles), dim3(AG_BLOCK), 0, stream, sizes, order, n_order, indptr,
                       n, count, tiles);
    SCAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ag_tile_offsets_kernel, dim3(1), dim3(AG_BLOCK), 0, stream, n_tiles, count, tiles, out);
  SCAMD_LAUNCH_CHECK();
  if (n_tiles > 0) {
    hipLaunchKernelGGL((ag_tile_scan_kernel<ROWS>), dim3((unsigned)n_tiles), dim3(AG_BLOCK), 0, stream, sizes, order, n_order, indptr,
                       n, count, tiles, out);
    SCAMD_LAUNCH_CHECK();
  }
  return SCAMD_OK;
}

template <int MODE>
int ag_launch_sweep(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int g, int64_t nnz,
                    const int32_t* codes, const int32_t* order, int64_t n_order, const AgWorkspace& ws, const int64_t* group_sizes,
                    int64_t n_groups, const double* sum, uint32_t* flags, hipStream_t stream) {
  const int part = ag_part_entries(nnz);
  const int n_windows = ceil_div(g, AG_WINDOW);
  const int64_t blocks = (nnz + part - 1) / part * n_windows;
  SCAMD_REQUIRE(blocks < ((int64_t)1 << 31), SCAMD_EUNSUPPORTED, "aggregate_moments: %lld workgroups", (long long)blocks);
  const size_t lds = (size_t)std::min<int64_t>(g, AG_WINDOW) * (MODE == 0 ? 16 : (MODE == 1 ? 4 : 8));
  SCAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ag_sweep_kernel<MODE>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((ag_sweep_kernel<MODE>), dim3((unsigned)blocks), dim3(AG_BLOCK), lds, stream, indptr, indices, data, n, g, nnz,
                     codes, order, n_order, ws.pos, ws.goff, group_sizes, n_groups, part, n_windows,
                     ag_log2(ag_lanes_per_row(n, nnz)), ws.amax, sum, ws.fix, ws.aux, reinterpret_cast<unsigned int*>(ws.aux), flags);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

// the checks both entry points share; `what` names the entry point
int ag_check_input(const char* what, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g, int64_t nnz,
                   const int32_t* order, int64_t n_order, const int64_t* group_sizes, int64_t n_groups) {
  SCAMD_REQUIRE(n >= 0 && g >= 0 && nnz >= 0 && n_groups >= 0 && n_order >= 0, SCAMD_EINVAL, "%s: negative size", what);
  SCAMD_REQUIRE(n < ((int64_t)1 << 31) && g < ((int64_t)1 << 31), SCAMD_EUNSUPPORTED, "%s: n or g exceeds int32 ids", what);
  SCAMD_REQUIRE(n_groups <= n && n_order <= n, SCAMD_EINVAL, "%s: %lld groups / %lld ordered rows of %lld rows", what,
                (long long)n_groups, (long long)n_order, (long long)n);
  SCAMD_REQUIRE(indptr && (nnz == 0 || (indices && data)) && (n_order == 0 || order) && (n_groups == 0 || group_sizes), SCAMD_EINVAL,
                "%s: null pointer", what);
  return SCAMD_OK;
}

}  // namespace
}  // namespace scamd

using namespace scamd;

extern "C" size_t scamd_aggregate_workspace_bytes(int64_t n, int64_t g, int64_t nnz, int64_t n_groups) {
  if (n < 0 || g < 0 || nnz < 0 || n_groups < 0 || n_groups > n) return 0;
  return std::max(ag_carve(nullptr, 0, n, g, nnz, n_groups, false).bytes, ag_carve(nullptr, 0, n, g, nnz, n_groups, true).bytes);
}

extern "C" int scamd_aggregate_part_entries(int64_t nnz) { return nnz < 0 ? 0 : ag_part_entries(nnz); }

extern "C" int scamd_aggregate_lanes_per_row(int64_t n, int64_t nnz) { return (n < 0 || nnz < 0) ? 0 : ag_lanes_per_row(n, nnz); }

extern "C" int scamd_aggregate_tier_bounds(int* gene_window, int* lds_min_run, int* median_wave_max, int* median_chunk) {
  if (!gene_window || !lds_min_run || !median_wave_max || !median_chunk) return SCAMD_EINVAL;
  *gene_window = AG_WINDOW;
  *lds_min_run = AG_LDS_MIN_RUN;
  *median_wave_max = AG_MED_WAVE_MAX;
  *median_chunk = AG_MED_CHUNK;
  return SCAMD_OK;
}

extern "C" int scamd_aggregate_moments_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                           int64_t nnz, const int32_t* codes, const int32_t* order, int64_t n_order,
                                           const int64_t* group_sizes, int64_t n_groups, double* sum, int64_t* count_nonzero,
                                           int64_t* count_negative, double* m2, uint32_t* flags, void* workspace,
                                           size_t workspace_bytes, scamd_stream_t stream) {
  const int rc = ag_check_input("aggregate_moments", indptr, indices, data, n, g, nnz, order, n_order, group_sizes, n_groups);
  if (rc != SCAMD_OK) return rc;
  const int64_t cells = n_groups * g;
  SCAMD_REQUIRE(flags && (n == 0 || codes) && (cells == 0 || (sum && count_nonzero && count_negative)), SCAMD_EINVAL,
                "aggregate_moments: null pointer");
  const size_t need = scamd_aggregate_workspace_bytes(n, g, nnz, n_groups);  // (one size serves both entry points)
  const AgWorkspace ws = ag_carve(workspace, workspace_bytes, n, g, nnz, n_groups, false);
  SCAMD_REQUIRE(workspace && ws.ok && workspace_bytes >= need, SCAMD_EWORKSPACE, "aggregate_moments: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  SCAMD_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(uint32_t), stream));
  if (cells == 0) return SCAMD_OK;
  const int gi = (int)g;
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.fix, 0, sizeof(long long) * (size_t)cells, stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.aux, 0, sizeof(unsigned long long) * (size_t)cells, stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.amax, 0, sizeof(unsigned int) * (size_t)g, stream));
  int src = ag_scan<false>(group_sizes, nullptr, 0, nullptr, 0, n_groups, ws.tiles, ws.goff, stream);
  if (src != SCAMD_OK) return src;
  src = ag_scan<true>(nullptr, order, n_order, indptr, n, n_order, ws.tiles, ws.pos, stream);
  if (src != SCAMD_OK) return src;
  const bool sweep = nnz > 0 && n_order > 0;
  if (sweep) {
    const int lanes = ag_lanes_per_row(n, nnz);
    hipLaunchKernelGGL(ag_range_kernel, dim3(ag_row_grid(n, lanes)), dim3(AG_BLOCK), 0, stream, indptr, indices, data, n, gi, nnz, codes,
                       n_groups, ag_log2(lanes), ws.amax, flags);
    SCAMD_LAUNCH_CHECK();
    src = ag_launch_sweep<0>(indptr, indices, data, n, gi, nnz, codes, order, n_order, ws, group_sizes, n_groups, sum, flags, stream);
    if (src != SCAMD_OK) return src;
  }
  hipLaunchKernelGGL(ag_convert_sums_kernel, dim3(ag_cell_grid(cells)), dim3(AG_BLOCK), 0, stream, gi, cells, group_sizes, ws.amax, ws.fix,
                     ws.aux, sum, count_nonzero, count_negative);
  SCAMD_LAUNCH_CHECK();
  if (!m2) return SCAMD_OK;
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.aux, 0, sizeof(unsigned int) * (size_t)cells, stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.fix, 0, sizeof(long long) * (size_t)cells, stream));
  if (sweep) {
    src = ag_launch_sweep<1>(indptr, indices, data, n, gi, nnz, codes, order, n_order, ws, group_sizes, n_groups, sum, flags, stream);
    if (src != SCAMD_OK) return src;
    src = ag_launch_sweep<2>(indptr, indices, data, n, gi, nnz, codes, order, n_order, ws, group_sizes, n_groups, sum, flags, stream);
    if (src != SCAMD_OK) return src;
  }
  hipLaunchKernelGGL(ag_convert_m2_kernel, dim3(ag_cell_grid(cells)), dim3(AG_BLOCK), 0, stream, gi, cells, group_sizes,
                     reinterpret_cast<const unsigned int*>(ws.aux), ws.fix, sum, count_nonzero, m2);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

extern "C" int scamd_aggregate_median_f32(const int64_t* indptr, const int32_t* indices, const float* data, int64_t n, int64_t g,
                                          int64_t nnz, const int32_t* order, int64_t n_order, const int64_t* group_sizes,
                                          int64_t n_groups, const int64_t* count_nonzero, const int64_t* count_negative,
                                          int mid_in_f32, double* median, int64_t* info_host, void* workspace,
                                          size_t workspace_bytes, scamd_stream_t stream) {
  const int rc = ag_check_input("aggregate_median", indptr, indices, data, n, g, nnz, order, n_order, group_sizes, n_groups);
  if (rc != SCAMD_OK) return rc;
  const int64_t cells = n_groups * g;
  SCAMD_REQUIRE(cells == 0 || (median && count_nonzero && count_negative), SCAMD_EINVAL, "aggregate_median: null pointer");
  SCAMD_REQUIRE(g * 4 <= 160 * 1024 - 64, SCAMD_EUNSUPPORTED, "aggregate_median: g=%lld exceeds the transpose (at most 40944)",
                (long long)g);
  const size_t need = scamd_aggregate_workspace_bytes(n, g, nnz, n_groups);  // (one size serves both entry points)
  const AgWorkspace ws = ag_carve(workspace, workspace_bytes, n, g, nnz, n_groups, true);
  SCAMD_REQUIRE(workspace && ws.ok && workspace_bytes >= need, SCAMD_EWORKSPACE, "aggregate_median: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  if (info_host) info_host[0] = info_host[1] = info_host[2] = 0;
  if (cells == 0) return SCAMD_OK;
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.counters, 0, 2 * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(ag_median_decide_kernel, dim3(ag_cell_grid(cells)), dim3(AG_BLOCK), 0, stream, g, cells, group_sizes, count_nonzero,
                     count_negative, median, ws.counters);
  SCAMD_LAUNCH_CHECK();
  unsigned long long open = 0ull;
  SCAMD_READBACK_NOW(&open, ws.counters, sizeof(open), stream);
  if (open == 0ull) {  // (count data, mostly)
    if (info_host) info_host[0] = cells;
    return SCAMD_OK;
  }
  int src = ag_scan<false>(group_sizes, nullptr, 0, nullptr, 0, n_groups, ws.tiles, ws.goff, stream);
  if (src != SCAMD_OK) return src;
  // pos over all n slots: the slots beyond n_order are empty rows of the matrix that is transposed
  src = ag_scan<true>(nullptr, order, n_order, indptr, n, n, ws.tiles, ws.pos, stream);
  if (src != SCAMD_OK) return src;
  int64_t total = 0;
  SCAMD_READBACK_NOW(&total, ws.pos + n, sizeof(total), stream);
  SCAMD_REQUIRE(total >= 0 && total <= nnz, SCAMD_EINVAL, "aggregate_median: the ordered rows hold %lld entries, the matrix %lld",
                (long long)total, (long long)nnz);
  if (total > 0) {
    const int lanes = ag_lanes_per_row(n, nnz);
    hipLaunchKernelGGL(ag_gather_rows_kernel, dim3(ag_row_grid(n_order, lanes)), dim3(AG_BLOCK), 0, stream, indptr, indices, data, n, nnz,
                       order, n_order, ws.pos, ag_log2(lanes), ws.p_indices, ws.p_data);
    SCAMD_LAUNCH_CHECK();
    src = scamd_csr_transpose_f32(ws.pos, ws.p_indices, ws.p_data, n, g, total, ws.t_indptr, ws.t_indices, ws.t_data, ws.transpose_ws,
                                  ws.transpose_bytes, stream);
    if (src != SCAMD_OK) return src;
  } else {
    SCAMD_HIP_CHECK(hipMemsetAsync(ws.t_indptr, 0, sizeof(int64_t) * (size_t)(g + 1), stream));
  }
  SCAMD_HIP_CHECK(hipMemsetAsync(ws.counters, 0, 2 * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(ag_median_classify_kernel, dim3(ag_cell_grid(cells)), dim3(AG_BLOCK), 0, stream, g, cells, ws.goff, ws.t_indptr,
                     ws.t_indices, group_sizes, count_nonzero, count_negative, median, ws.list, ws.counters);
  SCAMD_LAUNCH_CHECK();
  unsigned long long todo[2] = {0ull, 0ull};
  SCAMD_READBACK_NOW(todo, ws.counters, sizeof(todo), stream);
  SCAMD_REQUIRE(todo[0] + todo[1] <= (unsigned long long)cells && todo[1] < (1ull << 31), SCAMD_EINTERNAL,
                "aggregate_median: work list of %llu + %llu pairs", todo[0], todo[1]);
  if (todo[0]) {
    hipLaunchKernelGGL(ag_median_wave_kernel, dim3((unsigned)ceil_div((int64_t)todo[0], AG_BLOCK / 64)), dim3(AG_BLOCK), 0, stream, g,
                       (int64_t)todo[0], ws.list, ws.goff, ws.t_indptr, ws.t_indices, ws.t_data, group_sizes, count_nonzero,
                       count_negative, mid_in_f32, median);
    SCAMD_LAUNCH_CHECK();
  }
  if (todo[1]) {
    hipLaunchKernelGGL(ag_median_block_kernel, dim3((unsigned)todo[1]), dim3(AG_BLOCK), 0, stream, g, cells, ws.list, ws.goff, ws.t_indptr,
                       ws.t_indices, ws.t_data, group_sizes, count_nonzero, count_negative, mid_in_f32, median);
    SCAMD_LAUNCH_CHECK();
  }
  if (info_host) {
    info_host[0] = cells - (int64_t)todo[0] - (int64_t)todo[1];
    info_host[1] = (int64_t)todo[0];
    info_host[2] = (int64_t)todo[1];
  }
  return SCAMD_OK;
}
