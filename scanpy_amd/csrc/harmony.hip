// Harmony batch correction (`pp.harmony_integrate`): soft k-means with a batch-diversity penalty on the
// L2-normalised embedding, then a closed-form ridge correction per cluster.  All arithmetic is float64.
//
// The state is R [n x K] (responsibilities, row-major) and the two tables O, E [B x K] (observed / expected mass of batch
// level b in cluster k).  One clustering round visits the cells in a keyed permutation cut into blocks; the blocks run ONE
// AFTER ANOTHER, each as
//     hm_assign_kernel<SUMS>    one read of the block's old rows: their sums per (level, cluster)
//     hm_tables_kernel          O -= sums, E -= pr_b * column sums, the B x K log-penalty table (single workgroup)
//     hm_assign_kernel<UPDATE>  fused: gather z through perm, dots against Y_norm (LDS), penalty, row-max-shifted softmax,
//                               write the rows, the block's new sums, the cells' two objective terms
//     hm_tables_kernel          O += sums, E += pr_b * column sums
// One wave owns one cell at a time: lane l holds clusters l, l + 64, l + 128, l + 192 (K <= 256); the cell's row of z sits in
// registers (lane j keeps columns j, j + 64; read back with v_readlane) and the next cell's row is loaded meanwhile.
//
// Every sum over cells is an INTEGER one: a value is rounded once to 64-bit fixed point (the scale follows from a bound on the
// sum) and added with integer atomics, in LDS first where the table fits, so the result does not depend on the order in which
// lanes, waves or workgroups run -- two calls give the same bits.  There are no float atomics.  Sums inside one wave are
// xor-butterflies (every lane ends with the same bits), sums inside one thread run in index order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

namespace scamd {

namespace {

constexpr int HM_BLOCK = 256;
constexpr int HM_WAVES = HM_BLOCK / 64;
constexpr int HM_MAX_D = SCAMD_HARMONY_MAX_D;
constexpr int HM_MAX_K = SCAMD_HARMONY_MAX_K;
constexpr int HM_MAX_B = SCAMD_HARMONY_MAX_LEVELS;
constexpr int HM_KQ = HM_MAX_K / 64;            // clusters per lane
constexpr int HM_DQ = HM_MAX_D / 64;            // columns per lane (correction)
constexpr int HM_CELLS_PER_WG = 64;             // cells of a block that one workgroup of the assign kernel takes
constexpr size_t HM_Y_LDS_BYTES = 41 * 1024;    // Y_norm stays in LDS up to this size (K = 100, d = 50: 40800 B)
constexpr size_t HM_TABLE_LDS_BYTES = 16 * 1024;  // the block sums are gathered in LDS up to this size (B * K <= 2048)
constexpr int HM_WS_CHUNK = 1024;               // cells per workgroup of the weighted-sum kernel
constexpr int HM_WS_CELLS = 16;                 // cells staged in LDS at a time (K = 256, d = 128: 49 KiB)
constexpr int HM_WS_TK = 4, HM_WS_TJ = 5;       // block of (weight column, data column) pairs of one thread
constexpr int HM_KM_CHUNK = 256;                // cells per partial sum of the D^2 sampling
constexpr double HM_SENTINEL = 1e30;            // lambda of a (level, cluster) pair that gets no correction
constexpr double HM_CLAMP = 1e-12;

enum { HM_UPDATE = 0, HM_INIT = 1, HM_SUMS = 2 };

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}
// v of lane `src` (wave-uniform) in every lane
__device__ __forceinline__ double lane_value(double v, int src) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)bits, src), hi = __builtin_amdgcn_readlane((int)(bits >> 32), src);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo));
}
__device__ __forceinline__ void fix_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// fractional bits with which `count` values of magnitude <= 1 add up below 2^62
inline int frac_unit(int64_t count) {
  int lg = 0;
  while (((int64_t)1 << lg) <= count && lg < 62) ++lg;  // 2^lg > count
  return 62 - lg;
}

// ---------------------------------------------------------------------------------------------------------------------
// the block permutation: a keyed bijection on [0, n) -- a balanced Feistel network of 6 rounds on 2h bits, 4^h >= n,
// walked along its cycle until it lands below n (4^h < 4n: fewer than four steps on average)
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__global__ __launch_bounds__(HM_BLOCK) void hm_permutation_kernel(int64_t n, uint64_t key, int h, int32_t* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * HM_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t mask = ((uint64_t)1 << h) - 1;
  uint64_t x = (uint64_t)i;
  do {
    uint64_t l = x >> h, r = x & mask;
    for (int t = 0; t < 6; ++t) {
      const uint64_t f = (mix64(key + (uint64_t)(t + 1) * 0xD1B54A32D192ED03ull + r) >> 32) & mask;
      const uint64_t nl = r;
      r = l ^ f;
      l = nl;
    }
    x = (l << h) | r;
  } while (x >= (uint64_t)n);
  perm[i] = (int32_t)x;
}

// ---------------------------------------------------------------------------------------------------------------------
// rows
// ---------------------------------------------------------------------------------------------------------------------
// out[i, :] = x[i, :] / max(|x[i, :]|, 1e-12); one wave per row
__global__ __launch_bounds__(HM_BLOCK) void hm_normalize_kernel(const double* __restrict__ x, int64_t n, int d, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * HM_WAVES + (threadIdx.x >> 6);
  if (i >= n) return;  // (whole waves leave)
  double v[HM_DQ], ss = 0.0;
  for (int q = 0; q < HM_DQ; ++q) {
    const int j = lane + 64 * q;
    v[q] = j < d ? x[i * d + j] : 0.0;
    ss += v[q] * v[q];
  }
  ss = wave_sum(ss);
  const double nrm = fmax(sqrt(ss), HM_CLAMP);
  for (int q = 0; q < HM_DQ; ++q) {
    const int j = lane + 64 * q;
    if (j < d) out[i * d + j] = v[q] / nrm;
  }
}

// max |x| as the bits of a non-negative double (they order as unsigned integers)
__global__ __launch_bounds__(HM_BLOCK) void hm_absmax_kernel(const double* __restrict__ x, int64_t count, unsigned long long* __restrict__ out) {
  unsigned long long mx = 0ull;
  for (int64_t p = (int64_t)blockIdx.x * HM_BLOCK + threadIdx.x; p < count; p += (int64_t)gridDim.x * HM_BLOCK) {
    const unsigned long long a = (unsigned long long)__double_as_longlong(fabs(x[p]));
    mx = a > mx ? a : mx;
  }
  if (mx) atomicMax(out, mx);
}

// fractional bits for sums of `count` products of a weight <= 1 and a value <= absmax
__global__ void hm_frac_kernel(const unsigned long long* __restrict__ absmax_bits, double count, int* __restrict__ frac) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double bound = count * (absmax_bits ? __longlong_as_double((long long)*absmax_bits) : 1.0);
  int e = 0;
  if (bound > 0.0 && bound < 1e300) frexp(bound, &e);  // bound < 2^e
  int f = 62 - e;
  f = f > 1000 ? 1000 : (f < -900 ? -900 : f);
  *frac = bound > 0.0 ? f : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// out[(k * nb + b) * d + j] += sum over the cells i of the chunk with codes[i] == b of w[i, k] * x[i, j], rounded once per
// (chunk, b, k, j) to fixed point.  w == nullptr: weight 1 (kw = 1); codes == nullptr: one group.
// grid (chunks, nb).  The rows of HM_WS_CELLS cells at a time are staged in LDS (every value read once from global memory,
// coalesced; the rows of cells of another group are not read at all); a thread owns a 4 x 5 block of (weight column, data column)
// pairs and takes the staged cells in index order: 9 LDS reads for 20 multiply-adds.  More than 256 blocks of pairs (K d > 5120)
// take several passes over the chunk.
// LDS: [HM_WS_CELLS x kw weights][HM_WS_CELLS x d values][HM_WS_CELLS flags]
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_BLOCK) void hm_wsum_kernel(const double* __restrict__ w, int kw, const double* __restrict__ x, int d,
                                                           const int32_t* __restrict__ codes, int nb, int64_t n,
                                                           const int* __restrict__ frac_ptr, long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long hm_smem[];
  double* s_w = reinterpret_cast<double*>(hm_smem);
  double* s_x = s_w + (size_t)HM_WS_CELLS * kw;
  int* s_in = reinterpret_cast<int*>(s_x + (size_t)HM_WS_CELLS * d);
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * HM_WS_CHUNK;
  const int64_t i1 = i0 + HM_WS_CHUNK < n ? i0 + HM_WS_CHUNK : n;
  const double sc = ldexp(1.0, *frac_ptr);
  const int tiles_j = (d + HM_WS_TJ - 1) / HM_WS_TJ, tiles = ((kw + HM_WS_TK - 1) / HM_WS_TK) * tiles_j;
  for (int pass0 = 0; pass0 < tiles; pass0 += HM_BLOCK) {
    const int tt = pass0 + tid;
    const bool active = tt < tiles;
    const int k0 = active ? (tt / tiles_j) * HM_WS_TK : 0, j0 = active ? (tt % tiles_j) * HM_WS_TJ : 0;
    int ko[HM_WS_TK], jo[HM_WS_TJ];  // clamped columns: a block that hangs over the edge reads valid LDS and drops the result
    for (int a = 0; a < HM_WS_TK; ++a) ko[a] = k0 + a < kw ? k0 + a : kw - 1;
    for (int c = 0; c < HM_WS_TJ; ++c) jo[c] = j0 + c < d ? j0 + c : d - 1;
    double acc[HM_WS_TK][HM_WS_TJ];
    for (int a = 0; a < HM_WS_TK; ++a)
      for (int c = 0; c < HM_WS_TJ; ++c) acc[a][c] = 0.0;
    for (int64_t t0 = i0; t0 < i1; t0 += HM_WS_CELLS) {
      const int cells = i1 - t0 < HM_WS_CELLS ? (int)(i1 - t0) : HM_WS_CELLS;
      __syncthreads();  // (the tile before this one has been read)
      if (tid < cells) s_in[tid] = !codes || codes[t0 + tid] == b;
      __syncthreads();
      for (int e = tid; e < cells * kw; e += HM_BLOCK) {
        const int c = e / kw;
        s_w[e] = s_in[c] ? (w ? w[t0 * kw + e] : 1.0) : 0.0;
      }
      for (int e = tid; e < cells * d; e += HM_BLOCK) {
        const int c = e / d;
        s_x[e] = s_in[c] ? x[t0 * d + e] : 0.0;
      }
      __syncthreads();
      for (int c = 0; c < cells; ++c) {
        if (!s_in[c]) continue;
        double wv[HM_WS_TK], xv[HM_WS_TJ];
        for (int a = 0; a < HM_WS_TK; ++a) wv[a] = s_w[c * kw + ko[a]];
        for (int q = 0; q < HM_WS_TJ; ++q) xv[q] = s_x[c * d + jo[q]];
        for (int a = 0; a < HM_WS_TK; ++a)
          for (int q = 0; q < HM_WS_TJ; ++q) acc[a][q] += wv[a] * xv[q];
      }
    }
    if (active)
      for (int a = 0; a < HM_WS_TK; ++a)
        for (int q = 0; q < HM_WS_TJ; ++q)
          if (k0 + a < kw && j0 + q < d && acc[a][q] != 0.0)
            fix_add(&out[((int64_t)(k0 + a) * nb + b) * d + j0 + q], llrint(acc[a][q] * sc));
  }
}

inline size_t wsum_lds_bytes(int kw, int d) { return (size_t)HM_WS_CELLS * (kw + d) * sizeof(double) + HM_WS_CELLS * sizeof(int); }

// centroids from their fixed-point sums, normalised: one workgroup per cluster
__global__ __launch_bounds__(HM_MAX_D) void hm_centroid_kernel(const long long* __restrict__ fix, const int* __restrict__ frac_ptr, int d,
                                                               double* __restrict__ y_norm) {
  __shared__ double s_v[HM_MAX_D];
  const int k = blockIdx.x, j = threadIdx.x;
  const double v = j < d ? ldexp((double)fix[(int64_t)k * d + j], -*frac_ptr) : 0.0;
  s_v[j] = v;
  __syncthreads();
  double ss = 0.0;
  for (int t = 0; t < d; ++t) ss += s_v[t] * s_v[t];
  const double nrm = fmax(sqrt(ss), HM_CLAMP);
  if (j < d) y_norm[(int64_t)k * d + j] = v / nrm;
}

// ---------------------------------------------------------------------------------------------------------------------
// the cells of one block: cells perm[start .. start + m) (perm == nullptr: start .. start + m)
//   HM_SUMS    delta[b, k] += R[i, k]
//   HM_INIT    R[i, :] = exp(term (1 - z_i . y_k)) / max(sum, 1e-12)                     (no shift: the reference's first R)
//   HM_UPDATE  R[i, :] = softmax_k(term (1 - z_i . y_k) + pen[b_i, k]), row max taken out, sum clamped at 1e-12
//   INIT / UPDATE also add the new rows to delta and the cell's two objective terms to obj_fix[0] (k-means error) and
//   obj_fix[1] (entropy / sigma).
// LDS: [Y_norm with rows padded to an odd length, if y_lds][B x K fixed-point sums, if tab_lds]
// ---------------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(HM_BLOCK) void hm_assign_kernel(const double* __restrict__ z, const int32_t* __restrict__ codes,
                                                             const int32_t* __restrict__ perm, int64_t start, int64_t m, int64_t n,
                                                             const double* __restrict__ y, const double* __restrict__ pen, double term,
                                                             double* __restrict__ R, long long* __restrict__ delta, int frac_delta,
                                                             long long* __restrict__ obj_fix, int frac_obj, int K, int d, int B, int y_lds,
                                                             int tab_lds) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long hm_smem[];
  const int dp = d | 1;
  double* s_y = reinterpret_cast<double*>(hm_smem);
  long long* s_tab = reinterpret_cast<long long*>(hm_smem + (MODE != HM_SUMS && y_lds ? (size_t)K * dp : 0));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (MODE != HM_SUMS && y_lds)
    for (int p = tid; p < K * d; p += HM_BLOCK) s_y[(p / d) * dp + p % d] = y[p];
  if (tab_lds)
    for (int p = tid; p < B * K; p += HM_BLOCK) s_tab[p] = 0;
  __syncthreads();
  const double* ysrc = y_lds ? s_y : y;
  const int ystride = y_lds ? dp : d;
  long long* tab = tab_lds ? s_tab : delta;
  const double sc = ldexp(1.0, frac_delta), so = ldexp(1.0, frac_obj);
  int kk[HM_KQ];
  bool valid[HM_KQ];
  for (int q = 0; q < HM_KQ; ++q) {
    valid[q] = lane + 64 * q < K;
    kk[q] = valid[q] ? lane + 64 * q : K - 1;
  }
  const int nq = (K + 63) / 64;
  long long acc_km = 0, acc_ent = 0;
  const int64_t c0 = (int64_t)blockIdx.x * HM_CELLS_PER_WG;
  const int64_t c1 = c0 + HM_CELLS_PER_WG < m ? c0 + HM_CELLS_PER_WG : m;
  // the next cell of this wave is fetched (its id, its level, its row of z: lane j keeps columns j and j + 64) before the current
  // one is worked on, so its loads are in flight during the arithmetic
  int i_next = -1, b_next = -1;
  double z_next[HM_DQ];
  auto fetch = [&](int64_t c) {
    i_next = -1;
    for (int q = 0; q < HM_DQ; ++q) z_next[q] = 0.0;
    if (c >= c1) return;
    const int i = __builtin_amdgcn_readfirstlane(perm ? perm[start + c] : (int)(start + c));
    if (i < 0 || (int64_t)i >= n) return;
    i_next = i;
    b_next = __builtin_amdgcn_readfirstlane(codes[i]);
    if (MODE != HM_SUMS)
      for (int q = 0; q < HM_DQ; ++q)
        if (lane + 64 * q < d) z_next[q] = z[(int64_t)i * d + lane + 64 * q];
  };
  fetch(c0 + wave);
  for (int64_t c = c0 + wave; c < c1; c += HM_WAVES) {
    const int i = i_next, b = b_next;
    double zr[HM_DQ];
    for (int q = 0; q < HM_DQ; ++q) zr[q] = z_next[q];
    fetch(c + HM_WAVES);
    if (i < 0) continue;
    if (b < 0 || b >= B) continue;  // (the front end refuses such codes; a stray one must not index the tables)
    double r[HM_KQ];
    if (MODE == HM_SUMS) {
      for (int q = 0; q < HM_KQ; ++q) r[q] = valid[q] ? R[(int64_t)i * K + kk[q]] : 0.0;
    } else {
      double dot[HM_KQ];
      for (int q = 0; q < HM_KQ; ++q) dot[q] = 0.0;
      for (int h = 0; h < HM_DQ; ++h) {
        const int jn = d - 64 * h < 64 ? d - 64 * h : 64;
        for (int jj = 0; jj < jn; ++jj) {
          const double zj = lane_value(zr[h], jj);
          const int j = 64 * h + jj;
          for (int q = 0; q < HM_KQ; ++q)
            if (q < nq) dot[q] += zj * ysrc[kk[q] * ystride + j];  // (wave-uniform: K = 100 costs two of the four columns)
        }
      }
      double e[HM_KQ], mx = -INFINITY;
      for (int q = 0; q < HM_KQ; ++q) {
        e[q] = term * (1.0 - dot[q]);
        if (MODE == HM_UPDATE) e[q] += pen[(int64_t)b * K + kk[q]];
        if (valid[q] && e[q] > mx) mx = e[q];
      }
      if (MODE == HM_UPDATE) mx = wave_max(mx);
      double s = 0.0;
      for (int q = 0; q < HM_KQ; ++q) {
        e[q] = valid[q] ? exp(MODE == HM_UPDATE ? e[q] - mx : e[q]) : 0.0;
        s += e[q];
      }
      s = fmax(wave_sum(s), HM_CLAMP);
      double s2 = 0.0;
      for (int q = 0; q < HM_KQ; ++q) {
        r[q] = e[q] / s;
        if (valid[q]) R[(int64_t)i * K + kk[q]] = r[q];
        s2 += r[q];
      }
      s2 = fmax(wave_sum(s2), HM_CLAMP);
      double km = 0.0, ent = 0.0;
      for (int q = 0; q < HM_KQ; ++q) {
        if (!valid[q]) continue;
        km += (r[q] * 2.0) * (1.0 - dot[q]);
        const double rn = r[q] / s2;
        ent += rn * log(rn + HM_CLAMP);
      }
      km = wave_sum(km);
      ent = wave_sum(ent);
      acc_km += llrint(km * so);
      acc_ent += llrint(ent * so);
    }
    for (int q = 0; q < HM_KQ; ++q) {
      if (!valid[q]) continue;
      const long long v = llrint(r[q] * sc);
      if (v) fix_add(&tab[(int64_t)b * K + kk[q]], v);
    }
  }
  if (MODE != HM_SUMS && lane == 0) {
    if (acc_km) fix_add(&obj_fix[0], acc_km);
    if (acc_ent) fix_add(&obj_fix[1], acc_ent);
  }
  if (tab_lds) {
    __syncthreads();
    for (int p = tid; p < B * K; p += HM_BLOCK) {
      const long long v = s_tab[p];
      if (v) fix_add(&delta[p], v);
    }
  }
}

// O, E and the log-penalty table from the sums of one block; single workgroup, thread k walks the levels in order.
//   sign -1 / +1: O += sign * delta, E += sign * pr_b * (column sum of delta);  sign 0: O = delta, E = pr_b * column sum
//   pen != nullptr: pen[b, k] = theta_b (log(E + 1) - log(O [+ E] + 1)).  delta is left zeroed.
__global__ __launch_bounds__(HM_BLOCK) void hm_tables_kernel(long long* __restrict__ delta, int frac, int sign, const double* __restrict__ pr_b,
                                                             const double* __restrict__ theta, int stabilized, double* __restrict__ O,
                                                             double* __restrict__ E, double* __restrict__ pen, int K, int B) {
  for (int k = threadIdx.x; k < K; k += HM_BLOCK) {
    long long cs = 0;
    for (int b = 0; b < B; ++b) cs += delta[(int64_t)b * K + k];
    const double ds = ldexp((double)cs, -frac);
    for (int b = 0; b < B; ++b) {
      const int64_t p = (int64_t)b * K + k;
      const double dv = ldexp((double)delta[p], -frac);
      const double de = pr_b[b] * ds;
      double o, e;
      if (sign == 0) {
        o = dv;
        e = de;
      } else if (sign > 0) {
        o = O[p] + dv;
        e = E[p] + de;
      } else {
        o = O[p] - dv;
        e = E[p] - de;
      }
      O[p] = o;
      E[p] = e;
      delta[p] = 0;
      if (pen) pen[p] = theta[b] * (log(e + 1.0) - log(stabilized ? o + e + 1.0 : o + 1.0));
    }
  }
}

// objective[0..3] = total, k-means error, entropy term, diversity term; single workgroup
__global__ __launch_bounds__(HM_BLOCK) void hm_objective_kernel(const long long* __restrict__ obj_fix, int frac_obj, const double* __restrict__ O,
                                                                const double* __restrict__ E, const double* __restrict__ theta, double sigma,
                                                                int stabilized, int K, int B, double* __restrict__ objective) {
  __shared__ double s_k[HM_MAX_K];
  for (int k = threadIdx.x; k < K; k += HM_BLOCK) {
    double a = 0.0;
    for (int b = 0; b < B; ++b) {
      const double o = O[(int64_t)b * K + k], e = E[(int64_t)b * K + k];
      a += theta[b] * (o * log((stabilized ? o + e + 1.0 : o + 1.0) / (e + 1.0)));
    }
    s_k[k] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double div = 0.0;
    for (int k = 0; k < K; ++k) div += s_k[k];
    div *= sigma;
    const double km = ldexp((double)obj_fix[0], -frac_obj);
    const double ent = sigma * ldexp((double)obj_fix[1], -frac_obj);
    objective[0] = km + ent + div;
    objective[1] = km;
    objective[2] = ent;
    objective[3] = div;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// k-means initialisation
// ---------------------------------------------------------------------------------------------------------------------
// mind2[i] = min(mind2[i], |z_i - z_sel|^2) (first: no min) and the sum of every chunk of HM_KM_CHUNK cells, a fixed tree
__global__ __launch_bounds__(HM_KM_CHUNK) void km_seed_update_kernel(const double* __restrict__ z, int64_t n, int d, const int32_t* __restrict__ sel,
                                                                     int first, double* __restrict__ mind2, double* __restrict__ partial) {
  __shared__ double s_p[HM_KM_CHUNK];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * HM_KM_CHUNK + tid;
  double v = 0.0;
  if (i < n) {
    const double* c = z + (int64_t)(*sel) * d;
    double a = 0.0;
    for (int j = 0; j < d; ++j) {
      const double t = z[i * d + j] - c[j];
      a += t * t;
    }
    v = first ? a : fmin(mind2[i], a);
    mind2[i] = v;
  }
  s_p[tid] = v;
  __syncthreads();
  for (int o = HM_KM_CHUNK / 2; o > 0; o >>= 1) {
    if (tid < o) s_p[tid] += s_p[tid + o];
    __syncthreads();
  }
  if (tid == 0) partial[blockIdx.x] = s_p[0];
}

// centre c: the first cell whose running sum of D^2 exceeds u * total (centre 0, or total == 0: cell floor(u n)); single workgroup
__global__ __launch_bounds__(HM_BLOCK) void km_seed_pick_kernel(const double* __restrict__ z, int64_t n, int d, const double* __restrict__ mind2,
                                                                const double* __restrict__ partial, int64_t n_partial, double u, int first,
                                                                int32_t* __restrict__ sel, double* __restrict__ centre) {
  __shared__ double s_seg[HM_BLOCK];
  __shared__ int64_t s_pick;
  const int tid = threadIdx.x;
  const int64_t per = (n_partial + HM_BLOCK - 1) / HM_BLOCK;
  if (!first) {
    double a = 0.0;
    for (int64_t p = tid * per; p < (tid + 1) * per && p < n_partial; ++p) a += partial[p];
    s_seg[tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    int64_t uniform_pick = (int64_t)(u * (double)n);
    uniform_pick = uniform_pick < 0 ? 0 : (uniform_pick >= n ? n - 1 : uniform_pick);
    int64_t pick = uniform_pick;
    if (!first) {
      double total = 0.0;
      for (int t = 0; t < HM_BLOCK; ++t) total += s_seg[t];
      if (total > 0.0) {
        const double target = u * total;
        double run = 0.0;
        int seg = 0;
        while (seg < HM_BLOCK - 1 && run + s_seg[seg] <= target) run += s_seg[seg++];
        int64_t p = seg * per;
        const int64_t p_end = (seg + 1) * per < n_partial ? (seg + 1) * per : n_partial;
        while (p < p_end - 1 && run + partial[p] <= target) run += partial[p++];
        if (p >= n_partial) p = n_partial - 1;
        int64_t i = p * HM_KM_CHUNK;
        const int64_t i_end = i + HM_KM_CHUNK < n ? i + HM_KM_CHUNK : n;
        pick = i_end - 1;
        for (; i < i_end; ++i) {
          run += mind2[i];
          if (run > target) {
            pick = i;
            break;
          }
        }
      }
    }
    s_pick = pick;
    *sel = (int32_t)pick;
  }
  __syncthreads();
  const int64_t pick = s_pick;
  for (int j = tid; j < d; j += HM_BLOCK) centre[j] = z[pick * d + j];
}

// labels[i] = the nearest centre (lowest index on ties); counts the cells per centre and the labels that changed.
// One wave per cell, the centres in LDS (rows padded to an odd length) where they fit.
__global__ __launch_bounds__(HM_BLOCK) void km_assign_kernel(const double* __restrict__ z, int64_t n, int d, int K, const double* __restrict__ centres,
                                                             int32_t* __restrict__ labels, unsigned long long* __restrict__ counts,
                                                             unsigned long long* __restrict__ changed, int y_lds) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long hm_smem[];
  const int dp = d | 1;
  double* s_y = reinterpret_cast<double*>(hm_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (y_lds)
    for (int p = tid; p < K * d; p += HM_BLOCK) s_y[(p / d) * dp + p % d] = centres[p];
  __syncthreads();
  const double* ysrc = y_lds ? s_y : centres;
  const int ystride = y_lds ? dp : d;
  const int nq = (K + 63) / 64;
  const int64_t c0 = (int64_t)blockIdx.x * HM_CELLS_PER_WG;
  const int64_t c1 = c0 + HM_CELLS_PER_WG < n ? c0 + HM_CELLS_PER_WG : n;
  for (int64_t i = c0 + wave; i < c1; i += HM_WAVES) {
    const double* zi = z + i * d;
    double d2[HM_KQ];
    int kk[HM_KQ];
    for (int q = 0; q < HM_KQ; ++q) {
      d2[q] = 0.0;
      kk[q] = lane + 64 * q < K ? lane + 64 * q : K - 1;
    }
    for (int j = 0; j < d; ++j) {
      const double zj = zi[j];
      for (int q = 0; q < HM_KQ; ++q) {
        if (q >= nq) break;
        const double t = zj - ysrc[kk[q] * ystride + j];
        d2[q] += t * t;
      }
    }
    double best = INFINITY;
    int best_k = HM_MAX_K;
    for (int q = 0; q < HM_KQ; ++q)
      if (lane + 64 * q < K && d2[q] < best) {
        best = d2[q];
        best_k = lane + 64 * q;
      }
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o);
      const int ok = __shfl_xor(best_k, o);
      if (ob < best || (ob == best && ok < best_k)) {
        best = ob;
        best_k = ok;
      }
    }
    if (lane == 0) {
      if (labels[i] != best_k) {
        labels[i] = best_k;
        atomicAdd(changed, 1ull);
      }
      atomicAdd(&counts[best_k], 1ull);
    }
  }
}

// centre k = the mean of its cells; a centre without cells stays
__global__ __launch_bounds__(HM_MAX_D) void km_centre_kernel(const long long* __restrict__ fix, const int* __restrict__ frac_ptr,
                                                             const unsigned long long* __restrict__ counts, int d, double* __restrict__ centres) {
  const int k = blockIdx.x, j = threadIdx.x;
  const unsigned long long c = counts[k];
  if (j < d && c > 0ull) centres[(int64_t)k * d + j] = ldexp((double)fix[(int64_t)k * d + j], -*frac_ptr) / (double)c;
}

// ---------------------------------------------------------------------------------------------------------------------
// correction
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_BLOCK) void hm_lambda_kernel(const double* __restrict__ O, const double* __restrict__ E, const double* __restrict__ n_b,
                                                             int dynamic_lambda, double alpha, double threshold, int prune, double ridge_lambda,
                                                             int K, int B, double* __restrict__ lambda_kb) {
  const int64_t p = (int64_t)blockIdx.x * HM_BLOCK + threadIdx.x;
  if (p >= (int64_t)B * K) return;
  const int b = (int)(p / K);
  const double o = O[p];
  double lam = ridge_lambda;
  if (dynamic_lambda) {
    lam = alpha * E[p];
    if (prune) {
      const double nb = n_b[b];
      if (o / (nb > 0.0 ? nb : 1.0) < threshold || nb == 0.0) lam = HM_SENTINEL;
    }
  }
  if (o + lam == 0.0) lam = HM_SENTINEL;
  lambda_kb[p] = lam;
}

// W[k, b, :] of the closed-form ridge solution of cluster k on the one-hot design with an intercept:
//   f_b = 1 / (O_bk + lambda_bk), p_b = -f_b O_bk, c = sum_b O_bk + sum_b (-f_b O_bk^2),
//   W_b = (p_b / c) (phi_0 + sum_b' p_b' phi_b') + f_b phi_b        (phi_b = sum over the cells of level b of R_ik x_i, phi_0 their sum)
// one workgroup per cluster, thread j one column; the sums over the levels run in level order
__global__ __launch_bounds__(HM_MAX_D) void hm_ridge_kernel(const long long* __restrict__ phi_fix, const int* __restrict__ frac_ptr,
                                                            const double* __restrict__ O, const double* __restrict__ lambda_kb, int K, int B, int d,
                                                            double* __restrict__ W) {
  const int k = blockIdx.x, j = threadIdx.x;
  if (j >= d) return;
  const int frac = *frac_ptr;
  double sum_o = 0.0, sum_fo2 = 0.0, acc = 0.0;
  long long tot = 0;
  for (int b = 0; b < B; ++b) {
    const double o = O[(int64_t)b * K + k];
    const double f = 1.0 / (o + lambda_kb[(int64_t)b * K + k]);
    const long long v = phi_fix[((int64_t)k * B + b) * d + j];
    sum_o += o;
    sum_fo2 += -f * (o * o);
    tot += v;
    acc += (-f * o) * ldexp((double)v, -frac);
  }
  const double c_inv = 1.0 / (sum_o + sum_fo2);
  const double t = ldexp((double)tot, -frac) + acc;
  for (int b = 0; b < B; ++b) {
    const double o = O[(int64_t)b * K + k];
    const double f = 1.0 / (o + lambda_kb[(int64_t)b * K + k]);
    const double phi = ldexp((double)phi_fix[((int64_t)k * B + b) * d + j], -frac);
    W[((int64_t)k * B + b) * d + j] = ((-f * o) * c_inv) * t + f * phi;
  }
}

// z_hat[i, :] = x[i, :] - sum_k R[i, k] W[k, b_i, :] (clusters in index order), z_norm its normalised rows; one wave per cell
__global__ __launch_bounds__(HM_BLOCK) void hm_apply_kernel(const double* __restrict__ x, const int32_t* __restrict__ codes, const double* __restrict__ R,
                                                            const double* __restrict__ W, int64_t n, int d, int K, int B, double* __restrict__ z_hat,
                                                            double* __restrict__ z_norm) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * HM_WAVES + (threadIdx.x >> 6);
  if (i >= n) return;  // (whole waves leave)
  const int b = __builtin_amdgcn_readfirstlane(codes[i]);
  double v[HM_DQ];
  int jj[HM_DQ];
  for (int q = 0; q < HM_DQ; ++q) {
    jj[q] = lane + 64 * q < d ? lane + 64 * q : d - 1;
    v[q] = x[i * d + jj[q]];
  }
  if (b >= 0 && b < B) {
    const double* ri = R + i * K;
    for (int k = 0; k < K; ++k) {
      const double rk = ri[k];
      const double* wk = W + ((int64_t)k * B + b) * d;
      for (int q = 0; q < HM_DQ; ++q) v[q] -= rk * wk[jj[q]];
    }
  }
  double ss = 0.0;
  for (int q = 0; q < HM_DQ; ++q)
    if (lane + 64 * q < d) ss += v[q] * v[q];
  ss = wave_sum(ss);
  const double nrm = fmax(sqrt(ss), HM_CLAMP);
  for (int q = 0; q < HM_DQ; ++q)
    if (lane + 64 * q < d) {
      z_hat[i * d + jj[q]] = v[q];
      z_norm[i * d + jj[q]] = v[q] / nrm;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
int check_shape(const char* what, int64_t n, int d, int K, int B, int n_covariates) {
  SCAMD_REQUIRE(n_covariates == 1, SCAMD_EUNSUPPORTED,
                "%s: %d batch variables; only one is supported (several need the general-design ridge solve)", what, n_covariates);
  SCAMD_REQUIRE(n >= 1 && d >= 1 && K >= 1 && B >= 1, SCAMD_EINVAL, "%s: bad shape n=%lld d=%d K=%d levels=%d", what, (long long)n, d, K, B);
  SCAMD_REQUIRE(n < ((int64_t)1 << 31), SCAMD_EUNSUPPORTED, "%s: n=%lld exceeds int32 cell ids", what, (long long)n);
  SCAMD_REQUIRE(d <= HM_MAX_D, SCAMD_EUNSUPPORTED, "%s: d=%d exceeds %d columns", what, d, HM_MAX_D);
  SCAMD_REQUIRE(K <= HM_MAX_K, SCAMD_EUNSUPPORTED, "%s: K=%d exceeds %d clusters", what, K, HM_MAX_K);
  SCAMD_REQUIRE(B <= HM_MAX_B, SCAMD_EUNSUPPORTED, "%s: %d batch levels exceed %d", what, B, HM_MAX_B);
  return SCAMD_OK;
}

inline bool y_fits_lds(int K, int d) { return (size_t)K * (d | 1) * sizeof(double) <= HM_Y_LDS_BYTES; }
inline bool table_fits_lds(int K, int B) { return (size_t)K * B * sizeof(long long) <= HM_TABLE_LDS_BYTES; }

// buffers shared by init and the clustering round
struct StateWs {
  double* y_norm;      // [K, d] (init: the normalised centroids)
  long long* y_fix;    // [K, d]
  long long* delta;    // [B, K]
  double* pen;         // [B, K]
  long long* obj_fix;  // [2]
  int* frac;           // [1]
  bool carve(Workspace& ws, int d, int K, int B) {
    y_norm = ws.take<double>((size_t)K * d);
    y_fix = ws.take<long long>((size_t)K * d);
    delta = ws.take<long long>((size_t)B * K);
    pen = ws.take<double>((size_t)B * K);
    obj_fix = ws.take<long long>(2);
    frac = ws.take<int>(1);
    return ws.ok;
  }
};

template <int MODE>
int launch_assign(const double* z, const int32_t* codes, const int32_t* perm, int64_t start, int64_t m, int64_t n, const double* y, const double* pen,
                  double term, double* R, long long* delta, long long* obj_fix, int frac_obj, int K, int d, int B, hipStream_t stream) {
  if (m <= 0) return SCAMD_OK;
  const int y_lds = MODE != HM_SUMS && y_fits_lds(K, d), tab_lds = table_fits_lds(K, B);
  const size_t lds = (y_lds ? (size_t)K * (d | 1) * sizeof(double) : 0) + (tab_lds ? (size_t)K * B * sizeof(long long) : 0);
  hipLaunchKernelGGL(hm_assign_kernel<MODE>, dim3((unsigned)ceil_div(m, HM_CELLS_PER_WG)), dim3(HM_BLOCK), lds, stream, z, codes, perm, start, m, n, y,
                     pen, term, R, delta, frac_unit(m), obj_fix, frac_obj, K, d, B, y_lds, tab_lds);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

inline int frac_objective(int64_t n) { return frac_unit(n) - 3; }  // a cell's terms stay below 8: |2 (1 - dot)| <= 4, |entropy| <= log 256

}  // namespace
}  // namespace scamd

using namespace scamd;

extern "C" size_t scamd_harmony_permutation_workspace_bytes(int64_t n) {
  (void)n;
  return 0;
}

extern "C" int scamd_harmony_permutation_i32(int64_t n, uint64_t seed, uint64_t round, int32_t* perm, void* workspace, size_t workspace_bytes,
                                             scamd_stream_t stream) {
  (void)workspace;
  (void)workspace_bytes;
  SCAMD_REQUIRE(n >= 1, SCAMD_EINVAL, "harmony_permutation: n=%lld", (long long)n);
  SCAMD_REQUIRE(n < ((int64_t)1 << 31), SCAMD_EUNSUPPORTED, "harmony_permutation: n=%lld exceeds int32 cell ids", (long long)n);
  SCAMD_REQUIRE(perm, SCAMD_EINVAL, "harmony_permutation: null output");
  int h = 1;
  while (((int64_t)1 << (2 * h)) < n) ++h;
  const uint64_t key = mix64(seed ^ mix64(round + 0x9E3779B97F4A7C15ull));
  hipLaunchKernelGGL(hm_permutation_kernel, dim3((unsigned)ceil_div(n, HM_BLOCK)), dim3(HM_BLOCK), 0, stream, n, key, h, perm);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

extern "C" int scamd_harmony_normalize_f64(const double* x, int64_t n, int d, double* z_norm, scamd_stream_t stream) {
  const int rc = check_shape("harmony_normalize", n, d, 1, 1, 1);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(x && z_norm, SCAMD_EINVAL, "harmony_normalize: null pointer");
  hipLaunchKernelGGL(hm_normalize_kernel, dim3((unsigned)ceil_div(n, HM_WAVES)), dim3(HM_BLOCK), 0, stream, x, n, d, z_norm);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

namespace {
struct KmeansWs {
  double* mind2;
  double* partial;
  long long* fix;
  unsigned long long* counts;  // [K] + 1: the labels that changed
  int32_t* sel;
  unsigned long long* absmax;
  int* frac;
  bool carve(Workspace& ws, int64_t n, int d, int K) {
    mind2 = ws.take<double>((size_t)n);
    partial = ws.take<double>((size_t)ceil_div(n, HM_KM_CHUNK));
    fix = ws.take<long long>((size_t)K * d);
    counts = ws.take<unsigned long long>((size_t)K + 1);
    sel = ws.take<int32_t>(1);
    absmax = ws.take<unsigned long long>(1);
    frac = ws.take<int>(1);
    return ws.ok;
  }
};
}  // namespace

extern "C" size_t scamd_harmony_kmeans_workspace_bytes(int64_t n, int d, int K) {
  if (n < 1 || d < 1 || K < 1 || d > HM_MAX_D || K > HM_MAX_K || n >= ((int64_t)1 << 31)) return 0;
  Workspace ws(nullptr, 0);
  KmeansWs w;
  w.carve(ws, n, d, K);
  return ws.used();
}

extern "C" int scamd_harmony_kmeans_f64(const double* z_norm, int64_t n, int d, int K, const double* uniforms_host, int max_iter, double* centroids,
                                        int32_t* labels, int* n_iter_host, void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  const int rc = check_shape("harmony_kmeans", n, d, K, 1, 1);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(z_norm && uniforms_host && centroids && labels, SCAMD_EINVAL, "harmony_kmeans: null pointer");
  SCAMD_REQUIRE(max_iter >= 0, SCAMD_EINVAL, "harmony_kmeans: max_iter=%d", max_iter);
  for (int c = 0; c < K; ++c)
    SCAMD_REQUIRE(uniforms_host[c] >= 0.0 && uniforms_host[c] < 1.0, SCAMD_EINVAL, "harmony_kmeans: uniform %d = %g outside [0, 1)", c, uniforms_host[c]);
  Workspace ws(workspace, workspace_bytes);
  KmeansWs w;
  w.carve(ws, n, d, K);
  SCAMD_REQUIRE(workspace && ws.ok && workspace_bytes >= ws.used(), SCAMD_EWORKSPACE, "harmony_kmeans: workspace %zu < required %zu", workspace_bytes,
                ws.used());
  const int64_t n_partial = ceil_div(n, HM_KM_CHUNK);
  // k-means++ seeding: centre c is drawn with probability proportional to the squared distance to the nearest earlier centre
  for (int c = 0; c < K; ++c) {
    if (c > 0) {
      hipLaunchKernelGGL(km_seed_update_kernel, dim3((unsigned)n_partial), dim3(HM_KM_CHUNK), 0, stream, z_norm, n, d, w.sel, c == 1 ? 1 : 0, w.mind2,
                         w.partial);
      SCAMD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(km_seed_pick_kernel, dim3(1), dim3(HM_BLOCK), 0, stream, z_norm, n, d, w.mind2, w.partial, n_partial, uniforms_host[c],
                       c == 0 ? 1 : 0, w.sel, centroids + (int64_t)c * d);
    SCAMD_LAUNCH_CHECK();
  }
  // Lloyd
  SCAMD_HIP_CHECK(hipMemsetAsync(labels, 0xff, (size_t)n * sizeof(int32_t), stream));  // -1: every cell changes in the first sweep
  SCAMD_HIP_CHECK(hipMemsetAsync(w.absmax, 0, sizeof(unsigned long long), stream));
  const int64_t count = n * d;
  const int grid = (int)(ceil_div(count, HM_BLOCK) < 4096 ? ceil_div(count, HM_BLOCK) : 4096);
  hipLaunchKernelGGL(hm_absmax_kernel, dim3((unsigned)grid), dim3(HM_BLOCK), 0, stream, z_norm, count, w.absmax);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_frac_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long*)w.absmax, (double)n, w.frac);
  SCAMD_LAUNCH_CHECK();
  const int y_lds = y_fits_lds(K, d);
  const size_t lds = y_lds ? (size_t)K * (d | 1) * sizeof(double) : 0;
  int it = 0;
  while (it < max_iter) {
    SCAMD_HIP_CHECK(hipMemsetAsync(w.counts, 0, ((size_t)K + 1) * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(km_assign_kernel, dim3((unsigned)ceil_div(n, HM_CELLS_PER_WG)), dim3(HM_BLOCK), lds, stream, z_norm, n, d, K, centroids, labels,
                       w.counts, w.counts + K, y_lds);
    SCAMD_LAUNCH_CHECK();
    ++it;
    unsigned long long changed = 0;
    SCAMD_READBACK_NOW(&changed, w.counts + K, sizeof(changed), stream);
    if (changed == 0ull) break;
    SCAMD_HIP_CHECK(hipMemsetAsync(w.fix, 0, (size_t)K * d * sizeof(long long), stream));
    hipLaunchKernelGGL(hm_wsum_kernel, dim3((unsigned)ceil_div(n, HM_WS_CHUNK), (unsigned)K), dim3(HM_BLOCK), wsum_lds_bytes(1, d), stream, (const double*)nullptr, 1, z_norm,
                       d, labels, K, n, w.frac, w.fix);
    SCAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_centre_kernel, dim3((unsigned)K), dim3(HM_MAX_D), 0, stream, w.fix, w.frac, w.counts, d, centroids);
    SCAMD_LAUNCH_CHECK();
  }
  if (n_iter_host) *n_iter_host = it;
  SCAMD_HIP_CHECK(hipStreamSynchronize(stream));
  return SCAMD_OK;
}

extern "C" size_t scamd_harmony_state_workspace_bytes(int64_t n, int d, int K, int n_levels) {
  if (n < 1 || d < 1 || K < 1 || n_levels < 1 || d > HM_MAX_D || K > HM_MAX_K || n_levels > HM_MAX_B) return 0;
  Workspace ws(nullptr, 0);
  StateWs w;
  w.carve(ws, d, K, n_levels);
  return ws.used();
}

extern "C" int scamd_harmony_init_f64(const double* z_norm, const int32_t* codes, int64_t n, int d, int K, int n_levels, int n_covariates,
                                      const double* centroids, const double* pr_b, const double* theta, double sigma, int stabilized, double* R,
                                      double* E, double* O, double* objective, void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  const int rc = check_shape("harmony_init", n, d, K, n_levels, n_covariates);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(z_norm && codes && centroids && pr_b && theta && R && E && O && objective, SCAMD_EINVAL, "harmony_init: null pointer");
  SCAMD_REQUIRE(sigma > 0.0, SCAMD_EINVAL, "harmony_init: sigma=%g", sigma);
  Workspace ws(workspace, workspace_bytes);
  StateWs w;
  w.carve(ws, d, K, n_levels);
  SCAMD_REQUIRE(workspace && ws.ok && workspace_bytes >= ws.used(), SCAMD_EWORKSPACE, "harmony_init: workspace %zu < required %zu", workspace_bytes,
                ws.used());
  const int B = n_levels;
  hipLaunchKernelGGL(hm_normalize_kernel, dim3((unsigned)ceil_div(K, HM_WAVES)), dim3(HM_BLOCK), 0, stream, centroids, (int64_t)K, d, w.y_norm);
  SCAMD_LAUNCH_CHECK();
  SCAMD_HIP_CHECK(hipMemsetAsync(w.delta, 0, (size_t)B * K * sizeof(long long), stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(w.obj_fix, 0, 2 * sizeof(long long), stream));
  const int fo = frac_objective(n);
  const int rc2 = launch_assign<HM_INIT>(z_norm, codes, nullptr, 0, n, n, w.y_norm, nullptr, -2.0 / sigma, R, w.delta, w.obj_fix, fo, K, d, B, stream);
  if (rc2 != SCAMD_OK) return rc2;
  hipLaunchKernelGGL(hm_tables_kernel, dim3(1), dim3(HM_BLOCK), 0, stream, w.delta, frac_unit(n), 0, pr_b, theta, stabilized, O, E, (double*)nullptr, K, B);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_objective_kernel, dim3(1), dim3(HM_BLOCK), 0, stream, w.obj_fix, fo, O, E, theta, sigma, stabilized, K, B, objective);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

extern "C" int scamd_harmony_cluster_round_f64(const double* z_norm, const int32_t* codes, int64_t n, int d, int K, int n_levels, int n_covariates,
                                               const int32_t* perm, int64_t n_blocks, const double* pr_b, const double* theta, double sigma,
                                               int stabilized, double* R, double* E, double* O, double* y_norm, double* objective, void* workspace,
                                               size_t workspace_bytes, scamd_stream_t stream) {
  const int rc = check_shape("harmony_cluster_round", n, d, K, n_levels, n_covariates);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(z_norm && codes && perm && pr_b && theta && R && E && O && y_norm && objective, SCAMD_EINVAL, "harmony_cluster_round: null pointer");
  SCAMD_REQUIRE(sigma > 0.0, SCAMD_EINVAL, "harmony_cluster_round: sigma=%g", sigma);
  SCAMD_REQUIRE(n_blocks >= 1 && n_blocks <= n, SCAMD_EINVAL, "harmony_cluster_round: %lld blocks for %lld cells", (long long)n_blocks, (long long)n);
  Workspace ws(workspace, workspace_bytes);
  StateWs w;
  w.carve(ws, d, K, n_levels);
  SCAMD_REQUIRE(workspace && ws.ok && workspace_bytes >= ws.used(), SCAMD_EWORKSPACE, "harmony_cluster_round: workspace %zu < required %zu",
                workspace_bytes, ws.used());
  const int B = n_levels;
  const double term = -2.0 / sigma;
  // centroids: Y = R^T Z_norm, rows normalised
  SCAMD_HIP_CHECK(hipMemsetAsync(w.y_fix, 0, (size_t)K * d * sizeof(long long), stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(w.delta, 0, (size_t)B * K * sizeof(long long), stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(w.obj_fix, 0, 2 * sizeof(long long), stream));
  hipLaunchKernelGGL(hm_frac_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long*)nullptr, (double)n, w.frac);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_wsum_kernel, dim3((unsigned)ceil_div(n, HM_WS_CHUNK), 1u), dim3(HM_BLOCK), wsum_lds_bytes(K, d), stream, (const double*)R, K, z_norm, d,
                     (const int32_t*)nullptr, 1, n, w.frac, w.y_fix);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_centroid_kernel, dim3((unsigned)K), dim3(HM_MAX_D), 0, stream, w.y_fix, w.frac, d, y_norm);
  SCAMD_LAUNCH_CHECK();
  // the blocks, one after another; their sizes are those of an even split: the first n % n_blocks blocks hold one cell more
  const int fo = frac_objective(n);
  const int64_t base = n / n_blocks, extra = n % n_blocks;
  int64_t start = 0;
  for (int64_t blk = 0; blk < n_blocks; ++blk) {
    const int64_t m = base + (blk < extra ? 1 : 0);
    int rcb = launch_assign<HM_SUMS>(z_norm, codes, perm, start, m, n, y_norm, nullptr, term, R, w.delta, w.obj_fix, fo, K, d, B, stream);
    if (rcb != SCAMD_OK) return rcb;
    hipLaunchKernelGGL(hm_tables_kernel, dim3(1), dim3(HM_BLOCK), 0, stream, w.delta, frac_unit(m), -1, pr_b, theta, stabilized, O, E, w.pen, K, B);
    SCAMD_LAUNCH_CHECK();
    rcb = launch_assign<HM_UPDATE>(z_norm, codes, perm, start, m, n, y_norm, w.pen, term, R, w.delta, w.obj_fix, fo, K, d, B, stream);
    if (rcb != SCAMD_OK) return rcb;
    hipLaunchKernelGGL(hm_tables_kernel, dim3(1), dim3(HM_BLOCK), 0, stream, w.delta, frac_unit(m), 1, pr_b, theta, stabilized, O, E, (double*)nullptr, K,
                       B);
    SCAMD_LAUNCH_CHECK();
    start += m;
  }
  hipLaunchKernelGGL(hm_objective_kernel, dim3(1), dim3(HM_BLOCK), 0, stream, w.obj_fix, fo, O, E, theta, sigma, stabilized, K, B, objective);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

namespace {
struct CorrectWs {
  long long* phi_fix;  // [K, B, d]
  double* W;           // [K, B, d]
  double* lambda_kb;   // [B, K]
  unsigned long long* absmax;
  int* frac;
  bool carve(Workspace& ws, int d, int K, int B) {
    phi_fix = ws.take<long long>((size_t)K * B * d);
    W = ws.take<double>((size_t)K * B * d);
    lambda_kb = ws.take<double>((size_t)B * K);
    absmax = ws.take<unsigned long long>(1);
    frac = ws.take<int>(1);
    return ws.ok;
  }
};
}  // namespace

extern "C" size_t scamd_harmony_correct_workspace_bytes(int64_t n, int d, int K, int n_levels) {
  if (n < 1 || d < 1 || K < 1 || n_levels < 1 || d > HM_MAX_D || K > HM_MAX_K || n_levels > HM_MAX_B) return 0;
  Workspace ws(nullptr, 0);
  CorrectWs w;
  w.carve(ws, d, K, n_levels);
  return ws.used();
}

extern "C" int scamd_harmony_correct_f64(const double* x, const int32_t* codes, int64_t n, int d, int K, int n_levels, int n_covariates, const double* R,
                                         const double* O, const double* E, const double* n_b, int dynamic_lambda, double alpha,
                                         double batch_prune_threshold, double ridge_lambda, double* z_hat, double* z_norm, double* lambda_kb_out,
                                         void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  const int rc = check_shape("harmony_correct", n, d, K, n_levels, n_covariates);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(x && codes && R && O && E && n_b && z_hat && z_norm, SCAMD_EINVAL, "harmony_correct: null pointer");
  Workspace ws(workspace, workspace_bytes);
  CorrectWs w;
  w.carve(ws, d, K, n_levels);
  SCAMD_REQUIRE(workspace && ws.ok && workspace_bytes >= ws.used(), SCAMD_EWORKSPACE, "harmony_correct: workspace %zu < required %zu", workspace_bytes,
                ws.used());
  const int B = n_levels;
  const int prune = batch_prune_threshold >= 0.0 ? 1 : 0;  // (negative: no pruning)
  hipLaunchKernelGGL(hm_lambda_kernel, dim3((unsigned)ceil_div((int64_t)B * K, HM_BLOCK)), dim3(HM_BLOCK), 0, stream, O, E, n_b, dynamic_lambda, alpha,
                     batch_prune_threshold, prune, ridge_lambda, K, B, w.lambda_kb);
  SCAMD_LAUNCH_CHECK();
  if (lambda_kb_out) SCAMD_HIP_CHECK(hipMemcpyAsync(lambda_kb_out, w.lambda_kb, (size_t)B * K * sizeof(double), hipMemcpyDeviceToDevice, stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(w.absmax, 0, sizeof(unsigned long long), stream));
  SCAMD_HIP_CHECK(hipMemsetAsync(w.phi_fix, 0, (size_t)K * B * d * sizeof(long long), stream));
  const int64_t count = n * d;
  const int grid = (int)(ceil_div(count, HM_BLOCK) < 4096 ? ceil_div(count, HM_BLOCK) : 4096);
  hipLaunchKernelGGL(hm_absmax_kernel, dim3((unsigned)grid), dim3(HM_BLOCK), 0, stream, x, count, w.absmax);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_frac_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long*)w.absmax, (double)n, w.frac);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_wsum_kernel, dim3((unsigned)ceil_div(n, HM_WS_CHUNK), (unsigned)B), dim3(HM_BLOCK), wsum_lds_bytes(K, d), stream, R, K, x, d, codes, B, n, w.frac,
                     w.phi_fix);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_ridge_kernel, dim3((unsigned)K), dim3(HM_MAX_D), 0, stream, w.phi_fix, w.frac, O, w.lambda_kb, K, B, d, w.W);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hm_apply_kernel, dim3((unsigned)ceil_div(n, HM_WAVES)), dim3(HM_BLOCK), 0, stream, x, codes, R, w.W, n, d, K, B, z_hat, z_norm);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}
