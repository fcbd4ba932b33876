// Marker genes (`tl.rank_genes_groups`): per-(group, gene) sums and Wilcoxon rank sums on the CSC copy of the cells x genes
// matrix.  One gene = one workgroup in both kernels; a gene's entries are gathered through codes[row].
//
// Every accumulation is an integer one (LDS atomics on 64-bit words), so the outputs do not depend on the order in which
// lanes, waves or workgroups run: two calls give the same bits.
//
//   group statistics  two sweeps over the column: max |value| (after the optional expm1), then the values rounded ONCE to
//                     64-bit fixed point with the column's own scale and added into the group's slot
//   rank sums         the column is cut into chunks of RG chunk entries; each chunk is sorted in LDS by a 64-bit key
//                     (bitonic network), and every stored entry then counts, by binary search in each sorted chunk of its
//                     column, the entries below it and equal to it.  The implicit zeros are one tie block handled in closed
//                     form.  No merge: rank sums need counts, not the sorted sequence.  A column that fits one chunk never
//                     leaves LDS; a longer one keeps its sorted chunks in the workspace.
//                     Cost for a column of L entries in C chunks: O(L log^2 chunk) for the sorts + O(L C log chunk) for the
//                     searches -- cheap while C is small, quadratic in L for a dense million-row column (a merge tree is the
//                     follow-up).
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

namespace scamd {

namespace {

constexpr int RG_BLOCK = 256;
constexpr int RG_MAX_GROUPS = SCAMD_RANK_GENES_MAX_GROUPS;
constexpr int RG_GROUPS_BIG_CHUNK = 1300;     // up to this many groups a chunk holds 4096 entries, beyond it 2048
constexpr int RG_SCRATCH_WORDS = 16;          // 64-bit words of per-column scalars in front of the LDS tables
constexpr unsigned long long RG_SENTINEL = ~0ull;  // key of an entry that does not take part; sorts behind every real key
constexpr unsigned int RG_ZERO_ORD = 0x80000000u;  // order-preserving bits of +0.0f
constexpr int64_t RG_MAX_CELLS = (int64_t)1 << 21;  // t^3 - t of a tie block of all cells stays below 2^63

// LDS of both kernels: [scratch 16 x 8 B][per group: 8 B + 8 B + 8 B][chunk x 8 B] <= 64 KiB
inline int chunk_entries(int n_groups) { return n_groups <= RG_GROUPS_BIG_CHUNK ? 4096 : 2048; }
inline size_t lds_bytes(int n_groups, int chunk) { return sizeof(unsigned long long) * ((size_t)RG_SCRATCH_WORDS + 3 * (size_t)n_groups + (size_t)chunk); }

__device__ __forceinline__ unsigned int ordered_bits(float v) {  // a < b  <=>  ordered_bits(a) < ordered_bits(b)
  const unsigned int u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// floor(62 - log2(p)) for p > 0 (a normal double): the number of fractional bits with which `count` values of magnitude
// <= absmax (p = count * absmax) add up below 2^62
__device__ __forceinline__ int scale_bits(double p) {
  if (!(p > 0.0)) return 0;
  const long long b = __double_as_longlong(p);
  const int fl = (int)((b >> 52) & 0x7ff) - 1023;  // floor(log2 p)
  const bool pow2 = (b & 0xfffffffffffffll) == 0;
  return pow2 ? 62 - fl : 61 - fl;
}

// transform 1: expm1(v * tscale) as a float32 value -- the product in float32, expm1 evaluated in float64 and rounded ONCE, i.e.
// the correctly rounded float32 result (the device's expm1f is off by a unit in the last place for about one value in ten; a
// t score of two nearly equal means of such values then moves by more than 1e-5 of itself)
__device__ __forceinline__ float rg_transform(float v, int transform, float tscale) {
  return transform == 1 ? (float)expm1((double)(v * tscale)) : v;
}

// sum[k, j], sumsq[k, j] (float64) and nnz[k, j] over the stored entries of gene j whose cell has code k
__global__ __launch_bounds__(RG_BLOCK) void rg_group_stats_kernel(const int64_t* __restrict__ t_indptr, const int32_t* __restrict__ t_indices,
                                                                  const float* __restrict__ t_data, int64_t n, int64_t g,
                                                                  const int32_t* __restrict__ codes, int n_groups, int transform,
                                                                  float tscale, double* __restrict__ sum, double* __restrict__ sumsq,
                                                                  int64_t* __restrict__ nnz) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long rg_smem[];
  unsigned int* s_absmax = reinterpret_cast<unsigned int*>(rg_smem);
  long long* s_sum = reinterpret_cast<long long*>(rg_smem + RG_SCRATCH_WORDS);
  long long* s_sq = s_sum + n_groups;
  unsigned long long* s_cnt = reinterpret_cast<unsigned long long*>(s_sq + n_groups);
  const int64_t j = blockIdx.x;
  const int64_t p0 = t_indptr[j], p1 = t_indptr[j + 1];
  const int tid = threadIdx.x;
  for (int k = tid; k < n_groups; k += RG_BLOCK) {
    s_sum[k] = 0;
    s_sq[k] = 0;
    s_cnt[k] = 0ull;
  }
  if (tid == 0) *s_absmax = 0u;
  __syncthreads();
  // sweep 1: max |value| after the transform (|float| bits compare as unsigned integers)
  unsigned int mx = 0u;
  for (int64_t p = p0 + tid; p < p1; p += RG_BLOCK) {
    const float v = t_data[p];
    const float tv = rg_transform(v, transform, tscale);
    const unsigned int a = __float_as_uint(tv) & 0x7fffffffu;
    mx = a > mx ? a : mx;
  }
  if (mx) atomicMax(s_absmax, mx);
  __syncthreads();
  const double absmax = (double)__uint_as_float(*s_absmax);
  const double cnt = (double)(p1 - p0);
  const int sb_sum = scale_bits(cnt * absmax), sb_sq = scale_bits(cnt * absmax * absmax);
  const double f_sum = ldexp(1.0, sb_sum), f_sq = ldexp(1.0, sb_sq);
  // sweep 2: one rounding per entry, integer adds
  for (int64_t p = p0 + tid; p < p1; p += RG_BLOCK) {
    const float v = t_data[p];
    if (v == 0.f) continue;  // a stored 0.0 / -0.0 is a zero
    const int64_t row = t_indices[p];
    if (row < 0 || row >= n) continue;
    const int k = codes[row];
    if (k < 0 || k >= n_groups) continue;
    const double tv = (double)rg_transform(v, transform, tscale);
    atomicAdd(reinterpret_cast<unsigned long long*>(&s_sum[k]), (unsigned long long)llrint(tv * f_sum));
    atomicAdd(reinterpret_cast<unsigned long long*>(&s_sq[k]), (unsigned long long)llrint(tv * tv * f_sq));
    atomicAdd(&s_cnt[k], 1ull);
  }
  __syncthreads();
  for (int k = tid; k < n_groups; k += RG_BLOCK) {
    const int64_t o = (int64_t)k * g + j;
    sum[o] = ldexp((double)s_sum[k], -sb_sum);
    sumsq[o] = ldexp((double)s_sq[k], -sb_sq);
    nnz[o] = (int64_t)s_cnt[k];
  }
}

// number of keys < key in the sorted array a[0, len)
__device__ __forceinline__ int lower_bound(const unsigned long long* a, int len, unsigned long long key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The sorted chunks of one column: chunk c = keys[c * chunk, (c + 1) * chunk) cut at len
struct SortedColumn {
  const unsigned long long* keys;
  int64_t len;
  int chunk;
  __device__ __forceinline__ int64_t below(unsigned long long key) const {  // entries of the column with a smaller key
    int64_t t = 0;
    for (int64_t b = 0; b < len; b += chunk) t += lower_bound(keys + b, len - b < chunk ? (int)(len - b) : chunk, key);
    return t;
  }
  // entries with this key in the whole column; *head: the entry at position `pos` is the first of them (lowest chunk, then
  // lowest slot) -- exactly one entry of every block of equal keys is its head
  __device__ __forceinline__ int64_t equal(unsigned long long key, int64_t pos, bool* head) const {
    int64_t eq = 0, eq_before = 0;
    int own_lb = -1;
    const int64_t own = pos / chunk * chunk;
    for (int64_t b = 0; b < len; b += chunk) {
      const int l = len - b < chunk ? (int)(len - b) : chunk;
      const int lo = lower_bound(keys + b, l, key), hi = lower_bound(keys + b, l, key + 1);
      if (b < own) eq_before += hi - lo;
      if (b == own) own_lb = lo;
      eq += hi - lo;
    }
    *head = eq_before == 0 && (int64_t)own_lb == pos - own;
    return eq;
  }
};

__device__ __forceinline__ unsigned long long tie_cube(unsigned long long t) { return t * t * t - t; }

// ranksum2[k, j] and the tie term of gene j (header: scamd_rank_genes_wilcoxon_f32).
//   reference < 0 ('rest'): key = ordered value bits << 32 | group; a block of equal VALUES is a key range [v << 32, (v + 1) << 32)
//   reference >= 0:         key = group << 32 | ordered value bits; a group's values are one sorted run, the reference's
//                           run is what every other group's entry searches
__global__ __launch_bounds__(RG_BLOCK) void rg_wilcoxon_kernel(const int64_t* __restrict__ t_indptr, const int32_t* __restrict__ t_indices,
                                                               const float* __restrict__ t_data, int64_t n, int64_t g,
                                                               const int32_t* __restrict__ codes, int n_groups,
                                                               const int64_t* __restrict__ group_sizes, int reference, int chunk,
                                                               int64_t* __restrict__ ranksum2, double* __restrict__ tie_term,
                                                               unsigned long long* __restrict__ ws_keys) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long rg_smem[];
  unsigned long long* s_scal = rg_smem;  // [0] participating cells, [1] their stored non-zeros, [2] negatives (of the reference), [3] first slot of the reference's run, [4] its length
  unsigned long long* s_rs = rg_smem + RG_SCRATCH_WORDS;
  unsigned long long* s_tie = s_rs + n_groups;
  unsigned long long* s_cnt = s_tie + n_groups;
  unsigned long long* s_keys = s_cnt + n_groups;
  const int64_t j = blockIdx.x;
  const int64_t p0 = t_indptr[j], p1 = t_indptr[j + 1], len = p1 - p0;
  const int tid = threadIdx.x;
  const bool rest = reference < 0;
  const bool want_tie = tie_term != nullptr;
  for (int k = tid; k < n_groups; k += RG_BLOCK) {
    s_rs[k] = 0ull;
    s_tie[k] = 0ull;
    s_cnt[k] = 0ull;
  }
  if (tid < RG_SCRATCH_WORDS) s_scal[tid] = 0ull;
  __syncthreads();
  unsigned long long part = 0ull;
  for (int k = tid; k < n_groups; k += RG_BLOCK) part += (unsigned long long)group_sizes[k];
  if (part) atomicAdd(&s_scal[0], part);

  // ---- phase 1: sort every chunk by key
  const bool in_lds = len <= chunk;  // the column is one chunk: it stays in LDS
  unsigned long long n_valid = 0ull;
  for (int64_t b = 0; b < len; b += chunk) {
    const int l = len - b < chunk ? (int)(len - b) : chunk;
    int sort_n = 2;  // the network's size: the power of two that holds the chunk
    while (sort_n < l) sort_n <<= 1;
    for (int i = tid; i < sort_n; i += RG_BLOCK) {
      unsigned long long key = RG_SENTINEL;
      if (i < l) {
        const int64_t p = p0 + b + i;
        const float v = t_data[p];
        const int64_t row = t_indices[p];
        if (v != 0.f && row >= 0 && row < n) {
          const int k = codes[row];
          if (k >= 0 && k < n_groups) {
            const unsigned long long vb = ordered_bits(v);
            key = rest ? (vb << 32 | (unsigned long long)k) : ((unsigned long long)k << 32 | vb);
            atomicAdd(&s_cnt[k], 1ull);
            ++n_valid;
          }
        }
      }
      s_keys[i] = key;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= sort_n; k2 <<= 1) {
      for (int d = k2 >> 1; d > 0; d >>= 1) {
        for (int t = tid; t < (sort_n >> 1); t += RG_BLOCK) {
          const int i = ((t / d) * 2 * d) + (t % d), m = i + d;
          const unsigned long long a = s_keys[i], c = s_keys[m];
          const bool up = (i & k2) == 0;
          if ((a > c) == up) {
            s_keys[i] = c;
            s_keys[m] = a;
          }
        }
        __syncthreads();
      }
    }
    if (!in_lds) {
      for (int i = tid; i < l; i += RG_BLOCK) ws_keys[p0 + b + i] = s_keys[i];
      __syncthreads();  // (the next chunk overwrites s_keys)
    }
  }
  if (n_valid) atomicAdd(&s_scal[1], n_valid);
  __threadfence();  // the sorted chunks in the workspace are read by the other lanes of this workgroup
  __syncthreads();

  SortedColumn col;
  col.keys = in_lds ? s_keys : ws_keys + p0;
  col.len = len;
  col.chunk = chunk;
  const unsigned long long ref_lo = (unsigned long long)(rest ? 0 : reference) << 32;
  if (tid == 0) {
    if (rest) {
      s_scal[2] = (unsigned long long)col.below((unsigned long long)RG_ZERO_ORD << 32);
    } else {
      const int64_t first = col.below(ref_lo);
      s_scal[3] = (unsigned long long)first;
      s_scal[4] = (unsigned long long)(col.below(ref_lo + ((unsigned long long)1 << 32)) - first);
      s_scal[2] = (unsigned long long)(col.below(ref_lo | RG_ZERO_ORD) - first);
    }
  }
  __syncthreads();
  const int64_t n_part = (int64_t)s_scal[0];
  const int64_t neg = (int64_t)s_scal[2];
  // zero cells: of all participating cells ('rest') / of the reference
  const int64_t zeros = rest ? n_part - (int64_t)s_scal[1] : group_sizes[reference] - (int64_t)s_scal[4];
  const int64_t ref_first = (int64_t)s_scal[3];

  // ---- phase 2: every stored entry counts what lies below it and what equals it
  for (int64_t pos = tid; pos < len; pos += RG_BLOCK) {
    const unsigned long long key = col.keys[pos];
    if (key == RG_SENTINEL) continue;
    if (rest) {
      const unsigned int vb = (unsigned int)(key >> 32);
      const int k = (int)(key & 0xffffffffu);
      const unsigned long long v_lo = (unsigned long long)vb << 32, v_hi = v_lo + ((unsigned long long)1 << 32);
      const int64_t less = col.below(v_lo) + (vb > RG_ZERO_ORD ? zeros : 0);
      const int64_t eq = col.below(v_hi) - col.below(v_lo);
      atomicAdd(&s_rs[k], (unsigned long long)(2 * less + eq + 1));
      if (want_tie) {
        // head of the value block = head of the block of equal keys of its lowest group: no smaller key with this value
        bool head;
        col.equal(key, pos, &head);
        if (head && col.below(key) == col.below(v_lo)) atomicAdd(&s_tie[0], tie_cube((unsigned long long)eq));
      }
    } else {
      const int k = (int)(key >> 32);
      const unsigned long long vb = key & 0xffffffffull;
      if (k == reference) {
        if (want_tie) {
          bool head;
          const int64_t t_r = col.equal(key, pos, &head);
          if (head) atomicAdd(&s_tie[k], tie_cube((unsigned long long)t_r));
        }
        continue;
      }
      const int64_t r_below = col.below(ref_lo | vb) - ref_first;
      const int64_t t_r = col.below((ref_lo | vb) + 1) - ref_first - r_below;
      const int64_t less = r_below + (vb > RG_ZERO_ORD ? zeros : 0);
      atomicAdd(&s_rs[k], (unsigned long long)(2 * less + t_r));
      if (want_tie) {
        bool head;
        const int64_t t_a = col.equal(key, pos, &head);
        if (head) atomicAdd(&s_tie[k], tie_cube((unsigned long long)(t_a + t_r)) - tie_cube((unsigned long long)t_r));
      }
    }
  }
  __syncthreads();

  // ---- the zero cells in closed form, and out
  for (int k = tid; k < n_groups; k += RG_BLOCK) {
    const int64_t o = (int64_t)k * g + j;
    const int64_t n_k = group_sizes[k], zeros_k = n_k - (int64_t)s_cnt[k];
    if (rest) {
      ranksum2[o] = (int64_t)s_rs[k] + zeros_k * (2 * neg + zeros + 1);
    } else if (k == reference) {
      ranksum2[o] = 0;
      if (want_tie) tie_term[o] = 0.0;
    } else {
      ranksum2[o] = n_k * (n_k + 1) + (int64_t)s_rs[k] + zeros_k * (2 * neg + zeros);
      if (want_tie) tie_term[o] = (double)(s_tie[k] + s_tie[reference] + tie_cube((unsigned long long)(zeros_k + zeros)));
    }
  }
  if (rest && want_tie && tid == 0) tie_term[j] = (double)(s_tie[0] + tie_cube((unsigned long long)zeros));
}

int check_common(const char* what, const void* t_indptr, const void* t_indices, const void* t_data, int64_t n, int64_t g, const void* codes,
                 int n_groups) {
  SCAMD_REQUIRE(n >= 0 && g >= 0 && n_groups >= 1, SCAMD_EINVAL, "%s: bad shape n=%lld g=%lld n_groups=%d", what, (long long)n, (long long)g,
                n_groups);
  SCAMD_REQUIRE(n < ((int64_t)1 << 31) && g < ((int64_t)1 << 31), SCAMD_EUNSUPPORTED, "%s: n or g exceeds int32 ids", what);
  SCAMD_REQUIRE(n_groups <= RG_MAX_GROUPS, SCAMD_EUNSUPPORTED, "%s: %d groups (remainder included) exceed the LDS tables (%d)", what, n_groups,
                RG_MAX_GROUPS);
  SCAMD_REQUIRE(t_indptr && (n == 0 || codes), SCAMD_EINVAL, "%s: null pointer", what);
  (void)t_indices;
  (void)t_data;
  return SCAMD_OK;
}

}  // namespace
}  // namespace scamd

using namespace scamd;

extern "C" size_t scamd_rank_genes_workspace_bytes(int64_t n, int64_t g, int64_t nnz, int n_groups) {
  if (n < 0 || g < 0 || nnz < 0 || n_groups < 1 || n_groups > RG_MAX_GROUPS) return 0;
  Workspace ws(nullptr, 0);
  ws.take<unsigned long long>((size_t)nnz);  // the sorted chunks of the columns longer than one chunk, in the CSC layout
  return ws.used();
}

extern "C" int scamd_rank_genes_chunk_entries(int n_groups) {
  if (n_groups < 1 || n_groups > RG_MAX_GROUPS) return 0;
  return chunk_entries(n_groups);
}

extern "C" int scamd_rank_genes_group_stats_f32(const int64_t* t_indptr, const int32_t* t_indices, const float* t_data, int64_t n, int64_t g,
                                                const int32_t* codes, int n_groups, int transform, double tscale, double* sum,
                                                double* sumsq, int64_t* nnz, void* workspace, size_t workspace_bytes,
                                                scamd_stream_t stream) {
  (void)workspace;
  (void)workspace_bytes;
  const int rc = check_common("rank_genes_group_stats", t_indptr, t_indices, t_data, n, g, codes, n_groups);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(transform == 0 || transform == 1, SCAMD_EINVAL, "rank_genes_group_stats: unknown transform %d", transform);
  SCAMD_REQUIRE(g == 0 || (sum && sumsq && nnz), SCAMD_EINVAL, "rank_genes_group_stats: null output");
  if (g == 0) return SCAMD_OK;
  int64_t total = 0;
  SCAMD_READBACK_NOW(&total, t_indptr + g, sizeof(total), stream);
  SCAMD_REQUIRE(total >= 0 && (total == 0 || (t_indices && t_data)), SCAMD_EINVAL, "rank_genes_group_stats: null matrix arrays");
  hipLaunchKernelGGL(rg_group_stats_kernel, dim3((unsigned)g), dim3(RG_BLOCK), lds_bytes(n_groups, 0), stream, t_indptr, t_indices, t_data, n, g,
                     codes, n_groups, transform, (float)tscale, sum, sumsq, nnz);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

extern "C" int scamd_rank_genes_wilcoxon_f32(const int64_t* t_indptr, const int32_t* t_indices, const float* t_data, int64_t n, int64_t g,
                                             const int32_t* codes, int n_groups, const int64_t* group_sizes, int reference,
                                             int64_t* ranksum2, double* tie_term, void* workspace, size_t workspace_bytes,
                                             scamd_stream_t stream) {
  const int rc = check_common("rank_genes_wilcoxon", t_indptr, t_indices, t_data, n, g, codes, n_groups);
  if (rc != SCAMD_OK) return rc;
  SCAMD_REQUIRE(group_sizes, SCAMD_EINVAL, "rank_genes_wilcoxon: null group sizes");
  SCAMD_REQUIRE(reference >= -1 && reference < n_groups, SCAMD_EINVAL, "rank_genes_wilcoxon: reference %d outside [-1, %d)", reference, n_groups);
  SCAMD_REQUIRE(g == 0 || ranksum2, SCAMD_EINVAL, "rank_genes_wilcoxon: null output");
  SCAMD_REQUIRE(n <= RG_MAX_CELLS, SCAMD_EUNSUPPORTED, "rank_genes_wilcoxon: n=%lld exceeds %lld (the tie term of one block of all cells)",
                (long long)n, (long long)RG_MAX_CELLS);
  if (g == 0) return SCAMD_OK;
  int64_t total = 0;
  SCAMD_READBACK_NOW(&total, t_indptr + g, sizeof(total), stream);
  SCAMD_REQUIRE(total >= 0 && (total == 0 || (t_indices && t_data)), SCAMD_EINVAL, "rank_genes_wilcoxon: null matrix arrays");
  Workspace ws(workspace, workspace_bytes);
  unsigned long long* keys = ws.take<unsigned long long>((size_t)total);
  SCAMD_REQUIRE((workspace || ws.used() == 0) && ws.ok && workspace_bytes >= ws.used(), SCAMD_EWORKSPACE, "rank_genes_wilcoxon: workspace %zu < required %zu", workspace_bytes,
                ws.used());
  const int chunk = chunk_entries(n_groups);
  hipLaunchKernelGGL(rg_wilcoxon_kernel, dim3((unsigned)g), dim3(RG_BLOCK), lds_bytes(n_groups, chunk), stream, t_indptr, t_indices, t_data, n, g,
                     codes, n_groups, group_sizes, reference, chunk, ranksum2, tie_term, keys);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}
