// Leiden community detection on gfx950: wave-per-vertex label moves over the CSR neighbour graph.
//
// Replaces leidenalg.find_partition(RBConfigurationVertexPartition) / igraph community_leiden
// (objective 'modularity') as called at src/scanpy/tools/_leiden.py:167-196 on the graph built by
// src/scanpy/_utils/__init__.py:278-304.  Same three phases as Traag et al. 2019,
// re-designed for a GPU:
//   1. local moving   -- SWEEPS of K class sub-rounds (K = 8 on large levels): the active vertices of a sweep are split
//                        into K hash classes; sub-round r decides (one wave / half / quarter wave per vertex: weight
//                        towards each neighbouring community in an LDS hash, best move from a snapshot of the community
//                        totals) and applies the moves of class r only, so class r + 1 sees them -- a deterministic
//                        stand-in for the sequential queue: every sub-round is a synchronous step on a snapshot, the
//                        classes are re-drawn every sweep, only vertices next to a change stay active.
//   2. refinement     -- ONE sweep of K class sub-rounds over the well-connected singletons of each community
//                        (leidenalg visits every vertex exactly once, in random order): the singletons of class r merge
//                        into a well-connected sub-community drawn with probability ~ exp(gain / beta); targets are
//                        grown sub-communities and singletons of OTHER classes, so simultaneous merges cannot chain.
//   3. aggregation    -- members of every coarse node gathered contiguously, one wave / workgroup per coarse node
//                        combines their rows in an LDS hash.
// ALL weight sums are 64-bit fixed point (weight * 2^32): integer addition is associative, so atomic
// accumulation order cannot change any result -- labels are bitwise reproducible run to run.
// Memory-latency / gather bound: per round ~E*(4+8+4) B of edge data + n*24 B of vertex data.
#include "common.h"
#include "scan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include <type_traits>

namespace scamd {

// Per-call statistics of the last Leiden run on this thread (scamd_leiden_last_stats; scamd_leiden_stat_name gives the key of a
// slot, the Python layers build their dicts from it).  What the keys of LD_STAT_NAMES do not say:
//   ST_LM_SWEEPS / ST_LM_SWEEP_MB  the levels that run as separate kernels, all iterations; the traffic is algorithmic: active
//                                   rows x (12 B per entry + 16 B per vertex), SURVEY.md 8(d)'s per-sweep figure restricted to
//                                   the rows a sweep visits
//   ST_POLISH_SKIPPED_PROVEN       the last iteration had already proven node optimality
//   ST_POLISH_SPLITS               communities the polish split off because a departure had cut them in two
//   ST_POLISH_ROUND_CAP            a polish pass stopped at MAX_POLISH_ROUNDS: node optimality then NOT proven
//   ST_LEVELS_REUSED               levels that took their coarse graph from the stored hierarchy (StoredLevel) instead of
//                                   refining and aggregating
//   ST_QUIET_REUSE_ITERS           iterations that ran on the stored hierarchy to its end without a move at any level
//   ST_L0_QUALITY_WALKS            launches of ld_internal_kernel over the level-0 graph (the quality after a polish pass, of a
//                                   given start partition, of an iteration that ended on level 0, the modularity report of a
//                                   CPM run); slot 14 has no key: the key
//                                   set is part of the Python layers' dicts, the slot is read by its number
//   ST_OVERFLOW_VERTICES / ST_HUB_VERTICES  rows too long for the main tier of a 16- / 32-lane decide launch (the wave-per-row
//                                   tier takes them, or a workgroup tier) / rows longer than the wave table: block tier and
//                                   giant tier together (decide_tiers: local moving, polish and refinement together; the
//                                   list builders' counts, so no read-back of their own)
enum LdStat : int {
  ST_ITERATIONS = 0, ST_LAUNCHES, ST_ROUND_TRIPS, ST_POLISH_FULL_SWEEPS, ST_POLISH_ROUNDS, ST_POLISH_MOVES,
  ST_POLISH_SKIPPED_PROVEN, ST_LEVELS_FIRST_ITER, ST_LM_SWEEPS, ST_LM_SWEEP_MB, ST_POLISH_SPLITS, ST_ENDED_BY_ITER_CAP,
  ST_POLISH_ROUND_CAP, ST_ITER_CAP, ST_L0_QUALITY_WALKS, ST_DEVICE_FILLS, ST_LEVELS_REUSED, ST_QUIET_REUSE_ITERS,
  ST_OVERFLOW_VERTICES, ST_HUB_VERTICES, LD_NSTATS
};
static_assert(LD_NSTATS == 20 && ST_L0_QUALITY_WALKS == 14, "the slot numbers are part of the C ABI (scamd_leiden_last_stats)");
struct LdStatName {
  int slot;
  const char* key;
};
static const LdStatName LD_STAT_NAMES[] = {
    {ST_ITERATIONS, "iterations"},
    {ST_LAUNCHES, "launches"},
    {ST_ROUND_TRIPS, "host_round_trips"},
    {ST_POLISH_FULL_SWEEPS, "polish_full_sweeps"},
    {ST_POLISH_ROUNDS, "polish_rounds"},
    {ST_POLISH_MOVES, "polish_moves"},
    {ST_POLISH_SKIPPED_PROVEN, "polish_skipped_proven"},
    {ST_LEVELS_FIRST_ITER, "levels_first_iteration"},
    {ST_LM_SWEEPS, "lm_sweeps"},
    {ST_LM_SWEEP_MB, "lm_sweep_algorithmic_MB"},
    {ST_POLISH_SPLITS, "polish_splits"},
    {ST_ENDED_BY_ITER_CAP, "ended_by_iteration_cap"},
    {ST_POLISH_ROUND_CAP, "polish_ended_by_round_cap"},
    {ST_ITER_CAP, "iteration_cap"},
    {ST_DEVICE_FILLS, "device_fills"},
    {ST_LEVELS_REUSED, "levels_reused"},
    {ST_QUIET_REUSE_ITERS, "quiet_reuse_iterations"},
    {ST_OVERFLOW_VERTICES, "overflow_pass_vertices"},
    {ST_HUB_VERTICES, "hub_pass_vertices"},
};
// table slots of a vertex of the sixteen-lanes-per-vertex kernels (the kNN graph itself); rows longer than 3/4 of them go to
// the wave-per-vertex tier
constexpr int G16_SLOTS = 128;
constexpr int G16_MAX = G16_SLOTS * 3 / 4;
static thread_local int g_ld_stats[LD_NSTATS] = {0};
static thread_local double g_ld_sweep_bytes = 0.0;  // -> ST_LM_SWEEP_MB
#undef SCAMD_LAUNCH_CHECK
#define SCAMD_LAUNCH_CHECK()                \
  do {                                      \
    ++g_ld_stats[ST_LAUNCHES];              \
    SCAMD_HIP_CHECK(hipGetLastError());     \
  } while (0)
// host round trips: the values the host decides on are fetched into a pinned page (common.h: HostReadback -- a copy into
// pageable memory is a blocking round trip of its own) and handed out by ONE synchronisation
#define LD_FETCH(dst, src, bytes, stream)                                          \
  do {                                                                             \
    const int rc_fetch_ = host_readback().fetch((dst), (src), (bytes), (stream)); \
    if (rc_fetch_ != SCAMD_OK) return rc_fetch_;                                   \
  } while (0)
#define LD_SYNC(stream)                                       \
  do {                                                        \
    ++g_ld_stats[ST_ROUND_TRIPS];                             \
    const int rc_sync_ = host_readback().sync(stream);        \
    if (rc_sync_ != SCAMD_OK) return rc_sync_;                \
  } while (0)

constexpr double WSCALE = 4294967296.0;  // 2^32
constexpr int MAX_LM_SWEEPS = 96;
constexpr int LM_DIR_AFTER = 32;  // sweeps after which the direction rule (termination guarantee) is switched on
constexpr int MAX_CLASSES = 32;   // most class sub-rounds per sweep (local moving) / per refinement
constexpr int DEF_CLASSES = 8;    // default
constexpr int CTR_STRIDE = 16;    // ints per sub-round counter block:
// [CTR_JOINED] joiners of the sub-round (refinement); the lengths of the class's tier lists, counted while the class lists
// are built (list_long_rows): [CTR_N_MID] rows of the wave-per-row tier (longer than the lanes-per-vertex table), [CTR_N_BLK] of
// the block tier (longer than the wave table), [CTR_N_GIANT] of the giant tier (longer than the block tier's table)
constexpr int CTR_JOINED = 0, CTR_N_MID = 8, CTR_N_BLK = 9, CTR_N_GIANT = 10;
// Phase counters (LeidenBuffers::counters, 16 ints), by the phase that owns a slot.  Slots [0, PH_PER_PHASE) are cleared when a
// phase begins (local_moving, polish_level0, refinement, aggregate / reuse_level: one after the other, never overlapping).
// The component split runs INSIDE a polish pass and clears its own three slots only: it must leave PH_MOVED, PH_BLOCKED and
// PHASE_ERR alone, and nothing of the aggregation is live then.
constexpr int PH_PER_PHASE = 8;
constexpr int PH_MOVED = 0, PH_BLOCKED = 1;  // local moving, polish: moves / blocked (polish: lost the lock), cumulative over the phase
constexpr int PH_CC_CHANGED = 2, PH_CC_COMPONENTS = 3, PH_CC_COMMUNITIES = 4;  // component split (split_disconnected)
// aggregation: pmoff slots handed out, parts of split rows, rows of the 512-thread tier, of the 1024-thread tier, split rows
constexpr int PH_AGG_PART_SLOTS = 2, PH_AGG_PARTS = 3, PH_AGG_MID = 4, PH_AGG_BIG = 5, PH_AGG_SPLIT = 6;
constexpr int PHASE_ERR = 7;      // every phase: raised by a kernel when a table overflows (and by the input checks of an entry)
constexpr int PH_MAX_DEG = 8;     // longest row of the level being built (ld_degstats_kernel)
// written by ld_small_levels_kernel through SmallArgs::info = counters + PH_SMALL_INFO
constexpr int PH_SMALL_INFO = 12, SM_INFO_LEVELS = 0, SM_INFO_MOVES = 1, SM_INFO_MERGES = 2, SM_INFO_NODES = 3;
// counter area of a sweep / a refinement: MAX_CLASSES class-list lengths, then one CTR_STRIDE block per sub-round
constexpr int CTR_AREA = MAX_CLASSES + CTR_STRIDE * MAX_CLASSES;
constexpr int MAX_LEVELS = 64;
// Outer iterations of an `n_iterations < 0` run ("until an iteration does not improve", src/scanpy/tools/_leiden.py:65, 166).
// On graphs without clear communities that takes dozens of iterations in the sequential algorithm as well: oracle/leiden.c
// needs 44 on the 1M-cell `weak` graph of bench.py (gains of 1e-7 .. 1e-5 Q per iteration from the 6th on; round-6 probe,
// profiles/r06a_oracle_iters_weak.log), 18 on a 100k sample.  The loop is bounded (SCAMD_LEIDEN_ITER_CAP overrides); a run the
// bound ends sets ST_ENDED_BY_ITER_CAP and `tl.leiden` warns.
constexpr int MAX_OUTER_ITERS = 32;

__host__ __device__ __forceinline__ unsigned int hash32(unsigned int x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ unsigned int prio(int c, unsigned int seed) { return hash32((unsigned int)c ^ seed); }

__device__ __forceinline__ long long readlane_i64(long long v, int l) {
  int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffll), l);
  int hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
  return ((long long)hi << 32) | (unsigned int)lo;
}

// ---- small utility kernels -----------------------------------------------------------------------
// Level 0 in one pass over the graph, sixteen lanes per row (four rows in flight per wave): wq = the weights in fixed point
// (llrint(w * 2^32), 0 for w <= 0: what ld_quantize_kernel did in a pass of its own),
// k[v] = sum of row v, diag[0] += the stored diagonal entries (the internal weight of the singleton partition; zeroed by the
// caller; integer: order free)
__global__ __launch_bounds__(256) void ld_level0_setup_kernel(const int64_t* __restrict__ indptr, const int* __restrict__ indices,
                                                              const float* __restrict__ w, int n, long long* __restrict__ wq,
                                                              long long* __restrict__ k, unsigned long long* __restrict__ diag) {
  const int lane = threadIdx.x & 63, sub = threadIdx.x & 15;
  const int v = blockIdx.x * 16 + (threadIdx.x >> 4);
  long long s = 0, d = 0;
  if (v < n) {
    const int64_t end = indptr[v + 1];
    for (int64_t e = indptr[v] + sub; e < end; e += 16) {
      const double x = (double)w[e];
      const long long q = (x > 0.0) ? (long long)llrint(x * WSCALE) : 0ll;
      wq[e] = q;
      s += q;
      if (indices[e] == v) d += q;
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (v < n && sub == 0) k[v] = s;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
  __shared__ long long sh_d[4];
  if (lane == 0) sh_d[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long tot = sh_d[0] + sh_d[1] + sh_d[2] + sh_d[3];
    if (tot != 0) atomicAdd(diag, (unsigned long long)tot);
  }
}

// one wave per row: k[v] = sum of row
__global__ void ld_strength_kernel(const int64_t* __restrict__ indptr, const long long* __restrict__ wq, int n,
                                   long long* __restrict__ k) {
  const int lane = threadIdx.x & 63;
  const int v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (v >= n) return;
  long long s = 0;
  for (int64_t e = indptr[v] + lane; e < indptr[v + 1]; e += 64) s += wq[e];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) k[v] = s;
}

// total += sum a[0..n)  (grid-stride, one atomic per wave; integer => order independent)
__global__ __launch_bounds__(256) void ld_sum_kernel(const long long* __restrict__ a, int n,
                                                     unsigned long long* __restrict__ total) {
  long long s = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s += a[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(total, (unsigned long long)s);
}

// out[0] = max(out[0], longest row of the level): levels without hubs skip the block-per-vertex kernels
__global__ __launch_bounds__(1024) void ld_degstats_kernel(const int64_t* __restrict__ indptr, int n, int* __restrict__ out) {
  // (one atomic per 1024-row block: a million rows through same-address atomics per WAVE took 0.3 ms)
  __shared__ int sh;
  if (threadIdx.x == 0) sh = 0;
  __syncthreads();
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  int d = (v < n) ? (int)(indptr[v + 1] - indptr[v]) : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d = max(d, __shfl_xor(d, o));
  if ((threadIdx.x & 63) == 0 && d > 0) atomicMax(&sh, d);
  __syncthreads();
  if (threadIdx.x == 0 && sh > 0) atomicMax(out, sh);
}

__global__ void ld_iota_kernel(int* __restrict__ a, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = i;
}

// CPM with the caller's vertex weights (igraph `node_weights`): fixed point with 16 fractional bits; a negative or non-finite
// weight raises the flag (the host turns it into SCAMD_EINVAL)
constexpr double NODE_WEIGHT_SCALE = 65536.0;
__global__ void ld_nodeweight_quantize_kernel(const float* __restrict__ w, int n, long long* __restrict__ k, int* __restrict__ err) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const float x = w[v];
  if (!(x >= 0.f) || !(x <= 1.0e6f)) {  // (the totals are int64 sums of 2^16 x: 1e6 x 1e8 vertices still fit)
    atomicOr(err, 1);
    k[v] = 0ll;
    return;
  }
  k[v] = llrint((double)x * NODE_WEIGHT_SCALE);
}
__global__ void ld_fill_i64_kernel(long long* __restrict__ a, int n, long long v) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = v;
}
// coarse vertex weights of CPM: kout[cid[v]] += k[v]  (kout zeroed by the caller; integer: order free)
__global__ void ld_agg_nodeweight_kernel(int n, const int* __restrict__ cid, const long long* __restrict__ k,
                                         long long* __restrict__ kout) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) atomicAdd(reinterpret_cast<unsigned long long*>(&kout[cid[v]]), (unsigned long long)k[v]);
}

__global__ void ld_fill_u8_kernel(unsigned char* __restrict__ a, int n, unsigned char v) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = v;
}

// Clears of the orchestration (round 6).  Every hipMemsetAsync / device-to-device hipMemcpyAsync is a blit kernel of the
// runtime (`__amd_rocclr_fillBufferAligned` / `__amd_rocclr_copyBuffer`: 365 launches and 4.35 ms per pass of the path in the
// round-5 profile).  What could not be folded into a kernel that is launched anyway (per-vertex initialisations, the counter
// blocks of the next sweep) goes through ONE launch of this kernel per phase: up to six regions, each filled with its own
// 32-bit pattern (0, 0x7f7f7f7f = the `memset 0x7f` sentinel of the atomicMin targets, 0xffffffff).
struct FillArgs {
  static constexpr int MAX_REGIONS = 6;
  unsigned int* p[MAX_REGIONS];
  unsigned long long words[MAX_REGIONS];
  unsigned int pat[MAX_REGIONS];
  int n;
};
__global__ __launch_bounds__(256) void ld_fill_kernel(FillArgs a) {
  const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x, stride = (unsigned long long)gridDim.x * 256ull;
  for (int r = 0; r < a.n; ++r) {
    const unsigned long long words = a.words[r];
    const unsigned int pat = a.pat[r];
    unsigned int* __restrict__ p = a.p[r];
    // (regions are carved on 256-byte boundaries: whole 16-byte stores, then the tail)
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
      const unsigned long long quads = words >> 2;
      uint4* __restrict__ q = reinterpret_cast<uint4*>(p);
      for (unsigned long long i = t; i < quads; i += stride) q[i] = make_uint4(pat, pat, pat, pat);
      for (unsigned long long i = (quads << 2) + t; i < words; i += stride) p[i] = pat;
    } else {
      for (unsigned long long i = t; i < words; i += stride) p[i] = pat;
    }
  }
}
// start of an outer iteration: comm = the partition it starts from, node_of = identity
__global__ void ld_iter_init_kernel(int n, const int* __restrict__ memb, int* __restrict__ comm, int* __restrict__ node_of) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) {
    comm[v] = memb[v];
    node_of[v] = v;
  }
}
__global__ void ld_copy_i32_kernel(int n, const int* __restrict__ src, int* __restrict__ dst) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) dst[v] = src[v];
}
// memb[v] = init[v]; *err |= 1 when an id lies outside [0, n)
__global__ void ld_copy_membership_kernel(int n, const int* __restrict__ init, int* __restrict__ memb, int* __restrict__ err) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int c = init[v];
  if (c < 0 || c >= n) {
    atomicOr(err, 1);
    memb[v] = v;
  } else {
    memb[v] = c;
  }
}

// ---- block-local pre-aggregation of per-community reductions ---------------------------------------
// Late in the optimisation a million vertices reduce into a few dozen communities: a global atomic per vertex
// serialises on those few L2 lines (~12 ns each).  Every 1024-thread block first combines its vertices in an LDS
// hash table (open addressing, <= 8 probes; a vertex that finds no slot goes to global memory directly) and then
// issues one global atomic per distinct community it saw.  All reductions are integer (+, min): order free.
constexpr int BH_SLOTS = 2048;
constexpr int BH_EMPTY = -1;
// Most workgroups that may touch one counter word in a launch, once each ("hot words"): the list
// builders, the apply kernels and the coarse-id reductions.  Device-scope atomics on one address run one after the other
// (~85 ns each), so a launch whose every workgroup ends on the same word lasts workgroups x 85 ns whatever it moves.
// SCAMD_LEIDEN_COUNT_GRID (1 .. COUNT_GRID_MAX) overrides it, so that a test graph of a few thousand vertices has span boundaries.
constexpr int COUNT_GRID = 128;
constexpr int COUNT_GRID_MAX = 256;

__device__ __forceinline__ int bh_find_slot(int* keys, int c) {
  unsigned int slot = hash32((unsigned int)c) & (BH_SLOTS - 1);
  for (int probe = 0; probe < 8; ++probe) {
    const int prev = atomicCAS(&keys[slot], BH_EMPTY, c);
    if (prev == BH_EMPTY || prev == c) return (int)slot;
    slot = (slot + 1) & (BH_SLOTS - 1);
  }
  return -1;
}

// Ktot[c] = sum k[v], csize[c] = #members   (both zeroed by the caller)
__global__ __launch_bounds__(1024) void ld_totals_kernel(const int* __restrict__ comm, const long long* __restrict__ k, int n,
                                                         unsigned long long* __restrict__ Ktot, int* __restrict__ csize,
                                                         unsigned long long* __restrict__ zero_me) {
  __shared__ int keys[BH_SLOTS];
  if (zero_me && blockIdx.x == 0 && threadIdx.x == 0) *zero_me = 0ull;  // (the internal-weight accumulator of `quality`)
  __shared__ unsigned long long ksum[BH_SLOTS];
  __shared__ int cnt[BH_SLOTS];
  for (int i = threadIdx.x; i < BH_SLOTS; i += 1024) {
    keys[i] = BH_EMPTY;
    ksum[i] = 0ull;
    cnt[i] = 0;
  }
  __syncthreads();
  // (at most COUNT_GRID workgroups walk the vertices: with a few dozen communities left, every workgroup ends with one
  // global atomic per community on the same few lines -- 977 workgroups at 1M vertices took 85 us, round 5 profile)
  for (int v = blockIdx.x * 1024 + threadIdx.x; v < n; v += gridDim.x * 1024) {
    const int c = comm[v];
    const int slot = bh_find_slot(keys, c);
    if (slot >= 0) {
      atomicAdd(&ksum[slot], (unsigned long long)k[v]);
      atomicAdd(&cnt[slot], 1);
    } else {
      atomicAdd(&Ktot[c], (unsigned long long)k[v]);
      atomicAdd(&csize[c], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BH_SLOTS; i += 1024) {
    const int c = keys[i];
    if (c != BH_EMPTY) {
      atomicAdd(&Ktot[c], ksum[i]);
      atomicAdd(&csize[c], cnt[i]);
    }
  }
}

// ---- wave-wide argmax helper ---------------------------------------------------------------------
struct Cand {
  double val;
  int c;
  unsigned int pr;
};
__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b) {  // is a better than b
  if (a.c < 0) return false;
  if (b.c < 0) return true;
  if (a.val != b.val) return a.val > b.val;
  if (a.pr != b.pr) return a.pr < b.pr;
  return a.c < b.c;
}
__device__ __forceinline__ Cand cand_none() { return Cand{0.0, -1, 0u}; }
// best candidate of the G lanes that work on one vertex (G = 64: of the wave), in every one of them
template <int G>
__device__ __forceinline__ Cand group_best(Cand x) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    Cand y;
    y.val = __shfl_xor(x.val, o);
    y.c = __shfl_xor(x.c, o);
    y.pr = (unsigned int)__shfl_xor((int)x.pr, o);
    if (cand_better(y, x)) x = y;
  }
  return x;
}
__device__ __forceinline__ Cand wave_best(Cand x) { return group_best<64>(x); }
template <int G>
__device__ __forceinline__ long long group_max(long long x) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o));
  return x;
}

// ---- per-wave LDS hash: weight towards each distinct neighbouring group --------------------------------
// A vertex with <= WH_MAX_DEG neighbours accumulates sum_w per distinct group id (community / refined community)
// in a 128-slot open-addressing table private to its wave: O(deg) LDS atomics instead of the O(deg^2) all-pairs
// readlane compare (which remains the path for the few high-degree coarse vertices).  Integer adds: the sums do
// not depend on the order of insertion; the table is read back two slots per lane.
constexpr int WH_SLOTS = 512;    // per wave (6 KB); a vertex uses the first 128 / 256 / 512 of them
constexpr int WH_MAX_DEG = 384;
constexpr int WH_EMPTY = -1;

struct WaveHash {
  int* keys;                 // [WH_SLOTS]
  unsigned long long* vals;  // [WH_SLOTS]
  int nslots;                // power of two >= 1.33 * deg
  __device__ __forceinline__ void size_for(int deg) { nslots = deg <= 96 ? 128 : (deg <= 192 ? 256 : 512); }
  __device__ __forceinline__ void clear(int lane) {
    for (int i = lane; i < nslots; i += 64) {
      keys[i] = WH_EMPTY;
      vals[i] = 0ull;
    }
  }
  __device__ __forceinline__ void add(int c, long long w) {
    unsigned int slot = hash32((unsigned int)c) & (nslots - 1);
    for (;;) {
      const int prev = atomicCAS(&keys[slot], WH_EMPTY, c);
      if (prev == WH_EMPTY || prev == c) break;
      slot = (slot + 1) & (nslots - 1);
    }
    atomicAdd(&vals[slot], (unsigned long long)w);
  }
  __device__ __forceinline__ int key(int slot) const { return __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ long long val(int slot) const {
    return (long long)__hip_atomic_load(&vals[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

// ---- high-degree vertices: one workgroup per vertex, 8192-slot LDS table ---------------------------------
// kNN graphs have hubs (in-degree in the thousands) and aggregated graphs are dense: the wave-per-vertex kernels
// leave every vertex with more than WH_MAX_DEG neighbours to a workgroup per vertex (the block tier of the fused decide
// launch up to BLK_MAX_DEG entries, these kernels beyond; lists written by list_long_rows) instead of letting ONE wave
// grind through an O(deg^2) compare while the grid waits.
constexpr int BHUB_SLOTS = 8192;
constexpr int BHUB_MAX_DEG = 6000;  // longest row one pass of the table takes (load <= 0.73)
// Longer rows (the coarse levels of a weakly clustered graph are nearly dense: 20k vertices with up to 18k
// neighbours each) are swept in P = ceil(deg / BHUB_PASS_DEG) passes: pass p only sees the neighbour groups of hash
// class p, so a pass holds ~deg / P <= 3072 distinct keys.  (Round 1 sent such rows through an all-pairs
// readlane compare, O(deg^2): 1.6 s for ONE local-moving round of a 26k-vertex level, 43 s per Leiden call on a
// structure-less 1M-cell graph.)
constexpr int BHUB_PASS_DEG = 3072;
__device__ __forceinline__ int bhub_passes(int deg) { return deg <= BHUB_MAX_DEG ? 1 : (deg + BHUB_PASS_DEG - 1) / BHUB_PASS_DEG; }
__device__ __forceinline__ int bhub_class(int c, int n_pass) {
  return (int)((hash32((unsigned int)c * 0x9E3779B1u + 0x7F4A7C15u) >> 7) % (unsigned int)n_pass);
}
// The pass count of a long row is set by its LENGTH (the only bound on its distinct neighbour groups known in advance), but
// on the coarse levels where such rows live the groups are few: a row of 19 000 entries pointing at a few hundred
// communities was swept seven times (round 5 profile of the structure-less graph: ld_move_hub_kernel 20 % of the Leiden time, a
// launch lasting as long as its longest row).  So a multi-pass row first tries ONE pass into the whole table with bounded
// probing; only if some key finds no slot within HUB_TRY_PROBES steps is the table cleared and the row swept class by class.
constexpr int HUB_TRY_PROBES = 64;

struct BlockHash {
  int* keys;
  unsigned long long* vals;
  int nslots;  // power of two >= 2 * deg (256 .. cap): clearing and scanning cost O(deg), not O(table)
  int cap = BHUB_SLOTS;  // slots behind keys / vals (the block tier of the fused decide kernels: BLK_SLOTS)
  __device__ __forceinline__ void size_for(int deg) {
    int s = 256;
    while (s < 2 * deg && s < cap) s <<= 1;
    nslots = s;
  }
  __device__ __forceinline__ void clear() {
    for (int i = threadIdx.x; i < nslots; i += blockDim.x) {
      keys[i] = WH_EMPTY;
      vals[i] = 0ull;
    }
  }
  __device__ __forceinline__ void add(int c, long long w) {
    unsigned int slot = hash32((unsigned int)c) & (nslots - 1);
    for (;;) {
      const int prev = atomicCAS(&keys[slot], WH_EMPTY, c);
      if (prev == WH_EMPTY || prev == c) break;
      slot = (slot + 1) & (nslots - 1);
    }
    atomicAdd(&vals[slot], (unsigned long long)w);
  }
  // optimistic single pass over a long row (see hub_row): gives up after max_probes occupied slots
  __device__ __forceinline__ bool add_limited(int c, long long w, int max_probes) {
    unsigned int slot = hash32((unsigned int)c) & (nslots - 1);
    for (int probes = 0; probes < max_probes; ++probes) {
      const int prev = atomicCAS(&keys[slot], WH_EMPTY, c);
      if (prev == WH_EMPTY || prev == c) {
        atomicAdd(&vals[slot], (unsigned long long)w);
        return true;
      }
      slot = (slot + 1) & (nslots - 1);
    }
    return false;
  }
  // multi-pass rows: the number of distinct keys of a pass is bounded only in expectation -> bounded probing;
  // false = table full (the caller raises the error flag, the host turns it into SCAMD_EINTERNAL)
  __device__ __forceinline__ bool add_bounded(int c, long long w) {
    unsigned int slot = hash32((unsigned int)c) & (nslots - 1);
    for (int probes = 0; probes < nslots; ++probes) {
      const int prev = atomicCAS(&keys[slot], WH_EMPTY, c);
      if (prev == WH_EMPTY || prev == c) {
        atomicAdd(&vals[slot], (unsigned long long)w);
        return true;
      }
      slot = (slot + 1) & (nslots - 1);
    }
    return false;
  }
};

// block-wide argmax of candidates (+ max of w_own); result valid in thread 0
__device__ __forceinline__ Cand block_best(Cand x, long long& w_own, Cand* sh_c, long long* sh_w) {
  x = wave_best(x);
  w_own = group_max<64>(w_own);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh_c[wv] = x;
    sh_w[wv] = w_own;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {
      if (cand_better(sh_c[i], x)) x = sh_c[i];
      w_own = max(w_own, sh_w[i]);
    }
  }
  return x;
}

// ---- phase 1: local moving -------------------------------------------------------------------------
// Round = decide (one wave per ACTIVE vertex, reads the state only) -> apply (one thread per active vertex,
// mutates the state, flags the vertices to revisit) -> compact (flags -> next active list + counters).  No
// kernel appends to a list through a single global counter: at 1M vertices that serialised on one L2 atomic
// (~12 ns each, 15 ms for the first round alone).

// G lanes per ACTIVE vertex (list[0..n_act)): decision[w] = community to move to, -1 = stay,
// -2 = wants to move but the direction rule forbids it this round (stays active).
//   G = 64: one wave per vertex, table of up to 512 slots (deg <= 384); longer rows are skipped: a workgroup tier has them.
//   G = 16: FOUR vertices per wave, 128 slots each (deg <= 96) -- a kNN graph's rows are ~2k long, and the kernel
//           is bound by its chain of dependent gathers (list -> indptr -> indices -> comm -> Ktot), so four
//           vertices per wave put four times as many gathers in flight per wave slot.  Longer rows are
//           skipped: the G = 64 instantiation decides them in indirect mode (sub_list = the class's wave-tier list:
//           positions in `list`, grid-strided), or a workgroup tier.
// THE move rule, shared by the wave and the hub kernel.  Score of moving v (weight kv) into community c, to which it has
// weight `sum` and whose total is Kc:
__device__ __forceinline__ Cand move_cand(int c, long long sum, unsigned long long Kc, double g, double kv, unsigned int seed) {
  return Cand{(double)sum - g * kv * (double)(long long)Kc, c, prio(c, seed)};
}
// ... and the verdict on vertex v of community a (w_own: its weight to a, Ka_wo: a's total without v) given the best
// candidate: the community to move to, -1 = stay, -2 = wants to move but the direction rule forbids it this round
__device__ __forceinline__ int move_verdict(const Cand& best, long long w_own, double g, double kv, double Ka_wo, int a, int v,
                                            int round, unsigned int seed, const int* __restrict__ csize) {
  const double stay = (double)w_own - g * kv * Ka_wo;
  int target = a;
  bool wants = false, allowed = true;
  if (best.c >= 0 && best.val > stay) {
    wants = true;
    target = best.c;
    const unsigned int pa = prio(a, seed), pb = best.pr;
    // direction rule (round >= 0 only: the termination guarantee of the late sweeps, see local_moving): moves towards
    // lower / higher priority communities alternate, so that two communities cannot keep swapping members
    if (round >= 0)
      allowed = (round & 1) ? (pb > pa || (pb == pa && target > a)) : (pb < pa || (pb == pa && target < a));
  } else if (stay < 0.0 && Ka_wo > 0.0 && csize[v] == 0) {
    // leaving for an empty community (id = own vertex id, free at the snapshot) beats staying
    wants = true;
    target = v;
  }
  return (wants && allowed) ? target : (wants ? -2 : -1);
}

// The long rows of a class list, as its builder left them (list_long_rows), and how the fused decide launch divides its
// workgroups among the tiers.  Entries are positions in the class list.
struct TierLists {
  const int* mid;       // wave-per-row tier: mid[0 .. n_mid)
  const int* blk_last;  // block tier, written downwards from the end of the class's region: blk_last[0], blk_last[-1], ...
  const int* giant;     // giant tier (ld_move_hub_kernel / ld_refine_propose_hub_kernel): giant[0 .. n_giant)
  int n_mid, n_blk, n_giant;
  int nb_main, nb_wave, nb_blk;  // workgroups of the main, the wave-per-row and the block tier in the fused launch
};
// the block tier's table lives in the 24 KB of LDS the main tier has anyway (2048 slots of 12 bytes): rows up to BLK_MAX_DEG
// entries in one pass at a load of 3/4
constexpr int BLK_SLOTS = 2048;
constexpr int BLK_MAX_DEG = BLK_SLOTS * 3 / 4;
constexpr int BLK_GRID = 4096;  // most workgroups of the block tier (one row each; beyond that they loop)

struct MoveArgs {
  int n_act;
  const int* list;
  const int64_t* indptr;
  const int* indices;
  const long long* wq;
  const long long* k;
  const int* comm;
  const unsigned long long* Ktot;
  const int* csize;
  double g;  // gamma / 2m
  int round;
  unsigned int seed;
  int* decision;
  TierLists tl;
};
// (the body takes its workgroup number and the number of workgroups as arguments: it runs on a block range of the fused
// launch, ld_move_tiers; sub_list != nullptr: indirect mode, the n_items positions listed there; hkeys / hvals: the
// workgroup's 2048 table slots, 256 / G tables of GSLOTS)
template <int G>
__device__ __forceinline__ void ld_move_body(int bid, int nblk, const MoveArgs& ma, const int* __restrict__ sub_list, int n_items,
                                             int* __restrict__ hkeys, unsigned long long* __restrict__ hvals) {
  const int* __restrict__ list = ma.list;
  const int64_t* __restrict__ indptr = ma.indptr;
  const int* __restrict__ indices = ma.indices;
  const long long* __restrict__ wq = ma.wq;
  const long long* __restrict__ k = ma.k;
  const int* __restrict__ comm = ma.comm;
  const unsigned long long* __restrict__ Ktot = ma.Ktot;
  const int* __restrict__ csize = ma.csize;
  const double g = ma.g;
  const int round = ma.round;
  const unsigned int seed = ma.seed;
  int* __restrict__ decision = ma.decision;
  constexpr int GROUPS = 256 / G;            // vertices per workgroup
  constexpr int GSLOTS = G == 16 ? G16_SLOTS : WH_SLOTS * G / 64;  // table slots per vertex
  constexpr int GMAX = GSLOTS * 3 / 4;       // longest row the table takes
  static_assert(GROUPS * GSLOTS == BLK_SLOTS, "the tiers share one table area");
  const int sub = threadIdx.x % G;
  const int grp = threadIdx.x / G;
  for (int item = bid * GROUPS + grp; item < n_items; item += nblk * GROUPS) {
    // The decision of one vertex is a chain of dependent gathers (list -> indptr -> indices -> comm -> Ktot) and the
    // kernel is bound by its length: everything that depends on the same address is requested together, before the
    // first branch that needs any of it (written the obvious way the compiler keeps seven round trips in series:
    // list, indptr, [degree branch] comm[v] / k[v], Ktot[a], indices, comm[u], Ktot[c]; now five).
    const int w = sub_list ? sub_list[item] : item;
    const int v = list[w];
    const int64_t beg = indptr[v];
    const int64_t end = indptr[v + 1];
    const int a = comm[v];
    const long long kq = k[v];
    const int deg = (int)(end - beg);
    // the row's first 2 G entries (rows of the kNN graph itself: all of them)
    int u_pre[2];
    long long w_pre[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int e = sub + t * G;
      u_pre[t] = e < deg ? indices[beg + e] : v;
      w_pre[t] = e < deg ? wq[beg + e] : 0ll;
    }
    const unsigned long long Ka = Ktot[a];
    int c_pre[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) c_pre[t] = comm[u_pre[t]];
    if (deg > GMAX) continue;  // a long row: on the list of another tier (list_long_rows)
    const double kv = (double)kq;
    const double Ka_wo = (double)(long long)(Ka - (unsigned long long)kq);  // own community without v
    Cand best = cand_none();
    long long w_own = 0;
    int* keys = hkeys + grp * GSLOTS;
    unsigned long long* vals = hvals + grp * GSLOTS;
    int nslots = 64;  // smallest power of two with load <= 3/4 (deg <= GMAX guarantees nslots <= GSLOTS)
    while (nslots * 3 / 4 < deg) nslots <<= 1;
    for (int i = sub; i < nslots; i += G) {
      keys[i] = WH_EMPTY;
      vals[i] = 0ull;
    }
    auto insert = [&](int c, long long wt) {
      unsigned int slot = hash32((unsigned int)c) & (nslots - 1);
      for (;;) {
        const int prev = atomicCAS(&keys[slot], WH_EMPTY, c);
        if (prev == WH_EMPTY || prev == c) break;
        slot = (slot + 1) & (nslots - 1);
      }
      atomicAdd(&vals[slot], (unsigned long long)wt);
    };
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (sub + t * G < deg && u_pre[t] != v) insert(c_pre[t], w_pre[t]);
    for (int e = sub + 2 * G; e < deg; e += G) {
      const int u = indices[beg + e];
      if (u != v) insert(comm[u], wq[beg + e]);
    }
    // candidates: the community totals of all occupied slots of this lane are requested before the first is used
    constexpr int MAXSL = GSLOTS / G;
    // (no per-lane branch around the gather and no constant merged into its result: either makes the compiler wait
    // for the load where it is issued; empty slots read Ktot[a], the wave skips slot ranges none of its tables has)
    int cs[MAXSL];
    unsigned long long kt[MAXSL];
#pragma unroll
    for (int t = 0; t < MAXSL; ++t) cs[t] = WH_EMPTY;
#pragma unroll
    for (int t = 0; t < MAXSL; ++t) {
      const int sl = sub + t * G;
      if (__ballot(sl < nslots)) {
        cs[t] = sl < nslots ? __hip_atomic_load(&keys[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : WH_EMPTY;
        kt[t] = Ktot[cs[t] != WH_EMPTY ? cs[t] : a];
      }
    }
#pragma unroll
    for (int t = 0; t < MAXSL; ++t) {
      const int c = cs[t];
      if (c != WH_EMPTY) {
        const long long sum =
            (long long)__hip_atomic_load(&vals[sub + t * G], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (c == a) {
          w_own = sum;
        } else {
          const Cand x = move_cand(c, sum, kt[t], g, kv, seed);
          if (cand_better(x, best)) best = x;
        }
      }
    }
    best = group_best<G>(best);
    w_own = group_max<G>(w_own);
    const int verdict = move_verdict(best, w_own, g, kv, Ka_wo, a, v, round, seed, csize);
    if (sub == 0) decision[w] = verdict;
  }
}
// HUB_THREADS = 1024 (round 3; 256 before): a launch lasts as long as its longest row -- up to 20k entries on the coarse
// levels of unstructured graphs, swept in 7 hash-class passes -- and the row is walked blockDim entries at a time.
constexpr int HUB_THREADS = 1024;
struct HubTry {
  int* err;        // raised when a class pass finds its table full (the host turns it into SCAMD_EINTERNAL)
  int try_probes;  // probe bound of the optimistic single pass over a multi-pass row (0: straight to the class passes)
};
// One long row through the workgroup's table: the weight of the row towards every distinct key, handed to visit(key, sum)
// once per key, by whichever thread scans the key's slot.  key_of(e) = the key of entry e of the row, or WH_EMPTY to
// leave the entry out; its weight is wrow[e] (read only for the entries that are inserted).  A row of more than
// BHUB_MAX_DEG entries first tries ONE pass with bounded probing (the comment at HUB_TRY_PROBES) and falls back to its
// bhub_passes(deg) hash-class passes.  Called by every thread of the workgroup; ends with a barrier.
template <typename KeyOf, typename Visit>
__device__ __forceinline__ void hub_row(BlockHash& bh, int deg, const long long* __restrict__ wrow, const HubTry& ht,
                                        int* sh_fail, KeyOf key_of, Visit visit) {
  const int n_pass = bhub_passes(deg);
  bh.size_for(n_pass > 1 ? BHUB_SLOTS : deg);
  bool filled = false;  // the table already holds the whole row (a successful optimistic pass)
  if (n_pass > 1 && ht.try_probes > 0) {
    if (threadIdx.x == 0) *sh_fail = 0;
    bh.clear();
    __syncthreads();
    for (int e = threadIdx.x; e < deg; e += blockDim.x) {
      if (__hip_atomic_load(sh_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
      const int c = key_of(e);
      if (c == WH_EMPTY) continue;
      if (!bh.add_limited(c, wrow[e], ht.try_probes)) __hip_atomic_store(sh_fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    filled = *sh_fail == 0;
    __syncthreads();  // (sh_fail is rewritten for the next row)
  }
  const int n_sweep = filled ? 1 : n_pass;
  for (int pass = 0; pass < n_sweep; ++pass) {
    if (!filled) {
      bh.clear();
      __syncthreads();
      for (int e = threadIdx.x; e < deg; e += blockDim.x) {
        const int c = key_of(e);
        if (c == WH_EMPTY) continue;
        if (n_pass == 1) bh.add(c, wrow[e]);
        else if (bhub_class(c, n_pass) == pass && !bh.add_bounded(c, wrow[e])) *ht.err = 1;
      }
      __syncthreads();
    }
    for (int sl = threadIdx.x; sl < bh.nslots; sl += blockDim.x) {
      const int c = bh.keys[sl];
      if (c != WH_EMPTY) visit(c, (long long)bh.vals[sl]);
    }
    __syncthreads();  // the scan of this pass is done before the next pass clears the table
  }
}

// The decision of the row at position w of the active list by a whole workgroup (block tier: 256 threads, giant tier: 1024).
__device__ __forceinline__ void ld_move_hub_row(const MoveArgs& ma, int w, BlockHash& bh, const HubTry& ht, Cand* sh_c,
                                                long long* sh_w, int* sh_fail) {
  const int v = ma.list[w];
  const int a = ma.comm[v];
  const double kv = (double)ma.k[v];
  const int64_t beg = ma.indptr[v];
  const int deg = (int)(ma.indptr[v + 1] - beg);
  const double Ka_wo = (double)(long long)(ma.Ktot[a] - (unsigned long long)ma.k[v]);
  const int* __restrict__ urow = ma.indices + beg;
  Cand best = cand_none();
  long long w_own = 0;
  hub_row(
      bh, deg, ma.wq + beg, ht, sh_fail,
      [&](int e) {
        const int u = urow[e];
        return u == v ? WH_EMPTY : ma.comm[u];
      },
      [&](int c, long long sum) {
        if (c == a) {
          w_own = sum;
        } else {
          const Cand x = move_cand(c, sum, ma.Ktot[c], ma.g, kv, ma.seed);
          if (cand_better(x, best)) best = x;
        }
      });
  best = block_best(best, w_own, sh_c, sh_w);
  if (threadIdx.x == 0) ma.decision[w] = move_verdict(best, w_own, ma.g, kv, Ka_wo, a, v, ma.round, ma.seed, ma.csize);
  __syncthreads();
}
// Giant tier: the rows beyond the block tier's table (positions in tl.giant), one 1024-thread workgroup each.
__global__ __launch_bounds__(HUB_THREADS) void ld_move_hub_kernel(MoveArgs ma, HubTry ht) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long hub_smem[];
  BlockHash bh{reinterpret_cast<int*>(hub_smem + BHUB_SLOTS), hub_smem, BHUB_SLOTS};
  __shared__ Cand sh_c[HUB_THREADS / 64];
  __shared__ long long sh_w[HUB_THREADS / 64];
  __shared__ int sh_fail;
  for (int i = blockIdx.x; i < ma.tl.n_giant; i += gridDim.x) ld_move_hub_row(ma, ma.tl.giant[i], bh, ht, sh_c, sh_w, &sh_fail);
}

// The static LDS of a fused decide kernel: the 2048 table slots its tiers share (main tier: 256 / G tables, wave-per-row tier:
// four, block tier: one) and the block tier's reduction scratch.
struct TierLds {
  unsigned long long hvals[BLK_SLOTS];
  int hkeys[BLK_SLOTS];
  Cand sh_c[256 / 64];
  long long sh_w[256 / 64];
  int sh_fail;
};
// ALL tiers of a decide step that a 256-thread workgroup can take, as block ranges of one grid: they read the same snapshot
// and write different vertices' decisions.  bid: the workgroup's number among the ma.tl.nb_main + nb_wave + nb_blk of them.
template <int G>
__device__ __forceinline__ void ld_move_tiers(int bid, const MoveArgs& ma, TierLds& lds) {
  const TierLists& tl = ma.tl;
  if (bid < tl.nb_main) {
    ld_move_body<G>(bid, tl.nb_main, ma, nullptr, ma.n_act, lds.hkeys, lds.hvals);
    return;
  }
  bid -= tl.nb_main;
  if constexpr (G < 64) {
    if (bid < tl.nb_wave) {
      ld_move_body<64>(bid, tl.nb_wave, ma, tl.mid, tl.n_mid, lds.hkeys, lds.hvals);
      return;
    }
  }
  bid -= tl.nb_wave;
  BlockHash bh{lds.hkeys, lds.hvals, BLK_SLOTS, BLK_SLOTS};
  const HubTry no_try{nullptr, 0};  // (one pass: a row of this tier is no longer than BLK_MAX_DEG <= BHUB_MAX_DEG)
  for (int i = bid; i < tl.n_blk; i += tl.nb_blk) ld_move_hub_row(ma, tl.blk_last[-i], bh, no_try, lds.sh_c, lds.sh_w, &lds.sh_fail);
}
template <int G>
__global__ __launch_bounds__(256) void ld_move_kernel(MoveArgs ma) {
  __shared__ TierLds lds;
  ld_move_tiers<G>((int)blockIdx.x, ma, lds);
}

// One thread per active vertex: apply the decided moves in place (integer atomics on the community totals); vertices
// blocked by the direction rule stay active.  counters: [0] moved, [1] blocked
// At most COUNT_GRID workgroups of 1024 threads walk the list; moved and blocked are counted by ballot per wave, summed in
// LDS and added ONCE per workgroup (a workgroup per 256 vertices, each ending on counters[PH_MOVED]: 489 workgroups of a
// level-0 sub-round took 36 us over a few MB).
constexpr int APPLY_THREADS = 1024;
// the workgroup's two sums -> counters[PH_MOVED], counters[PH_BLOCKED]; every thread calls it, `moved` / `blocked` are its wave's
__device__ __forceinline__ void ld_apply_count(int moved, int blocked, int* __restrict__ counters) {
  __shared__ int s_sum[2];
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    if (moved) atomicAdd(&s_sum[0], moved);
    if (blocked) atomicAdd(&s_sum[1], blocked);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_sum[threadIdx.x]) atomicAdd(&counters[threadIdx.x == 0 ? PH_MOVED : PH_BLOCKED], s_sum[threadIdx.x]);
}
__global__ __launch_bounds__(APPLY_THREADS) void ld_apply_kernel(int n_act, const int* __restrict__ list,
                                                                 const int* __restrict__ decision, const long long* __restrict__ k,
                                                                 int* __restrict__ comm, unsigned long long* __restrict__ Ktot,
                                                                 int* __restrict__ csize, int* __restrict__ flag,
                                                                 int* __restrict__ counters) {
  int moved = 0, blocked = 0;  // of this wave
  for (int w0 = blockIdx.x * APPLY_THREADS; w0 < n_act; w0 += gridDim.x * APPLY_THREADS) {
    const int w = w0 + (int)threadIdx.x;
    const int d = w < n_act ? decision[w] : -1;
    if (d >= 0) {
      const int v = list[w];
      const int a = comm[v];
      comm[v] = d;
      const unsigned long long kq = (unsigned long long)k[v];
      atomicAdd(&Ktot[d], kq);
      atomicAdd(&Ktot[a], 0ull - kq);
      atomicAdd(&csize[d], 1);
      atomicSub(&csize[a], 1);
    } else if (d == -2) {
      flag[list[w]] = 1;
    }
    moved += __popcll(__ballot(d >= 0));
    blocked += __popcll(__ballot(d == -2));
  }
  ld_apply_count(moved, blocked, counters);
}

// After ALL moves of the sub-round are applied: every mover re-activates its neighbours that are NOT in its new
// community (the queue rule of the sequential algorithm, leidenalg `move_nodes`: a neighbour inside the new community can
// only have become more attached).  A separate launch, because the test reads the neighbours' communities and those
// must be the sub-round's final ones for the flags to be reproducible.  Round 2 flagged every neighbour: after the first
// sweep of a level most of the active list was vertices deep inside their community.
// The rows are walked by the whole wave, two movers at a time (32 lanes each, coalesced row reads).
__device__ __forceinline__ void ld_requeue_body(int bid, int n_act, const int* __restrict__ list,
                                                const int* __restrict__ decision, const int64_t* __restrict__ indptr,
                                                const int* __restrict__ indices, const int* __restrict__ comm,
                                                int* __restrict__ flag) {
  const int w = bid * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int64_t beg = 0, end = 0;
  int d = -1;
  if (w < n_act) {
    d = decision[w];
    if (d >= 0) {
      const int v = list[w];
      beg = indptr[v];
      end = indptr[v + 1];
    }
  }
  unsigned long long m = __ballot(d >= 0);
  while (m) {
    const int b0 = __ffsll((long long)m) - 1;
    m &= m - 1;
    int b1 = b0;
    if (m) {
      b1 = __ffsll((long long)m) - 1;
      m &= m - 1;
    }
    const int src = lane < 32 ? b0 : b1;
    // (all shuffles run with every lane active: a bpermute under a partial exec mask reads 0 from disabled lanes)
    const int64_t rb = __shfl(beg, src), re_s = __shfl(end, src);
    const int dd = __shfl(d, src);
    const int64_t re = (lane >= 32 && b1 == b0) ? rb : re_s;
    for (int64_t e = rb + (lane & 31); e < re; e += 32) {
      const int u = indices[e];
      if (comm[u] != dd) flag[u] = 1;
    }
  }
}
__global__ __launch_bounds__(256) void ld_requeue_kernel(int n_act, const int* __restrict__ list,
                                                         const int* __restrict__ decision,
                                                         const int64_t* __restrict__ indptr,
                                                         const int* __restrict__ indices, const int* __restrict__ comm,
                                                         int* __restrict__ flag) {
  ld_requeue_body((int)blockIdx.x, n_act, list, decision, indptr, indices, comm, flag);
}
// Sub-round c's re-queue and sub-round c + 1's decisions in ONE launch (round 4).  They are independent: the re-queue
// reads the decisions of class c (their own buffer: `decision` alternates between two buffers from sub-round to
// sub-round) and the communities after apply(c), and writes flags; the decisions of class c + 1 read the same state and
// write their own buffer and lists.  The first nb_rq workgroups re-queue, the rest decide.  One launch of ~16 us less per
// sub-round (152 per call at 1M cells).  The decide blocks are ALL tiers of the sub-round (ld_move_tiers).
template <int G>
__global__ __launch_bounds__(256) void ld_requeue_move_kernel(int nb_rq, int rq_n_act, const int* __restrict__ rq_list,
                                                              const int* __restrict__ rq_decision,
                                                              const int64_t* __restrict__ indptr,
                                                              const int* __restrict__ indices, const int* __restrict__ comm,
                                                              int* __restrict__ flag, MoveArgs ma) {
  __shared__ TierLds lds;
  if ((int)blockIdx.x < nb_rq) ld_requeue_body((int)blockIdx.x, rq_n_act, rq_list, rq_decision, indptr, indices, comm, flag);
  else ld_move_tiers<G>((int)blockIdx.x - nb_rq, ma, lds);
}

// ---- final polish (n_iterations < 0): strictly monotone single-vertex moves ----------------------------------------
// The class sub-rounds above apply many moves decided on ONE snapshot: fast, but not monotone, and the outer loop keeps the
// best partition it saw -- which, on ambiguous graphs, may be one whose last coarse-level moves left a few level-0
// vertices improvable (round 4: 9 / 186 of 300k vertices, gains < 1e-6 Q; the paper's "node optimality" of a stable
// partition, oracle/leiden_guarantees.py, violated by that residue).  The polish decides on a snapshot as before, but
// applies a move v: A -> B only if v holds the locks of BOTH communities: lock[c] = max over this round's movers touching
// c of (round << 32 | ~v) -- the smallest vertex id wins, stale rounds lose to the current one, nothing is ever reset.
// The gain of v's move depends on k_v(A), k_v(B), K_A, K_B only; moves with disjoint community pairs leave those four
// untouched, so every applied move realises exactly the gain it was decided on: Q rises strictly, round after round,
// and at least one mover (the smallest id) wins per round.  Losers stay flagged.
__global__ __launch_bounds__(256) void ld_polish_lock_kernel(int n_act, const int* __restrict__ list,
                                                             const int* __restrict__ decision, const int* __restrict__ comm,
                                                             unsigned long long* __restrict__ lock, unsigned int round) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_act) return;
  const int d = decision[w];
  if (d < 0) return;
  const int v = list[w];
  const unsigned long long key = ((unsigned long long)round << 32) | (unsigned long long)(0xffffffffu - (unsigned int)v);
  atomicMax(&lock[comm[v]], key);
  atomicMax(&lock[d], key);
}
// winners move (as ld_apply_kernel), losers keep their flag and their decision becomes "stay" (the re-queue that follows
// reads decision >= 0 as "moved").  counters: [0] moved, [1] lost a lock
__global__ __launch_bounds__(APPLY_THREADS) void ld_polish_apply_kernel(int n_act, const int* __restrict__ list, int* __restrict__ decision,
                                                                        const long long* __restrict__ k, int* __restrict__ comm,
                                                                        unsigned long long* __restrict__ Ktot, int* __restrict__ csize,
                                                                        const unsigned long long* __restrict__ lock, unsigned int round,
                                                                        int* __restrict__ flag, int* __restrict__ counters) {
  int moved = 0, lost = 0;  // of this wave
  for (int w0 = blockIdx.x * APPLY_THREADS; w0 < n_act; w0 += gridDim.x * APPLY_THREADS) {
    const int w = w0 + (int)threadIdx.x;
    const int d = w < n_act ? decision[w] : -1;
    bool won = false;
    if (d >= 0) {
      const int v = list[w];
      const int a = comm[v];
      const unsigned long long key = ((unsigned long long)round << 32) | (unsigned long long)(0xffffffffu - (unsigned int)v);
      won = lock[a] == key && lock[d] == key;
      if (won) {
        comm[v] = d;
        const unsigned long long kq = (unsigned long long)k[v];
        atomicAdd(&Ktot[d], kq);
        atomicAdd(&Ktot[a], 0ull - kq);
        atomicAdd(&csize[d], 1);
        atomicSub(&csize[a], 1);
      } else {
        decision[w] = -1;
        flag[v] = 1;
      }
    }
    moved += __popcll(__ballot(won));
    lost += __popcll(__ballot(d >= 0 && !won));
  }
  ld_apply_count(moved, lost, counters);
}

// A vertex that leaves may have been the only link between two parts of its community.  After a polish that moved
// anything: connected components INSIDE the communities by min-label propagation (comp[v] -> the smallest vertex id of
// its component; in place, monotone, with one pointer jump per visit), and every component becomes a community of its
// own (splitting a community along a cut without edges raises Q by 2 g K1 K2 / (2m)^2 > 0).
__global__ __launch_bounds__(256) void ld_cc_prop_kernel(int n, const int64_t* __restrict__ indptr, const int* __restrict__ indices,
                                                         const int* __restrict__ comm, int* __restrict__ comp, int* __restrict__ changed) {
  // 16 lanes per vertex: the row is read coalesced, the neighbours' labels gathered 16 at a time (a thread per vertex walked
  // its row one dependent gather after the other: 1.0 ms per pass at 1M vertices)
  const int v = (blockIdx.x * 256 + threadIdx.x) >> 4, sub = threadIdx.x & 15;
  const bool live = v < n;
  const int vv = live ? v : 0;
  const int c = comm[vv];
  const int old = __hip_atomic_load(&comp[vv], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int m = old;
  if (live) {
    for (int64_t e = indptr[v] + sub; e < indptr[v + 1]; e += 16) {
      const int u = indices[e];
      if (comm[u] == c) m = min(m, __hip_atomic_load(&comp[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));  // (every lane of the wave takes part)
  if (live && sub == 0) {
    m = min(m, __hip_atomic_load(&comp[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));  // (comp[m] <= m, same component)
    if (m < old) {
      atomicMin(&comp[v], m);
      *changed = 1;
    }
  }
}
// out[0] += components (roots), out[1] += non-empty communities
__global__ __launch_bounds__(256) void ld_cc_count_kernel(int n, const int* __restrict__ comp, const int* __restrict__ csize,
                                                          int* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool root = v < n && comp[v] == v, alive = v < n && csize[v] > 0;
  const unsigned long long mr = __ballot(root), ma = __ballot(alive);
  if ((threadIdx.x & 63) == 0) {
    if (mr) atomicAdd(&out[0], __popcll(mr));
    if (ma) atomicAdd(&out[1], __popcll(ma));
  }
}

// Class of a vertex in a sweep: a fresh hash per sweep (salt), so two neighbours that shared a class -- and could
// therefore move at the same time, e.g. swap communities -- almost surely do not share it in the next sweep.
__device__ __forceinline__ int lm_class(int v, unsigned int salt, int n_cls) {
  return (int)((hash32((unsigned int)v * 0x9E3779B1u + salt) >> 9) & (unsigned int)(n_cls - 1));
}

// flags -> n_cls class lists (lists[c * n ..]), counts in cls_count[0 .. n_cls); clears the flags.  flag == nullptr:
// every vertex is active (first sweep of a level).  The order inside a list is irrelevant (every decision of a
// sub-round reads the same snapshot).  One atomic per class and workgroup (ld_build_class_lists).
// Long rows of a class, listed while its list is built: the tier of a row is known from its length, so the decide step of
// a sub-round finds the rows of every tier on a list of their own and runs the tiers side by side in one launch (until
// then the main decide kernel appended them at run time, and the tiers ran one launch behind the other).  The list lengths
// double as the host's launch sizes: a tier without rows gets no workgroups, the giant tier no launch.
struct TierDst {
  const int64_t* indptr;  // of the level (nullptr: no tier lists)
  int* lists;             // class c: lists[c * n ..]: its wave-tier positions upwards from [0], its block-tier positions
                          // downwards from [n - 1] (both tiers together are at most the n_act <= n rows of the class)
  int* giant;             // class c: giant[c * giant_stride ..]
  int giant_stride;       // > entries of the level / (BLK_MAX_DEG + 1): more giant rows do not exist
  int thr_mid;            // longest row of the main tier (the lanes-per-vertex table); < 0: the main tier IS the wave tier
};
// tier of a vertex's row: 0 main (and inactive vertices), 1 wave-per-row, 2 block, 3 giant
__device__ __forceinline__ int long_row_tier(int cls, int v, const TierDst& d) {
  if (cls < 0 || !d.indptr) return 0;
  const int deg = (int)(d.indptr[v + 1] - d.indptr[v]);
  return deg > BLK_MAX_DEG ? 3 : (deg > WH_MAX_DEG ? 2 : ((d.thr_mid >= 0 && deg > d.thr_mid) ? 1 : 0));
}
// Long rows of one wave's vertices, per tier and class (the same ballots in both passes of ld_build_class_lists; every lane
// of the wave calls it; waves without long rows -- nearly all of a kNN graph's -- pay three ballots).  tcnt: the workgroup's
// LDS words per (tier, class).  PLACE = false: count.  PLACE = true: tcnt holds the next free position of the workgroup's
// range in the tier list; w, the vertex's position in the list of its class, is written there.
template <bool PLACE>
__device__ __forceinline__ void list_long_rows(int cls, int tier, int w, int n, int lane, int (*tcnt)[MAX_CLASSES], const TierDst& d) {
  for (int t = 1; t <= 3; ++t) {
    unsigned long long todo = __ballot(tier == t);
    while (todo) {  // (the same for every lane)
      const int c = __shfl(cls, __ffsll((long long)todo) - 1);
      const unsigned long long m = __ballot(tier == t && cls == c);
      todo &= ~m;
      int base = 0;
      if (lane == 0) base = atomicAdd(&tcnt[t - 1][c], __popcll(m));
      if constexpr (PLACE) {
        base = __shfl(base, 0);
        if (tier == t && cls == c) {
          const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
          if (t == 1) d.lists[(size_t)c * n + pos] = w;
          else if (t == 2) d.lists[(size_t)c * n + (n - 1 - pos)] = w;
          else d.giant[(size_t)c * d.giant_stride + pos] = w;
        }
      }
    }
  }
}

// The list builder of ld_compact_cls_kernel.  cls_of(v, second_pass): the class of vertex v, -1 when it is not listed; both
// passes must answer the same.  (ld_refine_candidates_kernel keeps its one-pass builder: under this one its per-pass time did
// not fall -- it waits for its four loads per vertex, not for its counters; profiles/leiden_hot_words_ab.log.)
// A workgroup owns a contiguous span of whole 1024-vertex chunks, ceil(chunks / gridDim.x) of them (the last spans may be
// short or empty), and walks it twice; wave i takes vertices [64 i, 64 i + 64) of every chunk.  Pass 1 counts the listed
// vertices per wave and class (lane c of a wave holds its count for class c) and the span's long rows per (class, tier), and
// reserves ONE range per word for the whole span: one returning atomic per word and workgroup -- the builders before it did
// one per class and 1024 vertices and one per wave, class and tier, all on the same few words (977 workgroups at 1M vertices:
// 81 us for ~20 MB).  The waves' shares of a range follow each other in wave order.  Pass 2 recomputes class, tier and rank
// and writes the class lists and the tier lists; no barrier in it.  The order inside a list is now span order, not arrival
// order; nobody observes it.  A wave skips the chunks in which it lists nothing, and pass 2 when it lists nothing at all (late
// sweeps list a few hundred of a million vertices).
constexpr int LIST_BATCH = 4;  // chunks whose classes pass 1 asks for before it counts them (loads in flight)
struct ClassListLds {
  int wpos[16][MAX_CLASSES];  // wave, class: the wave's count, then the first position of its share of the span's range
  int tcnt[3][MAX_CLASSES];   // tier, class: the span's long rows, then the next free position of the span's range
};
template <typename ClsOf>
__device__ __forceinline__ void ld_build_class_lists(int n, int* __restrict__ lists, int* __restrict__ cls_count, int n_cls,
                                                     const TierDst& tiers, ClassListLds& s, ClsOf cls_of) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int chunks = (n + 1023) >> 10;
  const int per = (chunks + (int)gridDim.x - 1) / (int)gridDim.x;
  const int ch0 = (int)blockIdx.x * per, ch1 = min(chunks, ch0 + per);
  if (threadIdx.x < 3 * MAX_CLASSES) (&s.tcnt[0][0])[threadIdx.x] = 0;
  __syncthreads();
  int mine = 0;  // lane c: the wave's vertices of class c
  for (int cb = ch0; cb < ch1; cb += LIST_BATCH) {
    int cl[LIST_BATCH];
#pragma unroll
    for (int j = 0; j < LIST_BATCH; ++j) {
      const int v = (cb + j) * 1024 + (int)threadIdx.x;
      cl[j] = (cb + j < ch1 && v < n) ? cls_of(v, false) : -1;
    }
#pragma unroll
    for (int j = 0; j < LIST_BATCH; ++j) {
      const int cls = cl[j];
      if (!__ballot(cls >= 0)) continue;  // (the same for every lane of the wave)
      for (int c = 0; c < n_cls; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (lane == c) mine += __popcll(m);
      }
      list_long_rows<false>(cls, long_row_tier(cls, (cb + j) * 1024 + (int)threadIdx.x, tiers), 0, n, lane, s.tcnt, tiers);
    }
  }
  if (lane < MAX_CLASSES) s.wpos[wv][lane] = mine;
  __syncthreads();
  if ((int)threadIdx.x < n_cls) {
    const int c = threadIdx.x;
    int tot = 0;
    for (int i = 0; i < 16; ++i) tot += s.wpos[i][c];
    int at = tot ? atomicAdd(&cls_count[c], tot) : 0;
    for (int i = 0; i < 16; ++i) {
      const int t = s.wpos[i][c];
      s.wpos[i][c] = at;
      at += t;
    }
  } else if (threadIdx.x >= 64 && threadIdx.x < 64 + 3 * MAX_CLASSES) {
    const int t = (threadIdx.x - 64) / MAX_CLASSES, c = (threadIdx.x - 64) % MAX_CLASSES;
    const int tot = s.tcnt[t][c];
    if (tot) s.tcnt[t][c] = atomicAdd(&cls_count[MAX_CLASSES + CTR_STRIDE * c + CTR_N_MID + t], tot);
  }
  __syncthreads();
  if (!__ballot(mine != 0)) return;  // (the wave lists nothing; no barrier follows)
  int pos = lane < MAX_CLASSES ? s.wpos[wv][lane] : 0;  // lane c: where the wave's next vertex of class c goes
  for (int ch = ch0; ch < ch1; ++ch) {
    const int v = ch * 1024 + (int)threadIdx.x;
    const int cls = v < n ? cls_of(v, true) : -1;
    if (!__ballot(cls >= 0)) continue;
    int w = 0;
    for (int c = 0; c < n_cls; ++c) {
      const unsigned long long m = __ballot(cls == c);
      const int at = __shfl(pos, c);
      if (cls == c) w = at + __popcll(m & ((1ull << lane) - 1ull));
      if (lane == c) pos += __popcll(m);
    }
    if (cls >= 0) lists[(size_t)cls * n + w] = v;
    list_long_rows<true>(cls, long_row_tier(cls, v, tiers), w, n, lane, s.tcnt, tiers);
  }
}

__global__ __launch_bounds__(1024) void ld_compact_cls_kernel(int n, int* __restrict__ flag, int* __restrict__ lists,
                                                              int* __restrict__ cls_count, int n_cls, unsigned int salt,
                                                              TierDst tiers, int* __restrict__ clear_next, int clear_words) {
  __shared__ ClassListLds s;
  // (the counter block the NEXT sweep will count into: its last users were the sub-rounds of the sweep before this one)
  if (clear_next && blockIdx.x == 0)
    for (int i = threadIdx.x; i < clear_words; i += 1024) clear_next[i] = 0;
  // (the flag words are read twice, the second time from L2; the second pass clears them)
  ld_build_class_lists(n, lists, cls_count, n_cls, tiers, s, [&](int v, bool second_pass) {
    if (flag) {
      if (!flag[v]) return -1;
      if (second_pass) flag[v] = 0;
    }
    return lm_class(v, salt, n_cls);
  });
}

// Packed mirrors of the refinement's state (round 4).  Counters of the decision kernels (profiles/r04n_leiden_kernels_pmc*.csv):
// ld_refine_propose_kernel<16> waits 55 % of its wave-cycles on memory and moves 0.7 GB (FETCH_SIZE with the gfx950
// correction) through the memory side of L2 per launch of ~100k candidates -- ~7 KB per candidate: a 64-byte sector for every
// 4- or 8-byte gather of comm[u], ref[u] (two per neighbour) and Kref[c], refsize[c], Eref[c] (three per distinct target),
// at an L2 hit rate of 24 %.  The proposing kernels and the cut update therefore read ONE record per neighbour and ONE per
// target; the plain arrays stay the authoritative copy for everything else (aggregation, coarse ids), every writer of
// the refinement updates both.  All fields are integers: same results.  Measured: 31.3 -> 30.6 ms on the planted 1M graph
// (profiles/r04p_leiden_packed_records_ab.log) -- less than the sector count promised: the kernels wait on the length of
// their dependency chain as much as on the bytes.
struct alignas(16) VertRec {  // per vertex: phase-1 community, refined community, sub-round in which it joined (-1: never)
  int comm, ref, stamp, pad;
};
struct alignas(32) TargRec {  // per refined community (indexed by its representative vertex)
  unsigned long long Kref, Eref;
  int refsize, pad0, pad1, pad2;
};

// ---- phase 2: refinement ---------------------------------------------------------------------------
// a_in[v] = w(v, C(v) - v): weight from v to the rest of its (phase-1) community
template <int G>
__global__ __launch_bounds__(256) void ld_within_kernel(int n, const int64_t* __restrict__ indptr,
                                                        const int* __restrict__ indices,
                                                        const long long* __restrict__ wq, const int* __restrict__ comm,
                                                        long long* __restrict__ a_in) {
  const int sub = threadIdx.x % G;
  const int v = blockIdx.x * (256 / G) + threadIdx.x / G;
  if (v >= n) return;
  const int a = comm[v];
  const int64_t beg = indptr[v], end = indptr[v + 1];
  long long s = 0;
  // four entries per lane in flight: a hub row (1.4k entries on the 1M kNN graph) walked one dependent gather pair at
  // a time by 16 lanes is ~90 serial round trips -- the tail of the whole launch
  for (int64_t e = beg + sub; e < end; e += 4 * G) {
    int u[4], cu[4];
    long long we[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t ee = e + t * G;
      u[t] = ee < end ? indices[ee] : v;
      we[t] = ee < end ? wq[ee] : 0ll;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) cu[t] = comm[u[t]];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (u[t] != v && cu[t] == a) s += we[t];
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (sub == 0) a_in[v] = s;
}

// The long rows of ld_refine_candidates_kernel, which builds its lists in one pass (below):
// w: the vertex's position in the list of its class.  One atomic per wave, class and tier (coarse levels of unstructured
// graphs are mostly long rows); waves without long rows -- nearly all of a kNN graph's -- pay three ballots.  Every lane of
// the wave calls it.
__device__ __forceinline__ void list_long_rows_per_wave(int cls, int tier, int w, int n, int lane, int* __restrict__ cls_count, const TierDst& d) {
  for (int t = 1; t <= 3; ++t) {
    unsigned long long todo = __ballot(tier == t);
    while (todo) {  // (the same for every lane)
      const int c = __shfl(cls, __ffsll((long long)todo) - 1);
      const unsigned long long m = __ballot(tier == t && cls == c);
      todo &= ~m;
      int base = 0;
      if (lane == 0) base = atomicAdd(&cls_count[MAX_CLASSES + CTR_STRIDE * c + (t == 1 ? CTR_N_MID : (t == 2 ? CTR_N_BLK : CTR_N_GIANT))], __popcll(m));
      base = __shfl(base, 0);
      if (tier == t && cls == c) {
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (t == 1) d.lists[(size_t)c * n + pos] = w;
        else if (t == 2) d.lists[(size_t)c * n + (n - 1 - pos)] = w;
        else d.giant[(size_t)c * d.giant_stride + pos] = w;
      }
    }
  }
}

// candidates of the refinement: vertices that are well connected inside their community
// (w(v, C - v) >= gamma k_v (K_C - k_v) / 2m); all of them start as singletons.  They are written as n_cls class lists
// (lists[c * n ..], counts in cls_count[0 .. n_cls)): class c is visited in sub-round c of the refinement.
__global__ __launch_bounds__(1024) void ld_refine_candidates_kernel(
    int n, const long long* __restrict__ k, const int* __restrict__ comm, const unsigned long long* __restrict__ Ktot,
    const long long* __restrict__ a_in, double g, int* __restrict__ lists, int* __restrict__ cls_count, int n_cls,
    unsigned int salt, TierDst tiers) {
  __shared__ int wcnt[16][MAX_CLASSES];
  __shared__ int base[MAX_CLASSES];
  const int v = blockIdx.x * 1024 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int cls = -1;
  if (v < n) {
    const double kv = (double)k[v];
    const double KC = (double)(long long)Ktot[comm[v]];
    if ((double)a_in[v] >= g * kv * (KC - kv)) cls = lm_class(v, salt, n_cls);
  }
  const int tier = long_row_tier(cls, v, tiers);
  int rank = 0;
  for (int c = 0; c < n_cls; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if (cls == c) rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wv][c] = __popcll(m);
  }
  __syncthreads();
  if ((int)threadIdx.x < n_cls) {
    const int c = threadIdx.x;
    int tot = 0;
    for (int i = 0; i < 16; ++i) {
      const int t = wcnt[i][c];
      wcnt[i][c] = tot;
      tot += t;
    }
    base[c] = tot ? atomicAdd(&cls_count[c], tot) : 0;
  }
  __syncthreads();
  const int w = cls >= 0 ? base[cls] + wcnt[wv][cls] + rank : 0;
  if (cls >= 0) lists[(size_t)cls * n + w] = v;
  list_long_rows_per_wave(cls, tier, w, n, lane, cls_count, tiers);
}

// Exact incremental update of w(r, C - r) after a round of merges.  For a vertex v that joined t this round
// (stamp[v] == round), with t_old = the members t had before the round and J = the other joiners of the round:
//   Eref[t] += w(v, C - v) - 2 w(v, t_old) - w(v, J)
// (summed over the joiners every {v, v'} in J x J pair is subtracted twice, as the cut of the union requires).
// One wave per joiner; all integer, so the result equals a from-scratch recomputation bit for bit.
template <int G>
__global__ __launch_bounds__(256) void ld_refine_cut_update_kernel(
    int n_join, const int* __restrict__ jlist, const int64_t* __restrict__ indptr, const int* __restrict__ indices,
    const long long* __restrict__ wq, const int* __restrict__ comm, const int* __restrict__ ref,
    const int* __restrict__ stamp, const long long* __restrict__ a_in, int round,
    unsigned long long* __restrict__ Eref, const int* __restrict__ n_join_dev, const VertRec* __restrict__ vr,
    TargRec* __restrict__ tr) {
  const int sub = threadIdx.x % G;
  n_join = *n_join_dev;
  for (int w = blockIdx.x * (256 / G) + threadIdx.x / G; w < n_join; w += gridDim.x * (256 / G)) {
  // (everything that hangs on the same address is requested together: the && chain of the obvious form is four
  // round trips per neighbour -- comm[u], then ref[u], then stamp[u], then the weight)
  const int v = jlist[w];
  const int a = comm[v], t = ref[v];
  const int64_t beg = indptr[v], end = indptr[v + 1];
  const long long av = a_in[v];
  long long s = 0;
  for (int64_t e = beg + sub; e < end; e += 2 * G) {  // two entries per lane in flight (hub rows: see ld_within_kernel)
    int u[2], cu[2], ru[2], su[2];
    long long we[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t ee = e + j * G;
      u[j] = ee < end ? indices[ee] : v;
      we[j] = ee < end ? wq[ee] : 0ll;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {  // one 16-byte record per neighbour instead of three gathers
      const VertRec r = vr[u[j]];
      cu[j] = r.comm;
      ru[j] = r.ref;
      su[j] = r.stamp;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (u[j] != v && cu[j] == a && ru[j] == t) s += (su[j] == round) ? we[j] : 2 * we[j];
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (sub == 0) {
    atomicAdd(&Eref[t], (unsigned long long)(av - s));
    atomicAdd(&tr[t].Eref, (unsigned long long)(av - s));
  }
  }
}

// Sub-round c of the refinement: the singletons of class c propose, the targets are grown sub-communities and singletons
// of OTHER classes (a singleton of the same class may itself leave in this sub-round), so simultaneous merges cannot
// chain; classes < c have had their turn (their results are visible), classes > c get theirs later unless somebody
// joins them first.  After the n_cls sub-rounds every candidate was considered exactly once -- leidenalg's
// `merge_nodes_constrained` visits every vertex once, in random order.
// Randomised merge rule of the refinement (Traag et al. 2019, leidenalg's `refine_consider_comms` with theta = beta):
// v joins r with probability ~ exp(gain(v, r) / beta) among the well-connected candidates of non-negative gain, "stay"
// (gain 0) included.  Sampled with the Gumbel-max trick: argmax_r gain_r / beta + G(v, r, round, seed) with
// counter-based noise, so the choice is a pure function of its arguments -- every kernel variant draws the same
// target, runs are bitwise reproducible.  (Round 1 took the beta -> 0 limit; on graphs without clean structure the
// greedy rule ends in visibly worse optima: 0.8101 vs 0.8121 on the bundled fixture, the same value the CPU oracle
// reaches when its beta is set to 1e-7.)  c = v encodes "stay".
__device__ __forceinline__ double refine_noise(int v, int c, int round, unsigned int seed) {
  const unsigned int h = hash32((unsigned int)v * 0x9E3779B1u ^
                                hash32((unsigned int)c * 0x85EBCA77u + (unsigned int)round * 0xC2B2AE3Du + seed));
  const double u = ((double)h + 0.5) * (1.0 / 4294967296.0);
  return -log(-log(u));
}

struct RefineRule {
  double g;         // gamma / 2m
  double inv_beta;  // 1 / (beta * 2^32); 0 = greedy
  int round;        // the sub-round = the class that proposes
  int n_cls;
  unsigned int salt, seed;
};
// THE merge rule, shared by the wave and the hub kernel.  Candidate v (weight kv, in a phase-1 community of total KC) and
// the refined community c (record t) to which it has weight `sum`: if c is an admissible target -- grown, or a singleton of
// another class; well connected -- of non-negative gain, its value in the draw goes into *x
__device__ __forceinline__ bool refine_cand(const RefineRule& r, int v, double kv, double KC, int c, long long sum,
                                            unsigned long long Kref, int refsize, unsigned long long Eref, Cand* x) {
  const double Kr = (double)(long long)Kref;
  const bool single = refsize == 1;
  const bool ok_target = (!single || lm_class(c, r.salt, r.n_cls) != r.round) &&
                         ((double)(long long)Eref >= r.g * Kr * (KC - Kr));  // target well connected
  const double gain = (double)sum - r.g * kv * Kr;
  if (!(ok_target && gain >= 0.0)) return false;
  *x = Cand{r.inv_beta > 0.0 ? gain * r.inv_beta + refine_noise(v, c, r.round, r.seed) : gain, c, prio(c, r.seed)};
  return true;
}
// ... and what v does given the best of them: the refined community to join, -1 = no admissible target, -2 = "stay" was
// drawn against the best candidate (a singleton that stays is done; it may still be joined)
__device__ __forceinline__ int refine_verdict(const RefineRule& r, int v, const Cand& best) {
  return (r.inv_beta > 0.0 && best.c >= 0 && !(best.val > refine_noise(v, v, r.round, r.seed))) ? -2 : best.c;
}

struct ProposeArgs {
  int n_act;        // length of ...
  const int* list;  // ... the candidates of class rule.round
  const int64_t* indptr;
  const int* indices;
  const long long* wq;
  const long long* k;
  const int* comm;
  const unsigned long long* Ktot;
  const int* ref;
  const int* refsize;
  const VertRec* vr;
  const TargRec* tr;
  RefineRule rule;
  int* target;
  TierLists tl;
};
// G lanes per candidate (see ld_move_body: G = 16 puts four candidates in a wave on short-rowed levels, rows longer
// than the table are on the list of another tier and proposed there: by the G = 64 instantiation in indirect mode, or by
// a workgroup).  target[v] = refined community to join, -1 = no admissible target, -2 = no longer a singleton (somebody
// joined it) or "stay" was drawn.
template <int G>
__device__ __forceinline__ void ld_refine_propose_body(int bid, int nblk, const ProposeArgs& pa, const int* __restrict__ sub_list,
                                                       int n_items, int* __restrict__ hkeys, unsigned long long* __restrict__ hvals) {
  const int* __restrict__ list = pa.list;
  const int64_t* __restrict__ indptr = pa.indptr;
  const int* __restrict__ indices = pa.indices;
  const long long* __restrict__ wq = pa.wq;
  const long long* __restrict__ k = pa.k;
  const int* __restrict__ comm = pa.comm;
  const unsigned long long* __restrict__ Ktot = pa.Ktot;
  const int* __restrict__ ref = pa.ref;
  const int* __restrict__ refsize = pa.refsize;
  const VertRec* __restrict__ vr = pa.vr;
  const TargRec* __restrict__ tr = pa.tr;
  const RefineRule rule = pa.rule;
  constexpr int GROUPS = 256 / G;
  constexpr int GSLOTS = G == 16 ? G16_SLOTS : WH_SLOTS * G / 64;
  constexpr int GMAX = GSLOTS * 3 / 4;
  static_assert(GROUPS * GSLOTS == BLK_SLOTS, "the tiers share one table area");
  const int sub = threadIdx.x % G;
  const int grp = threadIdx.x / G;
  for (int item = bid * GROUPS + grp; item < n_items; item += nblk * GROUPS) {
    // (gathers grouped by what they depend on, as in ld_move_kernel: list -> {refsize, ref, k, comm, indptr}[v] ->
    // {Ktot[a], indices, wq} -> {comm, ref}[u] -> {Kref, refsize, Eref}[c]; most launches of a refinement are short
    // lists whose time IS the length of this chain)
    const int w = sub_list ? sub_list[item] : item;
    const int v = list[w];
    const int rs_v = refsize[v], ref_v = ref[v];
    const long long kq = k[v];
    const int a = comm[v];
    const int64_t beg = indptr[v];
    const int64_t end = indptr[v + 1];
    const int deg = (int)(end - beg);
    if (deg > GMAX) continue;  // a long row: on the list of another tier (list_long_rows), which writes target[v]
    int tgt = -1;
    if (rs_v != 1 || ref_v != v) {
      tgt = -2;
    } else {
      int u_pre[2];
      long long w_pre[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int e = sub + t * G;
        u_pre[t] = e < deg ? indices[beg + e] : v;
        w_pre[t] = e < deg ? wq[beg + e] : 0ll;
      }
      const double KC = (double)(long long)Ktot[a];
      int cm_pre[2], rf_pre[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const VertRec r = vr[u_pre[t]];
        cm_pre[t] = r.comm;
        rf_pre[t] = r.ref;
      }
      const double kv = (double)kq;
      Cand best = cand_none();
      int* keys = hkeys + grp * GSLOTS;
      unsigned long long* vals = hvals + grp * GSLOTS;
      const int nslots = G < 64 ? (deg <= 48 ? 64 : 128) : (deg <= 96 ? 128 : (deg <= 192 ? 256 : 512));
      for (int i = sub; i < nslots; i += G) {
        keys[i] = WH_EMPTY;
        vals[i] = 0ull;
      }
      auto insert = [&](int c, long long wt) {
        unsigned int slot = hash32((unsigned int)c) & (nslots - 1);
        for (;;) {
          const int prev = atomicCAS(&keys[slot], WH_EMPTY, c);
          if (prev == WH_EMPTY || prev == c) break;
          slot = (slot + 1) & (nslots - 1);
        }
        atomicAdd(&vals[slot], (unsigned long long)wt);
      };
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (sub + t * G < deg && u_pre[t] != v && cm_pre[t] == a) insert(rf_pre[t], w_pre[t]);
      for (int e = sub + 2 * G; e < deg; e += G) {
        const int u = indices[beg + e];
        const VertRec r = vr[u];
        if (u != v && r.comm == a) insert(r.ref, wq[beg + e]);
      }
      constexpr int MAXSL = GSLOTS / G;
      int cs[MAXSL], rsz[MAXSL];
      unsigned long long kr[MAXSL], er[MAXSL];
#pragma unroll
      for (int t = 0; t < MAXSL; ++t) cs[t] = WH_EMPTY;
#pragma unroll
      for (int t = 0; t < MAXSL; ++t) {
        const int sl = sub + t * G;
        if (__ballot(sl < nslots)) {  // (see ld_move_kernel: uniform skip, no per-lane branch around the gathers)
          int c = sl < nslots ? __hip_atomic_load(&keys[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : WH_EMPTY;
          if (c == v) c = WH_EMPTY;
          cs[t] = c;
          const int ci = c != WH_EMPTY ? c : v;
          const TargRec x = tr[ci];  // one 32-byte record per target instead of three gathers
          kr[t] = x.Kref;
          rsz[t] = x.refsize;
          er[t] = x.Eref;
        }
      }
#pragma unroll
      for (int t = 0; t < MAXSL; ++t) {
        const int c = cs[t];
        if (c != WH_EMPTY) {
          const long long sum =
              (long long)__hip_atomic_load(&vals[sub + t * G], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          Cand x;
          if (refine_cand(rule, v, kv, KC, c, sum, kr[t], rsz[t], er[t], &x) && cand_better(x, best)) best = x;
        }
      }
      best = group_best<G>(best);
      tgt = refine_verdict(rule, v, best);
    }
    if (sub == 0) pa.target[v] = tgt;
  }
}

// The proposal of the candidate at position w of the class list by a whole workgroup (block tier: 256 threads, giant: 1024).
__device__ __forceinline__ void ld_refine_propose_hub_row(const ProposeArgs& pa, int w, BlockHash& bh, const HubTry& ht,
                                                          Cand* sh_c, long long* sh_w, int* sh_fail) {
  const int v = pa.list[w];
  if (pa.refsize[v] != 1 || pa.ref[v] != v) {  // no longer a singleton (the same for every thread: no barrier is skipped by some)
    if (threadIdx.x == 0) pa.target[v] = -2;
    return;
  }
  const double kv = (double)pa.k[v];
  const int a = pa.comm[v];
  const double KC = (double)(long long)pa.Ktot[a];
  const int64_t beg = pa.indptr[v];
  const int deg = (int)(pa.indptr[v + 1] - beg);
  const int* __restrict__ urow = pa.indices + beg;
  Cand best = cand_none();
  long long dummy = 0;
  hub_row(
      bh, deg, pa.wq + beg, ht, sh_fail,
      [&](int e) {
        const int u = urow[e];
        const VertRec r = pa.vr[u];
        return (u == v || r.comm != a) ? WH_EMPTY : r.ref;
      },
      [&](int c, long long sum) {
        if (c == v) return;
        const TargRec t = pa.tr[c];
        Cand x;
        if (refine_cand(pa.rule, v, kv, KC, c, sum, t.Kref, t.refsize, t.Eref, &x) && cand_better(x, best)) best = x;
      });
  best = block_best(best, dummy, sh_c, sh_w);
  if (threadIdx.x == 0) pa.target[v] = refine_verdict(pa.rule, v, best);
  __syncthreads();
}
// Giant tier of the refinement (see ld_move_hub_kernel)
__global__ __launch_bounds__(HUB_THREADS) void ld_refine_propose_hub_kernel(ProposeArgs pa, HubTry ht) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long hub_smem[];
  BlockHash bh{reinterpret_cast<int*>(hub_smem + BHUB_SLOTS), hub_smem, BHUB_SLOTS};
  __shared__ Cand sh_c[HUB_THREADS / 64];
  __shared__ long long sh_w[HUB_THREADS / 64];
  __shared__ int sh_fail;
  for (int i = blockIdx.x; i < pa.tl.n_giant; i += gridDim.x)
    ld_refine_propose_hub_row(pa, pa.tl.giant[i], bh, ht, sh_c, sh_w, &sh_fail);
}
// All tiers of a sub-round's proposals that a 256-thread workgroup can take, as block ranges of one grid (see ld_move_tiers)
template <int G>
__global__ __launch_bounds__(256) void ld_refine_propose_kernel(ProposeArgs pa) {
  __shared__ TierLds lds;
  const TierLists& tl = pa.tl;
  int bid = (int)blockIdx.x;
  if (bid < tl.nb_main) {
    ld_refine_propose_body<G>(bid, tl.nb_main, pa, nullptr, pa.n_act, lds.hkeys, lds.hvals);
    return;
  }
  bid -= tl.nb_main;
  if constexpr (G < 64) {
    if (bid < tl.nb_wave) {
      ld_refine_propose_body<64>(bid, tl.nb_wave, pa, tl.mid, tl.n_mid, lds.hkeys, lds.hvals);
      return;
    }
  }
  bid -= tl.nb_wave;
  BlockHash bh{lds.hkeys, lds.hvals, BLK_SLOTS, BLK_SLOTS};
  const HubTry no_try{nullptr, 0};
  for (int i = bid; i < tl.n_blk; i += tl.nb_blk)
    ld_refine_propose_hub_row(pa, tl.blk_last[-i], bh, no_try, lds.sh_c, lds.sh_w, &lds.sh_fail);
}

// counters: the sub-round's counter block; [CTR_JOINED] merges of this sub-round (= joiner list length)
__global__ void ld_refine_apply_kernel(int n_cand, const int* __restrict__ list, const int* __restrict__ target,
                                       const long long* __restrict__ k, int* __restrict__ ref,
                                       int* __restrict__ refsize, unsigned long long* __restrict__ Kref,
                                       unsigned long long* __restrict__ Eref, int* __restrict__ stamp, int round,
                                       int* __restrict__ jlist, int* __restrict__ counters, VertRec* __restrict__ vr,
                                       TargRec* __restrict__ tr) {
  const int lane = threadIdx.x & 63;
  for (int w0 = blockIdx.x * blockDim.x; w0 < n_cand; w0 += gridDim.x * blockDim.x) {
    const int w = w0 + threadIdx.x;
    const int v = (w < n_cand) ? list[w] : -1;
    const int t = (v >= 0) ? target[v] : -2;
    // list appends are aggregated per wave: one returning atomic per wave instead of one per element
    const unsigned long long mj = __ballot(t >= 0);
    int bj = 0;
    if (lane == 0 && mj) bj = atomicAdd(&counters[CTR_JOINED], __popcll(mj));
    bj = __shfl(bj, 0);
    if (t >= 0) {
      // v is a singleton (ref[v] == v) joining t; t's members do not move in this sub-round
      ref[v] = t;
      atomicAdd(&refsize[t], 1);
      atomicAdd(&Kref[t], (unsigned long long)k[v]);
      refsize[v] = 0;
      Kref[v] = 0;
      Eref[v] = 0;
      stamp[v] = round;
      // the packed mirrors (v's community field does not change during the refinement)
      vr[v].ref = t;
      vr[v].stamp = round;
      atomicAdd(&tr[t].refsize, 1);
      atomicAdd(&tr[t].Kref, (unsigned long long)k[v]);
      tr[v].Kref = 0;
      tr[v].Eref = 0;
      tr[v].refsize = 0;
      jlist[bj + __popcll(mj & ((1ull << lane) - 1ull))] = v;
    }
  }
}

__global__ void ld_refine_init_kernel(int n, const long long* __restrict__ k, const long long* __restrict__ a_in,
                                      const int* __restrict__ comm, int* __restrict__ ref, int* __restrict__ refsize,
                                      unsigned long long* __restrict__ Kref, unsigned long long* __restrict__ Eref,
                                      VertRec* __restrict__ vr, TargRec* __restrict__ tr, int* __restrict__ touched,
                                      int* __restrict__ rc0, int rc0_words, int* __restrict__ counters) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0) {  // class list lengths + per-sub-round counters of this refinement, phase counters
    for (int i = threadIdx.x; i < rc0_words; i += blockDim.x) rc0[i] = 0;
    if (threadIdx.x < PH_PER_PHASE) counters[threadIdx.x] = 0;
  }
  if (v < n) {
    touched[v] = -1;  // join sub-round stamps: -1 = never
    ref[v] = v;
    refsize[v] = 1;
    Kref[v] = (unsigned long long)k[v];
    Eref[v] = (unsigned long long)a_in[v];  // singleton: w(v, C - v)
    vr[v] = VertRec{comm[v], v, -1, 0};
    tr[v] = TargRec{(unsigned long long)k[v], (unsigned long long)a_in[v], 1, 0, 0, 0};
  }
}

// Test entry scamd_leiden_debug_level_f32 with a caller-supplied refined partition: ref[v] = given[v]; *err |= 1 when an id
// lies outside [0, n), |= 2 when a group is not named by one of its members or does not lie inside one community of `comm`
__global__ void ld_given_ref_kernel(int n, const int* __restrict__ given, const int* __restrict__ comm, int* __restrict__ ref,
                                    int* __restrict__ err) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int r = given[v];
  if (r < 0 || r >= n) {
    atomicOr(err, 1);
    ref[v] = v;
    return;
  }
  if (given[r] != r || comm[r] != comm[v]) atomicOr(err, 2);
  ref[v] = r;
}

// ---- phase 3: aggregation --------------------------------------------------------------------------
__global__ void ld_flag_kernel(int n, const int* __restrict__ size, int* __restrict__ flag, int* __restrict__ fill_max) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) {
    flag[v] = size[v] > 0 ? 1 : 0;
    if (fill_max) fill_max[v] = 0x7f7f7f7f;  // (`rep`: the atomicMin target of ld_coarse_ids_kernel)
  }
}

// coarse id of every node + representative coarse id of its phase-1 community (min over its members)
__global__ __launch_bounds__(1024) void ld_coarse_ids_kernel(int n, const int* __restrict__ ref,
                                                             const int64_t* __restrict__ newid_of_ref,
                                                             const int* __restrict__ comm, int* __restrict__ cid,
                                                             int* __restrict__ rep) {
  __shared__ int keys[BH_SLOTS];
  __shared__ int mn[BH_SLOTS];
  for (int i = threadIdx.x; i < BH_SLOTS; i += 1024) {
    keys[i] = BH_EMPTY;
    mn[i] = 0x7fffffff;
  }
  __syncthreads();
  // (at most COUNT_GRID workgroups, as ld_totals_kernel: each ends with one atomicMin per community it saw)
  for (int v = blockIdx.x * 1024 + threadIdx.x; v < n; v += gridDim.x * 1024) {
    const int c = (int)newid_of_ref[ref[v]];
    cid[v] = c;
    const int cm = comm[v];
    const int slot = bh_find_slot(keys, cm);
    if (slot >= 0) atomicMin(&mn[slot], c);
    else atomicMin(&rep[cm], c);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BH_SLOTS; i += 1024)
    if (keys[i] != BH_EMPTY) atomicMin(&rep[keys[i]], mn[i]);
}
// the same representatives from a STORED vertex map (a level that reuses the stored hierarchy: no refinement has run, `cid` is
// the map of the iteration that built the level)
__global__ __launch_bounds__(1024) void ld_coarse_rep_kernel(int n, const int* __restrict__ cid, const int* __restrict__ comm,
                                                             int* __restrict__ rep) {
  __shared__ int keys[BH_SLOTS];
  __shared__ int mn[BH_SLOTS];
  for (int i = threadIdx.x; i < BH_SLOTS; i += 1024) {
    keys[i] = BH_EMPTY;
    mn[i] = 0x7fffffff;
  }
  __syncthreads();
  for (int v = blockIdx.x * 1024 + threadIdx.x; v < n; v += gridDim.x * 1024) {
    const int c = cid[v];
    const int cm = comm[v];
    const int slot = bh_find_slot(keys, cm);
    if (slot >= 0) atomicMin(&mn[slot], c);
    else atomicMin(&rep[cm], c);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BH_SLOTS; i += 1024)
    if (keys[i] != BH_EMPTY) atomicMin(&rep[keys[i]], mn[i]);
}
// SCAMD_LEIDEN_DEBUG, before a level is reused: the stored groups must be nested in the current partition.  Pass 0 notes the
// community of one member per group (whichever write lands), pass 1 compares every member against it.
__global__ void ld_nest_check_kernel(int n, int nn, const int* __restrict__ cid, const int* __restrict__ comm,
                                     int* __restrict__ group_comm, int pass, int* __restrict__ err) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int c = cid[v];
  if (c < 0 || c >= nn) {
    if (pass == 0) atomicOr(err, 2);
    return;
  }
  if (pass == 0) group_comm[c] = comm[v];
  else if (group_comm[c] != comm[v]) atomicOr(err, 1);
}
__global__ void ld_coarse_comm_kernel(int n, const int* __restrict__ cid, const int* __restrict__ comm,
                                      const int* __restrict__ rep, int* __restrict__ comm_new, int nn,
                                      int* __restrict__ cursor, int* __restrict__ counters) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) comm_new[cid[v]] = rep[comm[v]];
  if (v < nn) cursor[v] = 0;  // (nn <= n: fill cursors of the member scatter)
  if (v < PH_PER_PHASE) counters[v] = 0;
}
__global__ void ld_remap_kernel(int n_orig, const int* __restrict__ cid, int* __restrict__ node_of) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_orig) node_of[i] = cid[node_of[i]];
}

// Coarse-graph construction, member-grouped: the members of every coarse node are gathered contiguously
// (counting sort by coarse id), then ONE wave / workgroup per coarse node accumulates its members' rows into an
// LDS hash keyed by the neighbour's coarse id and emits the combined row.  No global hash table and no global
// atomics on the edges: the level-0 graph (24M entries) is read once, sequentially per member.
//   rows land at an upper-bound offset (sum of the members' degrees) in a scratch CSR and are compacted after
//   the row lengths are scanned.
constexpr int AGG_MID_SLOTS = 4096;   // workgroup tier for <= 2048 distinct neighbours (48 KB LDS: 3 blocks/CU)
constexpr int AGG_MID_MAX = 2048;
constexpr int AGG_BIG_PASS = 4096;    // the 8192-slot tier takes ~4096 distinct keys per pass

__global__ void ld_agg_mcount_kernel(int n, const int* __restrict__ refsize, const int64_t* __restrict__ newid,
                                     int* __restrict__ mcount) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n && refsize[r] > 0) mcount[(int)newid[r]] = refsize[r];
}

__global__ void ld_agg_scatter_kernel(int n, const int* __restrict__ cid, const int64_t* __restrict__ moff,
                                      int* __restrict__ cursor, const int64_t* __restrict__ indptr,
                                      int* __restrict__ members, int* __restrict__ mdeg) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int c = cid[v];
  const int64_t p = moff[c] + atomicAdd(&cursor[c], 1);
  members[p] = v;
  mdeg[p] = (int)(indptr[v + 1] - indptr[v]);
}

// distinct neighbours of a coarse node are bounded by both its degree sum and the coarse node count
__device__ __forceinline__ int64_t agg_need(int64_t dsum, int nn) { return dsum < nn ? dsum : (int64_t)nn; }
// a split row's parts are merged through ONE 8192-slot table: every key of the level must fit it (load <= 0.69)
constexpr int AGG_SPLIT_NN_MAX = 5600;

// one wave per coarse node; nodes needing more than the wave table go to the mid / big lists
// (counters[PH_AGG_MID] / counters[PH_AGG_BIG]); rows to be split go to split_list (counters[PH_AGG_SPLIT])
__global__ __launch_bounds__(256) void ld_agg_wave_kernel(
    int nn, const int64_t* __restrict__ moff, const int64_t* __restrict__ eoff, const int* __restrict__ members,
    const int64_t* __restrict__ indptr, const int* __restrict__ indices, const long long* __restrict__ wq,
    const int* __restrict__ cid, int* __restrict__ s_col, long long* __restrict__ s_w, int* __restrict__ rowcnt,
    int* __restrict__ mid_list, int* __restrict__ big_list, int* __restrict__ counters, int wave_max, int mid_max,
    int wave_work, int mid_work, int* __restrict__ split_list, int64_t split_work) {
  __shared__ int hkeys[4][WH_SLOTS];
  __shared__ unsigned long long hvals[4][WH_SLOTS];
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= nn) return;
  const int64_t m0 = moff[c], m1 = moff[c + 1];
  const int64_t u0 = eoff[m0];
  const int64_t dsum = eoff[m1] - u0;
  const int64_t need = agg_need(dsum, nn);
  // tiers by table size (distinct neighbours: `need`) AND by work (member entries: `dsum`).  Round 5: on the coarse levels of
  // a graph without clear clusters a coarse vertex has few distinct neighbours (need <= nn, a few hundred) but tens of
  // thousands of member entries -- one wave walked them all (this kernel was 26 % of the Leiden time on the weak 1M graph,
  // single launches of up to 7.9 ms); rows beyond wave_work entries go to a workgroup, beyond mid_work to the 1024-thread one
  if (need > wave_max || dsum > wave_work) {
    if (lane == 0) {
      // (the very largest rows of a coarse level -- ~1e6 member entries behind a few hundred distinct neighbours -- are cut
      // into parts for several workgroups and merged: ld_agg_parts_kernel; only where one table holds every key of the level)
      if (dsum > split_work && nn <= AGG_SPLIT_NN_MAX) split_list[atomicAdd(&counters[PH_AGG_SPLIT], 1)] = c;
      else if (need <= mid_max && dsum <= mid_work) mid_list[atomicAdd(&counters[PH_AGG_MID], 1)] = c;
      else big_list[atomicAdd(&counters[PH_AGG_BIG], 1)] = c;
    }
    return;
  }
  WaveHash wh{hkeys[threadIdx.x >> 6], hvals[threadIdx.x >> 6], WH_SLOTS};
  wh.size_for((int)need);
  wh.clear(lane);
  // The members' row extents are fetched 64 at a time (one coalesced gather), then two rows are in flight at once:
  // walking the members one by one is a chain members -> indptr -> indices -> cid per 24-entry row with nothing else
  // in flight.
  for (int64_t i0 = m0; i0 < m1; i0 += 64) {
    const int cnt = (int)(m1 - i0 < 64 ? m1 - i0 : 64);
    long long mb = 0, me = 0;
    if (lane < cnt) {
      const int v = members[i0 + lane];
      mb = indptr[v];
      me = indptr[v + 1];
    }
    for (int j = 0; j < cnt; j += 2) {
      const int j1 = j + 1 < cnt ? j + 1 : j;
      const long long b0 = readlane_i64(mb, j), e0 = readlane_i64(me, j);
      const long long b1 = readlane_i64(mb, j1), e1 = j1 != j ? readlane_i64(me, j1) : b1;
      const bool h0 = b0 + lane < e0, h1 = b1 + lane < e1;
      const int x0 = h0 ? indices[b0 + lane] : 0, x1 = h1 ? indices[b1 + lane] : 0;
      const long long w0 = h0 ? wq[b0 + lane] : 0ll, w1 = h1 ? wq[b1 + lane] : 0ll;
      const int c0 = cid[x0], c1 = cid[x1];
      if (h0) wh.add(c0, w0);
      if (h1) wh.add(c1, w1);
      for (int64_t e = b0 + 64 + lane; e < e0; e += 64) wh.add(cid[indices[e]], wq[e]);
      for (int64_t e = b1 + 64 + lane; e < e1; e += 64) wh.add(cid[indices[e]], wq[e]);
    }
  }
  int base = 0;
  for (int s0 = 0; s0 < wh.nslots; s0 += 64) {
    const int key = wh.key(s0 + lane);
    const bool has = key != WH_EMPTY;
    const unsigned long long m = __ballot(has);
    if (has) {
      const int64_t p = u0 + base + __popcll(m & ((1ull << lane) - 1ull));
      s_col[p] = key;
      s_w[p] = wh.val(s0 + lane);
    }
    base += __popcll(m);
  }
  if (lane == 0) rowcnt[c] = base;
}

// one workgroup per listed coarse node.  SLOTS-entry LDS table; when the node may have more distinct neighbours
// than pass_keys the keys are split into hash classes and the members' rows are swept once per class.
template <int SLOTS, int THREADS>
__global__ __launch_bounds__(THREADS) void ld_agg_block_kernel(
    const int* __restrict__ list, const int* __restrict__ list_len, int nn, const int64_t* __restrict__ moff,
    const int64_t* __restrict__ eoff, const int* __restrict__ members, const int64_t* __restrict__ indptr,
    const int* __restrict__ indices, const long long* __restrict__ wq, const int* __restrict__ cid,
    int* __restrict__ s_col, long long* __restrict__ s_w, int* __restrict__ rowcnt, int* __restrict__ err,
    int pass_keys, int try_probes) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long agg_smem[];
  unsigned long long* vals = agg_smem;
  int* keys = reinterpret_cast<int*>(agg_smem + SLOTS);
  __shared__ int sh_cnt, sh_fail;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n_list = *list_len;
  for (int li = blockIdx.x; li < n_list; li += gridDim.x) {
    const int c = list[li];
    const int64_t m0 = moff[c], m1 = moff[c + 1];
    const int64_t u0 = eoff[m0];
    const int64_t need = agg_need(eoff[m1] - u0, nn);
    // (a part of a split row may be empty -- a member row longer than the part size spans several cuts: need = 0)
    const unsigned int n_pass = (unsigned int)std::max<int64_t>(1, (need + pass_keys - 1) / pass_keys);
    int nslots = 256;
    {
      const int64_t per_pass = (need + n_pass - 1) / n_pass;
      while (nslots < 2 * per_pass && nslots < SLOTS) nslots <<= 1;
      if (n_pass > 1) nslots = SLOTS;
    }
    if (threadIdx.x == 0) {
      sh_cnt = 0;
      sh_fail = 0;
    }
    // pass -1 (rows that would need several passes): ONE optimistic pass over all keys with bounded probing -- the bound
    // `need` is the members' entry count or the coarse vertex count, the distinct neighbours are usually far fewer (the
    // comment at HUB_TRY_PROBES); if a key finds no slot the class-by-class passes 0 .. n_pass - 1 follow as before
    for (int pass = ((n_pass > 1 && try_probes > 0) ? -1 : 0); pass < (int)n_pass; ++pass) {
      for (int i = threadIdx.x; i < nslots; i += THREADS) {
        keys[i] = WH_EMPTY;
        vals[i] = 0ull;
      }
      __syncthreads();
      // the extent of a wave's next member row is requested while the current row is walked
      int64_t nb = 0, ne = 0;
      if (m0 + wv < m1) {
        const int v = members[m0 + wv];
        nb = indptr[v];
        ne = indptr[v + 1];
      }
      for (int64_t i = m0 + wv; i < m1; i += THREADS / 64) {
        if (pass < 0 && __hip_atomic_load(&sh_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;  // (trial lost)
        const int64_t rb = nb, re = ne;
        if (i + THREADS / 64 < m1) {
          const int vn = members[i + THREADS / 64];
          nb = indptr[vn];
          ne = indptr[vn + 1];
        }
        auto add_entry = [&](int key, long long we) {
          if (pass >= 0 && n_pass > 1 && (hash32((unsigned int)key * 0x9E3779B1u + 0x7F4A7C15u) >> 8) % n_pass != (unsigned int)pass) return;
          unsigned int slot = hash32((unsigned int)key) & (nslots - 1);
          const int max_tries = pass < 0 ? try_probes : nslots;
          int tries = 0;
          for (;;) {
            const int prev = atomicCAS(&keys[slot], WH_EMPTY, key);
            if (prev == WH_EMPTY || prev == key) {
              atomicAdd(&vals[slot], (unsigned long long)we);
              break;
            }
            slot = (slot + 1) & (nslots - 1);
            if (++tries > max_tries) {
              // trial pass: fall back to the class passes; class pass: table full -- cannot happen for uniformly
              // hashed classes; reported, not hidden
              if (pass < 0) __hip_atomic_store(&sh_fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              else *err = 1;
              break;
            }
          }
        };
        // Long member rows (the coarse levels of a graph without clear clusters: thousands of entries per row, a million
        // per coarse vertex) were walked 64 entries per dependent round trip (indices -> cid): four steps' loads are
        // requested before the first is used (round 5)
        int64_t e = rb + lane;
        for (; e + 192 < re; e += 256) {
          const int x0 = indices[e], x1 = indices[e + 64], x2 = indices[e + 128], x3 = indices[e + 192];
          const long long w0 = wq[e], w1 = wq[e + 64], w2 = wq[e + 128], w3 = wq[e + 192];
          const int k0 = cid[x0], k1 = cid[x1], k2 = cid[x2], k3 = cid[x3];
          add_entry(k0, w0);
          add_entry(k1, w1);
          add_entry(k2, w2);
          add_entry(k3, w3);
        }
        for (; e < re; e += 64) add_entry(cid[indices[e]], wq[e]);
      }
      __syncthreads();
      if (pass < 0 && sh_fail) continue;  // (read by every thread after the barrier: uniform)
      for (int s0 = 0; s0 < nslots; s0 += THREADS) {
        const int sl = s0 + threadIdx.x;
        const int key = sl < nslots ? keys[sl] : WH_EMPTY;  // the table in use may be shorter than the workgroup
        const bool has = key != WH_EMPTY;
        const unsigned long long m = __ballot(has);
        int wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&sh_cnt, __popcll(m));
        wbase = __shfl(wbase, 0);
        if (has) {
          const int64_t p = u0 + wbase + __popcll(m & ((1ull << lane) - 1ull));
          s_col[p] = key;
          s_w[p] = (long long)vals[sl];
        }
      }
      __syncthreads();
      if (pass < 0) break;  // the one pass held every key
    }
    if (threadIdx.x == 0) rowcnt[c] = sh_cnt;
    __syncthreads();
  }
}

// Split rows (round 5).  A launch of the workgroup builders lasts as long as its longest row, and on the coarse levels of a
// graph without clear clusters a few coarse vertices hold ~1e6 member entries each (ld_agg_block_kernel<8192, 1024>: launches
// of 1-3.5 ms, 10-13 % of the Leiden time on the weak / structure-less 1M graphs).  Such a row is cut into PARTS of ~chunk
// member entries (whole member rows: the cut points are found by bisection in the members' entry offsets); every part is
// built like a row of its own by ld_agg_block_kernel -- the parts are given pseudo-row ids whose member ranges live in
// `pmoff` (one extra slot per row closes its last part), their lists land at their own members' scratch offsets -- and one
// workgroup per split row merges the parts' lists through a table and writes the row.  Integer sums: the row is the same.
__global__ void ld_agg_parts_kernel(const int* __restrict__ split_list, int* __restrict__ counters, const int64_t* __restrict__ moff,
                                    const int64_t* __restrict__ eoff, int64_t chunk, int64_t* __restrict__ pmoff,
                                    int* __restrict__ part_list, int* __restrict__ split_first, int* __restrict__ split_np) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= counters[PH_AGG_SPLIT]) return;
  const int c = split_list[s];
  const int64_t m0 = moff[c], m1 = moff[c + 1];
  const int64_t u0 = eoff[m0], dsum = eoff[m1] - u0;
  const int np = (int)((dsum + chunk - 1) / chunk);
  const int base = atomicAdd(&counters[PH_AGG_PART_SLOTS], np + 1);
  split_first[s] = base;
  split_np[s] = np;
  for (int j = 0; j < np; ++j) {
    int64_t lo = m0;
    if (j > 0) {  // first member whose entries start at or after the j-th cut
      const int64_t target = u0 + (int64_t)j * chunk;
      int64_t hi = m1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (eoff[mid] < target) lo = mid + 1;
        else hi = mid;
      }
    }
    pmoff[base + j] = lo;
    part_list[atomicAdd(&counters[PH_AGG_PARTS], 1)] = base + j;
  }
  pmoff[base + np] = m1;
}

__global__ __launch_bounds__(1024) void ld_agg_merge_kernel(const int* __restrict__ split_list, const int* __restrict__ counters,
                                                            const int64_t* __restrict__ moff, const int64_t* __restrict__ eoff,
                                                            const int64_t* __restrict__ pmoff, const int* __restrict__ part_cnt,
                                                            const int* __restrict__ split_first, const int* __restrict__ split_np,
                                                            int* __restrict__ s_col, long long* __restrict__ s_w,
                                                            int* __restrict__ rowcnt, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long agg_smem[];
  unsigned long long* vals = agg_smem;
  int* keys = reinterpret_cast<int*>(agg_smem + BHUB_SLOTS);
  __shared__ int sh_cnt;
  const int lane = threadIdx.x & 63;
  const int n_split = counters[PH_AGG_SPLIT];
  for (int s = blockIdx.x; s < n_split; s += gridDim.x) {
    const int c = split_list[s];
    const int64_t u0 = eoff[moff[c]];
    const int first = split_first[s], np = split_np[s];
    for (int i = threadIdx.x; i < BHUB_SLOTS; i += 1024) {
      keys[i] = WH_EMPTY;
      vals[i] = 0ull;
    }
    if (threadIdx.x == 0) sh_cnt = 0;
    __syncthreads();
    for (int j = 0; j < np; ++j) {
      const int64_t up = eoff[pmoff[first + j]];
      const int cnt = part_cnt[first + j];
      for (int t = threadIdx.x; t < cnt; t += 1024) {
        const int key = s_col[up + t];
        const long long w = s_w[up + t];
        unsigned int slot = hash32((unsigned int)key) & (BHUB_SLOTS - 1);
        for (int tries = 0;; ++tries) {
          const int prev = atomicCAS(&keys[slot], WH_EMPTY, key);
          if (prev == WH_EMPTY || prev == key) {
            atomicAdd(&vals[slot], (unsigned long long)w);
            break;
          }
          slot = (slot + 1) & (BHUB_SLOTS - 1);
          if (tries > BHUB_SLOTS) {  // (cannot happen: at most AGG_SPLIT_NN_MAX distinct keys; reported, not hidden)
            *err = 1;
            break;
          }
        }
      }
    }
    __syncthreads();  // every partial list has been read: the row is written over them
    for (int s0 = 0; s0 < BHUB_SLOTS; s0 += 1024) {
      const int sl = s0 + threadIdx.x;
      const int key = keys[sl];
      const bool has = key != WH_EMPTY;
      const unsigned long long m = __ballot(has);
      int wbase = 0;
      if (lane == 0 && m) wbase = atomicAdd(&sh_cnt, __popcll(m));
      wbase = __shfl(wbase, 0);
      if (has) {
        const int64_t p = u0 + wbase + __popcll(m & ((1ull << lane) - 1ull));
        s_col[p] = key;
        s_w[p] = (long long)vals[sl];
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) rowcnt[c] = sh_cnt;
    __syncthreads();
  }
}

// scratch rows (upper-bound offsets) -> final CSR rows; one wave per coarse node
__global__ __launch_bounds__(256) void ld_agg_compact_kernel(int nn, const int64_t* __restrict__ moff,
                                                             const int64_t* __restrict__ eoff,
                                                             const int64_t* __restrict__ indptr_new,
                                                             const int* __restrict__ s_col,
                                                             const long long* __restrict__ s_w,
                                                             int* __restrict__ out_col, long long* __restrict__ out_w,
                                                             int* __restrict__ dstat) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) dstat[0] = 0;  // (longest row of the level being built: ld_degstats_kernel follows)
  if (c >= nn) return;
  const int64_t u0 = eoff[moff[c]];
  const int64_t p0 = indptr_new[c];
  const int cnt = (int)(indptr_new[c + 1] - p0);
  for (int i = lane; i < cnt; i += 64) {
    out_col[p0 + i] = s_col[u0 + i];
    out_w[p0 + i] = s_w[u0 + i];
  }
}

// ---- small levels: everything in ONE workgroup ---------------------------------------------------------
// The last levels of every run are tiny (planted 1M cells: 170, 80, 67, 64 nodes; the 700-cell fixture is such a level
// from the start): as separate kernels each of them costs ~65 launches and 5 host round trips = 0.5 ms of pure
// latency, ten such levels per call.  From the first level with at most SMALL_N nodes and SMALL_NNZ entries on, ONE
// workgroup runs local moving, refinement and aggregation of all remaining levels: the per-node state lives in LDS, the
// rows stay in global memory (written by this workgroup, read after a device-scope fence), 8 waves take 8 nodes at a
// time -- decide on a snapshot, barrier, apply, barrier -- so at most 8 nodes move at once, closer to the sequential
// algorithm than any class schedule (a node's neighbour weights are summed in a dense per-wave table indexed by
// community, with a touched list: no hashing, any row length).  Same arithmetic and same rules as the kernels above.
constexpr int SMALL_N = 1024;
constexpr int SMALL_NNZ = 65536;
constexpr int SM_WAVES = 8;
constexpr int SM_THREADS = SM_WAVES * 64;

struct SmallArgs {
  const int64_t* indptr;   // entry level
  const int* indices;
  const long long* wq;
  const long long* k;
  int n;
  int* ix[2];              // coarse levels, ping-pong
  long long* w[2];
  int first_dst;
  int* comm;               // in: partition of the entry nodes; out: final community of every entry node
  double gg;               // gamma / 2m
  double inv_beta;
  unsigned int seed;
  int iter;
  int lm_stop_permille;
  int seq_n;               // levels of at most this many vertices move one vertex at a time
  int* info;               // counters + PH_SMALL_INFO: [SM_INFO_LEVELS], [SM_INFO_MOVES], [SM_INFO_MERGES], [SM_INFO_NODES] of the last level
  // what the quality of the result needs, taken from the last level: totals[c], c < n, = the total vertex weight of
  // community c of the last level (0 from its vertex count on), internal[0] = the weight of its stored entries inside a community
  unsigned long long* totals;
  unsigned long long* internal;
};

struct SmallLds {
  unsigned long long acc[SM_WAVES][SMALL_N];
  unsigned short touched[SM_WAVES][SMALL_N];
  unsigned long long Ktot[SMALL_N];
  long long kk[SMALL_N];
  int ip[SMALL_N + 1];
  int comm[SMALL_N];
  int csize[SMALL_N];          // local moving: community sizes; aggregation: new partition of the coarse nodes
  unsigned short order[SMALL_N];
  unsigned short tail_of[SMALL_N];
  unsigned char flag[SMALL_N];
  int ref[SMALL_N];
  int refsize[SMALL_N];
  union {
    struct {
      unsigned long long Kref[SMALL_N];
      unsigned long long Eref[SMALL_N];
      long long a_in[SMALL_N];
      int stamp[SMALL_N];
    } rf;
    struct {
      int cid[SMALL_N];
      int members[SMALL_N];
      int moff[SMALL_N + 1];
      int rep[SMALL_N];
      int rowptr[SMALL_N + 1];
    } ag;
  } u;
  int tcnt[SM_WAVES];
  int dec[SM_WAVES];
  int rset[SM_WAVES];
  int scan_w[SM_WAVES];
  int s_n_act, s_moved, s_merged, s_nn;
  unsigned long long s_internal;
};
static_assert(sizeof(SmallLds) <= 160 * 1024, "SmallLds must fit the 160 KB of LDS");

// exclusive scan of x[0 .. n) (n <= 2 * SM_THREADS) in place; returns the total.  All threads call.
__device__ __forceinline__ int small_scan(int* x, int n, int* scan_w) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int i0 = 2 * t, i1 = 2 * t + 1;
  const int a0 = i0 < n ? x[i0] : 0, a1 = i1 < n ? x[i1] : 0;
  int inc = a0 + a1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o);
    if (lane >= o) inc += y;
  }
  if (lane == 63) scan_w[wv] = inc;
  __syncthreads();
  int off = 0, tot = 0;
  for (int i = 0; i < SM_WAVES; ++i) {
    const int s = scan_w[i];
    if (i < wv) off += s;
    tot += s;
  }
  const int ex = off + inc - (a0 + a1);
  if (i0 < n) x[i0] = ex;
  if (i1 < n) x[i1] = ex + a0;
  __syncthreads();
  return tot;
}

// flagged items of [0, n) -> order[0 .. count), ascending; returns count.  pred(v) evaluated by thread v % SM_THREADS.
template <typename P>
__device__ __forceinline__ int small_compact(int n, P pred, unsigned short* order, int* scan_w) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int base = 0;
  for (int v0 = 0; v0 < n; v0 += SM_THREADS) {
    const int v = v0 + t;
    const bool f = v < n && pred(v);
    const unsigned long long m = __ballot(f);
    if (lane == 0) scan_w[wv] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < SM_WAVES; ++i) {
      const int s = scan_w[i];
      if (i < wv) off += s;
      tot += s;
    }
    if (f) order[base + off + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)v;
    base += tot;
    __syncthreads();
  }
  return base;
}

constexpr int SMALL_SEQ_N = 16;   // levels of at most this many vertices: local moving one vertex at a time
__global__ __launch_bounds__(SM_THREADS) void ld_small_levels_kernel(SmallArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char small_smem[];
  SmallLds& L = *reinterpret_cast<SmallLds*>(small_smem);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n_in = a.n;
  int n = a.n;
  const int* ix = a.indices;
  const long long* wq = a.wq;
  int dst = a.first_dst;
  // ---- entry level into LDS
  for (int v = t; v < n; v += SM_THREADS) {
    L.ip[v] = (int)(a.indptr[v] - a.indptr[0]);
    L.kk[v] = a.k[v];
    L.comm[v] = a.comm[v];
    L.tail_of[v] = (unsigned short)v;
  }
  if (t == 0) L.ip[n] = (int)(a.indptr[n] - a.indptr[0]);
  ix += a.indptr[0];
  wq += a.indptr[0];
  for (int i = t; i < SM_WAVES * SMALL_N; i += SM_THREADS) (&L.acc[0][0])[i] = 0ull;
  __syncthreads();
  int levels = 0, tot_moves = 0, tot_merges = 0;
  unsigned long long* acc = L.acc[wv];
  unsigned short* touched = L.touched[wv];

  // weight from row v towards each distinct group key(u) of its neighbours u (u != v, pass(u)): dense table + touched
  // list of this wave; returns the number of distinct groups.  Entries of weight 0 carry nothing and are skipped (the
  // first-touch test is `old sum == 0`).
  auto gather_row = [&](int v, auto key, auto pass) -> int {
    if (lane == 0) L.tcnt[wv] = 0;
    const int beg = L.ip[v], end = L.ip[v + 1];
    for (int e = beg + lane; e < end; e += 64) {
      const int u = ix[e];
      const long long w = wq[e];
      if (u != v && w != 0 && pass(u)) {
        const int c = key(u);
        const unsigned long long old = atomicAdd(&acc[c], (unsigned long long)w);
        if (old == 0ull) touched[atomicAdd(&L.tcnt[wv], 1)] = (unsigned short)c;
      }
    }
    return __hip_atomic_load(&L.tcnt[wv], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };

  for (;;) {
    ++levels;
    // ================= local moving =================
    for (int c = t; c < n; c += SM_THREADS) {
      L.Ktot[c] = 0ull;
      L.csize[c] = 0;
      L.flag[c] = 1;
    }
    __syncthreads();
    for (int v = t; v < n; v += SM_THREADS) {
      atomicAdd(&L.Ktot[L.comm[v]], (unsigned long long)L.kk[v]);
      atomicAdd(&L.csize[L.comm[v]], 1);
    }
    __syncthreads();
    int moved_prev2 = 0, quiet = 0;
    for (int sweep = 0; sweep < MAX_LM_SWEEPS; ++sweep) {
      const int n_act = small_compact(n, [&](int v) { return L.flag[v] != 0; }, L.order, L.scan_w);
      if (n_act == 0) break;
      if (t == 0) L.s_moved = 0;
      int m = 1;
      while (m < n_act) m <<= 1;
      const unsigned int hs = hash32(a.seed + 0x85EBCA77u * (unsigned int)(sweep + 1) + 0xC2B2AE3Du * (unsigned int)a.iter +
                                     0x27D4EB2Fu * (unsigned int)levels);
      const unsigned int pa = hs | 1u, pb = hs >> 11;
      const int dir_round = sweep >= LM_DIR_AFTER ? sweep : -1;
      __syncthreads();
      // Vertices that decide in the same round do not see each other's moves.  Eight at a time is harmless among
      // hundreds of vertices; on the small DENSE graphs of the upper levels (every pair adjacent) it made neighbours swap
      // communities round after round -- found on the host emulator: a 2-vertex graph ended as two singletons
      // (Q = -0.5), 21 of 60 random graphs of <= 40 vertices below the CPU oracle.  There the vertices decide one at a
      // time, as in the sequential algorithm (a round is three barriers: 128 rounds cost less than one launch).
      const int par = n <= a.seq_n ? 1 : SM_WAVES;
      for (int r0 = 0; r0 < m; r0 += par) {
        const int pos = (int)(((unsigned int)(r0 + wv) * pa + pb) & (unsigned int)(m - 1));
        const int v = (wv < par && pos < n_act) ? (int)L.order[pos] : -1;
        int decision = -1;
        if (v >= 0) {
          const int ca = L.comm[v];
          const long long kq = L.kk[v];
          const double kv = (double)kq;
          const double Ka_wo = (double)(long long)(L.Ktot[ca] - (unsigned long long)kq);
          const int tc = gather_row(v, [&](int u) { return L.comm[u]; }, [&](int) { return true; });
          Cand best;
          best.val = 0.0;
          best.c = -1;
          best.pr = 0;
          long long w_own = 0;
          for (int i = lane; i < tc; i += 64) {
            const int c = touched[i];
            const long long sum = (long long)acc[c];
            acc[c] = 0ull;
            if (c == ca) {
              w_own = sum;
            } else {
              Cand x;
              x.val = (double)sum - a.gg * kv * (double)(long long)L.Ktot[c];
              x.c = c;
              x.pr = prio(c, a.seed);
              if (cand_better(x, best)) best = x;
            }
          }
          best = wave_best(best);
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) w_own = max(w_own, __shfl_xor(w_own, o));
          const double stay = (double)w_own - a.gg * kv * Ka_wo;
          if (best.c >= 0 && best.val > stay) {
            bool allowed = true;
            if (dir_round >= 0) {
              const unsigned int p0 = prio(ca, a.seed), p1 = best.pr;
              allowed = (dir_round & 1) ? (p1 > p0 || (p1 == p0 && best.c > ca)) : (p1 < p0 || (p1 == p0 && best.c < ca));
            }
            decision = allowed ? best.c : -2;
          } else if (stay < 0.0 && Ka_wo > 0.0 && L.csize[v] == 0) {
            decision = v;  // an empty community (its id = the node's own id) beats staying
          }
        }
        if (lane == 0) {
          L.dec[wv] = decision;
          if (v >= 0) L.flag[v] = 0;  // (cleared BEFORE the barrier: flags set by this round's movers must survive)
        }
        __syncthreads();
        if (v >= 0) {
          const int d = L.dec[wv];
          if (d == -2 && lane == 0) L.flag[v] = 1;  // blocked by the direction rule: stays active
          if (d >= 0) {
            if (lane == 0) {
              const int ca = L.comm[v];
              const unsigned long long kq = (unsigned long long)L.kk[v];
              L.comm[v] = d;
              atomicAdd(&L.Ktot[d], kq);
              atomicAdd(&L.Ktot[ca], 0ull - kq);
              atomicAdd(&L.csize[d], 1);
              atomicSub(&L.csize[ca], 1);
              atomicAdd(&L.s_moved, 1);
            }
          }
        }
        __syncthreads();
        if (v >= 0 && L.dec[wv] >= 0) {  // after every move of the round: re-activate the neighbours outside the new community
          const int d = L.dec[wv];
          for (int e = L.ip[v] + lane; e < L.ip[v + 1]; e += 64) {
            const int u = ix[e];
            if (L.comm[u] != d) L.flag[u] = 1;
          }
        }
        __syncthreads();
      }
      const int moved = L.s_moved;
      tot_moves += moved;
      __syncthreads();
      if (moved == 0 && dir_round < 0) break;
      quiet = moved == 0 ? quiet + 1 : 0;
      if (quiet >= 2) break;
      if (a.iter == 0 && sweep >= 1) {
        if ((long long)moved * 1000 < (long long)n * a.lm_stop_permille) break;
        if (sweep >= 2 && (long long)moved * 10 > (long long)moved_prev2 * 9) break;
      }
      moved_prev2 = moved;
    }
    __syncthreads();
    // ================= refinement =================
    for (int v0 = 0; v0 < n; v0 += SM_WAVES) {  // a_in[v] = w(v, C(v) - v)
      const int v = v0 + wv;
      if (v < n) {
        const int ca = L.comm[v];
        long long s = 0;
        for (int e = L.ip[v] + lane; e < L.ip[v + 1]; e += 64) {
          const int u = ix[e];
          if (u != v && L.comm[u] == ca) s += wq[e];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) {
          L.u.rf.a_in[v] = s;
          L.ref[v] = v;
          L.refsize[v] = 1;
          L.u.rf.Kref[v] = (unsigned long long)L.kk[v];
          L.u.rf.Eref[v] = (unsigned long long)s;
          L.u.rf.stamp[v] = -1;
        }
      }
    }
    if (t == 0) L.s_merged = 0;
    __syncthreads();
    const unsigned int rseed = a.seed + 0x9E3779B9u * (unsigned int)a.iter;
    const int n_cand = small_compact(n, [&](int v) {
      const double kv = (double)L.kk[v];
      const double KC = (double)(long long)L.Ktot[L.comm[v]];
      return (double)L.u.rf.a_in[v] >= a.gg * kv * (KC - kv);
    }, L.order, L.scan_w);
    if (n_cand > 0) {
      int m = 1;
      while (m < n_cand) m <<= 1;
      const unsigned int hs = hash32(rseed ^ (0x5bd1e995u + 0x27D4EB2Fu * (unsigned int)levels));
      const unsigned int pa = hs | 1u, pb = hs >> 11;
      int round = 0;
      for (int r0 = 0; r0 < m; r0 += SM_WAVES, ++round) {
        const int pos = (int)(((unsigned int)(r0 + wv) * pa + pb) & (unsigned int)(m - 1));
        int v = pos < n_cand ? (int)L.order[pos] : -1;
        if (v >= 0 && (L.refsize[v] != 1 || L.ref[v] != v)) v = -1;  // somebody joined it: no longer a singleton
        if (lane == 0) L.rset[wv] = v;
        __syncthreads();
        int tgt = -1;
        if (v >= 0) {
          const int ca = L.comm[v];
          const double kv = (double)L.kk[v];
          const double KC = (double)(long long)L.Ktot[ca];
          const int tc = gather_row(v, [&](int u) { return L.ref[u]; }, [&](int u) { return L.comm[u] == ca; });
          Cand best;
          best.val = 0.0;
          best.c = -1;
          best.pr = 0;
          for (int i = lane; i < tc; i += 64) {
            const int c = touched[i];
            const long long sum = (long long)acc[c];
            acc[c] = 0ull;
            if (c == v) continue;
            const double Kr = (double)(long long)L.u.rf.Kref[c];
            bool ok = (double)(long long)L.u.rf.Eref[c] >= a.gg * Kr * (KC - Kr);  // target well connected
            if (ok && L.refsize[c] == 1) {  // a singleton that proposes in this very round may leave: not a target
#pragma unroll
              for (int j = 0; j < SM_WAVES; ++j) ok = ok && L.rset[j] != c;
            }
            const double gain = (double)sum - a.gg * kv * Kr;
            if (ok && gain >= 0.0) {
              Cand x;
              x.val = a.inv_beta > 0.0 ? gain * a.inv_beta + refine_noise(v, c, round, rseed) : gain;
              x.c = c;
              x.pr = prio(c, rseed);
              if (cand_better(x, best)) best = x;
            }
          }
          best = wave_best(best);
          tgt = best.c;
          if (a.inv_beta > 0.0 && tgt >= 0 && !(best.val > refine_noise(v, v, round, rseed))) tgt = -1;  // "stay" drawn
        }
        __syncthreads();  // every proposal of the round is made before any is applied
        if (v >= 0 && tgt >= 0 && lane == 0) {
          L.ref[v] = tgt;
          atomicAdd(&L.refsize[tgt], 1);
          atomicAdd(&L.u.rf.Kref[tgt], (unsigned long long)L.kk[v]);
          L.refsize[v] = 0;
          L.u.rf.Kref[v] = 0ull;
          L.u.rf.Eref[v] = 0ull;
          L.u.rf.stamp[v] = round;
          atomicAdd(&L.s_merged, 1);
        }
        __syncthreads();
        if (v >= 0 && tgt >= 0) {  // exact update of w(t, C - t): see ld_refine_cut_update_kernel
          const int ca = L.comm[v];
          long long s = 0;
          for (int e = L.ip[v] + lane; e < L.ip[v + 1]; e += 64) {
            const int u = ix[e];
            if (u != v && L.comm[u] == ca && L.ref[u] == tgt) s += (L.u.rf.stamp[u] == round) ? wq[e] : 2 * wq[e];
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
          if (lane == 0) atomicAdd(&L.u.rf.Eref[tgt], (unsigned long long)(L.u.rf.a_in[v] - s));
        }
        __syncthreads();
      }
    }
    __syncthreads();
    const int merged = L.s_merged;
    tot_merges += merged;
    if (merged == 0) break;
    // ================= aggregation =================
    __syncthreads();
    for (int r = t; r < n; r += SM_THREADS) L.u.ag.rowptr[r] = L.refsize[r] > 0 ? 1 : 0;  // (rowptr as scratch: new ids)
    __syncthreads();
    const int nn = small_scan(L.u.ag.rowptr, n, L.scan_w);
    if (nn == n) break;
    for (int v = t; v < n; v += SM_THREADS) L.u.ag.rep[v] = 0x7fffffff;
    __syncthreads();
    for (int v = t; v < n; v += SM_THREADS) {
      const int c = L.u.ag.rowptr[L.ref[v]];
      L.u.ag.cid[v] = c;
      atomicMin(&L.u.ag.rep[L.comm[v]], c);
    }
    __syncthreads();
    for (int r = t; r < n; r += SM_THREADS)
      if (L.refsize[r] > 0) L.u.ag.moff[L.u.ag.rowptr[r]] = L.refsize[r];  // member counts per coarse node
    for (int v = t; v < n; v += SM_THREADS) L.csize[L.u.ag.cid[v]] = L.u.ag.rep[L.comm[v]];  // partition of the coarse nodes
    for (int i = t; i < n_in; i += SM_THREADS) L.tail_of[i] = (unsigned short)L.u.ag.cid[L.tail_of[i]];
    __syncthreads();
    small_scan(L.u.ag.moff, nn, L.scan_w);
    if (t == 0) L.u.ag.moff[nn] = n;
    __syncthreads();
    // members of every coarse node in ascending node order: every node counts the members of its coarse node that
    // precede it (n <= 1024: ~1000 LDS reads per thread) -- an atomic cursor would make the order run dependent
    for (int v = t; v < n; v += SM_THREADS) {
      const int c = L.u.ag.cid[v];
      int before = 0;
      for (int u = 0; u < v; ++u) before += L.u.ag.cid[u] == c ? 1 : 0;
      L.u.ag.members[L.u.ag.moff[c] + before] = v;
    }
    __syncthreads();
    int* nix = a.ix[dst];
    long long* nw = a.w[dst];
    for (int pass = 0; pass < 2; ++pass) {
      for (int c0 = 0; c0 < nn; c0 += SM_WAVES) {
        const int c = c0 + wv;
        if (c < nn) {
          if (lane == 0) L.tcnt[wv] = 0;
          for (int mi = L.u.ag.moff[c]; mi < L.u.ag.moff[c + 1]; ++mi) {
            const int v = L.u.ag.members[mi];
            for (int e = L.ip[v] + lane; e < L.ip[v + 1]; e += 64) {
              const long long w = wq[e];
              if (w != 0) {
                const int key = L.u.ag.cid[ix[e]];
                const unsigned long long old = atomicAdd(&acc[key], (unsigned long long)w);
                if (old == 0ull) touched[atomicAdd(&L.tcnt[wv], 1)] = (unsigned short)key;
              }
            }
          }
          const int tc = __hip_atomic_load(&L.tcnt[wv], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          long long ksum = 0;
          const int p0 = pass ? L.u.ag.rowptr[c] : 0;
          for (int i = lane; i < tc; i += 64) {
            const int col = touched[i];
            const unsigned long long s = acc[col];
            acc[col] = 0ull;
            if (pass) {
              nix[p0 + i] = col;
              nw[p0 + i] = (long long)s;
              ksum += (long long)s;
            }
          }
          if (pass) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ksum += __shfl_xor(ksum, o);
            if (lane == 0) L.kk[c] = ksum;   // (kk of the OLD level is dead: nothing reads it during aggregation)
          } else if (lane == 0) {
            L.u.ag.rep[c] = tc;  // (rep is dead after the partition of the coarse nodes was written)
          }
        }
      }
      __syncthreads();
      if (pass == 0) {
        for (int c = t; c < nn; c += SM_THREADS) L.u.ag.rowptr[c] = L.u.ag.rep[c];
        __syncthreads();
        const int nnz_new = small_scan(L.u.ag.rowptr, nn, L.scan_w);
        if (t == 0) L.u.ag.rowptr[nn] = nnz_new;
        __syncthreads();
      }
    }
    // switch to the coarse level
    for (int c = t; c <= nn; c += SM_THREADS) L.ip[c] = L.u.ag.rowptr[c];
    for (int c = t; c < nn; c += SM_THREADS) L.comm[c] = L.csize[c];
    __threadfence();  // the rows just written are read through the vector cache from now on
    __syncthreads();
    ix = nix;
    wq = nw;
    dst ^= 1;
    n = nn;
  }
  __syncthreads();
  for (int i = t; i < n_in; i += SM_THREADS) a.comm[i] = L.comm[L.tail_of[i]];
  // ---- the last level's community totals and internal weight.  Coarse graphs are P^T W P entry for entry and all weights are
  // integers: these ARE the totals and the internal weight of the partition just written, on the entry graph and on level 0.
  for (int c = t; c < n_in; c += SM_THREADS) L.Ktot[c] = 0ull;
  if (t == 0) L.s_internal = 0ull;
  __syncthreads();
  for (int v = t; v < n; v += SM_THREADS) atomicAdd(&L.Ktot[L.comm[v]], (unsigned long long)L.kk[v]);
  for (int v0 = 0; v0 < n; v0 += SM_WAVES) {
    const int v = v0 + wv;
    if (v < n) {
      const int ca = L.comm[v];
      long long s = 0;
      for (int e = L.ip[v] + lane; e < L.ip[v + 1]; e += 64)
        if (L.comm[ix[e]] == ca) s += wq[e];  // (self entries included)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0 && s != 0) atomicAdd(&L.s_internal, (unsigned long long)s);
    }
  }
  __syncthreads();
  for (int c = t; c < n_in; c += SM_THREADS) a.totals[c] = L.Ktot[c];
  if (t == 0) {
    a.internal[0] = L.s_internal;
    a.info[SM_INFO_LEVELS] = levels;
    a.info[SM_INFO_MOVES] = tot_moves;
    a.info[SM_INFO_MERGES] = tot_merges;
    a.info[SM_INFO_NODES] = n;
  }
}

// ---- quality ---------------------------------------------------------------------------------------
// internal[0] += sum over stored entries inside a community (self loops included)
// G lanes per vertex (16 on the kNN graph itself: four rows in flight per wave instead of one)
template <int G>
__global__ __launch_bounds__(256) void ld_internal_kernel(int n, const int64_t* __restrict__ indptr,
                                                          const int* __restrict__ indices,
                                                          const long long* __restrict__ wq, const int* __restrict__ comm,
                                                          unsigned long long* __restrict__ internal) {
  const int lane = threadIdx.x & 63, sub = threadIdx.x % G;
  long long s = 0;
  for (int v = blockIdx.x * (256 / G) + threadIdx.x / G; v < n; v += gridDim.x * (256 / G)) {
    const int a = comm[v];
    const int64_t beg = indptr[v], end = indptr[v + 1];
    for (int64_t e = beg + sub; e < end; e += 4 * G) {  // (four entries per lane in flight: see ld_within_kernel)
      int u[4], cu[4];
      long long we[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t ee = e + t * G;
        u[t] = ee < end ? indices[ee] : v;
        we[t] = ee < end ? wq[ee] : 0ll;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) cu[t] = comm[u[t]];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (cu[t] == a) s += we[t];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  // (one global atomic per workgroup: the per-wave version serialised 8192 atomics on one address, 0.2 ms)
  __shared__ long long sh_s[4];
  if (lane == 0) sh_s[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long tot = sh_s[0] + sh_s[1] + sh_s[2] + sh_s[3];
    if (tot != 0) atomicAdd(internal, (unsigned long long)tot);
  }
}

// sumsq[0] = sum_c (Ktot[c] / 2m)^2 in a fixed order: SUMSQ_BLOCKS partial sums (fixed ranges, fixed tree), then one
// block adds the partials
constexpr int SUMSQ_BLOCKS = 256;
__device__ __forceinline__ double block_sum_1024(double s, double* sh) {
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}
__global__ __launch_bounds__(1024) void ld_sumsq_kernel(int n, const unsigned long long* __restrict__ Ktot,
                                                        double m2, double* __restrict__ part) {
  __shared__ double sh[1024];
  double s = 0.0;
  for (int c = blockIdx.x * 1024 + threadIdx.x; c < n; c += SUMSQ_BLOCKS * 1024) {
    double f = (double)(long long)Ktot[c] / m2;
    s += f * f;
  }
  s = block_sum_1024(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(1024) void ld_sumsq_final_kernel(const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double sh[1024];
  double s = block_sum_1024((int)threadIdx.x < SUMSQ_BLOCKS ? part[threadIdx.x] : 0.0, sh);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- final renumbering by decreasing size ------------------------------------------------------------
__global__ __launch_bounds__(1024) void ld_minmember_kernel(int n, const int* __restrict__ memb,
                                                            int* __restrict__ minmember, int* __restrict__ size) {
  __shared__ int keys[BH_SLOTS];
  __shared__ int mn[BH_SLOTS];
  __shared__ int cnt[BH_SLOTS];
  for (int i = threadIdx.x; i < BH_SLOTS; i += 1024) {
    keys[i] = BH_EMPTY;
    mn[i] = 0x7fffffff;
    cnt[i] = 0;
  }
  __syncthreads();
  for (int v = blockIdx.x * 1024 + threadIdx.x; v < n; v += gridDim.x * 1024) {
    const int c = memb[v];
    const int slot = bh_find_slot(keys, c);
    if (slot >= 0) {
      atomicMin(&mn[slot], v);
      atomicAdd(&cnt[slot], 1);
    } else {
      atomicMin(&minmember[c], v);
      atomicAdd(&size[c], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BH_SLOTS; i += 1024)
    if (keys[i] != BH_EMPTY) {
      atomicMin(&minmember[keys[i]], mn[i]);
      atomicAdd(&size[keys[i]], cnt[i]);
    }
}
// compact list of non-empty communities: key = (~size << 32) | minmember  (ascending = size desc)
__global__ void ld_commkeys_kernel(int n, const int* __restrict__ size, const int* __restrict__ minmember,
                                   const int64_t* __restrict__ pos, unsigned long long* __restrict__ keys,
                                   int* __restrict__ ids) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n && size[c] > 0) {
    const int64_t p = pos[c];
    keys[p] = ((unsigned long long)(~(unsigned int)size[c]) << 32) | (unsigned int)minmember[c];
    ids[p] = c;
  }
}
__global__ void ld_rank_kernel(int nc, const unsigned long long* __restrict__ keys, const int* __restrict__ ids,
                               int* __restrict__ newlabel /* indexed by old community id */) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const unsigned long long ki = keys[i];
  int rank = 0;
  for (int j = 0; j < nc; ++j) rank += keys[j] < ki ? 1 : 0;
  newlabel[ids[i]] = rank;
}
__global__ void ld_compact_label_kernel(int nc, const int* __restrict__ ids, int* __restrict__ newlabel) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nc) newlabel[ids[i]] = i;
}
__global__ void ld_relabel_kernel(int n, const int* __restrict__ newlabel, const int* memb, int* out) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) out[v] = newlabel[memb[v]];  // (out may be memb itself)
}
__global__ void ld_gather_kernel(int n, const int* __restrict__ comm, const int* __restrict__ node_of,
                                 int* __restrict__ out) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) out[v] = comm[node_of[v]];
}

// ---- host orchestration --------------------------------------------------------------------------
struct LevelGraph {
  int n = 0;
  int max_deg = 0;  // largest row length (debug trace)
  int64_t nnz = 0;
  const int64_t* indptr = nullptr;
  const int* indices = nullptr;
  const long long* wq = nullptr;
  const long long* k = nullptr;
};

struct CoarseBuf {
  int64_t* indptr; int* indices; long long* wq; long long* k;
};

// The coarse levels of an iteration are built one behind the other into ONE pool (what used to be two ping-pong buffers
// of E entries): the hierarchy of the best partition stays there, and a later iteration whose local moving moves nothing
// takes its levels from it (leiden_iteration).  Level l >= 1 = the graph of the level + the vertex map (l - 1) -> l.
struct StoredLevel {
  LevelGraph g;
  size_t e_off = 0, p_off = 0, c_off = 0;  // first entry / first row pointer and vertex weight / first map element
  size_t c_n = 0;                          // map elements (vertices of the level below)
  const int* cid = nullptr;                // the map (n of the level below elements): in the pool, or b.cid for a level off the store
};
constexpr size_t POOL_ALIGN = 64;  // (elements: levels start on 256-byte boundaries like the buffers they replaced)

struct LeidenBuffers {
  long long* wq0; long long* k0;
  CoarseBuf pool;          // 2 (N + 1) row pointers and vertex weights, 2 E entries
  int* cid_pool;           // 2 N map elements
  int* sm_ix[2]; long long* sm_w[2];  // coarse levels of ld_small_levels_kernel (SMALL_NNZ entries each): it leaves the pool alone
  int* comm; int* csize; unsigned long long* Ktot;
  int* cls_lists; int* rlist; int* touched; int* hub_list;
  int* tier_lists; int* giant_lists;  // per class: the long rows of its list, by decide tier (TierDst)
  int* ref; int* target; int* target2; int* refsize; unsigned long long* Kref; unsigned long long* Eref; long long* a_in;
  VertRec* vrec; TargRec* trec;  // packed mirrors of {comm, ref, stamp} and {Kref, Eref, refsize} for the refinement's gathers
  int* flag; int64_t* newid; int64_t* scan_tmp; int* cid; int* rep; int* comm_tmp;
  int* node_of; int* memb; int* memb_work;  // memb: the best partition so far = the input of the next iteration; memb_work: its output
  int* agg_col; long long* agg_w;  // scratch CSR of the coarse-graph build (rows at upper-bound offsets)
  int* mcount; int64_t* moff; int64_t* eoff; int* members; int* mdeg; int* mid_list; int* big_list;
  int64_t* pmoff; int* part_list; int* part_cnt;  // split rows of the coarse-graph build (ld_agg_parts_kernel)
  int* rowcnt; int* cursor;
  int* counters; int* rcounters; unsigned long long* total; double* dscratch;
  unsigned long long* ckeys; int* cids; int* newlabel; int* minmember;
};

// member entries per part of a split coarse row / entries from which a row is split (SCAMD_LEIDEN_AGG_SPLIT_CHUNK / _WORK:
// tests push small graphs through the split path; resolved here so that the workspace query and the run agree)
static int64_t agg_split_chunk() { return std::max(64, env_int("SCAMD_LEIDEN_AGG_SPLIT_CHUNK", 131072)); }
static int64_t agg_split_work() { return std::max<int64_t>(agg_split_chunk(), env_int("SCAMD_LEIDEN_AGG_SPLIT_WORK", 262144)); }
static void leiden_carve(Workspace& ws, int64_t n, int64_t nnz, LeidenBuffers* b) {
  const size_t N = (size_t)n, E = (size_t)std::max<int64_t>(nnz, 1);
  b->wq0 = ws.take<long long>(E);
  b->k0 = ws.take<long long>(N);
  b->pool.indptr = ws.take<int64_t>(2 * (N + 1));
  b->pool.indices = ws.take<int>(2 * E);
  b->pool.wq = ws.take<long long>(2 * E);
  b->pool.k = ws.take<long long>(2 * (N + 1));
  b->cid_pool = ws.take<int>(2 * N);
  for (int i = 0; i < 2; ++i) {
    b->sm_ix[i] = ws.take<int>(SMALL_NNZ);
    b->sm_w[i] = ws.take<long long>(SMALL_NNZ);
  }
  b->comm = ws.take<int>(N);
  b->csize = ws.take<int>(N);
  b->Ktot = ws.take<unsigned long long>(N);
  // class lists of a sweep (local moving) / of the refinement: lists[c * n_level ..].  Levels above 4096 vertices use at
  // most DEF_CLASSES lists; only levels of <= 4096 vertices take MAX_CLASSES refinement sub-rounds.  (Round 3 carved
  // MAX_CLASSES x N: 1.28 GB at 10M cells for lists of which 8 were ever used)
  const size_t cls_ints = std::max((size_t)DEF_CLASSES * N, (size_t)MAX_CLASSES * std::min<size_t>(N, 4096));
  b->cls_lists = ws.take<int>(cls_ints);
  // tier lists of the classes (TierDst): a region per class like cls_lists for the wave tier (upwards) and the block tier
  // (downwards); a giant row has more than BLK_MAX_DEG entries, so a level has fewer than E / (BLK_MAX_DEG + 1) + 1 of them
  b->tier_lists = ws.take<int>(cls_ints);
  b->giant_lists = ws.take<int>((size_t)MAX_CLASSES * (E / (BLK_MAX_DEG + 1) + 1));
  b->rlist = ws.take<int>(N);
  b->hub_list = ws.take<int>(N);
  b->touched = ws.take<int>(N);
  b->ref = ws.take<int>(N);
  b->target = ws.take<int>(N);
  b->target2 = ws.take<int>(N);  // decisions of alternate sub-rounds (ld_requeue_move_kernel)
  b->refsize = ws.take<int>(N);
  b->Kref = ws.take<unsigned long long>(N);
  b->Eref = ws.take<unsigned long long>(N);
  b->a_in = ws.take<long long>(N);
  b->vrec = ws.take<VertRec>(N);
  b->trec = ws.take<TargRec>(N);
  b->flag = ws.take<int>(N);
  b->newid = ws.take<int64_t>(N + 1);
  b->scan_tmp = ws.take<int64_t>((size_t)scan_num_blocks(n) + 2);
  b->cid = ws.take<int>(N);
  b->rep = ws.take<int>(N);
  b->comm_tmp = ws.take<int>(N);
  b->node_of = ws.take<int>(N);
  b->memb = ws.take<int>(N);
  b->memb_work = ws.take<int>(N);
  b->agg_col = ws.take<int>(E);
  b->agg_w = ws.take<long long>(E);
  b->mcount = ws.take<int>(N);
  b->moff = ws.take<int64_t>(N + 1);
  b->eoff = ws.take<int64_t>(N + 1);
  b->members = ws.take<int>(N);
  b->mdeg = ws.take<int>(N);
  b->mid_list = ws.take<int>(N);
  b->big_list = ws.take<int>(N);
  {
    const size_t slots = 3 * E / (size_t)agg_split_chunk() + 16;  // parts + one closing slot per split row
    b->pmoff = ws.take<int64_t>(slots);
    b->part_list = ws.take<int>(slots);
    b->part_cnt = ws.take<int>(slots);
  }
  b->rowcnt = ws.take<int>(N);
  b->cursor = ws.take<int>(N);
  b->counters = ws.take<int>(16);  // the phase counters (PH_*)
  b->rcounters = ws.take<int>(2 * CTR_AREA);  // two counter areas: the sweeps of the local moving alternate between them
  b->total = ws.take<unsigned long long>(4);
  b->dscratch = ws.take<double>(4 + SUMSQ_BLOCKS);
  b->ckeys = ws.take<unsigned long long>(N);
  b->cids = ws.take<int>(N);
  b->newlabel = ws.take<int>(N);
  b->minmember = ws.take<int>(N);
}

#define GRID1(n) dim3((unsigned)ceil_div((n), 256)), dim3(256)
#define GRIDW(n) dim3((unsigned)ceil_div((n), 4)), dim3(256)
#define GRIDK(n) dim3((unsigned)ceil_div((n), 1024)), dim3(1024)
constexpr int HUB_GRID = 512;
// workgroups of the 512-thread tier of the coarse-row builder (the 1024-thread tier launches HUB_GRID); each loops over
// its share of the listed rows: a launch of N such workgroups costs ~0.27 us x N before any work is done (fewer were
// measured slower: DESIGN section 8)
constexpr int AGG_MID_GRID = 768;
// local moving of a level stops once < 2 % of its vertices move in a sweep (first iteration)
constexpr int LM_STOP_PERMILLE = 20;
// ... < 4 % on the levels that run four classes per sweep (lm_classes): 0.9 ms / 11 ms faster on the planted / weak 1M graph
// at the same Q / inside the seeds' spread (profiles/r06ze_lm_stop_with_4_classes.log); everywhere, one seed of the 700-cell
// fixture fell out of the oracle's seed distribution
constexpr int LM_STOP_PERMILLE_BIG = 40;
constexpr size_t HUB_LDS = (size_t)BHUB_SLOTS * 12;

// Which coarse levels of the pool belong to a partition, and how its hierarchy ended.
struct Hierarchy {
  int depth = 0;       // levels 1 .. depth of the pool belong to the hierarchy that produced the partition
  int end_level = -1;  // that hierarchy ended at this level ...
  int end_kind = 0;    // ... 1: its refinement merged nothing, 2: its aggregation merged nothing (0: otherwise)
};
// ... of the running iteration
struct IterHierarchy {
  int built = 0;       // its levels 1 .. built sit in the pool one behind the other (-1: a level did not fit)
  int end_level = -1, end_kind = 0;
  bool quiet = false;  // it ran on the stored hierarchy to its end and no separate-kernel level moved anything
  int small_moves = 0; // moves inside ld_small_levels_kernel (fetched when quiet, handed out by the sync of iteration_quality())
  // the pair (graph, partition in b.comm) the iteration ended on; in_small: inside ld_small_levels_kernel, which has left the
  // totals of its last level in b.Ktot[0 .. top.n) and the internal weight in b.total[1] (top: the level it was entered at)
  LevelGraph top{};
  bool in_small = false;
  // what the stored hierarchy is once the iteration's partition has been accepted as b.memb: what it built or reused
  Hierarchy accepted() const { return Hierarchy{std::max(built, 0), end_level, end_kind}; }
};

struct LeidenCtx {
  HostReadbackScope readback_scope;  // (the read-backs' destinations are locals of the functions this context is passed to)
  hipStream_t s;
  LeidenBuffers b;
  double gamma;
  double m2;  // total (quantised) weight = sum of strengths
  // Objective.  Modularity (default): vertex weight = strength, the gain of joining C is w(v, C) - (gamma / 2m) k_v K_C.
  // CPM (igraph `objective_function='CPM'`, src/scanpy/tools/_leiden.py:188-196): vertex weight = 1 (sums on the coarse
  // levels), resolution not normalised: w(v, C) - gamma n_v N_C.  Every kernel takes "the vertex weights" and "g": the two
  // objectives differ only in what the host hands them (weights are 2^32 fixed point: g carries the scale).
  bool cpm = false;
  // CPM vertex weights: ones (nw_scale 1), or the caller's in fixed point (nw_scale = NODE_WEIGHT_SCALE: a power of two, so
  // unit weights handed in as an array give bit-identical gains)
  const float* node_weights = nullptr;
  double nw_scale = 1.0;
  double gscale() const { return cpm ? gamma * WSCALE / (nw_scale * nw_scale) : gamma / m2; }
  double inv_beta = 0.0;  // 1 / (beta * 2^32): randomness of the refinement's merge rule (0 = greedy)
  int iter = 0;           // outer iteration: part of the refinement's noise seed
  unsigned int seed;
  unsigned long long diag0 = 0;  // sum of the stored diagonal entries of level 0: the internal weight of the singleton partition
  int l0_moves = -1;          // moves of the last iteration's level-0 local moving (0: its input was node optimal)
  int n_levels = 0;           // levels the last iteration went through
  // ---- the SCAMD_LEIDEN_* switches, all read by read_knobs() once per call (tools and tests flip them inside one process) ----
  bool debug = false;         // SCAMD_LEIDEN_DEBUG=1 / 2: trace on stderr
  bool debug_sync = false;    // ... =2: also drain the stream after every launch of the class sub-rounds and name it (LD_DBG_SYNC)
  bool small_levels = true;   // levels of <= SMALL_N nodes in one workgroup (SCAMD_LEIDEN_SMALL=0: separate kernels)
  bool polish = true;         // SCAMD_LEIDEN_POLISH=0: no final polish (A/B; the round-4 behaviour)
  bool reuse = true;          // SCAMD_LEIDEN_REUSE=0: every iteration refines and aggregates every level (test hook, A/B)
  int force_lanes = 0;        // SCAMD_LEIDEN_QUAD = 0 / 1 / 2: 64 / 16 / 32 lanes per vertex on every level (0: by row length)
  int iter_cap = MAX_OUTER_ITERS;  // SCAMD_LEIDEN_ITER_CAP: outer iterations of an n_iterations < 0 run
  int max_iters = 0;          // SCAMD_LEIDEN_MAX_ITERS (test knob, > 0: in force): cuts such a run short, so that the polish meets an
                              // unfinished partition
  // coarse-row build tiers (distinct-neighbour bounds); the env overrides exist so the tests can push small graphs
  // through the workgroup and multi-pass tiers
  int agg_wave_max = WH_MAX_DEG;
  int agg_mid_max = AGG_MID_MAX;
  int agg_pass_keys = AGG_BIG_PASS;
  // member entries beyond which a coarse row leaves the wave tier / the 512-thread tier whatever its table size
  // (SCAMD_LEIDEN_AGG_WAVE_WORK / _MID_WORK)
  int agg_wave_work = 2048;
  int agg_mid_work = 65536;
  int count_grid = COUNT_GRID;  // SCAMD_LEIDEN_COUNT_GRID: most workgroups that touch one counter word in a launch (tests: 1, 2)
  int hub_try_probes = HUB_TRY_PROBES;  // 0: no optimistic single pass over multi-pass rows (SCAMD_LEIDEN_HUB_TRY_PROBES; tests)
  int64_t agg_split_chunk = 0, agg_split_work = 0;  // (agg_split_chunk() / agg_split_work(): as the workspace query saw them)
  // rows the last aggregate() handed to the 512-thread builder, the 1024-thread builder, the split path (the debug trace and
  // the test entry scamd_leiden_debug_level_f32 report them)
  int agg_rows_mid = 0, agg_rows_big = 0, agg_rows_split = 0;
  // ---- the stored hierarchy (StoredLevel) ----
  size_t cap_e = 0, cap_p = 0, cap_c = 0;  // pool capacities: entries, row pointers / vertex weights, map elements
  StoredLevel lv[MAX_LEVELS + 1];          // [l], l >= 1: level l as the running iteration sees it
  Hierarchy kept;        // of the hierarchy that produced b.memb
  IterHierarchy it;      // of the running iteration (accept_iteration commits it when it accepts the iteration's partition)
};

// every SCAMD_LEIDEN_* switch (agg_split_chunk() / agg_split_work() are shared with the workspace query)
static void read_knobs(LeidenCtx& cx) {
  cx.debug = env_is("SCAMD_LEIDEN_DEBUG", '1') || env_is("SCAMD_LEIDEN_DEBUG", '2');
  cx.debug_sync = env_is("SCAMD_LEIDEN_DEBUG", '2');
  cx.small_levels = !env_is("SCAMD_LEIDEN_SMALL", '0');
  cx.polish = !env_is("SCAMD_LEIDEN_POLISH", '0');
  cx.reuse = !env_is("SCAMD_LEIDEN_REUSE", '0');
  bool quad_set = false;
  const int quad = env_int("SCAMD_LEIDEN_QUAD", 0, &quad_set);
  cx.force_lanes = !quad_set ? 0 : (quad == 1 ? 16 : (quad == 2 ? 32 : 64));
  const int cap = env_int("SCAMD_LEIDEN_ITER_CAP", 0);
  cx.iter_cap = cap > 0 ? cap : MAX_OUTER_ITERS;
  cx.max_iters = env_int("SCAMD_LEIDEN_MAX_ITERS", 0);
  cx.agg_wave_max = std::min(env_int("SCAMD_LEIDEN_AGG_WAVE_MAX", WH_MAX_DEG), (int)WH_MAX_DEG);
  cx.agg_mid_max = std::min(env_int("SCAMD_LEIDEN_AGG_MID_MAX", AGG_MID_MAX), (int)AGG_MID_MAX);
  cx.agg_pass_keys = std::max(16, std::min(env_int("SCAMD_LEIDEN_AGG_PASS_KEYS", AGG_BIG_PASS), (int)AGG_BIG_PASS));
  cx.agg_wave_work = std::max(1, env_int("SCAMD_LEIDEN_AGG_WAVE_WORK", 2048));
  cx.agg_mid_work = std::max(1, env_int("SCAMD_LEIDEN_AGG_MID_WORK", 65536));
  cx.hub_try_probes = std::max(0, env_int("SCAMD_LEIDEN_HUB_TRY_PROBES", HUB_TRY_PROBES));
  cx.count_grid = std::max(1, std::min(env_int("SCAMD_LEIDEN_COUNT_GRID", COUNT_GRID), (int)COUNT_GRID_MAX));
  cx.agg_split_chunk = agg_split_chunk();
  cx.agg_split_work = agg_split_work();
}

// grid of a launch whose 1024-thread workgroups each end on the same counter words: one per 1024 elements, at most cx.count_grid
static dim3 count_grid(const LeidenCtx& cx, int cnt) { return dim3((unsigned)std::max(1, std::min(cx.count_grid, ceil_div(cnt, 1024)))); }

// SCAMD_LEIDEN_DEBUG=2: drain the stream after every launch of the class sub-rounds and name it (a device fault then
// surfaces at the launch that caused it)
#define LD_DBG_SYNC(cx, ...)                                  \
  do {                                                        \
    if ((cx).debug_sync) {                                    \
      (void)hipStreamSynchronize((cx).s);                     \
      fprintf(stderr, "[leiden] done: " __VA_ARGS__);         \
      fputc('\n', stderr);                                    \
      fflush(stderr);                                         \
    }                                                         \
  } while (0)

// one launch of ld_fill_kernel for up to FillArgs::MAX_REGIONS regions (byte counts are multiples of 4)
struct Filler {
  FillArgs a;
  unsigned long long max_words = 0;
  Filler() { a.n = 0; }
  Filler& add(void* p, size_t bytes, unsigned int pat = 0u) {
    if (bytes == 0) return *this;
    a.p[a.n] = static_cast<unsigned int*>(p);
    a.words[a.n] = bytes / 4;
    a.pat[a.n] = pat;
    max_words = std::max<unsigned long long>(max_words, a.words[a.n]);
    ++a.n;
    return *this;
  }
};
static int run_fill(LeidenCtx& cx, const Filler& f) {
  if (f.a.n == 0) return SCAMD_OK;
  const unsigned grid = (unsigned)std::min<unsigned long long>(2048ull, std::max<unsigned long long>(1ull, (f.max_words / 4 + 255) / 256));
  hipLaunchKernelGGL(ld_fill_kernel, dim3(grid), dim3(256), 0, cx.s, f.a);
  SCAMD_LAUNCH_CHECK();
  ++g_ld_stats[ST_DEVICE_FILLS];
  return SCAMD_OK;
}

static int read_counters(LeidenCtx& cx, int* h, int cnt) {
  LD_FETCH(h, cx.b.counters, sizeof(int) * cnt, cx.s);
  LD_SYNC(cx.s);
  return SCAMD_OK;
}

// lanes per vertex -> the template instantiation: f(std::integral_constant<int, lanes>()).  WITH_32 = false for the kernels
// that exist for 16 and 64 lanes only.
template <bool WITH_32, typename F>
static void with_lanes(int lanes, F&& f) {
  if (lanes == 16) return f(std::integral_constant<int, 16>());
  if constexpr (WITH_32) {
    if (lanes == 32) return f(std::integral_constant<int, 32>());
  }
  return f(std::integral_constant<int, 64>());
}
// 256-thread workgroups that give `cnt` vertices `lanes` lanes each
static int blocks_for(int lanes, int cnt) { return ceil_div(cnt, 256 / lanes); }

// Ktot / csize of `comm`; `extra`: further regions the caller wants cleared by the same launch
static int compute_totals(LeidenCtx& cx, const LevelGraph& g, const int* comm, Filler extra = Filler()) {
  extra.add(cx.b.Ktot, sizeof(unsigned long long) * g.n).add(cx.b.csize, sizeof(int) * g.n);
  const int rcf = run_fill(cx, extra);
  if (rcf != SCAMD_OK) return rcf;
  hipLaunchKernelGGL(ld_totals_kernel, count_grid(cx, g.n), dim3(1024), 0, cx.s, comm, g.k, g.n, cx.b.Ktot, cx.b.csize,
                     cx.b.total + 1);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

// quality of `comm` on level graph g (needs Ktot up to date): modularity, or the CPM objective in the same units
// (b.total[1], the accumulator of the internal weight, was zeroed by the ld_totals_kernel launch of compute_totals)
// the quality from its two sums: `totals[0 .. n)` the total vertex weight per community (zeros add exactly nothing: the sum
// over the slots of a coarse level is bit for bit the sum over the level-0 array, whose other slots are empty), and the
// internal weight -- `internal_host`, or b.total[1] when that is NULL.  One synchronisation.
static int quality_from_sums(LeidenCtx& cx, int n, const unsigned long long* totals, const unsigned long long* internal_host, double* q) {
  // (CPM: sum of squared community SIZES, unnormalised)
  hipLaunchKernelGGL(ld_sumsq_kernel, dim3(SUMSQ_BLOCKS), dim3(1024), 0, cx.s, n, totals, cx.cpm ? cx.nw_scale : cx.m2, cx.b.dscratch + 4);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_sumsq_final_kernel, dim3(1), dim3(1024), 0, cx.s, cx.b.dscratch + 4, cx.b.dscratch);
  SCAMD_LAUNCH_CHECK();
  unsigned long long internal = internal_host ? *internal_host : 0ull;
  double sumsq = 0;
  if (!internal_host) LD_FETCH(&internal, cx.b.total + 1, sizeof(internal), cx.s);
  LD_FETCH(&sumsq, cx.b.dscratch, sizeof(double), cx.s);
  LD_SYNC(cx.s);
  *q = cx.cpm ? ((double)(long long)internal - cx.gamma * WSCALE * sumsq) / cx.m2
              : (double)(long long)internal / cx.m2 - cx.gamma * sumsq;
  return SCAMD_OK;
}

static int quality(LeidenCtx& cx, const LevelGraph& g, const int* comm, double* q) {
  if (g.wq == cx.b.wq0) ++g_ld_stats[ST_L0_QUALITY_WALKS];
  // (a group walks its vertices one after the other, three dependent loads each: the more groups, the fewer steps of that
  // walk -- and one same-word atomic per workgroup at the end)
  constexpr int qgrid = 2048;
  with_lanes<false>(g.nnz <= (int64_t)48 * g.n ? 16 : 64, [&](auto G) {
    constexpr int L = decltype(G)::value;
    hipLaunchKernelGGL(ld_internal_kernel<L>, dim3((unsigned)std::min(qgrid, blocks_for(L, g.n))), dim3(256), 0, cx.s, g.n,
                       g.indptr, g.indices, g.wq, comm, cx.b.total + 1);
  });
  SCAMD_LAUNCH_CHECK();
  return quality_from_sums(cx, g.n, cx.b.Ktot, nullptr, q);
}

// Ktot / csize and the quality of `comm` on g
static int evaluate(LeidenCtx& cx, const LevelGraph& g, const int* comm, double* q) {
  const int rc = compute_totals(cx, g, comm);
  return rc != SCAMD_OK ? rc : quality(cx, g, comm, q);
}

// levels whose rows are short on average (the kNN graph itself) take the four-vertices-per-wave kernels
static_assert(WH_SLOTS / 2 * 3 / 4 == 192 && WH_MAX_DEG == 384,
              "the table ladders of the decide kernels (rows <= 96 / 192 / 384) are written out in their nslots expressions");
// lanes per vertex of the decision kernels for this level: 16 (four vertices per wave, rows <= 96), 32 (two per wave,
// rows <= 192: the first coarse levels, ~64 entries per row) or 64.  SCAMD_LEIDEN_QUAD = 0 / 1 / 2 forces 64 / 16 / 32.
static int level_lanes(const LeidenCtx& cx, const LevelGraph& g) {
  if (cx.force_lanes) return cx.force_lanes;
  if (g.n <= 0) return 64;
  const int64_t avg = g.nnz / g.n;
  return avg <= 40 ? 16 : (avg <= 110 ? 32 : 64);
}
// ... of the refinement's kernels, which exist for 16 and 64 lanes
static int refine_lanes(const LeidenCtx& cx, const LevelGraph& g) { return level_lanes(cx, g) == 16 ? 16 : 64; }
// longest row the table of a `lanes`-lane decide kernel takes: longer rows of such a launch overflow to the 64-lane pass
// (-1: no such tier, the launch is the 64-lane one)
static int lanes_thr_mid(int lanes) { return lanes == 16 ? (int)G16_MAX : (lanes == 32 ? (int)(WH_SLOTS / 2 * 3 / 4) : -1); }

// where the list builders of a level write its tier lists (list_long_rows)
static int giant_stride(const LevelGraph& g) { return (int)(g.nnz / (BLK_MAX_DEG + 1)) + 1; }
static TierDst tier_dst(LeidenCtx& cx, const LevelGraph& g, int lanes) {
  return TierDst{g.indptr, cx.b.tier_lists, cx.b.giant_lists, giant_stride(g), lanes_thr_mid(lanes)};
}

// One decide step of a class sub-round: ONE launch for every tier a 256-thread workgroup can take -- the main tier (`lanes`
// lanes per vertex, the whole class list, long rows skipped), the wave-per-row tier and the block tier over the lists the
// class's builder left (TierLists), as block ranges of one grid -- and, only when the class has such a row, the 1024-thread
// launch of the giant tier.  rq: the sub-round before this one, whose movers re-queue their neighbours in the head of the
// same launch (local moving; nullptr: nothing to re-queue).  hctr: the host's copy of the sub-round's counter block as the
// list builder left it: the tiers' rows, from which the block ranges are sized -- a tier without rows gets no workgroups.
// The two flavours, by the argument struct: MoveArgs (local moving, polish) and ProposeArgs (refinement).
struct RequeueHead {
  int n_act;
  const int* list;
  const int* decision;
};
static int main_grid_cap(const MoveArgs&) { return 1 << 30; }
static int main_grid_cap(const ProposeArgs&) { return 32768; }
static void launch_fused_tiers(LeidenCtx& cx, const LevelGraph& g, int lanes, unsigned grid, const RequeueHead* rq, int nb_rq, const MoveArgs& a) {
  with_lanes<true>(lanes, [&](auto G) {
    constexpr int L = decltype(G)::value;
    if (rq)
      hipLaunchKernelGGL(ld_requeue_move_kernel<L>, dim3(grid), dim3(256), 0, cx.s, nb_rq, rq->n_act, rq->list, rq->decision, g.indptr,
                         g.indices, (const int*)cx.b.comm, cx.b.flag, a);
    else
      hipLaunchKernelGGL(ld_move_kernel<L>, dim3(grid), dim3(256), 0, cx.s, a);
  });
}
static void launch_fused_tiers(LeidenCtx& cx, const LevelGraph&, int lanes, unsigned grid, const RequeueHead*, int, const ProposeArgs& a) {
  with_lanes<false>(lanes, [&](auto G) {
    hipLaunchKernelGGL(ld_refine_propose_kernel<decltype(G)::value>, dim3(grid), dim3(256), 0, cx.s, a);
  });
}
static void launch_giant_tier(LeidenCtx& cx, unsigned grid, const MoveArgs& a, HubTry ht) {
  hipLaunchKernelGGL(ld_move_hub_kernel, dim3(grid), dim3(HUB_THREADS), HUB_LDS, cx.s, a, ht);
}
static void launch_giant_tier(LeidenCtx& cx, unsigned grid, const ProposeArgs& a, HubTry ht) {
  hipLaunchKernelGGL(ld_refine_propose_hub_kernel, dim3(grid), dim3(HUB_THREADS), HUB_LDS, cx.s, a, ht);
}
template <typename Args>
static int decide_tiers(LeidenCtx& cx, const char* what, const LevelGraph& g, int cls, int lanes, const RequeueHead* rq, const int* hctr,
                        Args a) {
  const int n_mid = hctr[CTR_N_MID], n_blk = hctr[CTR_N_BLK], n_giant = hctr[CTR_N_GIANT];
  const int n_main = a.n_act - n_mid - n_blk - n_giant;
  const int* region = cx.b.tier_lists + (size_t)cls * g.n;
  a.tl = TierLists{region, region + (g.n - 1), cx.b.giant_lists + (size_t)cls * giant_stride(g), n_mid, n_blk, n_giant,
                   n_main > 0 ? std::min(main_grid_cap(a), blocks_for(lanes, a.n_act)) : 0,
                   n_mid > 0 ? std::min(2048, blocks_for(64, n_mid)) : 0, std::min(BLK_GRID, n_blk)};
  const int nb_rq = rq ? ceil_div(rq->n_act, 256) : 0;
  const int grid = nb_rq + a.tl.nb_main + a.tl.nb_wave + a.tl.nb_blk;
  if (grid > 0) {
    launch_fused_tiers(cx, g, lanes, (unsigned)grid, rq, nb_rq, a);
    SCAMD_LAUNCH_CHECK();
    LD_DBG_SYNC(cx, "%s<%d> n=%d class=%d cnt=%d workgroups: re-queue %d main %d wave %d (%d rows) block %d (%d rows)", what, lanes, g.n,
                cls, a.n_act, nb_rq, a.tl.nb_main, a.tl.nb_wave, n_mid, a.tl.nb_blk, n_blk);
  }
  if (n_giant > 0) {
    launch_giant_tier(cx, (unsigned)std::min(HUB_GRID, n_giant), a, HubTry{cx.b.counters + PHASE_ERR, cx.hub_try_probes});
    SCAMD_LAUNCH_CHECK();
    LD_DBG_SYNC(cx, "%s giant tier n=%d class=%d rows=%d", what, g.n, cls, n_giant);
  }
  // (a 16- / 32-lane launch hands on every row beyond its table, whichever tier decides it)
  if (lanes != 64) g_ld_stats[ST_OVERFLOW_VERTICES] += n_mid + n_blk + n_giant;
  g_ld_stats[ST_HUB_VERTICES] += n_blk + n_giant;
  return SCAMD_OK;
}

// class sub-rounds per sweep: 8 everywhere.  (4 / 2 on levels below 16384 / 1024 vertices saved ~1 ms of launch latency
// per call, but the fewer the classes the more neighbours move at once: on the 700-cell fixture one seed in ten then
// ended in a worse optimum, Q 0.8101 against the oracle's minimum 0.8120.)
// Round 6, large levels: FOUR.  At 1M cells (five seeds, profiles/r06zb_leiden_classes.log) 8 / 4 / 2 classes take 457 / 413 / 390 ms
// on the weak graph at Q 0.83960 / 0.83969 / 0.84037 (means), 877 / 794 / 781 ms without structure at Q 0.3318 / 0.3327 / 0.3335,
// 26.6 / 25.2 / 26.5 ms on the planted one (same partition): a vertex of a kNN graph with 10^5 and more vertices has two dozen
// neighbours, half of which deciding on the same snapshot costs nothing the next sweep does not repair -- it is the SMALL levels
// where fewer classes lose quality (see rf_classes; with four classes from 65536 vertices on, the 100k weak sample of the bench
// fell below its agreement gate against the oracle: median ARI over seed pairs 0.02 under the oracle's own).  Four from 262144
// vertices on.
static int lm_classes(const LeidenCtx& cx, int n) {
  // (the iterations after the first move a few hundred vertices of a large level per sweep: TWO classes there -- weak 1M graph 429 ->
  // 418 ms over three seeds at the same Q, the others unchanged; one class: everybody on one snapshot, far slower to settle)
  if (n >= 262144) return cx.iter >= 1 ? 2 : 4;
  return DEF_CLASSES;
}
// (refinement: a singleton cannot join a singleton of its OWN class -- with 8 classes an eighth of the targets the
// sequential algorithm would see are excluded, which on small graphs costs quality: 700-cell fixture over 30 seeds, runs
// ending below Q 0.8115: oracle 0, 32 classes 0, 8 classes 2, 2 classes 5.  Small levels therefore take 32 sub-rounds.)
static int rf_classes(int n) { return n <= 4096 ? MAX_CLASSES : DEF_CLASSES; }

static int local_moving(LeidenCtx& cx, const LevelGraph& g, int* total_moves) {
  LeidenBuffers& b = cx.b;
  const double gg = cx.gscale();
  *total_moves = 0;
  const size_t n = (size_t)g.n;
  // (one clear launch: totals, re-queue flags, phase counters (PH_MOVED, PH_BLOCKED (cumulative), PHASE_ERR), the counter
  // area of sweep 0 -- every later sweep's area is cleared by the ld_compact_cls_kernel launch of the sweep before it)
  int rc = compute_totals(cx, g, b.comm, Filler().add(b.flag, sizeof(int) * n).add(b.counters, sizeof(int) * PH_PER_PHASE).add(b.rcounters, sizeof(int) * CTR_AREA));
  if (rc != SCAMD_OK) return rc;
  const int lanes = level_lanes(cx, g);
  const int n_cls = lm_classes(cx, g.n);
  int moved_before = 0, quiet = 0, moved_prev2 = 0;
  for (int sweep = 0; sweep < MAX_LM_SWEEPS; ++sweep) {
    // [0, MAX_CLASSES): class list lengths of the sweep; then one block per sub-round: hub / overflow counts
    int* sw = b.rcounters + (sweep & 1) * CTR_AREA;
    const unsigned int salt = hash32(cx.seed + 0x85EBCA77u * (unsigned int)(sweep + 1) + 0xC2B2AE3Du * (unsigned int)cx.iter);
    hipLaunchKernelGGL(ld_compact_cls_kernel, count_grid(cx, g.n), dim3(1024), 0, cx.s, g.n,
                       sweep == 0 ? (int*)nullptr : b.flag, b.cls_lists, sw, n_cls, salt, tier_dst(cx, g, lanes),
                       b.rcounters + ((sweep + 1) & 1) * CTR_AREA, (int)CTR_AREA);
    SCAMD_LAUNCH_CHECK();
    int hc[CTR_AREA], ht[PH_PER_PHASE];  // class list lengths, then per sub-round [CTR_N_MID] / [CTR_N_BLK] / [CTR_N_GIANT]: long rows of the class
    LD_FETCH(hc, sw, sizeof(int) * (MAX_CLASSES + CTR_STRIDE * n_cls), cx.s);
    LD_FETCH(ht, b.counters, sizeof(ht), cx.s);
    LD_SYNC(cx.s);
    SCAMD_REQUIRE(ht[PHASE_ERR] == 0, SCAMD_EINTERNAL, "leiden: hub table overflow (local moving)");
    int n_act = 0;
    for (int c = 0; c < n_cls; ++c) n_act += hc[c];
    const int moved_last = ht[PH_MOVED] - moved_before;  // moves of the previous sweep
    moved_before = ht[PH_MOVED];
    *total_moves = ht[PH_MOVED];
    if (cx.debug) {
      int tot[3] = {0, 0, 0};
      for (int c = 0; c < n_cls; ++c)
        for (int t = 0; t < 3; ++t) tot[t] += hc[MAX_CLASSES + CTR_STRIDE * c + CTR_N_MID + t];
      fprintf(stderr, "[leiden] lm n=%d sweep=%d classes=%d act=%d moved_prev=%d blocked_total=%d long rows: wave %d block %d giant %d\n", g.n,
              sweep, n_cls, n_act, moved_last, ht[PH_BLOCKED], tot[0], tot[1], tot[2]);
    }
    if (n_act == 0) break;
    ++g_ld_stats[ST_LM_SWEEPS];
    g_ld_sweep_bytes += (double)n_act * (12.0 * (double)g.nnz / (double)std::max(g.n, 1) + 16.0);
    if (sweep > 0) {
      // (with the direction rule on, blocked vertices stay active without anybody moving: two such sweeps end the level)
      quiet = (moved_last == 0) ? quiet + 1 : 0;
      if (quiet >= 2) break;
      // Vertex-by-vertex merging of whole communities is what the coarser levels are for: once fewer than
      // LM_STOP_PERMILLE/1000 of the level's vertices move in a sweep, go on to refinement + aggregation (the
      // outer iterations repeat until nothing improves, so no move is lost, it is only made at a cheaper level).
      // (first outer iteration only: the later ones polish, and a level of theirs moves few vertices anyway)
      // The other half of the rule: the move counts of a level fall geometrically while vertices settle (749k, 178k,
      // 55k, 19k, 12k at 1M planted cells) and then RISE again for twenty sweeps (15k ... 74k ... 8k) while fragments
      // coalesce one boundary vertex at a time -- exactly the work that is cheaper one level up.  A sweep that does not
      // move at least a tenth fewer vertices than the one before it ends the level (first outer iteration only).
      if (cx.iter == 0 && sweep >= 2) {
        if ((long long)moved_last * 1000 < (long long)g.n * (n_cls < DEF_CLASSES ? LM_STOP_PERMILLE_BIG : LM_STOP_PERMILLE)) break;
        if (sweep >= 3 && (long long)moved_last * 10 > (long long)moved_prev2 * 9) break;
      }
      moved_prev2 = moved_last;
    }
    // the direction rule is the termination guarantee only: synchronous sub-rounds without it converge in a few sweeps
    // on every graph tried, with it (round 2's scheme) about half of the wanted moves of a round were blocked
    const int dir_round = sweep >= LM_DIR_AFTER ? sweep : -1;
    // the non-empty classes of the sweep, in order: [re-queue of sub-round i - 1 + all tiers of sub-round i] -> apply; the
    // decisions alternate between two buffers (the re-queue reads those of the sub-round before)
    int cls[MAX_CLASSES], ncl = 0;
    for (int c = 0; c < n_cls; ++c)
      if (hc[c] > 0) cls[ncl++] = c;
    int* tgt[2] = {b.target, b.target2};
    RequeueHead prev{0, nullptr, nullptr};
    for (int i = 0; i < ncl; ++i) {
      const int c = cls[i];
      const int cnt = hc[c];
      const int* list = b.cls_lists + (size_t)c * n;
      int* tg = tgt[i & 1];
      rc = decide_tiers(cx, "lm move", g, c, lanes, i > 0 ? &prev : nullptr, hc + MAX_CLASSES + CTR_STRIDE * c,
                        MoveArgs{cnt, list, g.indptr, g.indices, g.wq, g.k, b.comm, b.Ktot, b.csize, gg, dir_round, cx.seed, tg, TierLists{}});
      if (rc != SCAMD_OK) return rc;
      hipLaunchKernelGGL(ld_apply_kernel, count_grid(cx, cnt), dim3(APPLY_THREADS), 0, cx.s, cnt, list, tg, g.k, b.comm, b.Ktot, b.csize, b.flag,
                         b.counters);
      SCAMD_LAUNCH_CHECK();
      prev = RequeueHead{cnt, list, tg};
    }
    // (the last sub-round's movers: a launch of their own)
    hipLaunchKernelGGL(ld_requeue_kernel, GRID1(prev.n_act), 0, cx.s, prev.n_act, prev.list, prev.decision, g.indptr, g.indices, b.comm, b.flag);
    SCAMD_LAUNCH_CHECK();
  }
  return SCAMD_OK;
}

// Final polish of the level-0 partition in b.memb (see ld_polish_lock_kernel): full sweeps of lock-arbitrated moves until
// a sweep over ALL vertices finds no improving move -- node optimality by construction.  b.memb is updated in place;
// *out = what the pass did.  Needs b.Kref (the refinement's scratch) as the lock table.
// b.comm: every connected component of a community becomes its own community (ids = smallest member); totals recomputed.
// *n_split = components - communities (0: nothing changed).  Scratch: b.cid, the PH_CC_* counters.
static int split_disconnected(LeidenCtx& cx, const LevelGraph& g, int* n_split) {
  LeidenBuffers& b = cx.b;
  *n_split = 0;
  hipLaunchKernelGGL(ld_iota_kernel, GRID1(g.n), 0, cx.s, b.cid, g.n);
  SCAMD_LAUNCH_CHECK();
  for (int it = 0; it < g.n; ++it) {
    {
      const int rcf = run_fill(cx, Filler().add(b.counters + PH_CC_CHANGED, sizeof(int) * 3));
      if (rcf != SCAMD_OK) return rcf;
    }
    // (several propagation steps per host round trip: the flag only says whether any of them changed something)
    for (int rep = 0; rep < 4; ++rep) {
      hipLaunchKernelGGL(ld_cc_prop_kernel, dim3((unsigned)ceil_div(g.n, 16)), dim3(256), 0, cx.s, g.n, g.indptr, g.indices,
                         (const int*)b.comm, b.cid, b.counters + PH_CC_CHANGED);
      SCAMD_LAUNCH_CHECK();
    }
    int changed = 0;
    LD_FETCH(&changed, b.counters + PH_CC_CHANGED, sizeof(int), cx.s);
    LD_SYNC(cx.s);
    if (!changed) break;
  }
  hipLaunchKernelGGL(ld_cc_count_kernel, GRID1(g.n), 0, cx.s, g.n, (const int*)b.cid, (const int*)b.csize, b.counters + PH_CC_COMPONENTS);
  SCAMD_LAUNCH_CHECK();
  static_assert(PH_CC_COMPONENTS == PH_CC_CHANGED + 1 && PH_CC_COMMUNITIES == PH_CC_COMPONENTS + 1, "one clear, one fetch");
  int cnt[2] = {0, 0};  // components, communities
  LD_FETCH(cnt, b.counters + PH_CC_COMPONENTS, sizeof(cnt), cx.s);
  LD_SYNC(cx.s);
  *n_split = cnt[0] - cnt[1];
  if (cx.debug) fprintf(stderr, "[leiden] components %d, communities %d\n", cnt[0], cnt[1]);
  if (*n_split > 0) {
    std::swap(b.comm, b.cid);  // (the component labels ARE the new partition; b.cid is scratch)
    return compute_totals(cx, g, b.comm);
  }
  return SCAMD_OK;
}

constexpr int MAX_POLISH_ROUNDS = 1 << 16;
constexpr int MAX_POLISH_PASSES = 6;  // polish -> verifying iteration -> polish ... (each accepted pass raises Q)
struct PolishPass {
  int full_sweeps = 0, rounds = 0, moves = 0;
  int splits = 0;  // communities split off (split_disconnected)
};
static int polish_level0(LeidenCtx& cx, const LevelGraph& g, PolishPass* out) {
  LeidenBuffers& b = cx.b;
  const double gg = cx.gscale();
  const size_t n = (size_t)g.n;
  PolishPass& ps = *out;
  ps = PolishPass();
  // the polish works on b.comm in place: the partition changes buffers instead of being copied (b.comm <-> b.memb now and
  // back at the end; what b.comm held is scratch between iterations)
  std::swap(b.comm, b.memb);
  unsigned long long* lock = b.Kref;
  int rc = compute_totals(cx, g, b.comm, Filler().add(lock, sizeof(unsigned long long) * n).add(b.flag, sizeof(int) * n).add(b.counters, sizeof(int) * PH_PER_PHASE)
                                              .add(b.rcounters, sizeof(int) * CTR_AREA));
  if (rc != SCAMD_OK) return rc;  // (cx.b lives for this call only: an error return need not swap back)
  const int lanes = level_lanes(cx, g);
  unsigned int round = 0, area = 0;  // (the rounds alternate between the two counter areas, as the sweeps of the local moving do)
  int moved_before = 0, moved_at_full = 0;
  int checked_at = 0;  // moves + splits when the communities were last known to be connected (the input is: an iteration's result)
  bool full = true;  // the next round decides for every vertex (else: for the flagged ones)
  for (;;) {
    int* sw = b.rcounters + (area & 1u) * CTR_AREA;
    hipLaunchKernelGGL(ld_compact_cls_kernel, count_grid(cx, g.n), dim3(1024), 0, cx.s, g.n,
                       full ? (int*)nullptr : b.flag, b.cls_lists, sw, 1, 0u, tier_dst(cx, g, lanes),
                       b.rcounters + ((area + 1u) & 1u) * CTR_AREA, (int)(MAX_CLASSES + CTR_STRIDE));
    SCAMD_LAUNCH_CHECK();
    ++area;
    int hc[MAX_CLASSES + CTR_STRIDE], ht[PH_PER_PHASE];
    LD_FETCH(hc, sw, sizeof(hc), cx.s);
    LD_FETCH(ht, b.counters, sizeof(ht), cx.s);
    LD_SYNC(cx.s);
    SCAMD_REQUIRE(ht[PHASE_ERR] == 0, SCAMD_EINTERNAL, "leiden: hub table overflow (polish)");
    const int cnt = hc[0];
    const int moved = ht[PH_MOVED];               // ... of the pass so far
    const int moved_last = moved - moved_before;  // moves of the previous round
    moved_before = moved;
    ps.moves = moved;
    if (cx.debug)
      fprintf(stderr, "[leiden] polish round=%u %s act=%d moved_prev=%d lost_total=%d\n", round, full ? "full" : "flagged", cnt,
              moved_last, ht[PH_BLOCKED]);
    if (round >= MAX_POLISH_ROUNDS) {  // (every round moves at least one vertex and raises Q: a cap, not a rule)
      g_ld_stats[ST_POLISH_ROUND_CAP] = 1;  // ... but one that leaves node optimality unproven: reported (scamd_leiden_last_stats, tl.leiden warns)
      break;
    }
    if (cnt == 0) {
      // nobody is flagged any more.  If nothing moved since the last sweep over ALL vertices, that sweep was the proof
      // of node optimality; otherwise another full sweep has to give it.
      if (moved == moved_at_full) {
        // ... and if anything has moved since the communities were last known to be connected: split what a departure
        // cut in two (the parts are communities of their own then, and the proof has to be given again)
        if (moved + ps.splits == checked_at) break;
        int n_split = 0;
        rc = split_disconnected(cx, g, &n_split);
        if (rc != SCAMD_OK) return rc;
        ps.splits += n_split;
        checked_at = moved + ps.splits;
        if (n_split == 0) break;
      }
      full = true;
      continue;
    }
    if (full) {
      ++ps.full_sweeps;
      moved_at_full = moved;
    }
    full = false;
    ++round;
    ++ps.rounds;
    const int* list = b.cls_lists;
    rc = decide_tiers(cx, "polish move", g, 0, lanes, nullptr, hc + MAX_CLASSES,
                      MoveArgs{cnt, list, g.indptr, g.indices, g.wq, g.k, b.comm, b.Ktot, b.csize, gg, -1, cx.seed, b.target, TierLists{}});
    if (rc != SCAMD_OK) return rc;
    hipLaunchKernelGGL(ld_polish_lock_kernel, GRID1(cnt), 0, cx.s, cnt, list, (const int*)b.target, (const int*)b.comm, lock, round);
    SCAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_polish_apply_kernel, count_grid(cx, cnt), dim3(APPLY_THREADS), 0, cx.s, cnt, list, b.target, g.k, b.comm, b.Ktot, b.csize,
                       (const unsigned long long*)lock, round, b.flag, b.counters);
    SCAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_requeue_kernel, GRID1(cnt), 0, cx.s, cnt, list, (const int*)b.target, g.indptr, g.indices,
                       (const int*)b.comm, b.flag);
    SCAMD_LAUNCH_CHECK();
  }
  std::swap(b.comm, b.memb);  // the polished partition (or, when nothing moved, the one that came in) is b.memb again
  return SCAMD_OK;
}

static int refinement(LeidenCtx& cx, const LevelGraph& g, int* n_merged) {
  LeidenBuffers& b = cx.b;
  const double gg = cx.gscale();
  // fresh merge noise and fresh classes every outer iteration
  const unsigned int rseed = cx.seed + 0x9E3779B9u * (unsigned int)cx.iter;
  const unsigned int salt = hash32(rseed ^ 0x5bd1e995u);
  const size_t n = (size_t)g.n;
  const int lanes = refine_lanes(cx, g);
  with_lanes<false>(lanes, [&](auto G) {
    constexpr int L = decltype(G)::value;
    hipLaunchKernelGGL(ld_within_kernel<L>, dim3((unsigned)blocks_for(L, g.n)), dim3(256), 0, cx.s, g.n, g.indptr, g.indices, g.wq,
                       b.comm, b.a_in);
  });
  SCAMD_LAUNCH_CHECK();
  const int n_cls = rf_classes(g.n);
  int* rc0 = b.rcounters;  // [0, MAX_CLASSES): class list lengths; then per sub-round c: [CTR_JOINED], [CTR_N_MID], [CTR_N_BLK], [CTR_N_GIANT]
  // (also clears rc0, the phase counters and the join stamps b.touched: three memsets until round 6)
  hipLaunchKernelGGL(ld_refine_init_kernel, GRID1(g.n), 0, cx.s, g.n, g.k, b.a_in, b.comm, b.ref, b.refsize, b.Kref,
                     b.Eref, b.vrec, b.trec, b.touched, rc0, (int)(MAX_CLASSES + CTR_STRIDE * n_cls), b.counters);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_refine_candidates_kernel, dim3((unsigned)ceil_div(g.n, 1024)), dim3(1024), 0, cx.s, g.n, g.k,
                     b.comm, b.Ktot, b.a_in, gg, b.cls_lists, rc0, n_cls, salt, tier_dst(cx, g, lanes));
  SCAMD_LAUNCH_CHECK();
  LD_DBG_SYNC(cx, "rf candidates n=%d classes=%d", g.n, n_cls);
  int hc[CTR_AREA];  // class list lengths, then per sub-round [CTR_N_MID] / [CTR_N_BLK] / [CTR_N_GIANT] (ld_refine_candidates_kernel)
  LD_FETCH(hc, rc0, sizeof(int) * (MAX_CLASSES + CTR_STRIDE * n_cls), cx.s);
  LD_SYNC(cx.s);
  *n_merged = 0;
  // ONE sweep of n_cls sub-rounds, no host round trip in between: every candidate is considered exactly once (see
  // ld_refine_propose_kernel); the joiner counts stay on the device until the end
  for (int c = 0; c < n_cls; ++c) {
    const int cnt = hc[c];
    if (cnt == 0) continue;
    const int* list = b.cls_lists + (size_t)c * n;
    int* ctr = rc0 + MAX_CLASSES + CTR_STRIDE * c;
    const unsigned tgrid = (unsigned)std::min(32768, ceil_div(cnt, 256));
    const unsigned lgrid = (unsigned)std::min(32768, blocks_for(lanes, cnt));
    int rc = decide_tiers(cx, "rf propose", g, c, lanes, nullptr, hc + MAX_CLASSES + CTR_STRIDE * c,
                          ProposeArgs{cnt, list, g.indptr, g.indices, g.wq, g.k, b.comm, b.Ktot, b.ref, b.refsize, b.vrec, b.trec,
                                      RefineRule{gg, cx.inv_beta, c, n_cls, salt, rseed}, b.target, TierLists{}});
    if (rc != SCAMD_OK) return rc;
    hipLaunchKernelGGL(ld_refine_apply_kernel, dim3(tgrid), dim3(256), 0, cx.s, cnt, list, b.target, g.k, b.ref,
                       b.refsize, b.Kref, b.Eref, b.touched, c, b.rlist, ctr, b.vrec, b.trec);
    SCAMD_LAUNCH_CHECK();
    LD_DBG_SYNC(cx, "rf apply n=%d class=%d", g.n, c);
    with_lanes<false>(lanes, [&](auto G) {
      hipLaunchKernelGGL(ld_refine_cut_update_kernel<decltype(G)::value>, dim3(lgrid), dim3(256), 0, cx.s, cnt, b.rlist, g.indptr,
                         g.indices, g.wq, b.comm, b.ref, b.touched, b.a_in, c, b.Eref, (const int*)(ctr + CTR_JOINED), b.vrec, b.trec);
    });
    SCAMD_LAUNCH_CHECK();
    LD_DBG_SYNC(cx, "rf cut update n=%d class=%d", g.n, c);
  }
  int hr[CTR_AREA], herr = 0;
  LD_FETCH(hr, rc0, sizeof(int) * (MAX_CLASSES + CTR_STRIDE * n_cls), cx.s);
  LD_FETCH(&herr, b.counters + PHASE_ERR, sizeof(int), cx.s);
  LD_SYNC(cx.s);
  SCAMD_REQUIRE(herr == 0, SCAMD_EINTERNAL, "leiden: hub table overflow (refinement)");
  for (int c = 0; c < n_cls; ++c) {
    *n_merged += hr[MAX_CLASSES + CTR_STRIDE * c + CTR_JOINED];
    if (cx.debug)
      fprintf(stderr, "[leiden] rf n=%d class=%d/%d cand=%d merges=%d\n", g.n, c, n_cls, hc[c], hr[MAX_CLASSES + CTR_STRIDE * c + CTR_JOINED]);
  }
  return SCAMD_OK;
}

// Where level `level` + 1 (nn vertices, at most g.nnz entries, a map of g.n elements) goes: behind level `level` in the pool
// while the iteration's levels sit there one behind the other and the next one fits.  The first that does not fit gives the
// store up (depth 0: it is written over the lowest levels) and the rest of the iteration alternates between two places that
// are free of its source, as the two buffers of E entries did.  Whatever is written over stops belonging to the stored
// hierarchy HERE, before the first launch that writes.
static int place_level(LeidenCtx& cx, const LevelGraph& g, int level, int nn, StoredLevel* out) {
  LeidenBuffers& b = cx.b;
  const bool ext = level == 0;  // (the level-0 graph is the caller's)
  const StoredLevel& src = cx.lv[level];
  const size_t need_e = (size_t)std::max<int64_t>(g.nnz, 1), need_p = (size_t)nn + 1, need_c = (size_t)g.n;
  StoredLevel d;
  d.c_n = need_c;
  if (cx.it.built == level) {
    d.e_off = ext ? 0 : align_up(src.e_off + (size_t)src.g.nnz, POOL_ALIGN);
    d.p_off = ext ? 0 : align_up(src.p_off + (size_t)src.g.n + 1, POOL_ALIGN);
    d.c_off = ext ? 0 : align_up(src.c_off + src.c_n, POOL_ALIGN);
    if (d.e_off + need_e <= cx.cap_e && d.p_off + need_p <= cx.cap_p && d.c_off + need_c <= cx.cap_c) {
      d.cid = b.cid_pool + d.c_off;
      cx.it.built = level + 1;
      cx.kept.depth = std::min(cx.kept.depth, level);
      *out = d;
      return SCAMD_OK;
    }
    cx.it.built = -1;
    if (cx.debug) fprintf(stderr, "[leiden] level %d does not fit behind level %d in the pool: the hierarchy is not kept\n", level + 1, level);
  }
  cx.kept.depth = 0;
  d.e_off = (ext || src.e_off >= need_e) ? 0 : cx.cap_e / 2;
  d.p_off = (ext || src.p_off >= need_p) ? 0 : cx.cap_p / 2;
  d.c_off = 0;
  d.cid = b.cid;
  // (a source in the pool has every lower level before it, each at least its size; one off the pool sits at 0 or at half)
  SCAMD_REQUIRE(d.e_off + need_e <= cx.cap_e && d.p_off + need_p <= cx.cap_p &&
                    (ext || d.e_off + need_e <= src.e_off || d.e_off >= src.e_off + (size_t)src.g.nnz) &&
                    (ext || d.p_off + need_p <= src.p_off || d.p_off >= src.p_off + (size_t)src.g.n + 1),
                SCAMD_EINTERNAL, "leiden: no room for level %d beside its source", level + 1);
  *out = d;
  return SCAMD_OK;
}

// builds the coarse graph of `g` (level `level`) under b.ref into the pool (place_level) and records it as cx.lv[level + 1];
// updates b.comm (coarse phase-1 partition) and b.node_of.  Returns the new node count in *n_new (== g.n means nothing
// merged: no graph built).
static int aggregate(LeidenCtx& cx, const LevelGraph& g, int n_orig, int level, LevelGraph* out, int* n_new) {
  LeidenBuffers& b = cx.b;
  hipLaunchKernelGGL(ld_flag_kernel, GRID1(g.n), 0, cx.s, g.n, b.refsize, b.flag, b.rep);  // (+ b.rep = the atomicMin sentinel)
  SCAMD_LAUNCH_CHECK();
  int rc = exclusive_scan_i32_i64(b.flag, g.n, b.newid, b.scan_tmp, cx.s);
  if (rc != SCAMD_OK) return rc;
  int64_t nn = 0;
  LD_FETCH(&nn, b.newid + g.n, sizeof(int64_t), cx.s);
  LD_SYNC(cx.s);
  *n_new = (int)nn;
  if (nn == g.n) return SCAMD_OK;
  StoredLevel sl;
  rc = place_level(cx, g, level, (int)nn, &sl);
  if (rc != SCAMD_OK) return rc;
  int* cid = const_cast<int*>(sl.cid);
  hipLaunchKernelGGL(ld_coarse_ids_kernel, count_grid(cx, g.n), dim3(1024), 0, cx.s, g.n, b.ref, b.newid, b.comm, cid, b.rep);
  SCAMD_LAUNCH_CHECK();
  // (+ the cursors of the member scatter and the phase counters cleared: two memsets until round 6)
  hipLaunchKernelGGL(ld_coarse_comm_kernel, GRID1(g.n), 0, cx.s, g.n, cid, b.comm, b.rep, b.comm_tmp, (int)nn, b.cursor, b.counters);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_remap_kernel, GRID1(n_orig), 0, cx.s, n_orig, cid, b.node_of);
  SCAMD_LAUNCH_CHECK();
  // group the members of every coarse node, then combine their rows per coarse node in LDS
  hipLaunchKernelGGL(ld_agg_mcount_kernel, GRID1(g.n), 0, cx.s, g.n, b.refsize, b.newid, b.mcount);
  SCAMD_LAUNCH_CHECK();
  rc = exclusive_scan_i32_i64(b.mcount, nn, b.moff, b.scan_tmp, cx.s);
  if (rc != SCAMD_OK) return rc;
  hipLaunchKernelGGL(ld_agg_scatter_kernel, GRID1(g.n), 0, cx.s, g.n, cid, b.moff, b.cursor, g.indptr, b.members,
                     b.mdeg);
  SCAMD_LAUNCH_CHECK();
  rc = exclusive_scan_i32_i64(b.mdeg, g.n, b.eoff, b.scan_tmp, cx.s);
  if (rc != SCAMD_OK) return rc;
  const int inn = (int)nn;
  hipLaunchKernelGGL(ld_agg_wave_kernel, GRIDW(inn), 0, cx.s, inn, b.moff, b.eoff, b.members, g.indptr, g.indices, g.wq,
                     cid, b.agg_col, b.agg_w, b.rowcnt, b.mid_list, b.big_list, b.counters, cx.agg_wave_max,
                     cx.agg_mid_max, cx.agg_wave_work, cx.agg_mid_work, b.hub_list, cx.agg_split_work);
  SCAMD_LAUNCH_CHECK();
  // workgroup tiers: 512 threads on the 48 KB tables (3 per CU), 1024 threads on the 96 KB table (1 per CU).  Their list
  // lengths are read back first: an empty launch of these shapes costs 40 / 140 us (768 x 512 / 512 x 1024 threads with
  // 48 / 96 KB of LDS each), a host round trip 15 -- and most levels of a clustered graph have no such rows at all.
  static_assert(PH_AGG_BIG == PH_AGG_MID + 1 && PH_AGG_SPLIT == PH_AGG_BIG + 1, "one fetch");
  int htier[3] = {0, 0, 0};
  LD_FETCH(htier, b.counters + PH_AGG_MID, sizeof(htier), cx.s);
  LD_SYNC(cx.s);
  const int n_mid = htier[0], n_big = htier[1], n_split = htier[2];
  cx.agg_rows_mid = n_mid;
  cx.agg_rows_big = n_big;
  cx.agg_rows_split = n_split;
  if (cx.debug && (n_mid || n_big))
    fprintf(stderr, "[leiden] aggregate n=%d -> %d: %d rows through the workgroup tier, %d through the 8192-slot tier\n", g.n, inn,
            n_mid, n_big);
  if (n_mid > 0) {
    hipLaunchKernelGGL((ld_agg_block_kernel<AGG_MID_SLOTS, 512>), dim3((unsigned)std::min(AGG_MID_GRID, n_mid)), dim3(512),
                       (size_t)AGG_MID_SLOTS * 12, cx.s, b.mid_list, b.counters + PH_AGG_MID, inn, b.moff, b.eoff, b.members, g.indptr,
                       g.indices, g.wq, cid, b.agg_col, b.agg_w, b.rowcnt, b.counters + PHASE_ERR, AGG_MID_MAX, cx.hub_try_probes);
    SCAMD_LAUNCH_CHECK();
  }
  if (n_big > 0) {
    hipLaunchKernelGGL((ld_agg_block_kernel<BHUB_SLOTS, 1024>), dim3((unsigned)std::min(HUB_GRID, n_big)), dim3(1024),
                       HUB_LDS, cx.s, b.big_list, b.counters + PH_AGG_BIG, inn, b.moff, b.eoff, b.members, g.indptr, g.indices, g.wq,
                       cid, b.agg_col, b.agg_w, b.rowcnt, b.counters + PHASE_ERR, cx.agg_pass_keys, cx.hub_try_probes);
    SCAMD_LAUNCH_CHECK();
  }
  if (n_split > 0) {
    // split rows: parts -> built as pseudo rows by the 1024-thread builder -> merged (ld_agg_parts_kernel).  The list of
    // split rows borrows b.hub_list, their first part / part count b.rlist / b.touched (refinement scratch, idle here)
    const int64_t chunk = cx.agg_split_chunk;
    if (cx.debug) fprintf(stderr, "[leiden] aggregate n=%d -> %d: %d rows split into parts of %lld entries\n", g.n, inn, n_split, (long long)chunk);
    hipLaunchKernelGGL(ld_agg_parts_kernel, GRID1(n_split), 0, cx.s, (const int*)b.hub_list, b.counters, b.moff, b.eoff, chunk,
                       b.pmoff, b.part_list, b.rlist, b.touched);
    SCAMD_LAUNCH_CHECK();
    const int64_t parts_bound = (int64_t)n_split + g.nnz / chunk + 1;
    hipLaunchKernelGGL((ld_agg_block_kernel<BHUB_SLOTS, 1024>), dim3((unsigned)std::min<int64_t>(HUB_GRID, parts_bound)), dim3(1024),
                       HUB_LDS, cx.s, (const int*)b.part_list, (const int*)(b.counters + PH_AGG_PARTS), inn, (const int64_t*)b.pmoff, b.eoff,
                       b.members, g.indptr, g.indices, g.wq, cid, b.agg_col, b.agg_w, b.part_cnt, b.counters + PHASE_ERR,
                       cx.agg_pass_keys, cx.hub_try_probes);
    SCAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_agg_merge_kernel, dim3((unsigned)std::min(HUB_GRID, n_split)), dim3(1024), HUB_LDS, cx.s,
                       (const int*)b.hub_list, (const int*)b.counters, b.moff, b.eoff, (const int64_t*)b.pmoff, (const int*)b.part_cnt,
                       (const int*)b.rlist, (const int*)b.touched, b.agg_col, b.agg_w, b.rowcnt, b.counters + PHASE_ERR);
    SCAMD_LAUNCH_CHECK();
  }
  const CoarseBuf cb{b.pool.indptr + sl.p_off, b.pool.indices + sl.e_off, b.pool.wq + sl.e_off, b.pool.k + sl.p_off};
  rc = exclusive_scan_i32_i64(b.rowcnt, nn, cb.indptr, b.scan_tmp, cx.s);
  if (rc != SCAMD_OK) return rc;
  // the order of a row's entries is arbitrary: nothing downstream depends on it (all sums are integer, every
  // choice is an argmax under a total order)
  hipLaunchKernelGGL(ld_agg_compact_kernel, GRIDW(inn), 0, cx.s, inn, b.moff, b.eoff, cb.indptr, b.agg_col, b.agg_w,
                     cb.indices, cb.wq, b.counters + PH_MAX_DEG);  // (+ clears the row-length statistics ld_degstats_kernel adds to)
  SCAMD_LAUNCH_CHECK();
  int64_t nnz_new = 0;
  int max_deg = 0;
  int agg_err = 0;
  LD_FETCH(&agg_err, b.counters + PHASE_ERR, sizeof(int), cx.s);
  hipLaunchKernelGGL(ld_degstats_kernel, GRIDK(nn), 0, cx.s, cb.indptr, (int)nn, b.counters + PH_MAX_DEG);
  SCAMD_LAUNCH_CHECK();
  LD_FETCH(&max_deg, b.counters + PH_MAX_DEG, sizeof(int), cx.s);
  LD_FETCH(&nnz_new, cb.indptr + nn, sizeof(int64_t), cx.s);
  if (cx.cpm) {  // sizes add up over the members; strengths are the row sums of the coarse graph
    rc = run_fill(cx, Filler().add(cb.k, sizeof(long long) * nn));
    if (rc != SCAMD_OK) return rc;
    hipLaunchKernelGGL(ld_agg_nodeweight_kernel, GRID1(g.n), 0, cx.s, g.n, (const int*)cid, g.k, cb.k);
  } else {
    hipLaunchKernelGGL(ld_strength_kernel, GRIDW(nn), 0, cx.s, cb.indptr, cb.wq, (int)nn, cb.k);
  }
  SCAMD_LAUNCH_CHECK();
  std::swap(b.comm, b.comm_tmp);  // (the coarse phase-1 partition ld_coarse_comm_kernel wrote is b.comm from here on)
  LD_SYNC(cx.s);
  SCAMD_REQUIRE(agg_err == 0, SCAMD_EINTERNAL, "leiden: coarse-row table overflow");
  *out = LevelGraph{(int)nn, max_deg, nnz_new, cb.indptr, cb.indices, cb.wq, cb.k};
  sl.g = *out;
  cx.lv[level + 1] = sl;
  return SCAMD_OK;
}

// Level `level` takes its coarse graph and its vertex map from the stored hierarchy (no refinement, no aggregation): the
// coarse partition and node_of as aggregate() leaves them, from the CURRENT b.comm.
static int reuse_level(LeidenCtx& cx, const LevelGraph& g, int n_orig, int level, LevelGraph* out) {
  LeidenBuffers& b = cx.b;
  const StoredLevel& sl = cx.lv[level + 1];
  const int nn = sl.g.n;
  SCAMD_REQUIRE(sl.c_n == (size_t)g.n && nn >= 1 && nn < g.n, SCAMD_EINTERNAL, "leiden: stored level %d does not belong to a level of %d vertices",
                level + 1, g.n);
  if (cx.debug) {
    // every stored group lies inside one community of b.comm (nothing has moved below: b.comm is the projection of b.memb)
    for (int pass = 0; pass < 2; ++pass) {
      hipLaunchKernelGGL(ld_nest_check_kernel, GRID1(g.n), 0, cx.s, g.n, nn, sl.cid, (const int*)b.comm, b.comm_tmp, pass, b.counters + PHASE_ERR);
      SCAMD_LAUNCH_CHECK();
    }
    int bad = 0;
    LD_FETCH(&bad, b.counters + PHASE_ERR, sizeof(int), cx.s);
    LD_SYNC(cx.s);
    SCAMD_REQUIRE(bad == 0, SCAMD_EINTERNAL, "leiden: the stored level %d is not nested in the partition it is reused for (%d)", level + 1, bad);
  }
  int rc = run_fill(cx, Filler().add(b.rep, sizeof(int) * (size_t)g.n, 0x7f7f7f7fu));
  if (rc != SCAMD_OK) return rc;
  hipLaunchKernelGGL(ld_coarse_rep_kernel, count_grid(cx, g.n), dim3(1024), 0, cx.s, g.n, sl.cid, (const int*)b.comm, b.rep);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_coarse_comm_kernel, GRID1(g.n), 0, cx.s, g.n, sl.cid, (const int*)b.comm, (const int*)b.rep, b.comm_tmp, nn, b.cursor, b.counters);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_remap_kernel, GRID1(n_orig), 0, cx.s, n_orig, sl.cid, b.node_of);
  SCAMD_LAUNCH_CHECK();
  std::swap(b.comm, b.comm_tmp);
  *out = sl.g;
  ++g_ld_stats[ST_LEVELS_REUSED];
  return SCAMD_OK;
}

// SCAMD_LEIDEN_DEBUG trace of an iteration's levels: stage times (every lap drains the stream) and the lines on stderr.  Idle when
// the trace is off: no synchronisation, no output.
struct LevelTrace {
  LeidenCtx& cx;
  double last = 0.0;
  char level[192] = "";  // the head of a level's line: the level and its local moving
  double lap() {  // ms since the lap before
    if (!cx.debug) return 0.0;
    (void)hipStreamSynchronize(cx.s);
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    const double now = ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6, ms = now - last;
    last = now;
    return ms;
  }
  void moved(int l, const LevelGraph& g, int moves) {
    if (cx.debug)
      snprintf(level, sizeof(level), "[leiden] level %d n=%d nnz=%lld maxdeg=%d: local moving %.2f ms (%d moves)", l, g.n,
               (long long)g.nnz, g.max_deg, lap(), moves);
  }
  __attribute__((format(printf, 2, 3))) void say(const char* fmt, ...) const {
    if (!cx.debug) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
  }
};

// all remaining levels in one workgroup (ld_small_levels_kernel); b.comm[i] = final community of entry node i
static int small_levels(LeidenCtx& cx, const LevelGraph& g, int level) {
  LeidenBuffers& b = cx.b;
  int* info = b.counters + PH_SMALL_INFO;
  // (first_dst = 0: the entry level lives in the pool or is the caller's graph)
  const SmallArgs a{g.indptr, g.indices, g.wq, g.k, g.n, {b.sm_ix[0], b.sm_ix[1]}, {b.sm_w[0], b.sm_w[1]}, /*first_dst=*/0, b.comm,
                    cx.gscale(), cx.inv_beta, cx.seed, cx.iter, LM_STOP_PERMILLE, SMALL_SEQ_N, info, b.Ktot, b.total + 1};
  hipLaunchKernelGGL(ld_small_levels_kernel, dim3(1), dim3(SM_THREADS), sizeof(SmallLds), cx.s, a);
  SCAMD_LAUNCH_CHECK();
  if (cx.debug) {
    int h[4];
    LD_FETCH(h, info, sizeof(h), cx.s);
    LD_SYNC(cx.s);
    fprintf(stderr, "[leiden] small levels from level %d (n=%d nnz=%lld): %d levels, %d moves, %d merges -> n=%d\n", level, g.n,
            (long long)g.nnz, h[SM_INFO_LEVELS], h[SM_INFO_MOVES], h[SM_INFO_MERGES], h[SM_INFO_NODES]);
  }
  return SCAMD_OK;
}

// (from the partition in b.memb; the result goes to b.memb_work)
// Reuse of the stored hierarchy (iterations after the first): while no level of this iteration has moved a vertex, b.comm is
// the projection of b.memb, and the groups of the hierarchy that produced b.memb are nested in it -- such a level takes the
// stored coarse graph and vertex map instead of refining and aggregating (reuse_level).  The first level that moves
// anything, and every level above it, is refined and aggregated as ever and replaces the stored levels from there up.
static int leiden_iteration(LeidenCtx& cx, const LevelGraph& g0) {
  LeidenBuffers& b = cx.b;
  hipLaunchKernelGGL(ld_iter_init_kernel, GRID1(g0.n), 0, cx.s, g0.n, (const int*)b.memb, b.comm, b.node_of);
  SCAMD_LAUNCH_CHECK();
  LevelGraph g = g0;
  cx.l0_moves = -1;  // (a graph small enough to start in the one-workgroup kernel reports no level-0 count)
  bool quiet = cx.reuse && cx.iter >= 1;  // no level so far has moved anything
  int reused = 0;
  cx.it = IterHierarchy();
  const Hierarchy& kept = cx.kept;  // (place_level lowers its depth as the iteration writes over stored levels)
  LevelTrace tr{cx};
  for (int level = 0; level < MAX_LEVELS; ++level) {
    tr.lap();
    if (cx.small_levels && g.n <= SMALL_N && g.nnz <= SMALL_NNZ) {
      const int rcs = small_levels(cx, g, level);
      if (rcs != SCAMD_OK) return rcs;
      tr.say("[leiden] small levels %.2f ms\n", tr.lap());
      cx.it.end_level = level;
      cx.it.in_small = true;
      if (quiet && level >= 1 && reused == level) {  // (its move count: handed out by the synchronisation of iteration_quality())
        cx.it.quiet = true;
        LD_FETCH(&cx.it.small_moves, b.counters + PH_SMALL_INFO + SM_INFO_MOVES, sizeof(int), cx.s);
      }
      break;
    }
    int moves = 0;
    int rc = local_moving(cx, g, &moves);
    if (rc != SCAMD_OK) return rc;
    if (level == 0) cx.l0_moves = moves;
    cx.n_levels = level + 1;
    tr.moved(level, g, moves);
    if (moves != 0) quiet = false;
    const bool on_store = quiet && cx.it.built == level;  // nothing has moved, and every level so far came from the store
    if (on_store && kept.depth >= level + 1) {  // reuse this level
      LevelGraph gs;
      rc = reuse_level(cx, g, g0.n, level, &gs);
      if (rc != SCAMD_OK) return rc;
      cx.it.built = level + 1;
      ++reused;
      tr.say("%s, reused %.2f ms -> n=%d\n", tr.level, tr.lap(), gs.n);
      g = gs;
      continue;
    }
    if (on_store && level >= 1 && reused == level && kept.depth == level && kept.end_level == level && kept.end_kind != 0) {
      // the stored hierarchy ended here because nothing merged: so does this one
      tr.say("%s, reused: the last level\n", tr.level);
      cx.it.end_level = level;
      cx.it.end_kind = kept.end_kind;
      cx.it.quiet = true;
      ++g_ld_stats[ST_LEVELS_REUSED];
      break;
    }
    // refine and aggregate
    int merged = 0;
    rc = refinement(cx, g, &merged);
    if (rc != SCAMD_OK) return rc;
    tr.say("%s, refinement %.2f ms (%d merged)\n", tr.level, tr.lap(), merged);
    cx.it.end_level = level;
    if (merged == 0) {
      cx.it.end_kind = 1;
      break;
    }
    LevelGraph gn;
    int n_new = 0;
    rc = aggregate(cx, g, g0.n, level, &gn, &n_new);
    if (rc != SCAMD_OK) return rc;
    tr.say("[leiden] level %d aggregate %.2f ms -> n=%d\n", level, tr.lap(), n_new);
    if (n_new == g.n) {
      cx.it.end_kind = 2;
      break;
    }
    cx.it.end_level = -1;
    g = gn;
  }
  cx.it.top = g;
  hipLaunchKernelGGL(ld_gather_kernel, GRID1(g0.n), 0, cx.s, g0.n, b.comm, b.node_of, b.memb_work);
  SCAMD_LAUNCH_CHECK();
  return SCAMD_OK;
}

// Quality of the partition leiden_iteration() has just written to b.memb_work, from the level it ended on instead of a walk
// over level 0: b.memb_work = comm_top[node_of] and every coarse graph is P^T W P in integers, so the internal weight and the
// community totals of (top level, b.comm) are those of (level 0, b.memb_work) -- the same integers, and the same float64 sum
// of squares (quality_from_sums).
static int iteration_quality(LeidenCtx& cx, double* q) {
  if (cx.it.in_small) return quality_from_sums(cx, cx.it.top.n, cx.b.Ktot, nullptr, q);
  return evaluate(cx, cx.it.top, cx.b.comm, q);
}

// b.memb (values < n) relabelled to consecutive ids ordered by (size desc, first member asc) -> out (the caller's buffer)
static int renumber(LeidenCtx& cx, int n, int* n_comm, int* out) {
  LeidenBuffers& b = cx.b;
  {
    const int rcf = run_fill(cx, Filler().add(b.minmember, sizeof(int) * n, 0x7f7f7f7fu).add(b.csize, sizeof(int) * n));
    if (rcf != SCAMD_OK) return rcf;
  }
  hipLaunchKernelGGL(ld_minmember_kernel, count_grid(cx, n), dim3(1024), 0, cx.s, n, b.memb, b.minmember, b.csize);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_flag_kernel, GRID1(n), 0, cx.s, n, b.csize, b.flag, (int*)nullptr);
  SCAMD_LAUNCH_CHECK();
  int rc = exclusive_scan_i32_i64(b.flag, n, b.newid, b.scan_tmp, cx.s);
  if (rc != SCAMD_OK) return rc;
  int64_t nc = 0;
  LD_FETCH(&nc, b.newid + n, sizeof(int64_t), cx.s);
  LD_SYNC(cx.s);
  hipLaunchKernelGGL(ld_commkeys_kernel, GRID1(n), 0, cx.s, n, b.csize, b.minmember, b.newid, b.ckeys, b.cids);
  SCAMD_LAUNCH_CHECK();
  if (nc <= 131072) {
    hipLaunchKernelGGL(ld_rank_kernel, GRID1(nc), 0, cx.s, (int)nc, b.ckeys, b.cids, b.newlabel);
  } else {
    // degenerate partitions (hundreds of thousands of communities): consecutive ids by first member only
    hipLaunchKernelGGL(ld_compact_label_kernel, GRID1(nc), 0, cx.s, (int)nc, b.cids, b.newlabel);
  }
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_relabel_kernel, GRID1(n), 0, cx.s, n, b.newlabel, (const int*)b.memb, out);
  SCAMD_LAUNCH_CHECK();
  *n_comm = (int)nc;
  return SCAMD_OK;
}

static int setup_level0(LeidenCtx& cx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                        int64_t nnz, LevelGraph* g0) {
  LeidenBuffers& b = cx.b;
  {
    const int rcf = run_fill(cx, Filler().add(b.total, sizeof(unsigned long long) * 4).add(b.counters, sizeof(int) * 16));
    if (rcf != SCAMD_OK) return rcf;
  }
  hipLaunchKernelGGL(ld_level0_setup_kernel, dim3((unsigned)ceil_div(n, 16)), dim3(256), 0, cx.s, indptr, indices, weights, (int)n,
                     b.wq0, b.k0, b.total + 2);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_sum_kernel, dim3(256), dim3(256), 0, cx.s, b.k0, (int)n, b.total);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_degstats_kernel, GRIDK(n), 0, cx.s, indptr, (int)n, b.counters + PH_MAX_DEG);
  SCAMD_LAUNCH_CHECK();
  unsigned long long tot = 0;
  int max_deg = 0;
  LD_FETCH(&tot, b.total, sizeof(tot), cx.s);
  LD_FETCH(&max_deg, b.counters + PH_MAX_DEG, sizeof(int), cx.s);
  LD_FETCH(&cx.diag0, b.total + 2, sizeof(cx.diag0), cx.s);
  LD_SYNC(cx.s);
  cx.m2 = (double)tot;
  *g0 = LevelGraph{(int)n, max_deg, nnz, indptr, indices, b.wq0, b.k0};
  if (cx.cpm && cx.node_weights) {
    // (b.counters[PHASE_ERR] is zero: cleared above, nothing has raised it since)
    hipLaunchKernelGGL(ld_nodeweight_quantize_kernel, GRID1(n), 0, cx.s, cx.node_weights, (int)n, b.k0, b.counters + PHASE_ERR);
    SCAMD_LAUNCH_CHECK();
    int bad = 0;
    LD_FETCH(&bad, b.counters + PHASE_ERR, sizeof(int), cx.s);
    LD_SYNC(cx.s);
    SCAMD_REQUIRE(bad == 0, SCAMD_EINVAL, "leiden: node weights must lie in [0, 1e6]");
    cx.nw_scale = NODE_WEIGHT_SCALE;
  } else if (cx.cpm) {  // the vertex weights of CPM are counts; the strengths above were only needed for 2m
    hipLaunchKernelGGL(ld_fill_i64_kernel, GRID1(n), 0, cx.s, b.k0, (int)n, 1ll);
    SCAMD_LAUNCH_CHECK();
  }
  return SCAMD_OK;
}

// What the three Leiden entries (the run, the component-split test entry, the modularity of a given partition) share: the
// checks of the graph's pointers and shape, the switches, the context over the caller's workspace, the level-0 graph.
// `what` prefixes the error messages ("leiden", "leiden split", "modularity").
static int leiden_open(LeidenCtx& cx, const char* what, const int64_t* indptr, const int32_t* indices, const float* weights,
                       int64_t n, int64_t nnz, void* workspace, size_t workspace_bytes, scamd_stream_t stream, LevelGraph* g0) {
  SCAMD_REQUIRE(indptr && (nnz == 0 || (indices && weights)), SCAMD_EINVAL, "%s: null pointer", what);
  SCAMD_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && nnz >= 0, SCAMD_EINVAL, "%s: bad shape n=%lld nnz=%lld", what, (long long)n,
                (long long)nnz);
  read_knobs(cx);
  cx.s = stream;
  cx.cap_e = 2 * (size_t)std::max<int64_t>(nnz, 1);
  cx.cap_p = 2 * ((size_t)n + 1);
  cx.cap_c = 2 * (size_t)n;
  Workspace ws(workspace, workspace_bytes);
  leiden_carve(ws, n, nnz, &cx.b);
  SCAMD_REQUIRE(workspace && ws.ok, SCAMD_EWORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes, ws.used());
  return setup_level0(cx, indptr, indices, weights, n, nnz, g0);
}

// what the four scamd_leiden_csr_* entries pass
struct LeidenCall {
  const int64_t* indptr; const int32_t* indices; const float* weights; int64_t n, nnz;
  double resolution; int n_iterations; double beta; uint64_t seed;
  int objective;  // 0 = modularity, 1 = CPM
  const float* node_weights; const int32_t* initial_membership;  // NULL: every vertex weighs 1 (CPM) / singletons
  int32_t* membership; double* modularity_host; int32_t* n_communities_host;
  void* workspace; size_t workspace_bytes; scamd_stream_t stream;
};

// One outer iteration from b.memb and its verdict: +1 improved (accepted: the partition is b.memb now and what the iteration
// built or reused is the stored hierarchy), 0 the same quality, -1 worse (b.memb stands either way: synchronous moves and the
// randomised refinement are not monotone).  *q_best is raised when the iteration is accepted.
static int accept_iteration(LeidenCtx& cx, const LevelGraph& g0, int it, double* q_best, int* verdict) {
  LeidenBuffers& b = cx.b;
  cx.iter = it;
  g_ld_stats[ST_ITERATIONS] = it + 1;
  double q = 0.0;
  int rc = leiden_iteration(cx, g0);
  if (rc == SCAMD_OK) rc = iteration_quality(cx, &q);
  if (rc != SCAMD_OK) return rc;
  if (cx.debug) fprintf(stderr, "[leiden] iteration %d: Q = %.10f (best before %.10f), level-0 moves %d\n", it, q, *q_best, cx.l0_moves);
  if (cx.it.quiet && cx.it.small_moves == 0) ++g_ld_stats[ST_QUIET_REUSE_ITERS];
  *verdict = q > *q_best + 1e-12 ? 1 : (q < *q_best - 1e-12 ? -1 : 0);
  if (*verdict > 0) {
    *q_best = q;
    std::swap(b.memb, b.memb_work);
    cx.kept = cx.it.accepted();
  }
  return SCAMD_OK;
}

// the kernels whose dynamic LDS exceeds the default limit of a launch (every entry that may launch one asks first)
static int allow_dynamic_lds() {
  const struct {
    const void* kernel;
    size_t lds;
  } dyn_lds[] = {{reinterpret_cast<const void*>(ld_move_hub_kernel), HUB_LDS},
                 {reinterpret_cast<const void*>(ld_refine_propose_hub_kernel), HUB_LDS},
                 {reinterpret_cast<const void*>(ld_agg_merge_kernel), HUB_LDS},
                 {reinterpret_cast<const void*>(ld_agg_block_kernel<BHUB_SLOTS, 1024>), HUB_LDS},
                 {reinterpret_cast<const void*>(ld_small_levels_kernel), sizeof(SmallLds)}};
  for (const auto& k : dyn_lds) SCAMD_HIP_CHECK(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));
  return SCAMD_OK;
}

// the merge rule's parameters as a run derives them from its arguments
static void set_rule(LeidenCtx& cx, double resolution, double beta, uint64_t seed) {
  cx.gamma = resolution;
  cx.inv_beta = beta > 0.0 ? 1.0 / (beta * WSCALE) : 0.0;  // beta <= 0: the greedy limit (largest gain, no "stay")
  cx.seed = (unsigned int)(seed ^ (seed >> 32)) * 0x9E3779B1u + 0x632BE5ABu;
}

static int leiden_run(const LeidenCall& c) {
  SCAMD_REQUIRE(c.membership, SCAMD_EINVAL, "leiden: null pointer");
  SCAMD_REQUIRE(c.resolution >= 0.0, SCAMD_EINVAL, "leiden: negative resolution");
  for (int i = 0; i < LD_NSTATS; ++i) g_ld_stats[i] = 0;
  g_ld_sweep_bytes = 0.0;
  const int64_t n = c.n;
  const int n_iterations = c.n_iterations;
  LeidenCtx cx;
  set_rule(cx, c.resolution, c.beta, c.seed);
  cx.cpm = c.objective == 1;
  cx.node_weights = c.node_weights;
  LevelGraph g0;
  int rc = leiden_open(cx, "leiden", c.indptr, c.indices, c.weights, n, c.nnz, c.workspace, c.workspace_bytes, c.stream, &g0);
  if (rc != SCAMD_OK) return rc;
  if (cx.cpm) cx.small_levels = false;  // (ld_small_levels_kernel derives its coarse vertex weights from row sums: strengths)
  rc = allow_dynamic_lds();
  if (rc != SCAMD_OK) return rc;
  LeidenBuffers& b = cx.b;
  if (c.initial_membership) {
    // (b.counters[PHASE_ERR] is zero: setup_level0 cleared the counters and checked whatever it raised)
    hipLaunchKernelGGL(ld_copy_membership_kernel, GRID1(n), 0, cx.s, (int)n, c.initial_membership, b.memb, b.counters + PHASE_ERR);
    SCAMD_LAUNCH_CHECK();
    int bad = 0;
    LD_FETCH(&bad, b.counters + PHASE_ERR, sizeof(int), cx.s);
    LD_SYNC(cx.s);
    SCAMD_REQUIRE(bad == 0, SCAMD_EINVAL, "leiden: initial membership ids must lie in [0, n)");
  } else {
    hipLaunchKernelGGL(ld_iota_kernel, GRID1(n), 0, cx.s, b.memb, (int)n);
    SCAMD_LAUNCH_CHECK();
  }
  double q_best = 0.0;
  if (cx.m2 > 0.0) {
    // (singletons: the totals are the vertex weights themselves, the internal weight is the stored diagonal)
    rc = c.initial_membership ? evaluate(cx, g0, b.memb, &q_best)
                              : quality_from_sums(cx, g0.n, reinterpret_cast<const unsigned long long*>(g0.k), &cx.diag0, &q_best);
    if (rc != SCAMD_OK) return rc;
    // b.memb is ALWAYS the best partition seen (the input of the next iteration); an iteration writes into b.memb_work and
    // the two change places when it improved -- no copies (round 5: two 4-byte-per-vertex blits per iteration)
    g_ld_stats[ST_ITER_CAP] = cx.iter_cap;
    int max_iter = n_iterations < 0 ? cx.iter_cap : n_iterations;
    if (n_iterations < 0 && cx.max_iters > 0) max_iter = std::min(max_iter, cx.max_iters);
    int bad_iters = 0;
    // true once b.memb has been the INPUT of an iteration whose level-0 local moving found nothing to move: its
    // first sweep decides for every vertex on the final state, so that is a proof of node optimality
    bool best_is_clean = false;
    bool ended_by_cap = true;  // the loop below ran out of iterations (n_iterations < 0: the iteration cap) instead of converging
    for (int it = 0; it < max_iter; ++it) {
      int verdict = 0;
      rc = accept_iteration(cx, g0, it, &q_best, &verdict);
      if (rc != SCAMD_OK) return rc;
      if (it == 0) g_ld_stats[ST_LEVELS_FIRST_ITER] = cx.n_levels;
      if (verdict > 0) {
        bad_iters = 0;
        best_is_clean = false;
      } else if (cx.l0_moves == 0) {
        best_is_clean = true;
      }
      // n_iterations < 0: until an iteration changes nothing (leidenalg: `while diff_inc > 0`).  An iteration that
      // reproduces the best quality exactly found nothing to move -> done.  One that came out WORSE was unlucky in its
      // random merges (the next one draws different noise, cx.iter is part of the noise seed): two of those in a row end
      // the run as well -- without this patience a single unlucky iteration right after the first one froze the
      // result of ONE iteration (Q 0.8028 instead of 0.812 on the 700-cell fixture).
      if (n_iterations < 0 && verdict <= 0) {
        ended_by_cap = false;
        if (verdict == 0 || ++bad_iters >= 2) break;
        ended_by_cap = true;
      }
    }
    // n_iterations < 0 promises a STABLE partition (leidenalg iterates until an iteration changes nothing; such a
    // partition is node optimal and g-separated).  Ours is the best of a run of non-monotone iterations.  Unless the last
    // iteration proved it (best_is_clean): strictly monotone single-vertex moves until a sweep over all vertices finds
    // none (polish_level0), then -- the moved vertices may have made two communities mergeable, or cut one in two -- ONE
    // ordinary iteration from the polished partition: its level-0 moving finds nothing, its refinement and coarse levels
    // re-examine everything else.  No gain: stable, done.  A gain: accepted, and the polish runs again.
    int n_iter_total = g_ld_stats[ST_ITERATIONS];
    ended_by_cap = ended_by_cap && max_iter == cx.iter_cap;  // (not the test knob's cap: that one is followed up)
    g_ld_stats[ST_ENDED_BY_ITER_CAP] = (n_iterations < 0 && ended_by_cap) ? 1 : 0;
    for (int pr = 0; n_iterations < 0 && cx.polish && pr <= MAX_POLISH_PASSES; ++pr) {
      if (best_is_clean) {
        if (pr == 0) g_ld_stats[ST_POLISH_SKIPPED_PROVEN] = 1;
        break;
      }
      PolishPass ps;
      rc = polish_level0(cx, g0, &ps);
      if (rc != SCAMD_OK) return rc;
      g_ld_stats[ST_POLISH_FULL_SWEEPS] += ps.full_sweeps;
      g_ld_stats[ST_POLISH_ROUNDS] += ps.rounds;
      g_ld_stats[ST_POLISH_MOVES] += ps.moves;
      g_ld_stats[ST_POLISH_SPLITS] += ps.splits;
      if (ps.moves == 0) break;  // the full sweep found no improving move: node optimal as it stands
      cx.kept.depth = 0;  // b.memb changed in place: the stored hierarchy is no longer its own, the iteration below runs in full
      double q = 0.0;
      rc = evaluate(cx, g0, b.memb, &q);
      if (rc != SCAMD_OK) return rc;
      if (cx.debug)
        fprintf(stderr, "[leiden] polish %d: %d full sweeps, %d rounds, %d moves: Q %.10f -> %.10f\n", pr, ps.full_sweeps, ps.rounds,
                ps.moves, q_best, q);
      SCAMD_REQUIRE(q >= q_best - 1e-12, SCAMD_EINTERNAL, "leiden: the monotone polish lowered the quality (%.12f -> %.12f)", q_best, q);
      q_best = q;
      // (the last pass only polishes what the last accepted iteration left.  A run that the iteration cap ended was still
      // gaining a little with every iteration -- structure-less graphs do that for dozens of iterations: there is no stable
      // partition to verify, the polished one is node optimal and connected, and that is what is returned)
      if (pr == MAX_POLISH_PASSES || ended_by_cap) break;
      int verdict = 0;
      rc = accept_iteration(cx, g0, n_iter_total++, &q_best, &verdict);
      if (rc != SCAMD_OK) return rc;
      if (verdict <= 0) break;  // stable: the polished partition (b.memb) stands
    }
  }
  if (cx.cpm && cx.m2 > 0.0) {
    // what is reported is the modularity of the partition (the reference stores `part.modularity`), not the CPM quality the
    // run maximised: strengths back into k0, totals, resolution 1
    hipLaunchKernelGGL(ld_strength_kernel, GRIDW(n), 0, cx.s, c.indptr, b.wq0, (int)n, b.k0);
    SCAMD_LAUNCH_CHECK();
    cx.cpm = false;
    cx.gamma = 1.0;
    rc = evaluate(cx, g0, b.memb, &q_best);
    if (rc != SCAMD_OK) return rc;
  }
  int nc = 0;
  rc = renumber(cx, (int)n, &nc, c.membership);  // (writes the caller's buffer directly)
  if (rc != SCAMD_OK) return rc;
  LD_SYNC(cx.s);
  if (c.modularity_host) *c.modularity_host = q_best;
  if (c.n_communities_host) *c.n_communities_host = nc;
  return SCAMD_OK;
}

}  // namespace scamd

using namespace scamd;

extern "C" size_t scamd_leiden_workspace_bytes(int64_t n, int64_t nnz) {
  if (n <= 0 || nnz < 0) return 0;
  Workspace ws(nullptr, 0);
  LeidenBuffers b;
  leiden_carve(ws, n, nnz, &b);
  return ws.used();
}

extern "C" int scamd_leiden_csr_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                    int64_t nnz, double resolution, int n_iterations, double beta, uint64_t seed,
                                    int32_t* membership, double* modularity_host, int32_t* n_communities_host,
                                    void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  return leiden_run(LeidenCall{indptr, indices, weights, n, nnz, resolution, n_iterations, beta, seed, 0, nullptr, nullptr, membership,
                               modularity_host, n_communities_host, workspace, workspace_bytes, stream});
}

// ... starting from a given partition instead of singletons (`initial_membership` of leidenalg.find_partition /
// igraph community_leiden, passed through `**clustering_args` at src/scanpy/tools/_leiden.py:66, 174-196): ids in [0, n),
// device pointer; n_iterations = 0 returns it renumbered with its modularity.
extern "C" int scamd_leiden_csr_init_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                         int64_t nnz, double resolution, int n_iterations, double beta, uint64_t seed,
                                         const int32_t* initial_membership, int32_t* membership,
                                         double* modularity_host, int32_t* n_communities_host, void* workspace,
                                         size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(initial_membership, SCAMD_EINVAL, "leiden: null initial membership");
  return leiden_run(LeidenCall{indptr, indices, weights, n, nnz, resolution, n_iterations, beta, seed, 0, nullptr, initial_membership,
                               membership, modularity_host, n_communities_host, workspace, workspace_bytes, stream});
}

// ... with the objective named: 0 = modularity (the two entry points above), 1 = CPM -- igraph's
// `community_leiden(objective_function='CPM')`, reachable through `sc.tl.leiden(flavor='igraph', objective_function='CPM')`
// (src/scanpy/tools/_leiden.py:188-196): every vertex weighs 1, the resolution is NOT divided by 2m, a community pays
// gamma n_C^2.  initial_membership may be NULL.  *modularity_host is the (resolution 1) modularity of the returned partition
// either way -- what the reference stores (`part.modularity`, :219) -- for objective 0 at the given resolution, as before.
extern "C" int scamd_leiden_csr_ex_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                       int64_t nnz, double resolution, int n_iterations, double beta, uint64_t seed,
                                       int objective, const int32_t* initial_membership, int32_t* membership,
                                       double* modularity_host, int32_t* n_communities_host, void* workspace,
                                       size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(objective == 0 || objective == 1, SCAMD_EINVAL, "leiden: objective %d (0 = modularity, 1 = CPM)", objective);
  return leiden_run(LeidenCall{indptr, indices, weights, n, nnz, resolution, n_iterations, beta, seed, objective, nullptr,
                               initial_membership, membership, modularity_host, n_communities_host, workspace, workspace_bytes, stream});
}

// ... CPM with the caller's vertex weights: igraph's `community_leiden(objective_function='CPM', node_weights=...)`, reachable
// through `sc.tl.leiden(flavor='igraph', objective_function='CPM', node_weights=...)` (`**clustering_args`,
// src/scanpy/tools/_leiden.py:66, 188-196): a community pays gamma (sum of its members' weights)^2.  node_weights: device
// pointer, n floats in [0, 1e6] (held in fixed point with 16 fractional bits); NULL = every vertex weighs 1.  With the
// modularity objective the vertex weights ARE the strengths: node_weights must be NULL there.
extern "C" int scamd_leiden_csr_nw_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                       int64_t nnz, double resolution, int n_iterations, double beta, uint64_t seed,
                                       int objective, const float* node_weights, const int32_t* initial_membership,
                                       int32_t* membership, double* modularity_host, int32_t* n_communities_host,
                                       void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(objective == 0 || objective == 1, SCAMD_EINVAL, "leiden: objective %d (0 = modularity, 1 = CPM)", objective);
  SCAMD_REQUIRE(objective == 1 || node_weights == nullptr, SCAMD_EUNSUPPORTED,
                "leiden: node weights with the modularity objective (its vertex weights are the strengths)");
  return leiden_run(LeidenCall{indptr, indices, weights, n, nnz, resolution, n_iterations, beta, seed, objective, node_weights,
                               initial_membership, membership, modularity_host, n_communities_host, workspace, workspace_bytes, stream});
}

// Test entry: the component split of the polish (split_disconnected) on a GIVEN membership (ids in [0, n)): every
// connected component of a community becomes a community of its own (id = its smallest vertex); membership is rewritten
// in place when anything was split, *n_split_host = components - communities.
extern "C" int scamd_leiden_debug_split_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                            int64_t nnz, int32_t* membership, int32_t* n_split_host, void* workspace,
                                            size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(membership && n_split_host, SCAMD_EINVAL, "leiden split: null pointer");
  LeidenCtx cx;
  cx.gamma = 1.0;
  cx.seed = 0;
  LevelGraph g0;
  int rc = leiden_open(cx, "leiden split", indptr, indices, weights, n, nnz, workspace, workspace_bytes, stream, &g0);
  if (rc != SCAMD_OK) return rc;
  hipLaunchKernelGGL(ld_copy_i32_kernel, GRID1(n), 0, cx.s, (int)n, (const int*)membership, cx.b.comm);
  SCAMD_LAUNCH_CHECK();
  rc = compute_totals(cx, g0, cx.b.comm);
  if (rc != SCAMD_OK) return rc;
  int n_split = 0;
  rc = split_disconnected(cx, g0, &n_split);
  if (rc != SCAMD_OK) return rc;
  if (n_split > 0) {
    hipLaunchKernelGGL(ld_copy_i32_kernel, GRID1(n), 0, cx.s, (int)n, (const int*)cx.b.comm, membership);
    SCAMD_LAUNCH_CHECK();
  }
  SCAMD_HIP_CHECK(hipStreamSynchronize(cx.s));
  *n_split_host = n_split;
  return SCAMD_OK;
}

// Test entry: ONE level of an iteration on a GIVEN partition -- the refinement and the coarse graph, by the functions the run
// itself calls (leiden_open, ld_iter_init_kernel, compute_totals, refinement, aggregate), with their results copied out.
// refined_in != NULL: the refinement is skipped and the coarse graph is built under the caller's refined partition (group
// shapes chosen, not drawn); Kref and refsize are then its totals (ld_totals_kernel), Eref is zero.
extern "C" int scamd_leiden_debug_level_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                            int64_t nnz, const int32_t* membership, const int32_t* refined_in, double resolution,
                                            double beta, uint64_t seed, int32_t* refined, uint64_t* Kref, uint64_t* Eref,
                                            int32_t* refsize, int32_t* cid, int64_t* coarse_indptr, int32_t* coarse_indices,
                                            int64_t* coarse_wq, int64_t* coarse_k, int32_t* coarse_comm, int64_t* info_host,
                                            void* workspace, size_t workspace_bytes, scamd_stream_t stream) {
  SCAMD_REQUIRE(membership && refined && Kref && Eref && refsize && cid && coarse_indptr && coarse_k && coarse_comm && info_host &&
                    (nnz == 0 || (coarse_indices && coarse_wq)),
                SCAMD_EINVAL, "leiden level: null pointer");
  SCAMD_REQUIRE(resolution >= 0.0, SCAMD_EINVAL, "leiden level: negative resolution");
  for (int i = 0; i < LD_NSTATS; ++i) g_ld_stats[i] = 0;  // (scamd_leiden_last_stats: the tiers of the propose steps of this call)
  g_ld_sweep_bytes = 0.0;
  LeidenCtx cx;
  set_rule(cx, resolution, beta, seed);
  LevelGraph g0;
  int rc = leiden_open(cx, "leiden level", indptr, indices, weights, n, nnz, workspace, workspace_bytes, stream, &g0);
  if (rc == SCAMD_OK) rc = allow_dynamic_lds();
  if (rc != SCAMD_OK) return rc;
  LeidenBuffers& b = cx.b;
  const int in = (int)n;
  // (b.counters[PHASE_ERR] is zero: setup_level0 cleared the counters and checked whatever it raised)
  hipLaunchKernelGGL(ld_copy_membership_kernel, GRID1(n), 0, cx.s, in, membership, b.memb, b.counters + PHASE_ERR);
  SCAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_iter_init_kernel, GRID1(n), 0, cx.s, in, (const int*)b.memb, b.comm, b.node_of);
  SCAMD_LAUNCH_CHECK();
  if (refined_in) {
    hipLaunchKernelGGL(ld_given_ref_kernel, GRID1(n), 0, cx.s, in, refined_in, (const int*)b.comm, b.ref, b.counters + PHASE_ERR);
    SCAMD_LAUNCH_CHECK();
  }
  int bad = 0;
  LD_FETCH(&bad, b.counters + PHASE_ERR, sizeof(int), cx.s);
  LD_SYNC(cx.s);
  SCAMD_REQUIRE(bad == 0, SCAMD_EINVAL,
                "leiden level: ids must lie in [0, n), a refined group is named by one of its members and lies inside one community");
  int merged = 0;
  if (refined_in) {
    rc = run_fill(cx, Filler().add(b.Kref, sizeof(unsigned long long) * n).add(b.Eref, sizeof(unsigned long long) * n).add(b.refsize, sizeof(int) * n));
    if (rc != SCAMD_OK) return rc;
    hipLaunchKernelGGL(ld_totals_kernel, count_grid(cx, in), dim3(1024), 0, cx.s, (const int*)b.ref,
                       g0.k, in, b.Kref, b.refsize, (unsigned long long*)nullptr);
    SCAMD_LAUNCH_CHECK();
  } else {
    SCAMD_REQUIRE(cx.m2 > 0.0, SCAMD_EINVAL, "leiden level: the refinement needs a graph with weight");
    rc = compute_totals(cx, g0, b.comm);
    if (rc == SCAMD_OK) rc = refinement(cx, g0, &merged);
    if (rc != SCAMD_OK) return rc;
  }
  // (before aggregate(): it borrows refinement scratch and swaps b.comm)
  SCAMD_HIP_CHECK(hipMemcpyAsync(refined, b.ref, sizeof(int) * n, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(Kref, b.Kref, sizeof(unsigned long long) * n, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(Eref, b.Eref, sizeof(unsigned long long) * n, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(refsize, b.refsize, sizeof(int) * n, hipMemcpyDeviceToDevice, cx.s));
  LevelGraph gc;
  int n_new = 0;
  rc = aggregate(cx, g0, in, 0, &gc, &n_new);
  if (rc != SCAMD_OK) return rc;
  const bool skipped = n_new == in;  // nothing merged: aggregate() builds no graph
  if (!skipped) {
    const size_t nn = (size_t)gc.n, ne = (size_t)gc.nnz;
    SCAMD_HIP_CHECK(hipMemcpyAsync(cid, cx.lv[1].cid, sizeof(int) * n, hipMemcpyDeviceToDevice, cx.s));
    SCAMD_HIP_CHECK(hipMemcpyAsync(coarse_indptr, gc.indptr, sizeof(int64_t) * (nn + 1), hipMemcpyDeviceToDevice, cx.s));
    if (ne > 0) {
      SCAMD_HIP_CHECK(hipMemcpyAsync(coarse_indices, gc.indices, sizeof(int) * ne, hipMemcpyDeviceToDevice, cx.s));
      SCAMD_HIP_CHECK(hipMemcpyAsync(coarse_wq, gc.wq, sizeof(long long) * ne, hipMemcpyDeviceToDevice, cx.s));
    }
    SCAMD_HIP_CHECK(hipMemcpyAsync(coarse_k, gc.k, sizeof(long long) * nn, hipMemcpyDeviceToDevice, cx.s));
    SCAMD_HIP_CHECK(hipMemcpyAsync(coarse_comm, b.comm, sizeof(int) * nn, hipMemcpyDeviceToDevice, cx.s));
  }
  SCAMD_HIP_CHECK(hipStreamSynchronize(cx.s));
  info_host[0] = refined_in ? (int64_t)(in - n_new) : (int64_t)merged;
  info_host[1] = n_new;
  info_host[2] = skipped ? 0 : gc.nnz;
  info_host[3] = skipped ? 0 : cx.agg_rows_mid;
  info_host[4] = skipped ? 0 : cx.agg_rows_big;
  info_host[5] = skipped ? 0 : cx.agg_rows_split;
  info_host[6] = skipped ? 1 : 0;
  info_host[7] = 0;
  return SCAMD_OK;
}

// Test entry: the counters of one local-moving sub-round structure on a GIVEN partition, by the functions and kernels the run
// itself uses -- compute_totals, the class-list builder of a sweep (ld_compact_cls_kernel; flags_in == NULL: every vertex is
// listed, as in the first sweep of a level) and ld_apply_kernel once per non-empty class, with the caller's decisions
// (decision[v]: >= 0 the community v moves to, -2 blocked, anything else stays) gathered to list positions.
extern "C" int scamd_leiden_debug_counters_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                               int64_t nnz, const int32_t* membership, const int32_t* flags_in, int n_cls,
                                               uint32_t salt, const int32_t* decision, int32_t* lists, int32_t* tier_lists,
                                               int32_t* giant_lists, uint64_t* Ktot_before, int32_t* csize_before,
                                               int32_t* comm_after, uint64_t* Ktot_after, int32_t* csize_after, int32_t* flags_after,
                                               int32_t* counts_host, int64_t* info_host, void* workspace, size_t workspace_bytes,
                                               scamd_stream_t stream) {
  SCAMD_REQUIRE(membership && decision && lists && tier_lists && giant_lists && Ktot_before && csize_before && comm_after && Ktot_after &&
                    csize_after && flags_after && counts_host && info_host,
                SCAMD_EINVAL, "leiden counters: null pointer");
  // (the workspace holds MAX_CLASSES lists for levels of at most 4096 vertices, DEF_CLASSES beyond: leiden_carve, rf_classes)
  const int most_cls = n <= 4096 ? MAX_CLASSES : DEF_CLASSES;
  SCAMD_REQUIRE(n_cls >= 1 && n_cls <= most_cls && (n_cls & (n_cls - 1)) == 0, SCAMD_EINVAL,
                "leiden counters: n_cls %d (a power of two up to %d at n = %lld)", n_cls, most_cls, (long long)n);
  LeidenCtx cx;
  set_rule(cx, 1.0, 0.01, 0);
  LevelGraph g;
  int rc = leiden_open(cx, "leiden counters", indptr, indices, weights, n, nnz, workspace, workspace_bytes, stream, &g);
  if (rc != SCAMD_OK) return rc;
  LeidenBuffers& b = cx.b;
  const int in = (int)n;
  hipLaunchKernelGGL(ld_copy_membership_kernel, GRID1(n), 0, cx.s, in, membership, b.comm, b.counters + PHASE_ERR);
  SCAMD_LAUNCH_CHECK();
  int bad = 0;
  LD_FETCH(&bad, b.counters + PHASE_ERR, sizeof(int), cx.s);
  LD_SYNC(cx.s);
  SCAMD_REQUIRE(bad == 0, SCAMD_EINVAL, "leiden counters: ids must lie in [0, n)");
  rc = compute_totals(cx, g, b.comm, Filler().add(b.flag, sizeof(int) * n).add(b.counters, sizeof(int) * PH_PER_PHASE).add(b.rcounters, sizeof(int) * CTR_AREA));
  if (rc != SCAMD_OK) return rc;
  SCAMD_HIP_CHECK(hipMemcpyAsync(Ktot_before, b.Ktot, sizeof(unsigned long long) * n, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(csize_before, b.csize, sizeof(int) * n, hipMemcpyDeviceToDevice, cx.s));
  if (flags_in) SCAMD_HIP_CHECK(hipMemcpyAsync(b.flag, flags_in, sizeof(int) * n, hipMemcpyDeviceToDevice, cx.s));
  const int lanes = level_lanes(cx, g);
  hipLaunchKernelGGL(ld_compact_cls_kernel, count_grid(cx, g.n), dim3(1024), 0, cx.s, g.n, flags_in ? b.flag : (int*)nullptr, b.cls_lists,
                     b.rcounters, n_cls, (unsigned int)salt, tier_dst(cx, g, lanes), b.rcounters + CTR_AREA, (int)CTR_AREA);
  SCAMD_LAUNCH_CHECK();
  LD_FETCH(counts_host, b.rcounters, sizeof(int) * CTR_AREA, cx.s);
  LD_SYNC(cx.s);
  const size_t gs = (size_t)giant_stride(g);
  SCAMD_HIP_CHECK(hipMemcpyAsync(lists, b.cls_lists, sizeof(int) * n * n_cls, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(tier_lists, b.tier_lists, sizeof(int) * n * n_cls, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(giant_lists, b.giant_lists, sizeof(int) * gs * n_cls, hipMemcpyDeviceToDevice, cx.s));
  for (int c = 0; c < n_cls; ++c) {
    const int cnt = counts_host[c];
    SCAMD_REQUIRE(cnt >= 0 && cnt <= in, SCAMD_EINTERNAL, "leiden counters: class %d lists %d of %d vertices", c, cnt, in);
    if (cnt == 0) continue;
    const int* list = b.cls_lists + (size_t)c * n;
    hipLaunchKernelGGL(ld_gather_kernel, GRID1(cnt), 0, cx.s, cnt, decision, list, b.target);
    SCAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_apply_kernel, count_grid(cx, cnt), dim3(APPLY_THREADS), 0, cx.s, cnt, list, (const int*)b.target, g.k, b.comm,
                       b.Ktot, b.csize, b.flag, b.counters);
    SCAMD_LAUNCH_CHECK();
  }
  int ph[PH_PER_PHASE];
  LD_FETCH(ph, b.counters, sizeof(ph), cx.s);
  SCAMD_HIP_CHECK(hipMemcpyAsync(comm_after, b.comm, sizeof(int) * n, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(Ktot_after, b.Ktot, sizeof(unsigned long long) * n, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(csize_after, b.csize, sizeof(int) * n, hipMemcpyDeviceToDevice, cx.s));
  SCAMD_HIP_CHECK(hipMemcpyAsync(flags_after, b.flag, sizeof(int) * n, hipMemcpyDeviceToDevice, cx.s));
  LD_SYNC(cx.s);
  info_host[0] = ph[PH_MOVED];
  info_host[1] = ph[PH_BLOCKED];
  info_host[2] = (int64_t)gs;
  info_host[3] = lanes;
  return SCAMD_OK;
}

extern "C" void scamd_leiden_last_stats(int32_t* out, int n) {
  g_ld_stats[ST_LM_SWEEP_MB] = (int)std::min(2.0e9, g_ld_sweep_bytes / 1.0e6);
  for (int i = 0; i < n && i < LD_NSTATS; ++i) out[i] = g_ld_stats[i];
}

// the longest rows of the decide tiers at `lanes` lanes per vertex (long_row_tier), for the tests that build rows at them
extern "C" int scamd_leiden_tier_bounds(int lanes, int* main_max, int* wave_max, int* block_max) {
  SCAMD_REQUIRE(lanes == 16 || lanes == 32 || lanes == 64, SCAMD_EINVAL, "leiden tier bounds: lanes must be 16, 32 or 64");
  const int thr_mid = lanes_thr_mid(lanes);
  if (main_max) *main_max = thr_mid >= 0 ? thr_mid : (int)WH_MAX_DEG;
  if (wave_max) *wave_max = WH_MAX_DEG;
  if (block_max) *block_max = BLK_MAX_DEG;
  return SCAMD_OK;
}

// key of a statistics slot (LD_STAT_NAMES); NULL: no such slot, or the unused one
extern "C" const char* scamd_leiden_stat_name(int slot) {
  for (const LdStatName& e : LD_STAT_NAMES)
    if (e.slot == slot) return e.key;
  return nullptr;
}

extern "C" int scamd_modularity_csr_f32(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t n,
                                        int64_t nnz, const int32_t* membership, double resolution,
                                        double* modularity_host, void* workspace, size_t workspace_bytes,
                                        scamd_stream_t stream) {
  SCAMD_REQUIRE(membership && modularity_host, SCAMD_EINVAL, "modularity: null pointer");
  LeidenCtx cx;
  cx.gamma = resolution;
  cx.seed = 0;
  LevelGraph g0;
  const int rc = leiden_open(cx, "modularity", indptr, indices, weights, n, nnz, workspace, workspace_bytes, stream, &g0);
  if (rc != SCAMD_OK) return rc;
  *modularity_host = 0.0;
  if (cx.m2 <= 0.0) return SCAMD_OK;
  return evaluate(cx, g0, membership, modularity_host);  // membership ids must lie in [0, n)
}
