"""TEST INFRASTRUCTURE shared by tests/test_gpu_connectivity_shapes.py and tests/test_gpu_sparse_pca_shapes.py (the product
library on the GPU) and tests/test_emu_graph_shapes_cpu.py (the same kernels on the host emulator): the shape tables of the
connectivity stage (csrc/fuzzy.hip: umap, gauss, jaccard, the row-sharded pair) and of the sparse half of PCA (csrc/pca.hip:
SpMM, float64-accumulating SpMM, column sums, CSR -> CSC, row statistics), restatements of the rules by which the host code
picks a kernel or a kernel picks a branch, input builders, and ONE checker per operation against a float64 reference.
Nothing here touches a device; the callers are tests/emu/harness.py:Abi over host or device memory.

Not covered: the `n * k >= 2^31` branch of fss_recip_rec_kernel (64-bit division of the slot number) needs index and
distance tables of tens of GB and stays untested."""
from __future__ import annotations

import re
from functools import lru_cache
from pathlib import Path

import numpy as np
from scipy import sparse

from knn_shape_cases import oracle_self_first
from oracle import connectivities as oconn

CSRC = Path(__file__).resolve().parent.parent / "scanpy_amd" / "csrc"
EINVAL, EWORKSPACE, EUNSUPPORTED, ECAPACITY = -1, -2, -4, -5  # include/scanpy_amd.h

# ---------------------------------------------------------------------------------------------------------------------
# The dispatch rules restated.  The library offers no getter of what it launched, so the tables below are tied to these
# rules, and `assert_sources_still_say_so` ties the rules to the text of the .hip files: a retuned constant fails there
# instead of silently moving a boundary away from its cases.
# ---------------------------------------------------------------------------------------------------------------------
SR_ROWS, SR_CAP = 32, 2048        # fss_sortrows_kernel: rows per workgroup, entries its LDS block holds
SEG = 2048                        # spmm_seg_f64_kernel: stored entries per segment of a row
COLSUM_BLOCKS = 512               # colsum_stage1_kernel: blocks of the first stage (fewer when n is smaller)
TRANSPOSE_MAX_G = 40944           # 160 KB of dynamic LDS less 64 B, 4 B per column
TRANSPOSE_HIST_BYTES = 96 << 20   # transpose_plan: rows_per_chunk doubles from 256 while the histogram table is larger
TRANSPOSE_ROWS_PER_CHUNK, TRANSPOSE_CHUNKS_PER_GROUP = 256, 64
SPMM_GRID_BLOCKS, SPMM_WAVES_PER_BLOCK = 8192, 4  # a wave takes a second row when n > 32768
GAUSS_JACCARD_MAX_K = 256


def sigma_kreg(k: int) -> int:
    """launch_sigma: fss_sigma_kernel<16> keeps the row in registers, <0> re-reads it"""
    return 16 if k <= 16 else 0


def record_pairs(k: int) -> int:
    """fuzzy_record_pairs: fss_recip_rec_kernel<16 | 32>, or 0 = the row-walking fss_recip_kernel"""
    return 16 if k <= 16 else (32 if k <= 32 else 0)


FILL_BRANCHES = ("in_wave", "prev_wave", "prev_wave_back64", "serial")


@lru_cache(maxsize=None)
def fill_branches(k: int, n: int | None = None) -> frozenset:
    """fss_fill_kernel: the branches by which SOME slot (i, j >= 1) of an n x k problem counts its position in its row.
    Slot e = i k + j sits in lane e % 64 (blocks of 256 threads); `in_wave`: j <= lane; `prev_wave`: 0 < j - lane <= 64 (with
    `prev_wave_back64` for j - lane == 64, the unshifted ballot); `serial`: j - lane > 64.  n = None: a long problem."""
    n = max(64, 2 * k) if n is None else n
    e = np.arange(n * k)
    j, lane = e % k, e % 64
    live = j >= 1  # (column 0 is the row itself: weight 0, the thread returns before it counts)
    back = (j - lane)[live]
    out = set()
    if (back <= 0).any():
        out.add("in_wave")
    if ((back > 0) & (back <= 64)).any():
        out.add("prev_wave")
    if (back == 64).any():
        out.add("prev_wave_back64")
    if (back > 64).any():
        out.add("serial")
    return frozenset(out)


def spmm_kernel(l: int) -> str:
    """scamd_spmm_csr_f32: kernel by the number of columns of B"""
    assert 1 <= l <= 256
    if 4 <= l <= 64:
        return "quad"
    return f"rows<{1 if l <= 64 else (2 if l <= 128 else (3 if l <= 192 else 4))}>"


def f64acc_cpl(l: int) -> int:
    """scamd_spmm_csr_f32_f64acc: spmm_seg_f64_kernel<1 | 2>"""
    assert 1 <= l <= 128
    return 1 if l <= 64 else 2


def transpose_rows_per_chunk(n: int, g: int) -> int:
    rpc = TRANSPOSE_ROWS_PER_CHUNK
    while -(-n // rpc) * g * 4 > TRANSPOSE_HIST_BYTES:
        rpc *= 2
    return rpc


def transpose_groups(n: int, g: int) -> int:
    return -(-(-(-n // transpose_rows_per_chunk(n, g))) // TRANSPOSE_CHUNKS_PER_GROUP)


def assert_sources_still_say_so():
    """the constants and thresholds above, read out of the text of csrc/fuzzy.hip and csrc/pca.hip"""
    fz, pc = (CSRC / "fuzzy.hip").read_text(), (CSRC / "pca.hip").read_text()

    def has(text, pattern, what):
        assert re.search(pattern, text), f"{what}: /{pattern}/ no longer in the source -- restate the rule and its cases"

    has(fz, rf"constexpr int SR_ROWS = {SR_ROWS};", "SR_ROWS")
    has(fz, rf"constexpr int SR_CAP = {SR_CAP};", "SR_CAP")
    has(fz, r"total64 <= SR_CAP", "sort-rows path choice")
    has(fz, r"if \(k <= 16\)\s+hipLaunchKernelGGL\(fss_sigma_kernel<16>", "launch_sigma")
    has(fz, r"return k <= 16 \? 16 : \(k <= 32 \? 32 : 0\);", "fuzzy_record_pairs")
    has(fz, r"if \(j <= lane\) \{", "fill: first branch")
    has(fz, r"\} else if \(j - lane <= 64\) \{", "fill: second branch")
    has(fz, r"back == 64 \? m_prev : m_prev >> \(64 - back\)", "fill: unshifted ballot")
    has(fz, r"dim3\(ceil_div\(total, 256\)\), dim3\(256\), 0, s, knn_idx, b\.w, b\.recw", "fill: 256-thread blocks")
    has(fz, rf"k >= 2 && k <= {GAUSS_JACCARD_MAX_K}, SCAMD_EINVAL", "gauss / jaccard k range")
    has(pc, rf"constexpr int SEG = {SEG};", "SEG")
    has(pc, rf"constexpr int COLSUM_BLOCKS = {COLSUM_BLOCKS};", "COLSUM_BLOCKS")
    has(pc, r"std::min<int64_t>\(COLSUM_BLOCKS, n\)", "colsum grid")
    assert TRANSPOSE_MAX_G == (160 * 1024 - 64) // 4
    has(pc, r"g \* 4 <= 160 \* 1024 - 64, SCAMD_EUNSUPPORTED", "transpose LDS limit")
    assert TRANSPOSE_HIST_BYTES == 96 << 20
    has(pc, rf"int64_t rpc = {TRANSPOSE_ROWS_PER_CHUNK};\s+while \(\(n \+ rpc - 1\) / rpc \* g \* 4 > \(\(int64_t\)96 << 20\)\) rpc \*= 2;", "transpose_plan")
    has(pc, rf"p\.chunks_per_group = {TRANSPOSE_CHUNKS_PER_GROUP};", "transpose groups")
    assert SPMM_GRID_BLOCKS == 256 * 32
    has(pc, r"std::min<int64_t>\(\(n \+ 3\) / 4, 256 \* 32\)", "SpMM grid cap")
    has(pc, r"const int64_t nwaves = \(int64_t\)gridDim\.x \* 4;", "SpMM waves per block")
    has(pc, r"if \(l <= 64 && l >= 4\)\s+hipLaunchKernelGGL\(spmm_rows_quad_f32_kernel", "SpMM quad range")
    for bound, cpl in ((128, 2), (192, 3)):
        has(pc, rf"else if \(l <= {bound}\)[^\n]*\n\s+hipLaunchKernelGGL\(spmm_rows_f32_kernel<{cpl}>", f"SpMM rows<{cpl}>")
    has(pc, r"l >= 1 && l <= 256, SCAMD_EINVAL", "SpMM l range")
    has(pc, r"if \(l <= 64\)\s+hipLaunchKernelGGL\(spmm_seg_f64_kernel<1>", "f64acc dispatch")
    has(pc, r"l >= 1 && l <= 128, SCAMD_EINVAL, \"spmm_f64acc", "f64acc l range")
    has(pc, r"u \+= 4 \* GU\)", "quad unroll (16 entries)")
    has(pc, r"constexpr int GU = 8;", "rows unroll (8 entries)")


# ---------------------------------------------------------------------------------------------------------------------
# connectivity tables
# ---------------------------------------------------------------------------------------------------------------------
CONN_K = (2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 66, 67, 129, 256)
COMPLETE_GRAPH_K = (2, 16, 33, 66)  # n = k: every list holds every row
CONN_KINDS = ("gauss_dup", "lattice")
CONN_METHODS = ("umap", "gauss", "jaccard")


def conn_n(k: int) -> int:
    """odd, so that n k is no multiple of 4, 64 or 256 for odd k -- and 301 k is none of 64 for any k of the table"""
    return 301 if k <= 67 else 2 * k + 7


CONN_CASES = [(conn_n(k), k, kind) for k in CONN_K for kind in CONN_KINDS] + [(k, k, "gauss_dup") for k in COMPLETE_GRAPH_K]
SORTROWS_RING = (640, 65)  # n, k of the hand-made lists at the LDS path's cap
EXTREME_ROWS = (64, 15)
SHARD_CASES = ((601, 15, (0, 200, 200, 555, 601)), (333, 40, (0, 1, 333)), (500, 70, (0, 250, 500)))


def assert_every_connectivity_path_has_a_case():
    ks = {k for _, k, _ in CONN_CASES}
    assert {sigma_kreg(k) for k in ks} == {16, 0} and {16, 17} <= ks
    assert {record_pairs(k) for k in ks} == {16, 32, 0} and {16, 17, 32, 33} <= ks  # both sides of both thresholds, full records
    reached = set().union(*(fill_branches(k, n) for n, k, _ in CONN_CASES))
    assert reached == set(FILL_BRANCHES), set(FILL_BRANCHES) - reached
    assert "prev_wave_back64" not in fill_branches(64) and "prev_wave_back64" in fill_branches(65, conn_n(65))
    # j - lane >= 65 needs k >= 66, and at k = 66 no slot gets there: lane = (2 i + j) % 64 is 0 for no odd j = 65
    assert "serial" not in fill_branches(65) | fill_branches(66) and "serial" in fill_branches(67, conn_n(67))
    # ordinary rows beyond the sort-rows LDS block: 32 rows of >= k - 1 entries
    assert any(SR_ROWS * (k - 1) > SR_CAP for k in ks) and any(SR_ROWS * 2 * (k - 1) <= SR_CAP for k in ks)
    n, k = SORTROWS_RING
    assert SR_ROWS * (k - 1) == SR_CAP and n % SR_ROWS == 0
    # gauss median: m = k - 1 both odd and even, on data with ties
    assert {(k - 1) % 2 for _, k, kind in CONN_CASES if kind == "lattice"} == {0, 1}
    assert max(ks) == GAUSS_JACCARD_MAX_K
    shard_k = {k for _, k, _ in SHARD_CASES}
    assert {record_pairs(k) for k in shard_k} >= {16, 0} and any(b - a == 0 for _, _, c in SHARD_CASES for a, b in zip(c, c[1:]))
    assert any(b - a == 1 for _, _, c in SHARD_CASES for a, b in zip(c, c[1:]))
    return sorted(ks)


# ---------------------------------------------------------------------------------------------------------------------
# connectivity inputs: built on the host.  The kNN kernel guarantees: ids in range, none twice in a row, the row itself in
# column 0 at distance 0, distances ascending -- the float64 brute force of oracle/knn.py with the self id put in front.
# Distances are cast to float32 ONCE; the same float32 values go to the kernel and to the oracle.
# ---------------------------------------------------------------------------------------------------------------------
def conn_points(n: int, kind: str, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 6))
    if kind == "lattice":  # half-integer lattice: many equal distances (ties in the gauss median, equal weights)
        return (np.round(2 * x) / 2).astype(np.float32)
    assert kind == "gauss_dup"
    ndup = max(1, n // 20)  # 5 % of the rows are exact copies of other rows: zero distances
    rows = rng.permutation(n)[: 2 * ndup]
    x[rows[:ndup]] = x[rows[ndup:]]
    return x.astype(np.float32)


@lru_cache(maxsize=None)
def knn_lists(n: int, k: int, kind: str):
    """-> (idx int32 [n, k], dist float32 [n, k]); cached and read-only: one reference per case for every test"""
    x = conn_points(n, kind, 1000 * k + n)
    idx, dist = oracle_self_first(x, np.arange(n), k)
    idx, dist = idx.astype(np.int32), dist.astype(np.float32)
    assert (idx[:, 0] == np.arange(n)).all() and (np.diff(np.sort(idx, axis=1), axis=1) > 0).all() and (np.diff(dist, axis=1) >= 0).all()
    idx.setflags(write=False)
    dist.setflags(write=False)
    return idx, dist


def ring_lists(extra_in_edge: bool):
    """k = 65, n = 640, neighbours i +- 1..32 on a ring: every list is mutual, every row of the symmetric graph has exactly 64
    entries and every sort-rows block of 32 rows exactly SR_CAP = 2048 -- the LDS path at its cap.  extra_in_edge: row 40's
    last neighbour becomes 300; row 300 gains an in-only entry and its block, at 2049, takes the wave-per-row path."""
    n, k = SORTROWS_RING
    off = np.empty(k - 1, dtype=np.int64)
    off[0::2], off[1::2] = np.arange(1, 33), -np.arange(1, 33)
    idx = np.hstack([np.arange(n)[:, None], (np.arange(n)[:, None] + off[None, :]) % n]).astype(np.int32)
    dist = np.hstack([[0.0], 0.25 + 0.05 * np.abs(off)]).astype(np.float32)
    dist = np.broadcast_to(dist, (n, k)).copy()
    if extra_in_edge:
        idx[40, 64] = 300
    return idx, dist


def sortrows_block_totals(indptr: np.ndarray) -> np.ndarray:
    n = len(indptr) - 1
    cuts = np.append(np.arange(0, n, SR_ROWS), n)
    return np.diff(np.asarray(indptr)[cuts])


def extreme_rows():
    """one 64 x 15 problem, random distinct neighbour ids; rows 1..9 carry the distance rows at which a bisection for sigma
    can go wrong.  Every value <= 2e30: the float32 sum of all distances stays finite (beyond it the oracle's own np.mean
    overflows and stops being a reference).  Rows 6 and 9 end on the floor 1e-3 x (mean of the row), which the scalar form
    of the oracle takes in float32 and the vectorised form (as the kernel) in float64: whether the two forms agree there
    depends on the draw, and the seed is the first one from 64015 on at which they do -- chosen on the oracle alone."""
    n, k = EXTREME_ROWS
    rng = np.random.default_rng(64036)
    idx = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        others = rng.permutation(n - 1)[: k - 1]
        idx[i] = [i, *(others + (others >= i))]
    dist = np.sort(rng.random((n, k)) + 0.1, axis=1)
    f32 = np.float32
    dist[1, 1:] = 0.0                                              # rho = 0: the floor by the mean of ALL distances
    dist[2, 1:] = 0.75
    dist[3, 1:] = np.logspace(-20, 20, k - 1)
    dist[4, 1:] = np.logspace(-38, -30, k - 1)
    dist[5, 1:] = [0.0] * 7 + [1.0] * 7
    dist[6, 1:] = np.sort(1e30 * (1 + rng.random(k - 1)))          # dmax >= 1e30: phase 1 is skipped
    dist[7, 1:] = [1.0] + [float(np.nextafter(f32(1), f32(2)))] * 13
    dist[8, 1:] = 1e-45                                            # subnormal
    dist[9, 1:] = 1000 + 1e-3 * np.sort(rng.random(k - 1))
    dist[:, 0] = 0.0
    dist = dist.astype(np.float32)
    assert dist.max() <= 2e30 and np.isfinite(dist.sum(dtype=np.float32))
    return idx, dist


# ---------------------------------------------------------------------------------------------------------------------
# connectivity checkers
# ---------------------------------------------------------------------------------------------------------------------
UMAP_DATA_ATOL = 2e-6          # the project's bound (test_gpu_kernels.py:_fuzzy_vs_oracle)
GAUSS_RTOL = 2.0 ** -23        # float64 arithmetic rounded once to float32 (2^-24), doubled for the last ulps of exp
JACCARD_RTOL = 2.0 ** -22      # one rounding each of the ratio, the float32 sum and the halving: 3 x 2^-24


@lru_cache(maxsize=None)
def _oracle_cached(method, case):
    """computed once per (method, (n, k, kind)) and shared by the tests that need it"""
    return oracle_connectivity(method, *knn_lists(*case))


def oracle_connectivity(method: str, idx, dist):
    """-> (CSR with sorted rows and no stored zeros, sigma, rho); sigma / rho None but for umap"""
    n, k = idx.shape
    if method == "umap":
        ref, sigma, rho = oconn.fuzzy_simplicial_set(idx, dist, n, k)
        return ref, sigma, rho
    if method == "gauss":
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = oconn.gauss_knn(idx, dist, n)
        # sigma_i = sigma_j = 0 (two copies of a point that are each other's only neighbours, k = 2): the reference's
        # formula is 0 / 0; the kernel stores nothing there (gauss_weight_kernel: `den > 0 ? ... : 0`).  Nowhere else may a
        # NaN appear.
        d_sq = np.asarray(dist, dtype=np.float64)[:, 1:] ** 2
        sig_sq = np.median(d_sq, axis=1)
        ref = ref.tocoo()
        undefined = (sig_sq[ref.row] + sig_sq[ref.col]) == 0
        assert np.array_equal(np.isnan(ref.data), undefined)
        ref = sparse.csr_matrix((np.where(undefined, 0.0, ref.data), (ref.row, ref.col)), shape=(n, n))
    else:
        ref = oconn.jaccard_knn(idx, n, k)
    ref.eliminate_zeros()
    ref.sort_indices()
    return ref, None, None


def check_connectivity(method: str, idx, dist, out, *, ref=None, label=""):
    """out: Abi.connectivity's tuple.  Asserts the pattern, ascending columns, exact symmetry and the method's bound on the
    values (umap: rho and sigma bit-equal to the oracle's float64 bisection).  -> the worst error in the bound's unit"""
    rc, indptr, indices, data, sigma, rho = out
    assert rc == 0, (label, rc)
    n, k = idx.shape
    ref, rs, rr = oracle_connectivity(method, idx, dist) if ref is None else ref
    assert indptr[0] == 0 and indptr[-1] == len(indices) == len(data), label
    assert np.array_equal(indptr, ref.indptr), f"{label}: indptr"
    assert np.array_equal(indices, ref.indices), f"{label}: indices"
    inner = np.ones(len(indices), dtype=bool)
    inner[indptr[1:-1][indptr[1:-1] < len(indices)]] = False
    assert (np.diff(indices.astype(np.int64))[inner[1:]] > 0).all(), f"{label}: columns must ascend within a row"
    assert np.isfinite(data).all() and (data > 0).all(), label
    got = sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    assert abs(got - got.T).max() == 0, f"{label}: connectivities must be exactly symmetric"
    if method == "umap":
        assert np.array_equal(rho, rr), f"{label}: rho"
        bad = np.flatnonzero(sigma != rs)
        assert bad.size == 0, f"{label}: sigma differs from the float64 bisection in rows {bad[:8].tolist()}: {sigma[bad[:8]].tolist()} != {rs[bad[:8]].tolist()}"
        err = float(np.abs(data.astype(np.float64) - ref.data).max()) if len(data) else 0.0
        print(f"{label} umap n={n} k={k}: sigma bit-equal, worst |data - oracle| = {err:.3g} (bound {UMAP_DATA_ATOL:g})")
        assert err <= UMAP_DATA_ATOL, (label, err)
        return err
    rtol = GAUSS_RTOL if method == "gauss" else JACCARD_RTOL
    err = float((np.abs(data.astype(np.float64) - ref.data) / ref.data).max()) if len(data) else 0.0
    print(f"{label} {method} n={n} k={k}: worst relative error = {err:.3g} = {err / rtol:.3f} of the bound")
    assert err <= rtol, (label, err, rtol)
    return err


def run_connectivity_case(abi, n, k, kind, label=""):
    idx, dist = knn_lists(n, k, kind)
    return {m: check_connectivity(m, idx, dist, abi.connectivity(m, idx, dist), ref=_oracle_cached(m, (n, k, kind)),
                                  label=f"{label} {kind}") for m in CONN_METHODS}


def run_sortrows_boundary(abi, extra_in_edge: bool, label=""):
    idx, dist = ring_lists(extra_in_edge)
    n, k = idx.shape
    for m in CONN_METHODS:
        ref = oracle_connectivity(m, idx, dist)
        totals = sortrows_block_totals(ref[0].indptr)
        if not extra_in_edge or m == "jaccard":  # (rows 40 and 300 share no neighbour: jaccard stores nothing for the pair)
            assert (totals == SR_CAP).all(), (m, totals)
        else:
            assert set(totals.tolist()) == {SR_CAP, SR_CAP + 1} and totals[300 // SR_ROWS] == SR_CAP + 1, (m, totals)
            assert totals[300 // SR_ROWS - 1] == totals[300 // SR_ROWS + 1] == SR_CAP
        check_connectivity(m, idx, dist, abi.connectivity(m, idx, dist), ref=ref, label=f"{label} ring{'+1' if extra_in_edge else ''}")


def run_extreme_rows(abi, label=""):
    idx, dist = extreme_rows()
    n, k = idx.shape
    s_scalar, r_scalar = oconn.smooth_knn_dist(dist, float(k))
    s_vec, r_vec = oconn.smooth_knn_dist_vec(dist, float(k))
    assert np.array_equal(s_scalar, s_vec) and np.array_equal(r_scalar, r_vec), "the two forms of the oracle must agree first"
    out = abi.connectivity("umap", idx, dist)
    assert out[0] == 0
    assert np.array_equal(out[5], r_vec), (out[5][:10], r_vec[:10])
    assert np.array_equal(out[4], s_vec), (out[4][:10].tolist(), s_vec[:10].tolist())
    check_connectivity("umap", idx, dist, out, label=f"{label} extreme rows")


class _OneRank:  # the communicator of a single process: every reduction is the identity
    def allreduce_max_(self, t):
        return t

    def allreduce_(self, t):
        return t


def distance_sum(dist32: np.ndarray) -> float:
    """the sum of all distances by the fixed-point rule the sharded pipeline uses (scanpy_amd/_pipeline.py), on the host"""
    import torch

    from scanpy_amd._pipeline import fixed_point_distance_sum

    return float(fixed_point_distance_sum(torch.from_numpy(np.array(dist32, dtype=np.float32)), dist32.size, _OneRank()).item())


def run_sharded_case(abi, n, k, cuts, label=""):
    """scamd_fuzzy_weights_f32 + scamd_fuzzy_merge_rows_f32 shard by shard, the in-edges routed with numpy: the
    concatenated rows are BITWISE the rows of the single call"""
    idx, dist = knn_lists(n, k, "gauss_dup")
    rc, indptr, indices, data, sigma, rho = abi.connectivity("umap", idx, dist)
    assert rc == 0
    total = distance_sum(dist)
    shards = list(zip(cuts, cuts[1:]))
    ws = []
    for a, b in shards:
        rc, w, sg, rh, cnt = abi.fuzzy_weights(idx[a:b], dist[a:b], a, n, total)
        assert rc == 0, (label, a, b, rc)
        assert np.array_equal(sg, sigma[a:b]) and np.array_equal(rh, rho[a:b]), (label, a, b)
        assert np.isfinite(w).all() and np.array_equal(cnt, (w > 0).sum(axis=1))
        ws.append(w)
    w_all = np.vstack(ws)
    src, col = np.nonzero(w_all > 0)
    tgt, wv = idx[src, col].astype(np.int64), w_all[src, col]
    order = np.lexsort((src, tgt))  # by (row that receives, source)
    tgt, src, wv = tgt[order], src[order], wv[order]
    ip_parts, ix_parts, dv_parts = [], [], []
    for (a, b), w in zip(shards, ws):
        sel = (tgt >= a) & (tgt < b)
        in_indptr = np.zeros(b - a + 1, dtype=np.int64)
        in_indptr[1:] = np.cumsum(np.bincount(tgt[sel] - a, minlength=b - a))
        rc, ip, ix, dv = abi.fuzzy_merge_rows(idx[a:b], w, in_indptr, src[sel].astype(np.int32), wv[sel])
        assert rc == 0 and ip[0] == 0 and len(ip) == b - a + 1, (label, a, b, rc)
        ip_parts.append(np.diff(ip))
        ix_parts.append(ix)
        dv_parts.append(dv)
    got_indptr = np.concatenate([[0], np.cumsum(np.concatenate(ip_parts))])
    assert np.array_equal(got_indptr, indptr), label
    assert np.array_equal(np.concatenate(ix_parts), indices), label
    assert np.array_equal(np.concatenate(dv_parts).view(np.int32), data.view(np.int32)), f"{label}: sharded rows are not bitwise the single call's"


def run_connectivity_argument_checks(abi, launches=None):
    """every one of these returns before any launch (`launches`: a counter of kernel launches, where there is one)"""
    n = 64  # (8 n bytes of gauss sigma^2 are a multiple of the workspace's 256-byte granule: the documented size is tight)
    before = launches() if launches else 0
    for k in (1, GAUSS_JACCARD_MAX_K + 1):
        idx = np.zeros((n, k), dtype=np.int32)
        idx[:, 0] = np.arange(n)
        for m in ("gauss", "jaccard"):
            assert abi.connectivity(m, idx, np.zeros((n, k), np.float32), cap=2 * n * max(k - 1, 1))[0] == EINVAL, (m, k)
    idx, dist = knn_lists(n, 5, "lattice")
    # scamd_fuzzy_workspace_bytes is one size for the three entry points: gauss and jaccard carve all of it; umap stops before
    # the n doubles of the gauss sigma^2, at its 4 doubles of sums (fuzzy_carve), so ITS last byte lies that much earlier
    umap_slack = 8 * n + (256 - 4 * 8)
    for m in CONN_METHODS:
        assert abi.connectivity(m, idx, dist, cap=2 * n * 4 - 1)[0] == ECAPACITY, m
        assert abi.connectivity(m, idx, dist, ws_short=1 + (umap_slack if m == "umap" else 0))[0] == EWORKSPACE, m
    if launches:
        assert launches() == before, "an argument check let a kernel start"
    for m in CONN_METHODS:  # (and the same arguments with the workspace to its last byte are accepted)
        assert abi.connectivity(m, idx, dist, ws_short=umap_slack if m == "umap" else 0)[0] == 0, m


# ---------------------------------------------------------------------------------------------------------------------
# sparse-PCA tables
# ---------------------------------------------------------------------------------------------------------------------
SPMM_L = (1, 3, 4, 5, 7, 61, 63, 64, 65, 128, 129, 192, 193, 256)
SPMM_ROW_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 200, 3)
SPMM_G = 300
SPMM_SECOND_TRIP_L = (1, 5, 65, 129, 193)  # one l per kernel: + 32768 + 7 short rows, waves take a second grid-stride trip
SPMM_SECOND_TRIP_ROWS = SPMM_GRID_BLOCKS * SPMM_WAVES_PER_BLOCK + 7
F64ACC_L = (1, 64, 65, 128)
F64ACC_ROW_LENGTHS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097)
F64ACC_G = 6000
COLSUM_N = (1, 2, 511, 512, 513, 1025)
COLSUM_L = (1, 127, 128)
ROW_STATS_LENGTHS = (0, 1, 63, 64, 65, 1000, 0)  # 7 rows: not a multiple of the 4 rows of a block
# (n, g, stored entries per row on average)
TRANSPOSE_CASES = ((300, TRANSPOSE_MAX_G, 6.0), (16384, 1000, 3.0), (16385, 1000, 3.0), (170000, TRANSPOSE_MAX_G, 1.0))


def assert_every_sparse_pca_path_has_a_case():
    kernels = {spmm_kernel(l) for l in range(1, 257)}
    assert kernels == {"rows<1>", "quad", "rows<2>", "rows<3>", "rows<4>"}
    assert {spmm_kernel(l) for l in SPMM_L} == kernels == {spmm_kernel(l) for l in SPMM_SECOND_TRIP_L}
    for l in (1, 3, 4, 64, 65, 128, 129, 192, 193, 256):  # both sides of every threshold
        assert l in SPMM_L
    assert {4, 5, 61, 63} <= set(SPMM_L)  # the quad kernel's shifted last quad: l = 4 (one quad), l % 4 = 1, 1, 3
    lens = set(SPMM_ROW_LENGTHS)
    assert {0, 63, 64, 65} <= lens and {7, 8, 9} <= lens and {15, 16, 17} <= lens and max(lens) > 3 * 64
    assert len(SPMM_ROW_LENGTHS) + SPMM_SECOND_TRIP_ROWS > SPMM_GRID_BLOCKS * SPMM_WAVES_PER_BLOCK >= len(SPMM_ROW_LENGTHS)
    assert {f64acc_cpl(l) for l in F64ACC_L} == {1, 2} and {64, 65} <= set(F64ACC_L)
    assert {0, SEG - 1, SEG, SEG + 1, 2 * SEG, 2 * SEG + 1} <= set(F64ACC_ROW_LENGTHS)
    assert {COLSUM_BLOCKS - 1, COLSUM_BLOCKS, COLSUM_BLOCKS + 1, 1} <= set(COLSUM_N) and max(COLSUM_N) > 2 * COLSUM_BLOCKS
    assert {1, 128} <= set(COLSUM_L)
    assert len(ROW_STATS_LENGTHS) % 4 and {0, 1, 63, 64, 65} <= set(ROW_STATS_LENGTHS)
    tr = {(transpose_rows_per_chunk(n, g), transpose_groups(n, g)) for n, g, _ in TRANSPOSE_CASES}
    assert {256, 512} == {r for r, _ in tr}
    assert transpose_groups(16384, 1000) == 1 and transpose_groups(16385, 1000) == 2
    assert any(g == TRANSPOSE_MAX_G and g * 4 > 64 * 1024 for _, g, _ in TRANSPOSE_CASES)
    return sorted(kernels)


# ---------------------------------------------------------------------------------------------------------------------
# sparse-PCA inputs: explicit row lengths, unique ascending columns, standard-normal values
# ---------------------------------------------------------------------------------------------------------------------
def csr_with_row_lengths(lengths, g: int, seed: int, short_rows: int = 0) -> sparse.csr_matrix:
    """rows of exactly `lengths` stored entries, then `short_rows` rows of 0..3 entries"""
    rng = np.random.default_rng(seed)
    cols = [np.sort(rng.choice(g, size=ln, replace=False)) for ln in lengths]
    counts = list(lengths)
    if short_rows:
        ln = rng.integers(0, 4, short_rows)
        third = g // 3
        c = rng.integers(0, third, (short_rows, 3)) + third * np.arange(3)[None, :]  # one per third of the columns: ascending
        keep = np.arange(3)[None, :] < ln[:, None]
        cols.append(c[keep])
        counts += ln.tolist()
    indices = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    data = rng.standard_normal(len(indices)).astype(np.float32)
    m = sparse.csr_matrix((data, indices, indptr), shape=(len(counts), g))
    assert m.has_sorted_indices and (np.diff(m.indptr) == np.asarray(counts)).all()
    return m


def random_csr(n: int, g: int, per_row: float, seed: int) -> sparse.csr_matrix:
    """about per_row entries per row at random places, duplicates merged away: empty rows and empty columns occur"""
    rng = np.random.default_rng(seed)
    nnz = int(n * per_row)
    key = np.unique(rng.integers(0, n, nnz).astype(np.int64) * g + rng.integers(0, g, nnz))
    rows, cols = key // g, key % g
    if n > 8 and g > 8:  # make sure of both
        keep = (rows != n // 2) & (rows != n - 1) & (cols != 0) & (cols != g - 1) & (cols != g // 3)
        rows, cols = rows[keep], cols[keep]
    data = rng.standard_normal(len(rows)).astype(np.float32)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return sparse.csr_matrix((data, cols.astype(np.int32), indptr), shape=(n, g))


# ---------------------------------------------------------------------------------------------------------------------
# sparse-PCA checkers.  The bounds are derived, not tuned: an fma chain of `len` terms is within len * u * sum|a||b| of the
# exact sum (u = unit roundoff of the accumulator), the final subtraction adds one rounding of the result, the "+ 2" covers
# it and the tree that joins partial chains.
# ---------------------------------------------------------------------------------------------------------------------
def spmm_bound(x: sparse.csr_matrix, b: np.ndarray, shift, u: float):
    lens = np.diff(x.indptr).astype(np.float64)[:, None]
    mag = abs(x).astype(np.float64) @ np.abs(b.astype(np.float64))
    if shift is not None:
        mag = mag + np.abs(np.asarray(shift, dtype=np.float64))[None, :]
    return (lens + 2) * u * mag


def check_spmm(x, b, shift, out, label=""):
    rc, y = out
    assert rc == 0, (label, rc)
    assert y.shape == (x.shape[0], b.shape[1]) and np.isfinite(y).all(), f"{label}: an element was not written (NaN prefill) or is not finite"
    ref = x.astype(np.float64) @ b.astype(np.float64)
    if shift is not None:
        ref = ref - shift.astype(np.float64)[None, :]
    bound = spmm_bound(x, b, shift, 2.0 ** -24)
    err = np.abs(y.astype(np.float64) - ref)
    over = err > bound
    assert not over.any(), f"{label}: {int(over.sum())} elements beyond the bound, first at {np.argwhere(over)[:4].tolist()}"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def run_spmm_case(abi, l: int, second_trip: bool, label=""):
    x = csr_with_row_lengths(SPMM_ROW_LENGTHS, SPMM_G, 7000 + l, SPMM_SECOND_TRIP_ROWS if second_trip else 0)
    rng = np.random.default_rng(l)
    b = rng.standard_normal((SPMM_G, l)).astype(np.float32)
    shift = rng.standard_normal(l).astype(np.float32)
    worst = 0.0
    for sh in (shift, None):
        out = abi.spmm(x, b, sh)
        worst = max(worst, check_spmm(x, b, sh, out, label=f"{label} l={l} shift={'yes' if sh is not None else 'NULL'}"))
        again = abi.spmm(x, b, sh)
        assert np.array_equal(out[1].view(np.int32), again[1].view(np.int32)), f"{label} l={l}: two calls differ"
    print(f"{label} spmm l={l} {spmm_kernel(l)} n={x.shape[0]}: worst error / bound = {worst:.3f}")
    return worst


def run_spmm_argument_checks(abi, launches=None):
    before = launches() if launches else 0
    x = csr_with_row_lengths((1, 2, 3), 8, 1)
    assert abi.spmm(x, np.zeros((8, 1), np.float32), l=0)[0] == EINVAL
    assert abi.spmm(x, np.zeros((8, 257), np.float32))[0] == EINVAL
    assert abi.spmm_f64acc(x, np.zeros((8, 129), np.float32))[0] == EINVAL
    wide = sparse.csr_matrix((np.ones(2, np.float32), np.array([0, TRANSPOSE_MAX_G], np.int32), np.array([0, 1, 2], np.int64)),
                             shape=(2, TRANSPOSE_MAX_G + 1))
    assert abi.csr_transpose(wide)[0] == EUNSUPPORTED
    if launches:
        assert launches() == before, "an argument check let a kernel start"


def run_f64acc_case(abi, l: int, label=""):
    x = csr_with_row_lengths(F64ACC_ROW_LENGTHS, F64ACC_G, 9000 + l)
    rng = np.random.default_rng(100 + l)
    b = rng.standard_normal((F64ACC_G, l)).astype(np.float32)
    scale, colsum = rng.standard_normal(x.shape[0]), rng.standard_normal(l) * 10
    u = 2.0 ** -53
    worst = 0.0
    for sc, cs in ((scale, colsum), (None, None)):
        rc, w = abi.spmm_f64acc(x, b, sc, cs)
        tag = f"{label} f64acc l={l} scale={'yes' if sc is not None else 'NULL'}"
        assert rc == 0 and np.isfinite(w).all(), f"{tag}: an element was not written"
        # the float64 reference carries its own rounding of the same size: compare with a float128 sum of exact products
        ref = np.zeros(w.shape, dtype=np.longdouble)
        for r in range(x.shape[0]):
            s, e = x.indptr[r], x.indptr[r + 1]
            ref[r] = (x.data[s:e].astype(np.longdouble)[:, None] * b[x.indices[s:e]].astype(np.longdouble)).sum(axis=0)
        bound = spmm_bound(x, b, None, u)
        if sc is not None:
            ref = ref - np.outer(sc.astype(np.longdouble), cs.astype(np.longdouble))
            bound = bound + 2.0 ** -52 * np.abs(np.outer(sc, cs))
        err = np.abs(w.astype(np.longdouble) - ref).astype(np.float64)
        assert not (err > bound).any(), f"{tag}: beyond the bound at {np.argwhere(err > bound)[:4].tolist()}"
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        rc2, w2 = abi.spmm_f64acc(x, b, sc, cs)
        assert rc2 == 0 and np.array_equal(w.view(np.int64), w2.view(np.int64)), f"{tag}: two calls differ"
    print(f"{label} f64acc l={l} <{f64acc_cpl(l)}>: worst error / bound = {worst:.3f}")
    return worst


def run_colsum_case(abi, n: int, l: int, label=""):
    y = np.random.default_rng(n * 131 + l).standard_normal((n, l)).astype(np.float32)
    rc, s = abi.colsum(y)
    assert rc == 0 and np.isfinite(s).all()
    ref = y.astype(np.longdouble).sum(axis=0)
    bound = (n + 2) * 2.0 ** -53 * np.abs(y.astype(np.float64)).sum(axis=0)
    err = np.abs(s.astype(np.longdouble) - ref).astype(np.float64)
    assert not (err > bound).any(), (label, n, l, err.max())
    rc2, s2 = abi.colsum(y)
    assert np.array_equal(s.view(np.int64), s2.view(np.int64))
    return float((err / bound).max())


def run_row_stats_case(abi, label=""):
    x = csr_with_row_lengths(ROW_STATS_LENGTHS, 1200, 4242)
    rc, s, q = abi.csr_row_stats(x)
    assert rc == 0 and np.isfinite(s).all() and np.isfinite(q).all(), "a row was not written"
    lens = np.diff(x.indptr)
    for r in range(x.shape[0]):
        v = x.data[x.indptr[r]: x.indptr[r + 1]].astype(np.longdouble)
        u = (lens[r] + 2) * 2.0 ** -53
        assert abs(s[r] - v.sum()) <= u * float(np.abs(v).sum()), (label, r)
        assert abs(q[r] - (v * v).sum()) <= u * float((v * v).sum()), (label, r)
    assert s[0] == 0 and q[0] == 0


def run_transpose_case(abi, n: int, g: int, per_row: float, label=""):
    x = random_csr(n, g, per_row, n + g)
    lens, col_lens = np.diff(x.indptr), np.bincount(x.indices, minlength=g)
    assert (lens == 0).any() and (col_lens == 0).any(), "the case is meant to hold empty rows and empty columns"
    rc, t_ip, t_ix, t_dv = abi.csr_transpose(x)
    assert rc == 0, (label, rc)
    ref = x.tocsc()
    ref.sort_indices()
    assert np.array_equal(t_ip, ref.indptr), f"{label}: indptr"
    assert np.array_equal(t_ix, ref.indices), f"{label}: indices"
    assert np.array_equal(t_dv.view(np.int32), ref.data.view(np.int32)), f"{label}: data"


def score_check(x: sparse.spmatrix, comps: np.ndarray, scores: np.ndarray, label=""):
    """every column of the device's scores against (X - mean) comps^T in float64 from the device's OWN components: what
    scamd_spmm_csr_f32 with `shift` computed, under the per-element SpMM bound.  -> worst error / bound"""
    x = x.tocsr().astype(np.float64)
    comps = np.asarray(comps, dtype=np.float64)
    mean = np.asarray(x.mean(axis=0)).ravel()
    shift = comps @ mean
    ref = x @ comps.T - shift[None, :]
    bound = spmm_bound(x, comps.T, shift, 2.0 ** -24)
    err = np.abs(np.asarray(scores, dtype=np.float64) - ref)
    over = err > bound
    ratio = float((err / bound).max())
    print(f"{label} scores, all {comps.shape[0]} columns: worst error / bound = {ratio:.3f}")
    assert not over.any(), f"{label}: score columns {np.unique(np.argwhere(over)[:, 1])[:10].tolist()} beyond the SpMM bound"
    return ratio


class DeviceMem:
    """tests/emu/harness.py:Abi over torch tensors on the GPU (the product library)"""

    def __init__(self):
        import torch

        from scanpy_amd._device import stream_ptr

        assert torch.cuda.is_available(), "GPU tests need a GPU"
        self.torch, self._stream = torch, stream_ptr

    @property
    def stream(self):
        return self._stream()

    def put(self, a, dtype):
        return self.torch.from_numpy(np.array(a, dtype=dtype, order="C", copy=True)).cuda()

    def full(self, shape, dtype, fill):
        return self.torch.from_numpy(np.full(shape, fill, dtype=dtype)).cuda()

    def ptr(self, a):
        import ctypes

        return ctypes.c_void_p(a.data_ptr() if a is not None and a.numel() else 0)

    def get(self, a):
        return a.cpu().numpy()

    def sync(self):
        self.torch.cuda.synchronize()
