"""TEST INFRASTRUCTURE shared by tests/test_gpu_knn_cells.py (the product library on the GPU) and
tests/test_emu_knn_cells_cpu.py (the same kernels on the host emulator): the cell tables behind the pruned exact search and the
approximate mode `scamd_knn_l2_ivf_f32` (csrc/knn.hip), handed out by the test entry `scamd_knn_debug_cell_tables`, against
numpy float64 on the float32 inputs; and the approximate lists against the rows those tables say a query was allowed to see.
Nothing here touches a device: `abi` is tests/emu/harness.py:Abi over HostMem or over graph_kernel_cases.DeviceMem."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import knn_shape_cases as S
from oracle import compare as ocmp

U = 2.0 ** -24      # unit roundoff of float32, round to nearest
U_BF16 = 2.0 ** -9  # ... of bf16 (8 significand bits), round to nearest even (bf16_rn)
MIN_CELL = 128      # ivf_cell_layout: a cell with fewer rows is folded into its nearest cell that keeps its own
META_CELLS = {"emulator": 4, "gpu": 64}  # IVF_META_CELLS: entries of the sweep's cell table in LDS, refilled every so many cells
EINVAL, EWORKSPACE = -1, -2
ENTRY_LAUNCHES = 2  # kernels the debug entry starts itself: the read-back of the image's end, the gather of row_cell


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    n: int
    d: int
    k: int
    env: dict = field(default_factory=dict)
    pad: int = 0          # ld = d + pad, the padding holds NaN
    data: str = "overlap"  # overlap | fold | offset

    @property
    def H(self):
        return S.plan(self.d, self.k)[0]

    @property
    def mfma_assign(self):
        """IvfSelect::train_quantiser: the bf16 assignment for H = 25 unless SCAMD_KNN_ASSIGN_MFMA=0"""
        return self.H == 25 and self.env.get("SCAMD_KNN_ASSIGN_MFMA") != "0"


CELL_ROWS = 256  # SCAMD_KNN_CELL_ROWS: n = 4096 -> 16 cells (the plan needs n >= 4096 and at most n / 256 cells)
_F32 = {"SCAMD_KNN_B3": "0", "SCAMD_KNN_ASSIGN_MFMA": "0"}
GEOMETRY_CASES = (
    Case("d10", 4096, 10, 15), Case("d20", 4096, 20, 15), Case("d50", 4096, 50, 15), Case("d50-f32", 4096, 50, 15, _F32),
    Case("d64", 4096, 64, 15), Case("d50-k2", 4096, 50, 2), Case("d50-k24", 4096, 50, 24), Case("d20-ld27", 4096, 20, 15, pad=7),
)
FOLD_CASE = Case("fold", 4096, 20, 15, data="fold")
OFFSET_CASE = Case("offset", 4096, 20, 15, data="offset")
SHARD_CASE, SHARD, SHARD_NPROBE = Case("shard", 4096, 20, 15), (1000, 1500), 3
EXACT_ANSWER_SHAPE = (4095, 65, 25, 2)  # n, d, k, nprobe: the approximate entry answers it exactly, the plan has no cells
BY_NAME = {c.name: c for c in (*GEOMETRY_CASES, FOLD_CASE, OFFSET_CASE, SHARD_CASE)}

# nprobe values at 16 cells; 4 | 5 and 8 | 9 straddle the refill of the emulator's 4-entry cell table, 1000 = every cell
NPROBE_16 = (1, 3, 4, 5, 8, 9, 15, 16, 1000)
# the GPU's table holds 64 entries: 128 cells, 64 | 65 straddle its refill
BIG_CASES = (Case("big-d20", 32768, 20, 15), Case("big-d50", 32768, 50, 15))
NPROBE_128 = (64, 65, 70, 128)
BIG_SAMPLE = 2048

# the emulator executes lane by lane: it runs every nprobe on one float32-engine and one bf16-engine geometry and both sides of
# the first refill on the others; the GPU suite runs the whole product
EMU_NPROBE = {"d20": NPROBE_16, "d50": NPROBE_16}
EMU_NPROBE_OTHER = (3, 5)


def min_share(case: Case, nprobe):
    """precondition of the promise check: the share of the queries whose nearest neighbours among the probed rows must differ from
    their exact ones, or the check could not tell the two lists apart.  Asked for where it is the point: one probed cell of 16
    on the overlapping clusters, and a list long enough to reach across a cell boundary (with k = 2 a list is one neighbour,
    which a query mostly finds in its own cell).  The more cells are probed and the higher d, the smaller the share."""
    return 0.1 if nprobe == 1 and case.k >= 15 else None


def emu_nprobe(case: Case):
    return EMU_NPROBE.get(case.name, EMU_NPROBE_OTHER)


def assert_every_cell_path_has_a_case():
    """every H of the register-list kernel and both assignment kernels have a geometry case; the folding / empty-cell, offset
    and shard cases exist; both sides of the cell-table refill are in the nprobe lists of both suites"""
    assert {c.H for c in GEOMETRY_CASES} == {8, 16, 25, 32}
    assert all(S.plan(c.d, c.k)[4] for c in (*GEOMETRY_CASES, *BIG_CASES, FOLD_CASE, OFFSET_CASE, SHARD_CASE))
    assert {c.mfma_assign for c in GEOMETRY_CASES} == {True, False}
    assert {c.mfma_assign for c in GEOMETRY_CASES if c.H == 25} == {True, False}  # (d = 50 both ways)
    assert {S.expected_engine(c.d, c.k, c.env.get("SCAMD_KNN_B3")) for c in GEOMETRY_CASES} == {0, 1}
    assert any(c.pad for c in GEOMETRY_CASES) and {c.k for c in GEOMETRY_CASES} >= {2, 15, 24}
    assert FOLD_CASE.data == "fold" and OFFSET_CASE.data == "offset" and SHARD[1] % 128 != 0 and SHARD[0] % 128 != 0
    emu, gpu = META_CELLS["emulator"], META_CELLS["gpu"]
    for c in GEOMETRY_CASES:  # the emulator suite: both sides of a refill on every geometry
        probes = emu_nprobe(c)
        assert any(p <= emu for p in probes) and any(emu < p <= 16 for p in probes), (c.name, probes)
    assert {emu, emu + 1, 2 * emu, 2 * emu + 1} <= set(NPROBE_16) and 1 in NPROBE_16 and max(NPROBE_16) > 16
    assert {gpu, gpu + 1} <= set(NPROBE_128) and max(NPROBE_128) >= 128  # the GPU suite: NPROBE_128 on BIG_CASES
    n, d, k, _ = EXACT_ANSWER_SHAPE
    assert n < 4096 and not S.plan(d, k)[4]
    return sorted({c.H for c in GEOMETRY_CASES})


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def overlapping(n, d, seed, n_centres=12):
    """Gaussian clusters whose centres are as far apart as the clusters are wide (tests/test_emu_cpu.py:
    test_knn_approximate_mode): the quantiser's cells cut through them, so a query's true neighbours lie in several cells"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((n_centres, d))
    return (cent[rng.integers(0, n_centres, n)] + rng.standard_normal((n, d))).astype(np.float32)


def folding(n, d, seed):
    """the quantiser starts cell c at row c * (n / nc) + (n / nc) / 2 (ivf_init_kernel; nc = 16: rows 128, 384, 640, ...) and
    runs three Lloyd iterations on every fourth row.
    Rows 100 .. 419 are ONE point far from everything, its coordinates exact in the 2^-20 fixed point of the centroid sums:
    cells 0 and 1 start on it and stay on it, the first of equal scores wins, so cell 0 takes all 320 rows and cell 1 never
    receives one -- empty.  Rows 620 .. 659 are a tight cluster far on the other side: cell 2 starts inside it and keeps
    these 40 rows only -- under 128, folded into its nearest kept cell, whose radius then reaches out to them."""
    x = overlapping(n, d, seed)
    x[100:420] = -40.0
    rng = np.random.default_rng(seed + 1)
    x[620:660] = (40.0 + 0.1 * rng.standard_normal((40, d))).astype(np.float32)
    return x


def make_data(case: Case, exact: bool):
    """-> (x [n, d + pad] float32 with NaN in the padding, the data x[:, :d]).  The approximate search gets overlapping
    clusters (its lists must differ from the exact ones for the promise to be told from exactness), the exact search the
    clusters of knn_shape_cases.clustered at spread 3: a cluster fills a few cells, cells of different clusters lie apart, so
    that cell_lb2 has positive entries whose soundness can fail."""
    seed = 1000 * case.d + case.k
    base = S.clustered(case.n, case.d, seed, 3.0) if exact else overlapping(case.n, case.d, seed)
    if case.data == "fold":
        x = folding(case.n, case.d, seed)
    elif case.data == "offset":  # coordinates around 1000, unit spread: cancellation in v - cent and in the centroid distances
        x = (base.astype(np.float64) + 1000.0).astype(np.float32)
    else:
        x = base
    buf = np.full((case.n, case.d + case.pad), np.nan, dtype=np.float32)
    buf[:, : case.d] = x
    return buf, x


def case_env(case: Case, nprobe: int) -> dict:
    """the SCAMD_KNN_* environment of a call: the exact search (nprobe = 0) must be told to prune at this size"""
    env = {"SCAMD_KNN_CELL_ROWS": str(CELL_ROWS), **case.env}
    if nprobe == 0:
        env["SCAMD_KNN_IVF"] = "1"
    return env


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------
def _d2(a, b):
    """[len(a), len(b)] squared distances as |a|^2 + |b|^2 - 2 a.b in float64: to SELECT candidates, never to assert"""
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)


def min_pair_d2(xa, xb):
    """smallest squared distance between a row of xa and a row of xb (float64 arrays): the Gram form picks every pair within
    its own rounding error of the smallest, the direct sum of squared differences of those decides"""
    g = _d2(xa, xb)
    scale = max(float((xa * xa).sum(1).max()), float((xb * xb).sum(1).max()))
    i, j = np.nonzero(g <= g.min() + 1e-9 * scale)
    return float(((xa[i] - xb[j]) ** 2).sum(1).min())


def lists_among(x64, rows, allowed, k):
    """the k-1 nearest OTHER rows of every query in `rows` among the rows `allowed` (sorted row numbers, the queries among
    them) by (float64 distance, index), the query itself in front -- the library's convention"""
    pos = np.searchsorted(allowed, rows)
    assert np.array_equal(allowed[pos], rows)
    ei, ed = S.oracle_self_first(x64[allowed], pos, k)
    return allowed[ei], ed


# ---------------------------------------------------------------------------------------------------------------------
# table checks
# ---------------------------------------------------------------------------------------------------------------------
def check_layout(x, T, label=""):
    """perm, tile ranges, folding.  -> (members of every merged cell, kept mask, empty quantiser cells)"""
    n, nc = x.shape[0], T["nc"]
    labels, row_cell, cell_map, tile0, ntiles, perm = (T[key] for key in ("labels", "row_cell", "cell_map", "tile0", "ntiles", "perm"))
    assert labels.min() >= 0 and labels.max() < nc, f"{label}: a row's cell is outside [0, nc)"
    assert np.array_equal(row_cell, cell_map[labels]), f"{label}: row_cell is not cell_map[labels]"
    assert np.array_equal(cell_map[cell_map], cell_map), f"{label}: cell_map folds into a folded cell"
    got = np.bincount(labels, minlength=nc)          # rows the quantiser gave every cell
    merged = np.bincount(row_cell, minlength=nc)     # rows after folding
    kept = cell_map == np.arange(nc)
    assert kept.any()
    assert (got[kept] >= MIN_CELL).all(), f"{label}: a cell under {MIN_CELL} rows was left as its own: {got[kept].min()}"
    assert (got[~kept] < MIN_CELL).all(), f"{label}: a cell of {MIN_CELL} rows or more was folded"
    assert (ntiles[~kept] == 0).all() and (merged[~kept] == 0).all(), f"{label}: a folded or empty cell owns tiles or rows"
    assert np.array_equal(ntiles, (merged + 63) // 64), f"{label}: ntiles != ceil(members / 64)"
    assert np.array_equal(tile0, np.concatenate([[0], np.cumsum(ntiles)[:-1]])), f"{label}: tile ranges are not disjoint and in cell order"
    assert len(perm) == 64 * int(ntiles.sum()), f"{label}: the image has {len(perm)} rows for {int(ntiles.sum())} tiles"
    members = []
    for c in range(nc):
        seg = perm[64 * tile0[c]: 64 * (tile0[c] + ntiles[c])]
        rows = np.sort(seg[seg >= 0])
        assert (seg[seg < 0] == -1).all() and len(rows) == merged[c], f"{label}: cell {c}: padding is not -1 or rows are missing"
        assert np.array_equal(rows, np.flatnonzero(row_cell == c)), f"{label}: cell {c}: the image rows are not the cell's members once each"
        members.append(rows)
    # a folded cell goes to the nearest kept centroid (float64 on the float32 centroids, the host's own arithmetic)
    cent = T["cent"].astype(np.float64)
    for c in np.flatnonzero(~kept):
        dd = ((cent[c] - cent[kept]) ** 2).sum(1)
        chosen = ((cent[c] - cent[cell_map[c]]) ** 2).sum()
        assert kept[cell_map[c]] and chosen <= dd.min(), f"{label}: cell {c} was folded into {cell_map[c]}, not into its nearest kept cell"
    return members, kept, np.flatnonzero(got == 0)


def radius_slack(d):
    """e_d of the radius: ivf_pack_image_kernel computes r = fl(fl(sqrt(s) * 1.0001f) + 1e-6f), s = the float32 sum of the d
    squares df^2, df = fl(v - c).  df carries one rounding (relative u, so 2u on its square; the fma does not round the square);
    summing d non-negative terms in ANY order (lanes, then a shuffle tree) rounds each term at most d - 1 times on its way into
    the sum: s_fl = s (1 + t), |t| <= (d + 1) u to first order.  The square root halves that and rounds once: (d + 1) / 2 + 1.
    Then the two constants as float32 (u each) and the product and the sum (u each): + 4.  e_d = ((d + 1) / 2 + 5) u, and 1 %
    on top for the second-order terms."""
    return ((d + 1) / 2.0 + 5.0) * U * 1.01


def check_radii(x, T, members, kept, label=""):
    """-> worst radius / true radius over the kept cells"""
    d = x.shape[1]
    x64, cent, radius = x.astype(np.float64), T["cent"].astype(np.float64), T["radius"].astype(np.float64)
    e_d = radius_slack(d)
    worst = 0.0
    for c in range(T["nc"]):
        if not kept[c]:
            assert radius[c] == 0.0, f"{label}: cell {c} has no rows and radius {radius[c]}"
            continue
        true_r = float(np.sqrt(((x64[members[c]] - cent[c]) ** 2).sum(1).max()))
        # soundness, no tolerance: the pruning and the float64 scan skip what lies beyond the ball
        assert radius[c] >= true_r, f"{label}: cell {c}: radius {radius[c]!r} < {true_r!r}, its farthest member (folded-in rows included)"
        # tightness: an infinite or merely generous radius passes everything else and ends the pruning
        assert radius[c] <= (true_r * 1.0001 + 1e-6) * (1.0 + e_d), f"{label}: cell {c}: radius {radius[c]!r} for a farthest member at {true_r!r}"
        if true_r > 0:
            worst = max(worst, radius[c] / true_r)
    return worst


def order_tables(T):
    """-> lb2_of [nc, nc]: the cell_lb2 entry of cell b in row a (rows are stored in sweep order)"""
    nc = T["nc"]
    lb2_of = np.empty((nc, nc), dtype=np.float64)
    np.put_along_axis(lb2_of, T["order"].astype(np.int64), T["lb2"].astype(np.float64), axis=1)
    return lb2_of


def check_order_rows(x, T, kept, nprobe, label=""):
    nc, d = T["nc"], x.shape[1]
    order, lb2 = T["order"], T["lb2"]
    cent = T["cent"].astype(np.float64)
    n_kept = int(kept.sum())
    for a in np.flatnonzero(kept):
        o, v = order[a], lb2[a]
        assert np.array_equal(np.sort(o), np.arange(nc)), f"{label}: order row {a} is no permutation of the cells"
        assert o[0] == a and v[0] == -1.0, f"{label}: order row {a} does not start with its own cell at -1"
        assert kept[o[:n_kept]].all() and not kept[o[n_kept:]].any(), f"{label}: order row {a}: the cells without tiles are not last"
        assert np.isposinf(v[n_kept:]).all(), f"{label}: order row {a}: a cell without tiles has a finite bound"
        assert (np.diff(o[n_kept:]) > 0).all(), f"{label}: order row {a}: equal (infinite) values are not in cell order"
        if nprobe == 0:
            assert np.isfinite(v[:n_kept]).all() and (v[1:n_kept] >= 0).all()
            assert (np.diff(v[:n_kept]) >= 0).all(), f"{label}: order row {a}: the bounds descend somewhere"
            tie = np.diff(v[:n_kept]) == 0
            assert (np.diff(o[:n_kept])[tie] > 0).all(), f"{label}: order row {a}: equal bounds are not in cell order"
        else:
            want = np.where(np.arange(nc) < min(nprobe, n_kept), 0.0, np.inf)
            want[0] = -1.0
            assert np.array_equal(v, want.astype(np.float32)), f"{label}: order row {a}: probed cells {v.tolist()}, nprobe {nprobe}, {n_kept} cells with rows"
            # by centroid distance: float32 d2 = sum of d squares of fl(ca - cb), relative error (d + 1) u as in radius_slack
            d2 = ((cent[a] - cent[o[:n_kept]]) ** 2).sum(1)
            tol = (d + 1) * U * 1.01 * (d2[1:-1] + d2[2:])
            assert (d2[2:] - d2[1:-1] >= -tol).all(), f"{label}: order row {a}: the cells are not in the order of their centroid distances"


def lb2_error(dist, lb64, d):
    """float32 error of ivf_cell_order_kernel's max(0, sqrt(d2) * (1 - 1e-4f) - ra - rb)^2 against the same formula in float64
    on the float32 centroids and radii.  D = the centroid distance.  sqrt(d2): (d + 1) / 2 + 1 roundings as in radius_slack; the
    constant and the product: 2 more: t = D (1 - 1e-4) (1 + e), |e| <= e_t = ((d + 1) / 2 + 3) u.  Two subtractions, each result
    at most D in magnitude: 2 u D.  max(0, .) is 1-Lipschitz.  So |lb - lb64| <= E = (e_t + 2 u) D, and the square, rounded
    once: |lb^2 - lb64^2| <= E (2 lb64 + E) + u (lb64 + E)^2.  1 % on top for second-order terms."""
    e = (((d + 1) / 2.0 + 3.0) * U + 2.0 * U) * dist
    return 1.01 * (e * (2.0 * lb64 + e) + U * (lb64 + e) ** 2)


def check_bounds(x, T, members, kept, label=""):
    """exact mode.  -> (worst lb2 / true minimum squared distance over the pairs with a positive bound, such pairs, pairs)"""
    d = x.shape[1]
    x64, cent, radius = x.astype(np.float64), T["cent"].astype(np.float64), T["radius"].astype(np.float64)
    lb2_of = order_tables(T)
    cells = np.flatnonzero(kept)
    # tightness, both ways: the entry IS the kernel's formula up to its float32 error -- a bound below it loses pruning, one
    # above it is not the bound the radii justify
    dist = np.sqrt(((cent[cells][:, None, :] - cent[cells][None, :, :]) ** 2).sum(-1))
    lb64 = np.maximum(0.0, dist * (1.0 - 1e-4) - radius[cells][:, None] - radius[cells][None, :])
    got = lb2_of[np.ix_(cells, cells)]
    off = ~np.eye(len(cells), dtype=bool)
    bad = off & ~(np.abs(got - lb64 * lb64) <= lb2_error(dist, lb64, d))
    assert not bad.any(), (f"{label}: lb2[{cells[np.nonzero(bad)[0][0]]}][{cells[np.nonzero(bad)[1][0]]}] = {got[bad][0]!r}, "
                           f"the formula gives {(lb64 * lb64)[bad][0]!r}")
    # soundness, no tolerance: a sweep stops at the first cell whose bound is beyond its queries' thresholds.  The Gram form
    # gives every pair's minimum to within gram_err (its float64 rounding is ~d 2^-53 of the largest squared norm; 1e-10 of it is
    # generous); a bound not below that by more than gram_err is decided by the direct sum of squared differences.
    rows = np.concatenate([members[c] for c in cells])
    starts = np.concatenate([[0], np.cumsum([len(members[c]) for c in cells])[:-1]])
    xs = x64[rows]
    gram_err = 1e-10 * float((xs * xs).sum(1).max())
    worst, positive = 0.0, 0
    for ia, a in enumerate(cells):
        mins = np.minimum.reduceat(_d2(x64[members[a]], xs).min(0), starts)
        for ib, b in enumerate(cells):
            if a == b or not got[ia, ib] > 0:
                continue
            positive += 1
            true_min = mins[ib]
            if got[ia, ib] > true_min - gram_err:
                true_min = min_pair_d2(x64[members[a]], x64[members[b]])
                assert got[ia, ib] <= true_min, f"{label}: lb2[{a}][{b}] = {got[ia, ib]!r} > {true_min!r}, the closest pair of the two cells"
            worst = max(worst, got[ia, ib] / true_min)
    return worst, positive, int(off.sum())


def assign_error(xn, cn, d, mfma):
    """|computed score - (x.c - |c|^2 / 2)| of one (row, centroid), |x| = xn, |c| = cn.
    float32 kernel (ivf_assign_kernel): a fused dot product of d + 1 terms in two accumulators, d + 2 roundings at most on any
    term, against sum |x_j c_j| + |c|^2 / 2 <= |x| |c| + |c|^2 / 2; the half norm (ivf_centpad_kernel) is itself a float32 sum
    of d squares: (d + 1) u more on |c|^2 / 2.
    bf16 kernel (ivf_centpad_bf16_kernel / ivf_assign_mfma_kernel): BOTH operands are the hi part alone, bf16_rn(x_j) and
    bf16_rn(c_j) -- no lo part -- so every product is off by (2 u_b + u_b^2) |x_j c_j|, u_b = 2^-9; the half norm rides in three
    bf16 pieces that sum to the float32 value exactly; the MFMA accumulates 64 products in float32."""
    f32 = (d + 2) * U * (xn * cn + 0.5 * cn * cn) + (d + 1) * U * 0.5 * cn * cn
    if not mfma:
        return 1.01 * f32
    return 1.01 * ((2.0 * U_BF16 + U_BF16 ** 2) * xn * cn + (64 + 2) * U * (xn * cn + 0.5 * cn * cn) + (d + 1) * U * 0.5 * cn * cn)


def check_assignment(x, T, mfma, label=""):
    """a row's own (unfolded) centroid against the float64-nearest one.  The kernel takes argmax of score = x.c - |c|^2 / 2,
    |x - c|^2 = |x|^2 - 2 score: if a won over the true nearest b on computed scores, then
    |x - c_a|^2 - |x - c_b|^2 <= 2 (err_a + err_b).  -> (worst excess / bound, share of rows not at their nearest centroid)"""
    d = x.shape[1]
    x64, cent = x.astype(np.float64), T["cent"].astype(np.float64)
    labels = T["labels"]
    xn, cn = np.sqrt((x64 * x64).sum(1)), np.sqrt((cent * cent).sum(1))
    worst, wrong = 0.0, 0
    for s in range(0, len(x64), 4096):
        q = x64[s: s + 4096]
        best = _d2(q, cent).argmin(1)  # (the Gram form selects; the two distances compared are direct sums)
        own = labels[s: s + 4096]
        excess = ((q - cent[own]) ** 2).sum(1) - ((q - cent[best]) ** 2).sum(1)
        bound = 2.0 * (assign_error(xn[s: s + 4096], cn[own], d, mfma) + assign_error(xn[s: s + 4096], cn[best], d, mfma))
        wrong += int((own != best).sum())
        bad = np.flatnonzero(excess > bound)
        assert len(bad) == 0, (f"{label}: row {s + bad[0]} sits in cell {own[bad[0]]}, {excess[bad[0]]!r} farther (squared) than its nearest "
                               f"centroid {best[bad[0]]}; the {'bf16' if mfma else 'float32'} scores allow {bound[bad[0]]!r}")
        worst = max(worst, float((excess / bound).max()))
    return worst, wrong / len(x64)


def check_tables(x, T, nprobe, mfma, label=""):
    """every table check of one call; x: the data [n, d].  -> dict of the measured figures"""
    members, kept, empty = check_layout(x, T, label)
    fig = {"cells": T["nc"], "kept": int(kept.sum()), "empty": len(empty)}
    fig["radius_ratio"] = check_radii(x, T, members, kept, label)
    check_order_rows(x, T, kept, nprobe, label)
    if nprobe == 0:
        fig["lb2_ratio"], fig["lb2_positive"], fig["lb2_pairs"] = check_bounds(x, T, members, kept, label)
    fig["assign_excess"], fig["assign_not_nearest"] = check_assignment(x, T, mfma, label)
    return fig


def assert_tables_equal(T1, T2, label="", perm_as_sets=True):
    for key in ("labels", "row_cell", "cell_map", "cent", "radius", "tile0", "ntiles", "order", "lb2"):
        assert T1[key].tobytes() == T2[key].tobytes(), f"{label}: {key} differs"
    # the scatter hands out image rows through atomic cursors: the order inside a cell is the race's
    t0, nt = T1["tile0"], T1["ntiles"]
    for c in range(T1["nc"]):
        a, b = (T["perm"][64 * t0[c]: 64 * (t0[c] + nt[c])] for T in (T1, T2))
        assert np.array_equal(np.sort(a), np.sort(b)), f"{label}: perm of cell {c} differs as a set"


# ---------------------------------------------------------------------------------------------------------------------
# the approximate promise
# ---------------------------------------------------------------------------------------------------------------------
_EXACT = {}


def exact_lists(x, rows, k, key):
    """the float64 brute force of the queries `rows`, computed once per `key` and set of rows"""
    key = (key, k, hash(np.asarray(rows).tobytes()))
    if key not in _EXACT:
        _EXACT[key] = S.oracle_self_first(x, rows, k)
    return _EXACT[key]


def check_promise(x, k, rows, idx, dist, n_fallback, T, label="", key=None):
    """rows: the queries of idx / dist.  For query i in cell a = row_cell[i]: P = the cells of order row a with a finite bound,
    V(i) = the other rows of those cells, R(i) = the k-1 best of V(i) by (float64 distance, index), E(i) = the exact list.
      1. every list is R(i) or E(i) beyond ties (a query whose certificate failed is scanned over EVERY cell within its bound);
      2. at most n_fallback queries have another list than R(i);
      3. at every rank the distance is at most R(i)'s.
    -> (share of the queries with R != E, queries whose list is not R)"""
    x64 = x.astype(np.float64)
    rows = np.asarray(rows)
    row_cell, order, lb2 = T["row_cell"], T["order"], T["lb2"]
    assert np.array_equal(idx[:, 0], rows) and not dist[:, 0].any(), f"{label}: self must come first at distance 0"
    true_d = np.sqrt(((x64[rows][:, None, :] - x64[idx]) ** 2).sum(-1))
    np.testing.assert_allclose(dist, true_d, rtol=1e-12, atol=0, err_msg=f"{label}: distance of the returned pair")
    ri, rd = np.empty_like(idx), np.empty_like(dist)
    for a in np.unique(row_cell[rows]):
        sel = np.flatnonzero(row_cell[rows] == a)
        probed = order[a][np.isfinite(lb2[a])]
        assert probed[0] == a
        allowed = np.flatnonzero(np.isin(row_cell, probed))
        ri[sel], rd[sel] = lists_among(x64, rows[sel], allowed, k)
    ei, ed = exact_lists(x, rows, k, key) if key else S.oracle_self_first(x, rows, k)
    r_ne_e = (np.sort(ri, axis=1) != np.sort(ei, axis=1)).any(1)
    not_r = np.flatnonzero((np.sort(idx, axis=1) != np.sort(ri, axis=1)).any(1))
    beyond_r = np.array([r for r in not_r if ocmp.knn_rows_differing_beyond_ties(idx[r: r + 1], dist[r: r + 1], ri[r: r + 1], rd[r: r + 1])[0]],
                        dtype=np.int64)
    if len(beyond_r):
        bad = ocmp.knn_rows_differing_beyond_ties(idx[beyond_r], dist[beyond_r], ei[beyond_r], ed[beyond_r])[0]
        assert bad == 0, (f"{label}: {bad} lists are neither the nearest neighbours among the probed rows nor the exact ones, "
                          f"first query {rows[beyond_r[0]]}")
    assert len(beyond_r) <= n_fallback, f"{label}: {len(beyond_r)} lists are not those of the probed rows, {n_fallback} queries were scanned"
    assert (dist <= rd * (1.0 + 1e-12)).all(), f"{label}: a list is worse at some rank than the best of the probed rows"
    return float(r_ne_e.mean()), len(beyond_r)


def check_swept_pairs(T, q0, nq, pairs, label=""):
    """approximate mode: scamd_knn_last_select_pairs() against the tables.  The queries of a cell form blocks of 128 slots, a
    block sweeps the cells of its order row up to the first infinite bound -- a bound of 0 can stop no sweep early -- and counts
    64 x 128 pairs per tile of every cell it enters.  A sweep that ends a cell early or late at a refill of its cell table, or
    follows another cell's order row, counts another number, whether or not a neighbour was lost by it."""
    row_cell, order, lb2, ntiles = T["row_cell"], T["order"], T["lb2"], T["ntiles"].astype(np.int64)
    queries = np.bincount(row_cell[q0: q0 + nq], minlength=T["nc"])
    want = 0
    for a in np.flatnonzero(queries):
        want += int(-(-queries[a] // 128)) * int(ntiles[order[a][np.isfinite(lb2[a])]].sum()) * 64 * 128
    assert pairs == want, f"{label}: the sweep evaluated {pairs!r} pairs, the cell tables say {want}"
    return want


def sample_covering_every_cell(T, m):
    """m query rows, the first members (by row number) of every cell with rows in turn"""
    row_cell = T["row_cell"]
    cells = np.flatnonzero(T["ntiles"] > 0)
    per = -(-m // len(cells))
    rows = np.concatenate([np.flatnonzero(row_cell == c)[:per] for c in cells])
    return np.sort(rows[:m])


# ---------------------------------------------------------------------------------------------------------------------
# whole cases: `setenv(name, value)` is monkeypatch.setenv
# ---------------------------------------------------------------------------------------------------------------------
_DATA = {}


def data_of(case: Case, exact: bool = False):
    if (case.name, exact) not in _DATA:
        _DATA[case.name, exact] = make_data(case, exact)
    return _DATA[case.name, exact]


def call(abi, setenv, case: Case, nprobe, **kw):
    for name, value in case_env(case, nprobe).items():
        setenv(name, value)
    buf, x = data_of(case, nprobe == 0)
    idx, dist, nfb, rc, T = abi.knn_with_cells(buf, case.k, nprobe=nprobe, d=case.d, **kw)
    return x, idx, dist, nfb, rc, T


# the emulator's query ranges where a case is not about the queries (the tables cover every row anyway); the folding case's
# begins at row 0: its two planted groups of rows are among its queries
EMU_SHARD, EMU_SMALL_SHARD, EMU_FOLD_SHARD = (1536, 1024), (1536, 256), (0, 1024)


def _shard_kw(case, shard):
    q0, nq = shard if shard else (0, case.n)
    return q0, nq, ({"q_begin": q0, "n_query": nq} if shard else {})


def run_exact_case(abi, setenv, case: Case, label="", shard=None, min_positive=0.1):
    """the pruned exact search: its lists against the float64 brute force, every table check, soundness of both bounds.
    min_positive: precondition on the data -- this share of the cell pairs at least has a positive lower bound (eight clusters:
    7 / 8 of the pairs of cells are pairs of different clusters, which lie apart unless d is small)."""
    q0, nq, kw = _shard_kw(case, shard)
    x, idx, dist, nfb, rc, T = call(abi, setenv, case, 0, **kw)
    assert rc == 0 and abi.lib.scamd_knn_last_nprobe() == 0
    label = f"{label} {case.name} exact"
    rows = S.checked_rows(nq, case.d, 5)
    S.check_against_f64(x, case.k, q0 + rows, idx[rows], dist[rows], n_fallback=nfb, n_query=nq, tie_fraction=None, label=label)
    fig = check_tables(x, T, 0, case.mfma_assign, label)
    fig["n_fallback"] = nfb
    print(f"{label}: {fig}")
    assert fig["lb2_positive"] >= min_positive * fig["lb2_pairs"], f"{label}: precondition: {fig['lb2_positive']} of {fig['lb2_pairs']} bounds are positive"
    return fig, T


def run_approx_case(abi, setenv, case: Case, nprobe, label="", sample=None, min_share=None, max_fallback=None, shard=None):
    """the approximate search at one nprobe: every table check, then the promise (on `sample` queries covering every cell, or
    on all).  min_share: precondition on the data -- this share of the queries at least must have R != E, or the test could not
    tell the two apart.  max_fallback: ... and at most this share may reach the float64 scan, whose lists are E."""
    q0, nq, kw = _shard_kw(case, shard)
    x, idx, dist, nfb, rc, T = call(abi, setenv, case, nprobe, **kw)
    assert rc == 0
    label = f"{label} {case.name} nprobe={nprobe}"
    assert abi.lib.scamd_knn_last_nprobe() == nprobe, f"{label}: the call was not answered by the approximate search"
    pairs = abi.lib.scamd_knn_last_select_pairs()
    fig = check_tables(x, T, nprobe, case.mfma_assign, label)
    rows = np.arange(nq) if sample is None else sample_covering_every_cell(T, sample)
    if sample is None:
        assert len(np.unique(T["row_cell"][q0 + rows])) == int((T["ntiles"] > 0).sum()), f"{label}: the queries do not cover every cell"
    fig["R_ne_E"], fig["not_R"] = check_promise(x, case.k, q0 + rows, idx[rows], dist[rows], nfb, T, label,
                                                   key=(case.n, case.d, case.k, case.data))
    fig["n_fallback"] = nfb
    fig["pairs_of_all"] = check_swept_pairs(T, q0, nq, pairs, label) / (float(nq) * case.n)
    print(f"{label}: {fig}")
    if min_share is not None:
        assert fig["R_ne_E"] >= min_share, f"{label}: precondition: only {fig['R_ne_E']:.3f} of the queries have other neighbours among the probed rows"
    if max_fallback is not None:
        assert nfb <= max_fallback * nq, f"{label}: precondition: {nfb} queries reached the float64 scan"
    return fig, T


def run_fold_case(abi, setenv, nprobes, label="", shard=None):
    """small and empty cells on purpose"""
    fig, T = run_exact_case(abi, setenv, FOLD_CASE, label, shard=shard)
    got = np.bincount(T["labels"], minlength=T["nc"])
    assert ((got > 0) & (got < MIN_CELL)).any(), f"{label}: precondition: no cell has between 1 and {MIN_CELL - 1} rows: {got.tolist()}"
    assert (got == 0).any(), f"{label}: precondition: no cell is empty: {got.tolist()}"
    assert (T["cell_map"] != np.arange(T["nc"])).sum() >= 2
    for nprobe in nprobes:
        run_approx_case(abi, setenv, FOLD_CASE, nprobe, label, shard=shard)
    return fig


SCAN_ENV = {"SCAMD_KNN_THR_MARGIN": "0"}  # the list threshold is the k-th entry itself: next to no query can be certified
SCAN_CASES = (Case("d20-scan", 4096, 20, 15, SCAN_ENV), Case("d50-tier2", 4096, 50, 15, {**SCAN_ENV, "SCAMD_KNN_TIER2_MIN": "0"}))
SCAN_NPROBE = 1


def run_scan_case(abi, setenv, case: Case, label="", shard=None):
    """What follows the sweep, on queries whose certificate fails (no margin between k and the threshold entry: most of them).
    d20-scan: they are scanned in float64 over EVERY cell within their bound, probed or not (knn_fallback_scan_cells_kernel),
    so their lists are the exact ones, not those of the probed rows.  Asserted: the promise as check_promise states it, and --
    so that 'among the probed rows OR BETTER' is known to be the statement that holds -- that some scanned query did come back
    with a better list.  d50-tier2: the bf16 engine's rejects go through the second tier first, a float32 sweep over the same
    tables and the same probed cells, whose lists are again those of the probed rows.
    Both: the tables read after the second tier and the scan are those of a call that needed neither."""
    plain = BY_NAME[case.name.split("-")[0]]
    assert np.array_equal(data_of(plain)[1], data_of(case)[1])
    q0, nq, kw = _shard_kw(case, shard)
    _, _, _, nfb0, rc, T0 = call(abi, setenv, plain, SCAN_NPROBE, **kw)  # (first: the scan environment is not set yet)
    assert rc == 0 and abi.lib.scamd_knn_last_second_tier_queries() == 0
    fig, T = run_approx_case(abi, setenv, case, SCAN_NPROBE, label, shard=shard, min_share=0.1)
    tier2 = abi.lib.scamd_knn_last_second_tier_queries()
    if "SCAMD_KNN_TIER2_MIN" in case.env:
        assert tier2 > nq // 2, f"{label}: precondition: the second tier saw {tier2} of {nq} queries"
    else:
        assert tier2 == 0 and fig["n_fallback"] > nq // 2, f"{label}: precondition: {fig['n_fallback']} of {nq} queries were scanned"
        assert fig["not_R"] > 0, f"{label}: precondition: no scanned query has a better list than the probed rows give: {fig}"
    assert_tables_equal(T0, T, f"{label} {case.name}: tables after the second tier and the scan against a call without them")
    return fig


def run_determinism_case(abi, setenv, case: Case, nprobe, label="", shard=None):
    """the quantiser's sums are 64-bit integers: two calls on the same input give the same tables bit for bit"""
    kw = _shard_kw(case, shard)[2]
    _, i1, d1, _, rc1, T1 = call(abi, setenv, case, nprobe, **kw)
    _, i2, d2, _, rc2, T2 = call(abi, setenv, case, nprobe, **kw)
    assert rc1 == 0 and rc2 == 0
    assert_tables_equal(T1, T2, f"{label} {case.name} nprobe={nprobe} twice")
    assert i1.tobytes() == i2.tobytes() and d1.tobytes() == d2.tobytes()


def run_shard_case(abi, setenv, label=""):
    """a query shard that starts and ends inside a 128-query block: the lists of the full call, the tables of the full call"""
    q0, nq = SHARD
    x, fi, fd, _, rc, TF = call(abi, setenv, SHARD_CASE, SHARD_NPROBE)
    _, si, sd, nfb, rc2, TS = call(abi, setenv, SHARD_CASE, SHARD_NPROBE, q_begin=q0, n_query=nq)
    assert rc == 0 and rc2 == 0
    assert_tables_equal(TF, TS, f"{label} shard against the full call")
    assert si.tobytes() == fi[q0: q0 + nq].tobytes(), f"{label}: the shard's index lists are not the full call's"
    assert sd.tobytes() == fd[q0: q0 + nq].tobytes(), f"{label}: the shard's distances are not the full call's"
    check_promise(x, SHARD_CASE.k, np.arange(q0, q0 + nq), si, sd, nfb, TS, f"{label} shard")


def run_exactly_answered_shape(abi, setenv, label="", shard=None):
    """n < 4096, k > 24, d > 64: the approximate entry answers exactly, there are no cell tables to hand out"""
    n, d, k, nprobe = EXACT_ANSWER_SHAPE
    setenv("SCAMD_KNN_CELL_ROWS", str(CELL_ROWS))
    x = overlapping(n, d, 3)
    q0, nq = shard if shard else (0, n)
    idx, dist, nfb, rc, T = abi.knn_with_cells(x, k, nprobe=nprobe, q_begin=q0, n_query=nq)
    assert abi.lib.scamd_knn_last_nprobe() == 0
    assert rc == EINVAL and T is None, f"{label}: the debug entry answered rc={rc} for a plan without cells"
    S.check_against_f64(x, k, np.arange(q0, q0 + nq), idx, dist, n_fallback=nfb, tie_fraction=None, label=f"{label} exactly answered")


def run_argument_checks(abi, setenv, launches=None, label="", shard=None):
    """a null or short workspace is refused before any copy: the outputs keep their prefill (knn_with_cells returns no tables),
    and on the emulator no kernel starts"""
    case = SHARD_CASE
    q0, nq, skw = _shard_kw(case, shard)
    for kw, want in (({"null_ws": True}, EINVAL), ({"ws_short": 64}, EWORKSPACE)):
        x, idx, dist, nfb, rc, T = call(abi, setenv, case, 3, **kw, **skw)
        assert rc == want and T is None, f"{label}: {kw}: rc={rc}"
    rc, nc, img = abi.knn_cell_sizes(case.n, case.d, nq, case.k, 3)
    assert (rc, nc) == (0, case.n // CELL_ROWS) and img >= case.n
    rc, nc, img = abi.knn_cell_sizes(case.n, 300, case.n, case.k, 3)  # d > 256: no plan at all
    assert rc == EINVAL and nc == 0 and img == 0
    if launches is not None:  # the entry's own kernels start only after its checks
        buf, _ = data_of(case)
        n0 = launches()
        abi.knn_with_cells(buf, case.k, nprobe=3, d=case.d, **skw)
        n1 = launches()
        abi.knn_with_cells(buf, case.k, nprobe=3, d=case.d, null_ws=True, **skw)
        n2 = launches()
        assert n2 - n1 == n1 - n0 - ENTRY_LAUNCHES, f"{label}: {n1 - n0} launches with the tables handed out, {n2 - n1} with the entry refusing"
