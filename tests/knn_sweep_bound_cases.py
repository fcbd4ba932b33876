"""TEST INFRASTRUCTURE shared by tests/test_gpu_knn_sweep_bound.py (the product library on the GPU) and
tests/test_emu_knn_sweep_bound_cpu.py (the same kernels on the host emulator): the tables the EXACT pruned kNN search sweeps
by (csrc/knn.hip: ivf_reach_kernel, ivf_sweep_order_kernel), handed out by `scamd_knn_debug_sweep_tables` next to the ball
tables of `scamd_knn_debug_cell_tables`, against numpy float64 on the float32 inputs.

The sweep bound of two cells a, b is max(ball bound, projection bound), the projection bound being
    |w| - (R[a][b] + R[b][a]) / |w|,  w = c_b - c_a,  R[p][o] = max over the members x of p of (x - c_p).(c_o - c_p),
with R[p][o] computed for the cells o of p's short list and replaced by the ball-derived r_p |w| elsewhere.
Nothing here touches a device: `abi` is tests/emu/harness.py:Abi over HostMem or over graph_kernel_cases.DeviceMem."""
from __future__ import annotations

import ctypes as C

import numpy as np

import knn_cell_cases as K
import knn_shape_cases as S

U = K.U
REACH_ERR_PAD = 4    # csrc/knn.hip: the float32 error charged to a reach is (d + 4) u r_p |w|
REACH_MIN_LIST = 8   # ... the short list's floor: the first 8 cells of the ball row
REACH_MAX_LIST = 64  # ... and its cap
LIST_FACTOR = np.float32(1.5)  # ... and its rule: squared ball bound <= fl(fl(1.5 r_p)^2)
GAP_DOWN = 1.0 - 1e-6          # ... the two factors that round the gap and its square down
REACH_DIRS = {"emulator": 4, "gpu": 32}  # directions a block of ivf_reach_kernel takes per pass over its rows
REACH_TILES = {"emulator": 2, "gpu": 8}  # ... and the tiles of 64 rows it takes of its cell: larger cells span several blocks
EINVAL = K.EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# cases: knn_cell_cases.Case with four more kinds of data
# ---------------------------------------------------------------------------------------------------------------------
Case = K.Case
SIGMA_CASE = Case("sigma", 4096, 50, 15, data="sigma")
SIGMA_F32_CASE = Case("sigma-f32", 4096, 50, 15, K._F32, data="sigma")
DUP_CASE = Case("dup", 4096, 20, 15, data="dup")
TWIN_CASE = Case("twin", 4096, 20, 15, data="twin")
GEOMETRY_CASES = tuple(K.BY_NAME[name] for name in ("d10", "d20", "d50", "d50-f32", "d64", "d20-ld27"))
EMU_CASES = GEOMETRY_CASES + (SIGMA_CASE, SIGMA_F32_CASE, K.OFFSET_CASE, K.FOLD_CASE, DUP_CASE, TWIN_CASE)
BIG_CASES = (Case("big-sigma", 32768, 50, 15, data="sigma"), Case("big-d20", 32768, 20, 15), Case("big-overlap", 32768, 20, 15, data="overlap32"),
             Case("big-cells-of-1024", 32768, 50, 15, {"SCAMD_KNN_CELL_ROWS": "1024"}, data="sigma"))  # 32 cells of ~16 tiles
SIGMA_MIN_SHARE = 0.5  # of the cell pairs: sweep bound strictly above the ball bound (pairs of cells of different clusters)
DUP_GROUPS = (10, 33, 300)
SHARD = (1000, 1500)   # begins and ends inside a block of 128 queries


def sigma_clusters(n, d, seed, n_centres=8):
    """isotropic unit-variance clusters whose centres are 16 - 27 sigma apart: the balls of two clusters' cells overlap or nearly
    touch (a cell's radius in 50 dimensions is ~ sqrt(50) + 2 = 9), so the ball bound is 0 or small there, while along the line
    through two centroids a cell reaches ~ 3 - 4.5 sigma: the projection bound is ~ 8 - 19.  Centres: N(0, 2.1^2) per
    coordinate, |c_i - c_j| ~ 2.1 sqrt(2 d) = 21 at d = 50."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((n_centres, d)) * 2.1
    dist = np.sqrt(((cent[:, None, :] - cent[None, :, :]) ** 2).sum(-1))[np.triu_indices(n_centres, 1)]
    assert d == 50 and dist.min() >= 16.0 and dist.max() <= 27.0, (dist.min(), dist.max())
    return (cent[rng.integers(0, n_centres, n)] + rng.standard_normal((n, d))).astype(np.float32)


def twin_start(n, d, seed):
    """the quantiser starts cell c at row c * (n / nc) + (n / nc) / 2: rows 128 and 384 (cells 0 and 1 of 16) are the same
    point INSIDE the data -- two centroids that coincide at first and stay close or equal, |w| = 0 or tiny"""
    x = S.clustered(n, d, seed, 3.0)
    x[384] = x[128]
    return x


_DATA = {}


def data_of(case: Case):
    """-> (x [n, d + pad] with NaN in the padding, the data x[:, :d]); the kinds of knn_cell_cases in their exact-search form"""
    if case.name not in _DATA:
        seed = 1000 * case.d + case.k
        if case.data == "sigma":
            x = sigma_clusters(case.n, case.d, seed)
        elif case.data == "dup":
            x, _ = S.with_duplicate_groups(S.clustered(case.n, case.d, seed, 3.0), DUP_GROUPS, seed + 1)
        elif case.data == "twin":
            x = twin_start(case.n, case.d, seed)
        elif case.data == "overlap32":  # every cell within 1.5 radii of every other: no structure, no lists
            x = K.overlapping(case.n, case.d, seed)
        else:
            return K.data_of(case, True)
        buf = np.full((case.n, case.d + case.pad), np.nan, dtype=np.float32)
        buf[:, : case.d] = x
        _DATA[case.name] = (buf, x)
    return _DATA[case.name]


# ---------------------------------------------------------------------------------------------------------------------
# one exact search, then both debug entries on the workspace it left
# ---------------------------------------------------------------------------------------------------------------------
def knn_with_sweep(abi, x, k, *, d=None, q_begin=0, n_query=None, nprobe=0):
    """-> (idx, dist, n_fallback, pairs, ball tables as Abi.knn_with_cells gives them, rc of the sweep entry, sweep tables or
    None: reach [nc, nc] (+inf = not computed), list_len [nc], order, lb2 [nc, nc] -- the sweep rows under the keys the
    checkers of knn_cell_cases read)"""
    m, lib, p = abi.mem, abi.lib, abi.mem.ptr
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, ld = x.shape
    d = ld if d is None else d
    nq = n if n_query is None else n_query
    dx = m.put(x, np.float32)
    idx, dist = m.full((nq, k), np.int32, -7), m.full((nq, k), np.float64, np.nan)
    ws, wsz = abi._ws(lib.scamd_knn_workspace_bytes(n, d, nq, k))
    nfb = C.c_int64(-1)
    if nprobe:
        rc = lib.scamd_knn_l2_ivf_f32(p(dx), n, d, ld, q_begin, nq, k, int(nprobe), p(idx), p(dist), C.byref(nfb), p(ws), wsz, m.stream)
    else:
        rc = lib.scamd_knn_l2_f32(p(dx), n, d, ld, q_begin, nq, k, p(idx), p(dist), 1.0, C.byref(nfb), p(ws), wsz, m.stream)
    m.sync()
    assert rc == 0, lib.scamd_last_error().decode()
    pairs = lib.scamd_knn_last_select_pairs()
    rc, nc, img = abi.knn_cell_sizes(n, d, nq, k, nprobe)
    assert rc == 0
    i32 = lambda shape: m.full(shape, np.int32, -7)  # noqa: E731
    f32 = lambda shape: m.full(shape, np.float32, np.nan)  # noqa: E731
    out = dict(labels=i32(n), row_cell=i32(n), cell_map=i32(nc), cent=f32((nc, d)), radius=f32(nc), tile0=i32(nc), ntiles=i32(nc),
               order=i32((nc, nc)), lb2=f32((nc, nc)), perm=i32(img))
    rows = C.c_int64(-1)
    rc = lib.scamd_knn_debug_cell_tables(n, d, nq, k, int(nprobe), p(ws), wsz, *(p(out[key]) for key in out), C.byref(rows), m.stream)
    m.sync()
    assert rc == 0
    T = {key: m.get(a) for key, a in out.items()}
    T["perm"] = T["perm"][: int(rows.value)]
    T["nc"] = nc
    sw = dict(reach=f32((nc, nc)), list_len=i32(nc), order=i32((nc, nc)), lb2=f32((nc, nc)))
    rc = lib.scamd_knn_debug_sweep_tables(n, d, nq, k, int(nprobe), p(ws), wsz, *(p(sw[key]) for key in sw), m.stream)
    m.sync()
    W = None
    if rc == 0:
        W = {key: m.get(a) for key, a in sw.items()}
        W["nc"] = nc
    return m.get(idx), m.get(dist), int(nfb.value), pairs, T, rc, W


def call(abi, setenv, case: Case, shard=None, nprobe=0):
    for name, value in K.case_env(case, nprobe).items():
        setenv(name, value)
    buf, x = data_of(case)
    q0, nq = shard if shard else (0, case.n)
    return (x, q0, nq) + knn_with_sweep(abi, buf, case.k, d=case.d, q_begin=q0, n_query=nq, nprobe=nprobe)


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------
def ball_of(T):
    """-> the ball table by cell: lb2 [nc, nc] float32 (row a, column b)"""
    nc = T["nc"]
    out = np.empty((nc, nc), dtype=np.float32)
    np.put_along_axis(out, T["order"].astype(np.int64), T["lb2"], axis=1)
    return out


def check_short_lists(T, W, kept, label=""):
    """the list IS the rule: the head of the ball row -- the kept cells whose squared ball bound is <= fl(fl(1.5 r)^2), the first
    8 of them in any case, 64 at most; NO list where the rule names more than 64 cells and more than three quarters of the kept
    ones (no structure at the scale of the cells) --, the own cell on it, reach finite exactly there.
    -> on [nc, nc] bool by cell"""
    nc = T["nc"]
    n_kept = int(kept.sum())
    on = np.zeros((nc, nc), dtype=bool)
    for p in range(nc):
        t = LIST_FACTOR * T["radius"][p]
        t2 = np.float32(t * t)
        row = T["lb2"][p]
        near = int(((row <= t2) & np.isfinite(row)).sum())
        want = min(max(near, min(REACH_MIN_LIST, n_kept)), REACH_MAX_LIST) if kept[p] else 0
        if near > REACH_MAX_LIST and 4 * near > 3 * n_kept:
            want = 0
        assert W["list_len"][p] == want, f"{label}: cell {p}: short list of {W['list_len'][p]}, the rule gives {want}"
        on[p, T["order"][p][:want]] = True
        assert not want or on[p, p], f"{label}: cell {p} is not on its own list"
    assert np.array_equal(np.isfinite(W["reach"]), on), f"{label}: reach is finite on other entries than the short lists"
    assert np.isposinf(W["reach"][~on]).all(), f"{label}: an entry off the short lists is not +inf"
    return on


def check_reach(x, T, W, members, on, label=""):
    """tightness, both ways, of every computed reach against float64 on the float32 rows and centroids.  The kernel's error:
    one rounding each in fl(x - c_p) and fl(c_o - c_p), at most d on a term's way through the fused chain:
    <= (d + 2) u |x - c_p| |w|; it charges d + 4 of them on its radius, which is asserted here against the TRUE radius.
    -> worst |error| / bound"""
    x64, cent = x.astype(np.float64), T["cent"].astype(np.float64)
    worst = 0.0
    for p in np.flatnonzero(on.any(1)):
        o = np.flatnonzero(on[p])
        e = x64[members[p]] - cent[p]
        w = cent[o] - cent[p]
        want = (e @ w.T).max(0)
        tol = (x.shape[1] + REACH_ERR_PAD) * U * np.sqrt((e * e).sum(1).max()) * np.sqrt((w * w).sum(1))
        got = W["reach"][p, o].astype(np.float64)
        bad = ~(np.abs(got - want) <= tol)
        assert not bad.any(), f"{label}: reach[{p}][{o[bad][0]}] = {got[bad][0]!r}, float64 gives {want[bad][0]!r} (allowed {tol[bad][0]!r})"
        nz = tol > 0
        if nz.any():
            worst = max(worst, float((np.abs(got - want)[nz] / tol[nz]).max()))
        assert got[o == p] == 0.0, f"{label}: reach[{p}][{p}] = {got[o == p]!r}"
    return worst


def sweep_formula(T, W, kept):
    """the kernel's combination restated in float64 from ITS reaches, radii, centroids and ball entries.  -> (want [nc, nc] by cell,
    its tolerance, the projection part alone, |w|)"""
    nc = T["nc"]
    cent, radius = T["cent"].astype(np.float64), T["radius"].astype(np.float64)
    reach = W["reach"].astype(np.float64)
    w = np.sqrt(((cent[:, None, :] - cent[None, :, :]) ** 2).sum(-1))
    err = (T["cent"].shape[1] + REACH_ERR_PAD) * U
    r_w = radius[:, None] * w
    rab = np.where(np.isfinite(reach), reach + err * r_w, r_w)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = (w - (rab + rab.T) / w) * GAP_DOWN
    gap = np.where((w > 0) & (gap > 0), gap, 0.0)
    proj = gap * gap * GAP_DOWN
    ball = ball_of(T).astype(np.float64)
    want = np.maximum(ball, proj)
    want[~kept, :] = np.inf
    want[:, ~kept] = np.inf
    want[np.arange(nc), np.arange(nc)] = np.where(kept, -1.0, np.inf)
    # the float32 rounding of the square; the float64 roundings of |w|^2 (d terms) and of the gap, which is a difference of
    # numbers of the size of |w|
    tol = 1.01 * (U * proj + 1e-13 * w * w)
    return want, tol, proj, w


def sweep_of(W):
    nc = W["nc"]
    out = np.empty((nc, nc), dtype=np.float64)
    np.put_along_axis(out, W["order"].astype(np.int64), W["lb2"].astype(np.float64), axis=1)
    return out


def check_sweep_tables(x, T, W, members, kept, label=""):
    """dominance (exact), the formula (tight both ways), soundness (no tolerance).
    -> dict: share of the kept cell pairs strictly above the ball bound, worst bound / true minimum, positive entries"""
    nc = T["nc"]
    x64 = x.astype(np.float64)
    got = sweep_of(W)
    ball = ball_of(T).astype(np.float64)
    cells = np.flatnonzero(kept)
    sub = np.ix_(cells, cells)
    assert (got[sub] >= ball[sub]).all(), f"{label}: a sweep bound is below the ball bound of the same call"
    want, tol, proj, w = sweep_formula(T, W, kept)
    assert not np.isnan(got).any(), f"{label}: NaN in sweep_lb2"
    off = ~np.eye(len(cells), dtype=bool)
    bad = off & ~(np.abs(got[sub] - want[sub]) <= tol[sub])
    assert not bad.any(), (f"{label}: sweep_lb2[{cells[np.nonzero(bad)[0][0]]}][{cells[np.nonzero(bad)[1][0]]}] = {got[sub][bad][0]!r}, "
                           f"the formula gives {want[sub][bad][0]!r}")
    # soundness as knn_cell_cases.check_bounds: the Gram form selects, the direct sum of squares decides close calls
    rows = np.concatenate([members[c] for c in cells])
    starts = np.concatenate([[0], np.cumsum([len(members[c]) for c in cells])[:-1]])
    xs = x64[rows]
    gram_err = 1e-10 * float((xs * xs).sum(1).max())
    worst, positive = 0.0, 0
    for ia, a in enumerate(cells):
        mins = np.minimum.reduceat(K._d2(x64[members[a]], xs).min(0), starts)
        for ib, b in enumerate(cells):
            if a == b or not got[a, b] > 0:
                continue
            positive += 1
            true_min = mins[ib]
            if got[a, b] > true_min - gram_err:
                true_min = K.min_pair_d2(x64[members[a]], x64[members[b]])
                assert got[a, b] <= true_min, f"{label}: sweep_lb2[{a}][{b}] = {got[a, b]!r} > {true_min!r}, the closest pair of the two cells"
            worst = max(worst, got[a, b] / true_min)
    strict = (got[sub] > ball[sub]) & off
    return {"strict_share": float(strict.sum()) / max(int(off.sum()), 1), "sweep_ratio": worst, "sweep_positive": positive,
            "formula_strict_share": float(((proj[sub] > ball[sub] + tol[sub]) & off).sum()) / max(int(off.sum()), 1)}


def asymmetric_pairs(on, kept):
    """pairs (a, b) of kept cells with b on a's list and a not on b's: the stand-in on one side only"""
    return int((on & ~on.T & kept[:, None] & kept[None, :]).sum())


def check_swept_pairs(T, W, q0, nq, dist, thr_rank_min, pairs, label=""):
    """scamd_knn_last_select_pairs() between two figures computed from the verified float64 lists.  A block of 128 queries of
    cell a enters the cells of its row while bound * (1 - 1e-3) <= (largest threshold of the block) * (1 + 1e-3); a query's
    threshold is the squared distance of some list entry of rank >= thr_rank_min at every moment, so never below its true
    thr_rank_min-th smallest distance, and a block's largest threshold is never below the SMALLEST of those over the cell's
    queries, t_a.  So every block of a enters at least the cells whose bound is <= t_a -- by the table it follows.
      floor:   that count under the sweep rows -- the sweep never evaluates fewer;
      ceiling: the same count under the BALL rows -- a build that follows the ball rows never evaluates fewer than THIS, and the
               sweep by the tighter rows must evaluate strictly fewer (asserted where the case says so).
    -> (floor, pairs, ceiling)"""
    row_cell, ntiles = T["row_cell"], T["ntiles"].astype(np.int64)
    cells = row_cell[q0: q0 + nq]
    t_q = dist[:, thr_rank_min - 1] ** 2
    ball, sweep = ball_of(T).astype(np.float64), sweep_of(W)
    floor = ceiling = 0
    for a in np.unique(cells):
        t_a = float(t_q[cells == a].min())
        blocks = int(-(-int((cells == a).sum()) // 128))
        floor += blocks * int(ntiles[sweep[a] <= t_a].sum()) * 64 * 128
        ceiling += blocks * int(ntiles[ball[a] <= t_a].sum()) * 64 * 128
    assert pairs >= floor, f"{label}: the sweep evaluated {pairs!r} pairs, the cells its final thresholds reach hold {floor}"
    return floor, pairs, ceiling


def run_case(abi, setenv, case: Case, label="", shard=None, strict_pairs=False, min_strict=None, min_asymmetric=0):
    """one exact search: the lists against the float64 brute force, the ball rows' conventions (they stay what they were), and
    every check of the sweep tables"""
    x, q0, nq, idx, dist, nfb, pairs, T, rc, W = call(abi, setenv, case, shard)
    label = f"{label} {case.name}"
    assert rc == 0 and abi.lib.scamd_knn_last_nprobe() == 0
    rows = S.checked_rows(nq, case.d, 5)
    S.check_against_f64(x, case.k, q0 + rows, idx[rows], dist[rows], n_fallback=nfb, n_query=nq, tie_fraction=None, label=label)
    members, kept, _ = K.check_layout(x, T, label)
    K.check_order_rows(x, T, kept, 0, f"{label} ball rows")
    K.check_order_rows(x, {**T, "order": W["order"], "lb2": W["lb2"]}, kept, 0, f"{label} sweep rows")
    on = check_short_lists(T, W, kept, label)
    fig = {"cells": int(kept.sum()), "tiles_max": int(T["ntiles"].max()), "list_mean": float(W["list_len"][kept].mean()), "list_max": int(W["list_len"].max()),
           "asymmetric": asymmetric_pairs(on, kept), "reach_err": check_reach(x, T, W, members, on, label)}
    fig.update(check_sweep_tables(x, T, W, members, kept, label))
    # thresholds: the list entry of rank k + 6 (float32 engine) or k + 8 (bf16 engine), capped at 32 -- never below rank k;
    # the distances are the library's, just verified against the brute force (all of them where that is affordable)
    if len(rows) == nq or not strict_pairs:
        fig["pairs_floor"], fig["pairs"], fig["pairs_ball"] = check_swept_pairs(T, W, q0, nq, dist, case.k, pairs, label)
        if strict_pairs:
            assert pairs < fig["pairs_ball"], f"{label}: {pairs!r} pairs swept, the ball rows alone would allow {fig['pairs_ball']}"
    print(f"{label}: {fig}")
    if min_strict is not None:
        assert fig["formula_strict_share"] >= min_strict, f"{label}: precondition: the float64 formula lifts only {fig['formula_strict_share']:.3f} of the pairs"
        assert fig["strict_share"] >= min_strict, f"{label}: only {fig['strict_share']:.3f} of the cell pairs have a sweep bound above the ball bound"
    assert fig["asymmetric"] >= min_asymmetric, f"{label}: precondition: {fig['asymmetric']} one-sided pairs"
    return fig, T, W


def run_determinism_case(abi, setenv, case: Case, label="", shard=None):
    """max is exact in any order and a row's sum has a fixed order: two calls give bit-equal tables, whatever order the
    scatter's race left the rows of a cell in"""
    a = call(abi, setenv, case, shard)
    b = call(abi, setenv, case, shard)
    for key in ("reach", "list_len", "order", "lb2"):
        assert a[-1][key].tobytes() == b[-1][key].tobytes(), f"{label} {case.name}: {key} differs between two calls"
    assert a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes()


def run_approximate_mode(abi, setenv, case: Case, nprobe, label="", shard=None):
    """nprobe > 0: the sweep entry refuses (nothing was built), the ball tables and the swept pairs are those of the
    approximate mode as knn_cell_cases states them"""
    x, q0, nq, idx, dist, nfb, pairs, T, rc, W = call(abi, setenv, case, shard, nprobe=nprobe)
    assert rc == EINVAL and W is None, f"{label}: the sweep entry answered rc={rc} after an approximate call"
    assert abi.lib.scamd_knn_last_nprobe() == nprobe
    _, kept, _ = K.check_layout(x, T, label)
    K.check_order_rows(x, T, kept, nprobe, label)
    K.check_swept_pairs(T, q0, nq, pairs, label)
