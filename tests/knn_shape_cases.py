"""TEST INFRASTRUCTURE shared by tests/test_gpu_knn_shapes.py (the product library on the GPU) and tests/test_emu_cpu.py (the
same kernels on the host emulator): the shape tables of the exact kNN search (`scamd_knn_l2_f32`, csrc/knn.hip), a
restatement of `knn_plan()` that says which template instantiation a (d, k) reaches, and ONE checker against the float64
brute force of oracle/knn.py.  Nothing here touches a device."""
from __future__ import annotations

import numpy as np

from oracle import compare as ocmp
from oracle import knn as oknn

# ---------------------------------------------------------------------------------------------------------------------
# knn_plan() of csrc/knn.hip restated: (d, k) -> (H, TC, NW, KP, register-list kernel?).  The library offers no getter of
# the instantiation it launched, so the tables below are tied to this rule and the rule is short enough to compare
# with the C++ by eye; `assert_every_instantiation_has_a_case` fails when the rule gains a shape no table reaches.
# ---------------------------------------------------------------------------------------------------------------------
H_BY_D = ((16, 8), (32, 16), (50, 25), (64, 32), (128, 64), (256, 128))  # d <= bound -> H
KP_BY_K = ((24, 32, 8), (56, 64, 4), (120, 128, 2), (256, 288, 1))     # k <= bound -> KP, NW


def plan(d: int, k: int):
    H = next(h for bound, h in H_BY_D if d <= bound)
    KP, NW = next((kp, nw) for bound, kp, nw in KP_BY_K if k <= bound)
    TC = 32 if H == 128 else (64 if H == 64 else 128)
    if H == 128 and NW > 2:  # d > 128: blocks of at most two waves
        NW, KP = 2, max(KP, 128)
    reg = KP == 32 and H <= 32
    if reg:
        NW, TC = 4, 64  # knn_select_reg_kernel: 4 waves x 32 queries, 64-candidate tiles
    elif KP == 288:
        TC = min(TC, 64)  # dispatch_kp: one wave stages at most 64 norms per tile
    return H, TC, NW, KP, reg


def expected_engine(d: int, k: int, b3_env: str | None = None) -> int:
    """scamd_knn_last_select_engine(): 1 = bf16x3, only for 32 < d <= 50 and k <= 24 and unless SCAMD_KNN_B3=0"""
    H, _, _, _, reg = plan(d, k)
    return 1 if (reg and H == 25 and b3_env != "0") else 0


# (d, k) -> (H, TC, NW, KP): one case per LDS-list instantiation that tests/test_gpu_kernels.py::test_knn_vs_sklearn
# does not reach
#   (10, 100) -> (  8, 128, 2, 128)     (10, 200) -> (  8,  64, 1, 288)
#   (24,  40) -> ( 16, 128, 4,  64)     (24, 100) -> ( 16, 128, 2, 128)
#   (40,  40) -> ( 25, 128, 4,  64)
#   (60,  40) -> ( 32, 128, 4,  64)     (60, 100) -> ( 32, 128, 2, 128)     (60, 200) -> ( 32,  64, 1, 288)
#   (100, 40) -> ( 64,  64, 4,  64)     (100, 100) -> ( 64,  64, 2, 128)    (100, 200) -> ( 64,  64, 1, 288)
LDS_LIST_CASES = {
    (10, 100): (8, 128, 2, 128), (10, 200): (8, 64, 1, 288),
    (24, 40): (16, 128, 4, 64), (24, 100): (16, 128, 2, 128),
    (40, 40): (25, 128, 4, 64),
    (60, 40): (32, 128, 4, 64), (60, 100): (32, 128, 2, 128), (60, 200): (32, 64, 1, 288),
    (100, 40): (64, 64, 4, 64), (100, 100): (64, 64, 2, 128), (100, 200): (64, 64, 1, 288),
}

# boundaries of the plan: every d bound and its successor at k = 15, every k bound and its successor at d = 50 (H = 25,
# both engines' home) and d = 20 (H = 16); (33, *), (129, *), (*, 121), (*, 256) are test_knn_vs_sklearn's
BOUNDARY_D = (1, 2, 16, 17, 32, 50, 51, 64, 65, 128, 256)
BOUNDARY_K = (1, 2, 24, 25, 56, 57, 120)
BOUNDARY_CASES = [(d, 15) for d in BOUNDARY_D] + [(d, k) for d in (50, 20) for k in BOUNDARY_K]

# the cell-pruned sweep away from (d = 50 | 30 | 20, k = 15): every H of the register-list kernel with both of its d
# bounds, k from the smallest list threshold (rank 8 / 10) to its cap (k = 24: rank 30, and 32 = the list's end for bf16)
PRUNED_D = (8, 16, 17, 32, 33, 40, 50, 51, 64)
PRUNED_K = (2, 5, 10, 24)
PRUNED_FLOAT_ENGINE_ON_H25 = ((50, 24), (40, 5))  # with SCAMD_KNN_B3=0: otherwise the second tier's code only
PRUNED_DEFAULT_SIZE_CASES = ((12, 10), (30, 24), (40, 20), (64, 5))  # one per H at n >= 65536, no environment

SHARD_CASES = ((50, 30), (100, 15), (50, 100), (200, 256))  # LDS-list kernels: QB = NW * 32 = 128, 256, 64, 32
DUPLICATE_GROUPS = (10, 16, 33, 100, 600)
DUPLICATE_CASES = ((50, 15), (20, 15), (50, 30), (100, 15))
FALLBACK_CAP = 2048  # csrc/knn.hip: rows the float64 scan's table holds per query

# cert_scale = 1e30 (no query can be certified) on every path that follows the sweep: (n, d, k, environment, query shard
# (q_begin, n_query) or None = all rows, queries the second tier must report).  Without pruning one case per re-rank kernel:
# the row-wise one of the register-list kernels and knn_rerank_kernel<32 | 64 | 128 | 288>, then the plain float64 scan.
# With pruning the row-wise re-rank in slot order and the scan over cells, once past the second tier (its threshold out of
# reach) and once through it (threshold 0: it re-ranks every query and rejects every one again).
_BRUTE, _PRUNED = {"SCAMD_KNN_IVF": "0"}, {"SCAMD_KNN_IVF": "1", "SCAMD_KNN_CELL_ROWS": "512"}
FORCED_SCAN_CASES = (
    (700, 20, 10, _BRUTE, None, 0),
    (700, 100, 15, _BRUTE, None, 0),
    (700, 50, 30, _BRUTE, None, 0),
    (700, 24, 100, _BRUTE, None, 0),
    (700, 10, 200, _BRUTE, None, 0),
    (4300, 50, 15, {**_PRUNED, "SCAMD_KNN_TIER2_MIN": str(2 ** 30)}, (0, 256), 0),
    (4300, 50, 15, {**_PRUNED, "SCAMD_KNN_TIER2_MIN": "0"}, (0, 256), 256),
)
FORCED_SCAN_IDS = [f"n{n}-d{d}-k{k}-" + ("brute" if e is _BRUTE else f"pruned-tier2min{e['SCAMD_KNN_TIER2_MIN']}")
                   for n, d, k, e, _, _ in FORCED_SCAN_CASES]


def assert_every_instantiation_has_a_case(already_run_elsewhere):
    """`already_run_elsewhere`: the (n, d, k) list of test_gpu_kernels.py::test_knn_vs_sklearn.  Every (H, KP) of the LDS-list
    kernel that plan() can produce has a case there or in LDS_LIST_CASES, the comment table is what plan() says, and every H
    of the register-list kernel runs brute force (BOUNDARY_CASES, small n) and pruned (PRUNED_D x PRUNED_K)."""
    for (d, k), inst in LDS_LIST_CASES.items():
        assert plan(d, k) == (*inst, False), (d, k, plan(d, k), inst)
    lds, reg_h = set(), set()
    for d in range(1, 257):
        for k in range(1, 257):
            H, _, _, KP, reg = plan(d, k)
            (reg_h if reg else lds).add(H if reg else (H, KP))
    here = {(plan(d, k)[0], plan(d, k)[3]) for d, k in LDS_LIST_CASES}
    there = {(plan(d, k)[0], plan(d, k)[3]) for _, d, k in already_run_elsewhere if not plan(d, k)[4]}
    assert len(lds) == 18 and lds <= here | there, sorted(lds - here - there)
    assert not here & there, sorted(here & there)  # (a case per UNTESTED pair: nothing is run twice for nothing)
    brute = {plan(d, k)[0] for d, k in BOUNDARY_CASES if plan(d, k)[4]}
    pruned = {plan(d, k)[0] for d in PRUNED_D for k in PRUNED_K if plan(d, k)[4]}
    default = {plan(d, k)[0] for d, k in PRUNED_DEFAULT_SIZE_CASES if plan(d, k)[4]}
    assert reg_h == {8, 16, 25, 32} == brute == pruned == default, (reg_h, brute, pruned, default)
    assert all(plan(d, k)[4] for d in PRUNED_D for k in PRUNED_K) and all(plan(d, k)[4] for d, k in PRUNED_DEFAULT_SIZE_CASES)
    assert all(not plan(d, k)[4] for d, k in SHARD_CASES)
    return sorted(lds), sorted(reg_h)


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def clustered(n: int, d: int, seed: int, spread: float = 3.0) -> np.ndarray:
    """eight Gaussian clusters of unit variance, centres drawn with standard deviation `spread` per coordinate; spread = 3 is
    the data of test_gpu_kernels.py::test_knn_vs_sklearn"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((8, d)).astype(np.float32) * np.float32(spread)
    return (centers[rng.integers(0, 8, n)] + rng.standard_normal((n, d))).astype(np.float32)


# The pruned-sweep cases assert `pairs < n_query * n`, and a cell is skipped only when its ball lies beyond a query's
# threshold.  Two centres are spread * sqrt(2 d) apart on average and a cluster of a few thousand rows reaches to about
# sqrt(d) + 2.5 from its centre: at spread = 3 and d = 8 that is 12 against 2 x 5.3 -- the balls of neighbouring clusters touch,
# little is skipped, and the padding of the cell-sorted layout (up to 64 rows and 128 query slots per cell, 16 cells: a factor
# 1.26 at n = 12289) outweighs it.  At spread = 8 the clusters are apart at every d of the grid (32 against 10.6 at d = 8).
PRUNED_SPREAD = 8.0


def gaussian(n: int, d: int, seed: int) -> np.ndarray:
    """no structure: the cell bounds of the pruned sweep prune next to nothing, its stopping rule must never stop early"""
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def with_duplicate_groups(x: np.ndarray, sizes, seed: int):
    """-> (x with groups of `sizes` identical rows at random positions, list of the groups' sorted row numbers).  Every
    group takes the coordinates of one of its own rows, so it sits inside the data."""
    rng = np.random.default_rng(seed)
    x = x.copy()
    rows = rng.permutation(x.shape[0])[: sum(sizes)]
    groups, at = [], 0
    for s in sizes:
        g = np.sort(rows[at: at + s])
        x[g] = x[g[0]]
        groups.append(g)
        at += s
    return x, groups


def checked_rows(n: int, d: int, seed: int, sample: int = 1000) -> np.ndarray:
    """all rows while the float64 brute force is small (n * n * d <= 1e9), otherwise a fixed seeded sample"""
    if n * n * d <= 1e9:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, sample, replace=False))


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def oracle_self_first(x: np.ndarray, rows: np.ndarray, k: int):
    """the float64 brute force in the library's convention: column 0 the query itself at distance 0, then its k-1 nearest
    OTHER rows by (distance, index) -- the oracle's k columns with the query taken out (or the last column, when k or more
    identical rows kept the query out of its own list) and put in front"""
    n, d = x.shape
    f = oknn.knn_exact_f64 if len(rows) * n * d <= 2e9 else oknn.knn_exact_f64_sample
    kk = min(k, n)
    ei, ed = f(x, np.asarray(rows), kk)
    keep = ei != np.asarray(rows)[:, None]
    keep[keep.all(axis=1), -1] = False
    m = len(rows)
    ei, ed = ei[keep].reshape(m, kk - 1), ed[keep].reshape(m, kk - 1)
    return np.hstack([np.asarray(rows)[:, None], ei]), np.hstack([np.zeros((m, 1)), ed])


def check_against_f64(x: np.ndarray, k: int, rows: np.ndarray, idx: np.ndarray, dist: np.ndarray, *, n_fallback=None,
                      n_query=None, tie_fraction=1e-3, label=""):
    """idx / dist: the library's rows for the queries `rows` of x.  Asserts, for every one of them:
      column 0 is the row itself at distance exactly 0, indices lie in [0, n), none twice; every distance IS the float64
      distance of the returned pair (rtol 1e-12, as test_gpu_kernels.py); distances ascend; the distance row equals the
      oracle's (rtol 1e-12: whatever ties do, this catches a neighbour swapped for a farther one); no index set differs
      from the oracle's beyond ties at the k-th distance, and at most `tie_fraction` of the rows differ at all (the bound of
      test_knn_full_size_sampled_exact; None where the data is MADE of ties, see the duplicate tests).
    -> rows that differ at all"""
    n, d = x.shape
    rows = np.asarray(rows)
    m = len(rows)
    assert idx.shape == (m, k) and dist.shape == (m, k) and n >= k
    if n_fallback is not None:
        assert 0 <= n_fallback <= (m if n_query is None else n_query), n_fallback
    assert (idx[:, 0] == rows).all(), f"{label}: column 0 must be the query itself"
    assert (dist[:, 0] == 0).all(), f"{label}: the self distance must be exactly 0"
    assert idx.min() >= 0 and idx.max() < n, f"{label}: index outside [0, n)"
    if k > 1:
        assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all(), f"{label}: a row lists an index twice"
        assert (np.diff(dist, axis=1) >= 0).all(), f"{label}: distances must ascend"
    x64 = x.astype(np.float64)
    step = max(1, int(2e7 // (k * d)))
    for s in range(0, m, step):
        q = rows[s: s + step]
        true_d = np.sqrt(((x64[q][:, None, :] - x64[idx[s: s + step]]) ** 2).sum(-1))
        np.testing.assert_allclose(dist[s: s + step], true_d, rtol=1e-12, atol=0, err_msg=f"{label}: distance of the returned pair")
    ei, ed = oracle_self_first(x, rows, k)
    np.testing.assert_allclose(np.sort(dist, axis=1), ed, rtol=1e-12, atol=0, err_msg=f"{label}: distance row vs the float64 brute force")
    bad, differ = ocmp.knn_rows_differing_beyond_ties(idx, dist, ei, ed)
    print(f"{label}: n={n} d={d} k={k} plan={plan(d, k)} checked={m} n_fallback={n_fallback} rows differing at all={differ} beyond ties={bad}")
    assert bad == 0, f"{label}: {bad} rows differ from the float64 brute force beyond ties ({differ} incl. ties)"
    if tie_fraction is not None:
        assert differ <= tie_fraction * m, f"{label}: {differ} of {m} rows needed the tie exemption"
    return differ


def check_forced_scan(knn, second_tier_queries, case, label=""):
    """one row of FORCED_SCAN_CASES (its environment already set).  knn(x, k, q_begin, n_query, cert_scale) -> (idx, dist,
    n_fallback) as numpy; second_tier_queries() -> scamd_knn_last_second_tier_queries().  With cert_scale = 1e30 every query
    goes through the float64 scan, the lists are the float64 brute force's, and they are BITWISE those of the same call at
    cert_scale = 1: both routes sum (q - c)^2 by fma in coordinate order and order by the key (distance, row), and a
    certified list holds every row at or below its k-th distance."""
    n, d, k, _, shard, tier2 = case
    q_begin, n_query = shard if shard else (0, n)
    x = clustered(n, d, 7 * d + k, PRUNED_SPREAD)
    i1, d1, _ = knn(x, k, q_begin, n_query, 1.0)
    i2, d2, n_scan = knn(x, k, q_begin, n_query, 1e30)
    assert n_scan == n_query, f"{label}: {n_scan} of {n_query} queries reached the float64 scan"
    assert second_tier_queries() == tier2, f"{label}: second tier saw {second_tier_queries()} queries, expected {tier2}"
    assert plan(d, k)[4] or not shard
    check_against_f64(x, k, np.arange(q_begin, q_begin + n_query), i2, d2, n_fallback=n_scan, n_query=n_query, label=label)
    assert i1.tobytes() == i2.tobytes(), f"{label}: index lists differ between cert_scale 1 and 1e30"
    assert d1.tobytes() == d2.tobytes(), f"{label}: distances differ bitwise between cert_scale 1 and 1e30"


def check_duplicate_groups(groups, k: int, idx: np.ndarray, dist: np.ndarray, label="", q_begin: int = 0):
    """what the key (distance, index) promises inside a group of identical rows: a member's list is itself, then the other
    members in ascending row order, all at distance 0 (as many as fit), whichever rows a race may have favoured.
    idx / dist: the lists of the queries q_begin .. q_begin + len(idx) - 1"""
    for g in groups:
        for r in g[(g >= q_begin) & (g < q_begin + len(idx))]:
            others = g[g != r][: k - 1]
            got_i, got_d = idx[r - q_begin], dist[r - q_begin]
            assert np.array_equal(got_i[1: 1 + len(others)], others), f"{label}: row {r} of a group of {len(g)}: {got_i.tolist()}"
            assert not got_d[: 1 + len(others)].any(), f"{label}: row {r} of a group of {len(g)}"
