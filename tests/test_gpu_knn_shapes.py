"""Every template instantiation of the exact kNN search (`scamd_knn_l2_f32`, csrc/knn.hip) against the float64 brute force
(run with -m gpu): the LDS-list kernels test_gpu_kernels.py does not reach, the boundaries of `knn_plan()`, the cell-pruned
sweep away from k = 15, query shards on the LDS-list kernels, a row stride larger than d, groups of identical rows up
to and beyond the float64 scan's table, and the float64 scan forced behind every path that follows the sweep.  Tables and checker: tests/knn_shape_cases.py (shared with the emulator's
counterparts in test_emu_cpu.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import knn_shape_cases as S
import test_gpu_kernels as _older

pytestmark = pytest.mark.gpu

# CPU side, at import: a new instantiation in knn_plan()'s restatement without a case here fails the collection of this
# file on any machine (the emulator suite repeats it as a test of its own)
_VS_SKLEARN = _older.test_knn_vs_sklearn.pytestmark[0].args[1]
COVERED = S.assert_every_instantiation_has_a_case(_VS_SKLEARN)


@pytest.fixture(scope="module")
def K():
    import torch

    from scanpy_amd import _kernels

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _kernels


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _knn(K, xd, k, **kw):
    idx, dist, nfb = K.knn(xd, k, **kw)
    return idx.cpu().numpy(), dist.cpu().numpy(), nfb


def _ran(K, d, k, n_query, n, *, pruned, b3_env=None, expect_pruning=True, label=""):
    """the getters of the call just made: the engine the shape promises, and the sweep it claims -- the brute-force path
    reports exactly n_query * n pairs and no pre-pass, the pruned one a pre-pass and (on clustered data) fewer pairs"""
    lib = K._lib.load()
    assert lib.scamd_knn_last_select_engine() == S.expected_engine(d, k, b3_env), label
    pairs, pre = lib.scamd_knn_last_select_pairs(), lib.scamd_knn_last_select_prepass_pairs()
    if not pruned:
        assert pairs == float(n_query) * float(n) and pre == 0.0, (label, pairs, pre)
    else:
        assert pre > 0.0, (label, "the call did not take the cell-pruned sweep")
        if expect_pruning:
            assert pairs < float(n_query) * float(n), (label, pairs, n_query * n)
    return pairs


def _run_and_check(K, x, k, *, pruned=False, b3_env=None, expect_pruning=True, seed=0, label="", tie_fraction=1e-3):
    n, d = x.shape
    idx, dist, nfb = _knn(K, _dev(x), k)
    _ran(K, d, k, n, n, pruned=pruned, b3_env=b3_env, expect_pruning=expect_pruning, label=label)
    rows = S.checked_rows(n, d, seed)
    assert (idx[:, 0] == np.arange(n)).all() and (dist[:, 0] == 0).all() and idx.min() >= 0 and idx.max() < n
    assert k == 1 or (np.diff(dist, axis=1) >= 0).all()
    S.check_against_f64(x, k, rows, idx[rows], dist[rows], n_fallback=nfb, n_query=n, label=label, tie_fraction=tie_fraction)
    return idx, dist, nfb


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("d", "k"), sorted(S.LDS_LIST_CASES))
def test_every_lds_list_instantiation(K, d, k):
    """knn_select_kernel<H, TC, NW, KP> for the eleven (H, KP) no other test launches (table: knn_shape_cases.LDS_LIST_CASES);
    n = 2101 is no multiple of the candidate padding (256) nor of any query block (32 .. 256)"""
    x = S.clustered(2101, d, 1000 * d + k)
    _run_and_check(K, x, k, label=f"lds-list {S.LDS_LIST_CASES[(d, k)]}")


def test_the_tables_cover_every_instantiation():
    lds, reg = COVERED
    assert len(lds) == 18 and reg == [8, 16, 25, 32]


@pytest.mark.parametrize(("d", "k"), S.BOUNDARY_CASES)
def test_plan_boundaries(K, d, k):
    """both sides of every bound of knn_plan(); k = 1 returns the self column alone; d = 1 is many near-ties (a large share
    of the queries goes through the float64 scan: correctness is what is asserted)"""
    x = S.clustered(2101 if d <= 64 else 1301, d, 77 * d + k)
    idx, dist, _ = _run_and_check(K, x, k, label=f"boundary d={d} k={k}")
    if k == 1:
        assert idx.shape == (x.shape[0], 1) and (idx[:, 0] == np.arange(x.shape[0])).all() and not dist.any()


# ---------------------------------------------------------------------------------------------------------------------
def _pruned_equals_brute(K, monkeypatch, x, k, *, b3_env=None, expect_pruning=True, label=""):
    n, d = x.shape
    xd = _dev(x)
    if b3_env is not None:
        monkeypatch.setenv("SCAMD_KNN_B3", b3_env)
    monkeypatch.setenv("SCAMD_KNN_IVF", "0")
    i0, d0, _ = _knn(K, xd, k)
    _ran(K, d, k, n, n, pruned=False, b3_env=b3_env, label=label + " brute")
    monkeypatch.setenv("SCAMD_KNN_IVF", "1")
    i1, d1, nfb = _knn(K, xd, k)
    pairs = _ran(K, d, k, n, n, pruned=True, b3_env=b3_env, expect_pruning=expect_pruning, label=label + " pruned")
    print(f"{label}: pruned sweep evaluated {pairs / (float(n) * n):.3f} of all pairs")
    # both end in the same float64 re-rank: bitwise
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(d0, d1)
    rows = S.checked_rows(n, d, 5)
    S.check_against_f64(x, k, rows, i1[rows], d1[rows], n_fallback=nfb, n_query=n, label=label)


@pytest.mark.parametrize("kind", ["clustered", "gaussian"])
@pytest.mark.parametrize("k", S.PRUNED_K)
@pytest.mark.parametrize("d", S.PRUNED_D)
def test_pruned_sweep_d_k_grid(K, monkeypatch, d, k, kind):
    """SCAMD_KNN_IVF=1 at every H of the register-list kernel and list thresholds from rank 8 to the cap of 32; on data
    without structure nothing prunes and the sweep must visit every cell (no `pairs <` statement there)"""
    n = 12289
    x = S.clustered(n, d, 31 * d + k, S.PRUNED_SPREAD) if kind == "clustered" else S.gaussian(n, d, 31 * d + k)
    _pruned_equals_brute(K, monkeypatch, x, k, expect_pruning=kind == "clustered", label=f"grid {kind} d={d} k={k}")


@pytest.mark.parametrize("kind", ["clustered", "gaussian"])
@pytest.mark.parametrize(("d", "k"), S.PRUNED_FLOAT_ENGINE_ON_H25)
def test_pruned_sweep_float_engine_on_h25(K, monkeypatch, d, k, kind):
    """SCAMD_KNN_B3=0: the float32 engine's pruned instantiation for H = 25 is the second tier's code and otherwise sees
    rejected queries only"""
    n = 12289
    x = S.clustered(n, d, 47 * d + k, S.PRUNED_SPREAD) if kind == "clustered" else S.gaussian(n, d, 47 * d + k)
    _pruned_equals_brute(K, monkeypatch, x, k, b3_env="0", expect_pruning=kind == "clustered", label=f"grid B3=0 {kind} d={d} k={k}")


@pytest.mark.parametrize(("d", "k"), S.PRUNED_DEFAULT_SIZE_CASES)
def test_pruned_sweep_default_size_off_the_beaten_shape(K, d, k):
    """n = 70000: pruned by default, no environment -- these instantiations the way a user reaches them; sampled oracle"""
    x = S.clustered(70000, d, 13 * d + k, S.PRUNED_SPREAD)
    _run_and_check(K, x, k, pruned=True, seed=d + k, label=f"default-size d={d} k={k}")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("d", "k"), S.SHARD_CASES)
def test_query_shards_on_the_lds_list_kernels(K, d, k):
    """the multi-GPU call pattern on kernels that pad queries to QB = NW * 32: every shard bitwise equal to the same rows
    of the full call"""
    n = 2357
    x = S.clustered(n, d, 3 * d + k)
    xd = _dev(x)
    i_all, d_all, _ = _knn(K, xd, k)
    for qb, nq in ((0, 1), (0, 33), (1031, 129), (n - 77, 77), (500, 0)):
        i_s, d_s, nfb = _knn(K, xd, k, q_begin=qb, n_query=nq)
        assert i_s.shape == (nq, k) and d_s.shape == (nq, k) and 0 <= nfb <= nq
        if nq:
            _ran(K, d, k, nq, n, pruned=False, label=f"shard ({qb}, {nq})")
        np.testing.assert_array_equal(i_all[qb:qb + nq], i_s, err_msg=f"shard ({qb}, {nq})")
        np.testing.assert_array_equal(d_all[qb:qb + nq], d_s, err_msg=f"shard ({qb}, {nq})")
    rows = np.arange(1031, 1031 + 129)
    S.check_against_f64(x, k, rows, i_all[rows], d_all[rows], label=f"shard rows d={d} k={k}")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.FORCED_SCAN_CASES, ids=S.FORCED_SCAN_IDS)
def test_forced_float64_scan_on_every_path_after_the_sweep(K, monkeypatch, case):
    """cert_scale = 1e30 behind every re-rank kernel, past and through the second tier, over all rows and over cells: every
    query is scanned, the lists are the float64 brute force's and bitwise those of the certified call"""
    for name, value in case[3].items():
        monkeypatch.setenv(name, value)
    lib = K._lib.load()
    S.check_forced_scan(lambda x, k, qb, nq, cs: _knn(K, _dev(x), k, q_begin=qb, n_query=nq, cert_scale=cs),
                        lambda: int(lib.scamd_knn_last_second_tier_queries()), case, label=f"forced scan {case[:3]}")


# ---------------------------------------------------------------------------------------------------------------------
def _knn_strided(K, buf, d, k):
    """scamd_knn_l2_f32 on the first d columns of the device buffer buf [n, ld_x] -- `_kernels.knn` makes its input
    contiguous first and so never passes ld_x > d"""
    import torch

    lib = K._lib.load()
    n, ld = buf.shape
    assert buf.is_contiguous() and ld > d
    idx = torch.empty((n, k), dtype=torch.int32, device=buf.device)
    dist = torch.empty((n, k), dtype=torch.float64, device=buf.device)
    ws, wsz = K._ws(lib.scamd_knn_workspace_bytes(n, d, n, k), buf.device)
    nfb = C.c_int64(0)
    rc = lib.scamd_knn_l2_f32(K.ptr(buf), n, d, ld, 0, n, k, K.ptr(idx), K.ptr(dist), 1.0, C.byref(nfb), K.ptr(ws), wsz, K.stream_ptr())
    K._check(rc, "scamd_knn_l2_f32")
    return idx.cpu().numpy(), dist.cpu().numpy(), int(nfb.value)


# (d = 100 is an LDS-list kernel: no pruned sweep to run)
@pytest.mark.parametrize(("d", "ivf"), [(20, "0"), (20, "1"), (50, "0"), (50, "1"), (100, "0")])
def test_row_stride(K, monkeypatch, d, ivf):
    """ld_x = d + 7 (part of the C ABI): padding columns full of large finite garbage, then NaN -- nothing may read them"""
    monkeypatch.setenv("SCAMD_KNN_IVF", ivf)
    n, k = 4603, 15
    x = S.clustered(n, d, 9 * d, S.PRUNED_SPREAD)
    i0, d0, _ = _knn(K, _dev(x), k)
    _ran(K, d, k, n, n, pruned=ivf == "1", label="contiguous")
    for fill in (3.0e30, np.nan):
        buf = np.full((n, d + 7), fill, dtype=np.float32)
        buf[:, d:] *= np.random.default_rng(1).choice([-1.0, 1.0], (n, 7)).astype(np.float32)
        buf[:, :d] = x
        i1, d1, _ = _knn_strided(K, _dev(buf), d, k)
        _ran(K, d, k, n, n, pruned=ivf == "1", label=f"ld_x = d + 7, padding {fill}")
        np.testing.assert_array_equal(i0, i1, err_msg=f"padding {fill}")
        np.testing.assert_array_equal(d0, d1, err_msg=f"padding {fill}")
    rows = S.checked_rows(n, d, 2)
    S.check_against_f64(x, k, rows, i0[rows], d0[rows], label=f"row stride d={d} ivf={ivf}")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("d", "k", "ivf"), [(d, k, ivf) for d, k in S.DUPLICATE_CASES for ivf in ("0", "1") if ivf == "0" or S.plan(d, k)[4]])
def test_duplicate_groups(K, monkeypatch, d, k, ivf):
    """groups of 10 .. 600 identical rows inside clustered data.  The full checker, except its bound on the share of rows
    that use the tie exemption: here ties are the data (the oracle's argpartition keeps an arbitrary k + 1 of 600 rows at
    distance 0), so that bound is replaced by the exact statement of check_duplicate_groups -- self, then the other members
    in ascending row order"""
    monkeypatch.setenv("SCAMD_KNN_IVF", ivf)
    n = 4603
    x, groups = S.with_duplicate_groups(S.clustered(n, d, 5 * d + k, S.PRUNED_SPREAD), S.DUPLICATE_GROUPS, seed=d)
    idx, dist, _ = _run_and_check(K, x, k, pruned=ivf == "1", label=f"duplicates d={d} k={k} ivf={ivf}", tie_fraction=None)
    S.check_duplicate_groups(groups, k, idx, dist, label=f"duplicates d={d} k={k} ivf={ivf}")


@pytest.mark.parametrize("ivf", ["0", "1"])
@pytest.mark.parametrize("d", [20, 50])
@pytest.mark.parametrize("group", [2100, 5000])
def test_more_identical_rows_than_the_fallback_table_holds(K, monkeypatch, group, d, ivf):
    """more rows tied at the k-th distance than the float64 scan's table of FALLBACK_CAP = 2048 holds: the call returns
    (before the bound of the scan became a (distance, index) key it gave up with `rows tied within their k-th distance`
    after eight rescans), the k - 1 neighbours of a member are the other members of lowest row number, and a second call
    returns the same bits although other rows win the race for the table"""
    assert group > S.FALLBACK_CAP
    monkeypatch.setenv("SCAMD_KNN_IVF", ivf)
    n, k = group + 2101, 15
    x, groups = S.with_duplicate_groups(S.clustered(n, d, 11 * d + group, S.PRUNED_SPREAD), (group,), seed=group + d)
    idx, dist, nfb = _run_and_check(K, x, k, pruned=ivf == "1", label=f"{group} identical rows d={d} ivf={ivf}", tie_fraction=None)
    S.check_duplicate_groups(groups, k, idx, dist, label=f"{group} identical rows")
    idx2, dist2, _ = _knn(K, _dev(x), k)
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(dist, dist2)
