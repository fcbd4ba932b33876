"""`sc.pp.harmony_integrate` without a device: the CPU truth of tests/harmony_cases.py against facts that can be checked by hand
(lambda_kb, the closed-form correction against an explicit weighted ridge regression, the block count, batch codes, theta), the
precondition of the planted pipeline test, and every error and warning of the front end with the device stage stubbed."""
from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

import harmony_cases as H
import scanpy_amd as sc
from scanpy_amd.preprocessing import _harmony


# ---- lambda_kb --------------------------------------------------------------------------------------------------------
def test_lambda_dynamic_is_alpha_times_e():
    e, o = np.array([[10.0, 20.0], [30.0, 40.0]]), np.array([[5.0, 5.0], [5.0, 5.0]])
    lam = H.lambda_table(e, o, np.array([100.0, 100.0]), 0.2, None, 1.0, True)
    np.testing.assert_allclose(lam, 0.2 * e)


def test_lambda_fixed_is_the_ridge():
    lam = H.lambda_table(np.ones((2, 3)), np.ones((2, 3)), np.array([5.0, 5.0]), 0.2, 1e-5, 0.5, False)
    assert np.all(lam == 0.5)


def test_lambda_prunes_small_shares_and_empty_levels():
    e = np.full((3, 2), 10.0)
    o = np.array([[50.0, 0.0005], [1.0, 1.0], [0.0, 0.0]])
    lam = H.lambda_table(e, o, np.array([100.0, 100.0, 0.0]), 0.2, 1e-5, 1.0, True)
    assert lam[0, 0] == 2.0 and lam[0, 1] == H.SENTINEL  # 0.0005 / 100 < 1e-5
    assert np.all(lam[1] == 2.0) and np.all(lam[2] == H.SENTINEL)


def test_lambda_guards_a_zero_denominator():
    lam = H.lambda_table(np.zeros((1, 2)), np.array([[0.0, 3.0]]), np.array([4.0]), 0.2, None, 1.0, True)
    assert lam[0, 0] == H.SENTINEL and lam[0, 1] == 0.0


# ---- the correction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.CORRECT_CASES))
def test_closed_form_correction_is_the_ridge_regression(name):
    """the truth against np.linalg.lstsq on the one-hot design, every correction case, at the bound of every other comparison:
    16 x the float64-vs-longdouble sensitivity of the closed form, floor 1e-12 of the largest entry"""
    k = H.correct_case(name)
    sens, bnd = H.bound(k["f64"]["z_hat"], k["ld"]["z_hat"])
    dev = float(np.abs(k["f64"]["z_hat"] - k["lstsq"]).max())
    print(f"{name}: closed form vs lstsq {dev:.3e}, sensitivity {sens:.3e}, bound {bnd:.3e}")
    assert dev <= bnd
    moved = np.abs(k["f64"]["z_hat"] - k["state"]["x"]).max()
    assert moved > 1e-3 if k["state"]["B"] > 1 else moved < 1e-12  # the correction does something, except with one level


# ---- blocks, codes, theta ---------------------------------------------------------------------------------------------
def test_default_block_count_is_19():
    assert 1 // 0.05 == 19.0
    assert H.n_blocks_of(3000, 0.05) == 19 == _harmony._n_blocks(3000, 0.05)
    assert _harmony._n_blocks(12, 0.05) == 12 and _harmony._n_blocks(157, 1.0) == 1
    sizes = [len(b) for b in np.array_split(np.arange(2051), 19)]
    assert sizes == [108] * 18 + [107] and 2051 % 19 == 18  # the first n % n_blocks blocks hold one cell more


def test_default_cluster_count():
    assert [H.default_clusters(n) for n in (12, 700, 3000, 10 ** 6)] == [2, 23, 100, 100]


def test_batch_codes_are_offset_per_variable():
    df = pd.DataFrame({"a": ["x", "y", "x", "z"], "b": pd.Categorical([1, 1, 0, 1], categories=[0, 1, 2])})
    codes, levels = _harmony._encode_batches(df, ["a", "b"])
    assert codes.dtype == np.int32 and codes.tolist() == [[0, 4], [1, 4], [0, 3], [2, 4]] and levels.tolist() == [3, 3]
    c1, l1 = _harmony._encode_batches(df, "a")
    assert c1[:, 0].tolist() == [0, 1, 0, 2] and l1.tolist() == [3]
    c2, l2 = H.batch_codes([("a", df["a"]), ("b", df["b"])])
    assert np.array_equal(c2, codes) and np.array_equal(l2, levels)


def test_theta_expansion():
    for fn in (lambda t, l: _harmony._theta_per_level(t, l)[None, :], lambda t, l: H.theta_row(t, l)[None, :]):
        assert fn(2.0, [2, 3]).tolist() == [[2.0] * 5]
        assert fn([1.0, 4.0], [2, 3]).tolist() == [[1.0, 1.0, 4.0, 4.0, 4.0]]
        assert fn([1, 2, 3, 4, 5], [2, 3]).tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0]]
        with pytest.raises(ValueError, match=r"theta array size \(3\) must match"):
            fn([1, 2, 3], [2, 3])
        with pytest.raises(ValueError, match="theta must be a scalar or an array-like"):
            fn("much", [2, 3])


def test_tau_discount():
    th = H.tau_discount(np.array([2.0, 2.0]), np.array([10.0, 1000.0]), 5, 5)
    np.testing.assert_allclose(th, 2.0 * (1 - np.exp(-np.array([10.0, 1000.0]) / 25) ** 2))
    assert H.tau_discount(np.array([2.0]), np.array([10.0]), 5, 0)[0] == 2.0


def test_restated_permutation_is_a_bijection():
    for n in (1, 2, 17, 1000):
        assert np.array_equal(np.sort(H.device_permutation(n, 5, 2)), np.arange(n))


# ---- the planted input of the pipeline test -----------------------------------------------------------------------------
def test_planted_input_reference_way_runs_agree_with_each_other():
    """precondition of tests/test_gpu_harmony_pipeline.py: on this input two runs of the truth drawn the reference's way with
    different seeds meet the reference's own acceptance measure against each other"""
    x, types, codes = H.pipeline_input()
    caps = dict(max_iter_harmony=4, max_iter_clustering=8, tol_harmony=1e-4, tol_clustering=1e-5)
    runs = []
    for seed in (11, 12):
        cen, perms = H.reference_way_draws(H.unit_rows(x), H.default_clusters(x.shape[0]), seed)
        runs.append(H.harmony_truth(x, codes, 2, cen, perms, **caps)[0])
    r, l2 = H.acceptance(runs[0], runs[1])
    print(f"two reference-way runs: min column Pearson r {r:.4f}, relative L2 {l2:.4f}")
    assert r > 0.95 and l2 < 0.1
    before = H.other_batch_share(x, codes)
    assert H.other_batch_share(runs[0], codes) > before


# ---- the front end, device stage stubbed -----------------------------------------------------------------------------
@pytest.fixture
def adata():
    rng = np.random.default_rng(0)
    a = sc.AnnData(np.zeros((40, 3), np.float32))
    a.obsm["X_pca"] = rng.standard_normal((40, 5))
    a.obs["batch"] = pd.Categorical(np.arange(40) % 3)
    a.obs["run"] = pd.Categorical(np.arange(40) % 2)
    return a


@pytest.fixture
def stub(monkeypatch):
    calls = []

    def fit(self, x, codes, n_levels, theta, generator):
        calls.append(dict(x=x, codes=codes, n_levels=n_levels, theta=theta, flavor=self.flavor))
        return x + 1.0

    monkeypatch.setattr(_harmony.HarmonyRun, "fit", fit)
    return calls


def test_writes_the_slot_in_the_requested_dtype(adata, stub):
    assert sc.pp.harmony_integrate(adata, "batch") is None
    assert adata.obsm["X_pca_harmony"].dtype == np.float64 and np.array_equal(adata.obsm["X_pca_harmony"], adata.obsm["X_pca"] + 1)
    sc.pp.harmony_integrate(adata, "batch", dtype=np.float32, adjusted_basis="X_h", theta=[1.0, 2.0, 3.0], flavor="harmony1")
    assert adata.obsm["X_h"].dtype == np.float32 and stub[-1]["x"].dtype == np.float64
    assert np.array_equal(stub[-1]["x"], adata.obsm["X_pca"].astype(np.float32).astype(np.float64))  # dtype rounds the input
    assert stub[-1]["theta"].tolist() == [1.0, 2.0, 3.0] and stub[-1]["n_levels"] == 3 and stub[-1]["flavor"] == "harmony1"
    assert stub[-1]["codes"].tolist() == (np.arange(40) % 3).tolist()


@pytest.mark.parametrize("kwargs,exc,match", [
    (dict(flavor="harmony3"), ValueError, "flavor must be 'harmony1' or 'harmony2'"),
    (dict(correction_method="original"), ValueError, "correction_method must be 'fast'"),
    (dict(basis="X_nope"), ValueError, "not available"),
    (dict(key="nope"), KeyError, "nope"),
    (dict(key=[]), ValueError, "at least one column name"),
    (dict(alpha=0.0), ValueError, "alpha must be a finite positive number"),
    (dict(alpha=float("inf")), ValueError, "alpha must be a finite positive number"),
    (dict(batch_prune_threshold=1.5), ValueError, r"batch_prune_threshold must be in \[0, 1\] or None"),
    (dict(flavor="harmony1", ridge_lambda=0.0), ValueError, "ridge_lambda must be a finite positive number"),
    (dict(max_iter_harmony=0), ValueError, "max_iter_harmony must be >= 1"),
    (dict(theta=[1.0, 2.0]), ValueError, r"theta array size \(2\) must match"),
    (dict(theta="much"), ValueError, "theta must be a scalar"),
    (dict(key=["batch", "run"]), NotImplementedError, "general-design ridge solve"),
])
def test_errors(adata, stub, kwargs, exc, match):
    kwargs = dict(kwargs)
    key = kwargs.pop("key", "batch")
    with pytest.raises(exc, match=match):
        sc.pp.harmony_integrate(adata, key, **kwargs)
    assert not stub and "X_pca_harmony" not in adata.obsm


def test_nan_input_and_missing_batch_values(adata, stub):
    adata.obsm["X_pca"][3, 1] = np.nan
    with pytest.raises(ValueError, match="contains NaN values"):
        sc.pp.harmony_integrate(adata, "batch")
    adata.obsm["X_pca"][3, 1] = 0.0
    adata.obs["holes"] = pd.Categorical([None if i == 5 else "a" for i in range(40)])
    with pytest.raises(ValueError, match="Batch variable 'holes' contains missing values"):
        sc.pp.harmony_integrate(adata, "holes")
    assert not stub


@pytest.mark.parametrize("kwargs,match", [
    (dict(ridge_lambda=2.0), "ridge_lambda is ignored when flavor='harmony2'"),
    (dict(flavor="harmony1", alpha=0.5), "alpha is ignored when flavor='harmony1'"),
    (dict(flavor="harmony1", batch_prune_threshold=None), "batch_prune_threshold is ignored when flavor='harmony1'"),
])
def test_ignored_parameter_warnings(adata, stub, kwargs, match):
    with pytest.warns(UserWarning, match=match):
        sc.pp.harmony_integrate(adata, "batch", **kwargs)
    assert len(stub) == 1


def test_defaults_warn_nothing(adata, stub):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sc.pp.harmony_integrate(adata, "batch")
        sc.pp.harmony_integrate(adata, "batch", flavor="harmony1")


def test_limits_are_refused_before_any_device_call():
    with pytest.raises(NotImplementedError, match="at most 128 columns"):
        _harmony.HarmonyRun().fit(np.zeros((40, 129)), np.zeros(40, np.int32), 1, np.array([2.0]), np.random.default_rng(0))


# ---- the two convergence rules ---------------------------------------------------------------------------------------
def test_outer_convergence_rule():
    f = _harmony._outer_converged
    assert not f([], 1e-4) and not f([5.0], 1e-4)
    assert f([100.0, 99.995], 1e-4) and not f([100.0, 99.98], 1e-4)  # fell by 0.005 < 0.01; by 0.02 > 0.01
    assert f([100.0, 101.0], 1e-4)  # a rise counts as converged
    assert f([-100.0, -100.005], 1e-4) and not f([-100.0, -100.02], 1e-4)  # the tolerance scales with |objective|
    assert f([7.0, 100.0, 99.995], 1e-4)  # only the last two count
    assert not f([100.0, 100.0], 0.0) and f([100.0, 100.0 + 1e-9], 0.0)  # strict inequality


def test_clustering_convergence_rule_compares_two_windows_of_three():
    f = _harmony._clustering_converged
    assert not f([3.0, 2.0, 1.0], 1.0)  # needs four objectives, whatever the tolerance
    # windows [10, 9, 8] -> [9, 8, 7.999]: 27 - 24.999 = 2.001 against tol * 27
    assert not f([10.0, 9.0, 8.0, 7.999], 0.07) and f([10.0, 9.0, 8.0, 7.999], 0.075)
    assert f([50.0, 10.0, 9.0, 8.0, 7.999], 0.075)  # only the last four count
    assert f([10.0, 9.0, 8.0, 11.0], 1e-5)  # 27 -> 28: a rise counts as converged
    assert f([-10.0, -10.0, -10.0, -10.0001], 1e-5) and not f([-10.0, -10.0, -10.0, -10.001], 1e-5)


def test_a_clustering_that_hits_its_cap_records_no_objective():
    """the outer test sees the initial objective and those of the clusterings that converged, nothing else -- as the truth does"""
    calls = iter([10.0, 9.0, 8.5, 8.4, 8.39, 8.389, 8.3889])
    ours, inner = [20.0], []
    for cap in (3, 4):
        inner = []
        while len(inner) < cap:
            inner.append(next(calls))
            if _harmony._clustering_converged(inner, 0.01):
                ours.append(inner[-1])
                break
    # first clustering: 3 iterations, no decision, nothing recorded; second: 8.4, 8.39, 8.389, 8.3889 -> converged at its fourth
    assert ours == [20.0, 8.3889] and len(inner) == 4
