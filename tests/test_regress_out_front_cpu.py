"""Host logic of scanpy_amd.pp.regress_out on a CPU stand-in for the two device passes (tests/regress_cases.CpuStubRegressBackend:
float64 numpy): the reference's golden outputs on pbmc68k_reduced, its behavioural tests (tests/test_preprocessing.py:360-503 of
the reference) restated, the dtype rules, the errors and the refusals.  The same front end runs on the HIP kernels in
tests/test_gpu_regress_out.py."""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import regress_cases as R  # noqa: E402

import scanpy_amd as sc  # noqa: E402
from scanpy_amd.preprocessing import _csr_device, _regress_out  # noqa: E402


@pytest.fixture(autouse=True)
def _stub(monkeypatch):
    monkeypatch.setattr(_csr_device, "default_backend", lambda: R.CpuStubRegressBackend())


@pytest.fixture(scope="module")
def pbmc_obs(tmp_path_factory):
    return R.pbmc68k_obs(tmp_path_factory.mktemp("pbmc68k"))


def _adata(n=300, g=40, density=0.6, seed=0, dtype=np.float32, fmt="csr"):
    rng = np.random.default_rng(seed)
    x = sparse.random(n, g, density=density, format="csr", dtype=np.float64, random_state=seed)
    x.data = np.ceil(x.data * 50)
    x = x.astype(dtype)
    a = sc.AnnData(x if fmt == "csr" else (x.tocsc() if fmt == "csc" else x.toarray()))
    a.obs["percent_mito"] = rng.random(n)
    a.obs["n_counts"] = np.asarray(x.sum(axis=1)).ravel().astype(np.float64)
    a.obs["batch"] = pd.Categorical(rng.integers(1, 4, n))
    return a


def _dense(x):
    return x.toarray() if sparse.issparse(x) else np.asarray(x)


def test_exported():
    assert "regress_out" in sc.pp.__all__ and sc.pp.regress_out is _regress_out.regress_out


def test_numeric_golden(pbmc68k, pbmc_obs):
    """regress_test_small.npy of the reference: [n_counts, percent_mito] on raw_X[:200, :200], float32 out"""
    a = R.golden_adata(pbmc68k["raw_X"], pbmc_obs)
    assert sc.pp.regress_out(a, ["n_counts", "percent_mito"]) is None
    R.assert_matches_numeric_golden(a.X)


def test_categorical_golden(pbmc68k, pbmc_obs):
    """regress_test_small_cat.npy: bulk_labels, float64 out, the reference's own atol = 1e-6"""
    a = R.golden_adata(pbmc68k["raw_X"], pbmc_obs)
    sc.pp.regress_out(a, ["bulk_labels"])
    R.assert_matches_categorical_golden(a.X)
    b = R.golden_adata(pbmc68k["raw_X"], pbmc_obs)
    b.obs["bulk_labels"] = b.obs["bulk_labels"].astype(str).astype(object)   # a string column is made categorical first
    sc.pp.regress_out(b, "bulk_labels")
    assert np.array_equal(a.X, b.X) and isinstance(b.obs["bulk_labels"].dtype, pd.CategoricalDtype)


@pytest.mark.parametrize("fmt", ["csr", "csc", "dense"])
def test_equals_the_restatement(fmt):
    a = _adata(fmt=fmt)
    dense = _dense(a.X).astype(np.float64)
    keys = ["n_counts", "percent_mito"]
    out = sc.pp.regress_out(a, keys, copy=True, n_jobs=8)
    want = R.ref_numeric(dense, a.obs[keys].to_numpy(dtype=np.float64), keep_constant=False)
    R.assert_residual_close(out.X, want, np.abs(dense).max(axis=0), fmt)
    out = sc.pp.regress_out(a, "batch", copy=True)
    want = R.ref_categorical(dense, a.obs["batch"].cat.codes.to_numpy(), 3)
    R.assert_residual_close(out.X, want, np.abs(dense).max(axis=0), fmt)


@pytest.mark.parametrize(("dtype", "out_dtype"), [(np.int64, np.float64), (np.int32, np.float32), (np.float32, np.float32),
                                                  (np.uint16, np.float32)])
def test_layer_equals_x_and_dtype_rules(dtype, out_dtype):
    """`test_regress_out_layer`: the layer route gives what the X route gives; `_simple.py:603-609` for the dtypes"""
    a = _adata(dtype=dtype)
    a.layers["counts"] = a.X.copy()
    keys = ["n_counts", "percent_mito"]
    single = sc.pp.regress_out(a, keys, n_jobs=1, copy=True)
    layer = sc.pp.regress_out(a, keys, layer="counts", copy=True)
    assert single.X.dtype == out_dtype and single.X.shape == a.X.shape and isinstance(single.X, np.ndarray)
    assert np.array_equal(single.X, layer.layers["counts"])
    assert (layer.X != a.X).nnz == 0 and (single.layers["counts"] != a.X).nnz == 0   # the other representation is left alone


def test_categorical_and_singular_routes_return_float64():
    a = _adata()
    assert sc.pp.regress_out(a, "batch", copy=True).X.dtype == np.float64
    a.obs["const"] = 3.0
    seen = set()
    for keys in (["const"], ["const", "percent_mito"], ["percent_mito"]):
        design = np.c_[np.ones(a.n_obs), a.obs[keys].to_numpy()]
        singular = bool(np.linalg.det(design.T @ design) == 0)   # the reference's own test (`_simple.py:600`), rounding included
        seen.add(singular)
        out = sc.pp.regress_out(a, keys, copy=True)
        assert out.X.dtype == (np.float64 if singular else np.float32), keys
        dense = _dense(a.X).astype(np.float64)
        want = R.ref_numeric(dense, a.obs[keys].to_numpy(dtype=np.float64), keep_constant=singular)
        R.assert_residual_close(out.X, want, np.abs(dense).max(axis=0), str(keys))
    assert seen == {True, False}


def test_view_is_made_actual():
    """`test_regress_out_view`"""
    a = _adata(n=200, g=60)
    sub = a[:, :50]
    sub_copy = sub.copy()
    with pytest.warns(UserWarning, match=r"Received a view"):
        sc.pp.regress_out(sub, ["n_counts", "percent_mito"])
    sc.pp.regress_out(sub_copy, ["n_counts", "percent_mito"])
    assert not sub.is_view and np.array_equal(sub.X, sub_copy.X) and sub.X.shape == (200, 50)


def test_constant_columns_with_a_singular_design_come_back_equal():
    """`test_regress_out_constants`: n_counts is constant, so the design is singular and the GLM route keeps constant genes"""
    rng = np.random.default_rng(0)
    x = np.hstack((np.full((10, 1), 0.0), np.full((10, 1), 1.0))).astype(np.float32)
    a = sc.AnnData(x.copy())
    a.obs["percent_mito"] = rng.random(10)
    a.obs["n_counts"] = x.sum(axis=1)
    sc.pp.regress_out(a, ["n_counts", "percent_mito"])
    assert a.X.dtype == np.float64 and np.array_equal(a.X, x)


def test_zero_padded_columns_do_not_change_the_others():
    """`test_regress_out_constants_equivalent`"""
    rng = np.random.default_rng(1)
    cat = rng.integers(0, 3, 100)
    x = (rng.normal(size=(100, 20)) + cat[:, None]).astype(np.float32)
    a = sc.AnnData(np.hstack([x, np.zeros((100, 5), np.float32)]))
    b = sc.AnnData(x.copy())
    a.obs["cat"] = pd.Categorical(cat)
    b.obs["cat"] = pd.Categorical(cat)
    sc.pp.regress_out(a, "cat")
    sc.pp.regress_out(b, "cat")
    assert np.array_equal(a.X[:, :20], b.X) and np.array_equal(a.X[:, 20:], np.zeros((100, 5)))


def test_unused_category_is_allowed():
    a = _adata()
    a.obs["batch"] = pd.Categorical(a.obs["batch"].to_numpy(), categories=[1, 2, 3, 99])
    b = _adata()
    sc.pp.regress_out(a, "batch")
    sc.pp.regress_out(b, "batch")
    assert np.array_equal(a.X, b.X)


def test_copy_leaves_the_input_alone_and_in_place_returns_none():
    a = _adata()
    stored = a.X.copy()
    out = sc.pp.regress_out(a, "percent_mito", copy=True)
    assert out is not a and (a.X != stored).nnz == 0 and sparse.issparse(a.X) and isinstance(out.X, np.ndarray)
    assert sc.pp.regress_out(a, "percent_mito") is None and np.array_equal(a.X, out.X)


def test_all_keys_constant_removes_the_mean_only():
    """r = 0: span[1, keys] = span[1]"""
    a = _adata(fmt="dense")
    a.obs["c1"], a.obs["c2"] = 4.0, -1.5
    dense = a.X.astype(np.float64)
    out = sc.pp.regress_out(a, ["c1", "c2"], copy=True)
    assert _regress_out._numeric_basis(a.obs[["c1", "c2"]].to_numpy(dtype=np.float64)).shape == (a.n_obs, 0)
    const = R.constant_genes(dense)
    want = np.where(const[None, :], dense, dense - dense.mean(axis=0))   # (singular design: constant genes are kept)
    R.assert_residual_close(out.X, want, np.abs(dense).max(axis=0))


def test_empty_keys_mean_all_of_obs():
    a = _adata()
    del a.obs["batch"]
    b = a.copy()
    sc.pp.regress_out(a, [])
    sc.pp.regress_out(b, ["percent_mito", "n_counts"])
    assert np.array_equal(a.X, b.X)


def test_two_keys_with_a_categorical_first_is_the_references_error():
    a = _adata()
    with pytest.raises(ValueError) as e:
        sc.pp.regress_out(a, ["batch", "percent_mito"])
    assert str(e.value) == ("If providing categorical variable, only a single one is allowed. For this one we regress on the mean "
                            "for each category.")


def test_refusals():
    a = _adata()
    a.obs["holes"] = pd.Categorical(np.where(np.arange(a.n_obs) % 7 == 0, None, "x"))
    with pytest.raises(NotImplementedError, match="missing values"):
        sc.pp.regress_out(a, "holes")
    a.obs["inf"] = a.obs["percent_mito"].to_numpy()
    a.obs.loc[a.obs.index[3], "inf"] = np.inf
    a.obs["nan"] = a.obs["percent_mito"].to_numpy()
    a.obs.loc[a.obs.index[5], "nan"] = np.nan
    for key in ("inf", "nan"):
        with pytest.raises(ValueError, match="non-finite"):
            sc.pp.regress_out(a, ["percent_mito", key])
    for i in range(17):
        a.obs[f"k{i}"] = np.random.default_rng(i).random(a.n_obs)
    with pytest.raises(NotImplementedError, match="at most 16"):
        sc.pp.regress_out(a, [f"k{i}" for i in range(17)])
    sc.pp.regress_out(a, [f"k{i}" for i in range(16)], copy=True)   # 16 are served

    class Backed:
        is_backed, shape, dtype = True, a.X.shape, np.float32

    b = _adata()
    b.layers["disk"] = Backed()
    with pytest.raises(NotImplementedError, match="needs the matrix in memory"):
        sc.pp.regress_out(b, "percent_mito", layer="disk")
    c = _adata(dtype=np.float64)
    with pytest.raises(NotImplementedError, match="computes in float32"):
        sc.pp.regress_out(c, "percent_mito")
    d = _adata()
    d.X.data[7] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        sc.pp.regress_out(d, "percent_mito")


def test_no_warning_the_reference_does_not_emit():
    a = _adata()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sc.pp.regress_out(a, ["n_counts", "percent_mito"])
        sc.pp.regress_out(_adata(), "batch")
