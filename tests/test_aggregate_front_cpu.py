"""Host logic of `sc.get.aggregate` on a CPU stand-in for the device passes (tests/aggregate_cases.CpuStubAggregateBackend: numpy
in extended precision behind the backend's interface): the reference's behavioural tests (tests/test_aggregated.py of the
reference) restated -- the worked examples, `test_nan`, `test_factors`, the `_combine_categories` cases, the comparison with a
pandas groupby on the committed pbmc68k fixture -- and the routes, dtype rules, errors and refusals of this package.  The same
front end runs on the HIP kernels in tests/test_gpu_aggregate.py."""
from __future__ import annotations

import sys
import warnings
from itertools import product
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import aggregate_cases as A  # noqa: E402

import scanpy_amd as sc  # noqa: E402
from scanpy_amd import _get_aggregate as G  # noqa: E402

FUNCS = ("sum", "mean", "var", "count_nonzero", "median")


@pytest.fixture(autouse=True)
def stub(monkeypatch):
    be = A.CpuStubAggregateBackend()
    monkeypatch.setattr(G, "default_backend", lambda: be)
    return be


def _block():
    x = np.block([[np.ones((2, 2)), np.zeros((2, 2))], [np.zeros((2, 2)), np.ones((2, 2))]])
    obs = pd.DataFrame({"a": ["a", "a", "b", "b"], "b": ["c", "d", "d", "d"]}, index=["a_c", "a_d", "b_d1", "b_d2"])
    return sc.AnnData(x, obs=obs, var=pd.DataFrame(index=[f"gene_{i}" for i in range(4)]))


def test_worked_example_block_matrix():
    res = sc.get.aggregate(_block(), by=["a", "b"], func=["sum", "mean", "count_nonzero"])
    assert res.obs.index.tolist() == ["a_c", "a_d", "b_d"] and res.var.index.tolist() == [f"gene_{i}" for i in range(4)]
    assert res.obs["n_obs_aggregated"].tolist() == [1, 1, 2]
    assert res.obs["a"].tolist() == ["a", "a", "b"] and res.obs["b"].tolist() == ["c", "d", "d"]
    assert isinstance(res.obs["a"].dtype, pd.CategoricalDtype) and isinstance(res.obs["b"].dtype, pd.CategoricalDtype)
    assert list(res.layers) == ["sum", "mean", "count_nonzero"]
    assert np.array_equal(res.layers["sum"], [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 2, 2]])
    assert np.array_equal(res.layers["mean"], [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1]])
    assert np.array_equal(res.layers["count_nonzero"], [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 2, 2]])
    assert res.shape == (3, 4)
    only = sc.get.aggregate(_block(), by=["a", "b"], func="mean")
    assert list(only.layers) == ["mean"] and np.array_equal(only.layers["mean"], res.layers["mean"])


def test_nan_in_a_key_drops_the_cell():
    x = np.arange(6) + np.arange(6)[:, None]
    obs = pd.DataFrame(dict(cell_type=[np.nan, np.nan, "B", "C", "B", "B"], sample_id=["s1", "s1", "s1", "s2", "s2", "s2"],
                            patient_type=[*(["responder"] * 3), *(["control"] * 3)]), index=[f"cell{i}" for i in range(6)])
    agg = sc.get.aggregate(sc.AnnData(x, obs=obs), by=["sample_id", "patient_type", "cell_type"], func="sum", layer=None)
    assert agg.obs.index.tolist() == ["s1_responder_B", "s2_control_B", "s2_control_C"]
    assert agg.obs["n_obs_aggregated"].tolist() == [1, 2, 1]
    assert np.array_equal(agg.layers["sum"], np.stack([x[2], x[4] + x[5], x[3]]))


def test_factors():
    obs = pd.DataFrame(product(range(5), repeat=4), columns=list("abcd"))
    obs.index = [f"cell_{i:04d}" for i in range(obs.shape[0])]
    adata = sc.AnnData(np.arange(obs.shape[0]).reshape(-1, 1), obs=obs)
    res = sc.get.aggregate(adata, by=["a", "b", "c", "d"], func="sum")
    np.testing.assert_equal(res.layers["sum"], adata.X)
    assert res.layers["sum"].dtype == np.float64     # a dense integer matrix: the reference's matrix product gives float64


@pytest.mark.parametrize(("label_cols", "expected"), [
    (dict(a=["a", "b", "c"], b=["d", "d", "f"], c=["g", "h", "h"]), ["a_d_g", "b_d_h", "c_f_h"]),
    (dict(a=["a", "b", "c"], b=["d", "d", "f"]), ["a_d", "b_d", "c_f"]),
    (dict(a=["a", "b", "c"], c=["g", "h", "h"]), ["a_g", "b_h", "c_h"]),
    (dict(b=["d", "d", "f"], c=["g", "h", "h"]), ["d_g", "d_h", "f_h"]),
], ids=["three", "two-1", "two-2", "two-3"])
def test_combine_categories(label_cols, expected):
    label_df = pd.DataFrame({k: pd.Categorical(v) for k, v in label_cols.items()})
    result, table = G._combine_categories(label_df)
    assert isinstance(result, pd.Categorical)
    pd.testing.assert_extension_array_equal(result, pd.Categorical(expected))
    pd.testing.assert_index_equal(pd.Index(result), table.index.astype("category"))
    rebuilt = pd.DataFrame([x.split("_") for x in result], columns=list(label_cols), index=result.astype(str)).astype("category")
    pd.testing.assert_frame_equal(rebuilt, table)


def _small(n=60, g=7, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.poisson(0.8, size=(n, g)).astype(np.float32) * rng.choice([-1.0, 1.0, 1.0], size=(n, g)).astype(np.float32)
    obs = pd.DataFrame({"grp": pd.Categorical(rng.choice(list("abcd"), n)), "keep": rng.random(n) < 0.7,
                        "num": rng.normal(size=n)}, index=[f"c{i}" for i in range(n)])
    var = pd.DataFrame({"vg": pd.Categorical(rng.choice(list("xyz"), g))}, index=[f"g{i}" for i in range(g)])
    return sc.AnnData(x, obs=obs, var=var)


def test_mask_by_array_and_by_name_and_its_errors():
    a = _small()
    by_name = sc.get.aggregate(a, "grp", FUNCS, mask="keep")
    by_array = sc.get.aggregate(a, "grp", FUNCS, mask=a.obs["keep"].to_numpy())
    for f in FUNCS:
        assert by_name.layers[f].tobytes() == by_array.layers[f].tobytes(), f
    assert by_name.obs["n_obs_aggregated"].tolist() == a.obs[a.obs["keep"]].groupby("grp", observed=False).size().tolist()
    want = pd.DataFrame(a.X.astype(np.float64)[a.obs["keep"]]).groupby(a.obs["grp"][a.obs["keep"]].to_numpy()).sum()
    np.testing.assert_allclose(by_name.layers["sum"], want.to_numpy())
    with pytest.raises(ValueError, match=r"Did not find `adata.obs\['nope'\]`"):
        sc.get.aggregate(a, "grp", "sum", mask="nope")
    with pytest.raises(ValueError, match="The shape of the mask do not match the data"):
        sc.get.aggregate(a, "grp", "sum", mask=np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="Mask array must be boolean"):
        sc.get.aggregate(a, "grp", "sum", mask="num")
    # everything masked: sum 0, count 0, mean NaN, median NaN; dof = 0 gives var 0
    with pytest.warns(RuntimeWarning, match="Group counts matches dof"):
        none = sc.get.aggregate(a, "grp", FUNCS, mask=np.zeros(a.n_obs, dtype=bool))
    assert not none.layers["sum"].any() and not none.layers["count_nonzero"].any() and none.obs["n_obs_aggregated"].tolist() == [0] * 4
    assert np.isnan(none.layers["mean"]).all() and np.isnan(none.layers["median"]).all() and np.isnan(none.layers["var"]).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not sc.get.aggregate(a, "grp", "var", dof=0, mask=np.zeros(a.n_obs, dtype=bool)).layers["var"].any()


def test_layer_order_and_func_errors():
    a = _small()
    assert list(sc.get.aggregate(a, "grp", ["median", "var", "count_nonzero", "mean", "sum"]).layers) == \
        ["sum", "count_nonzero", "var", "mean", "median"]
    assert list(sc.get.aggregate(a, "grp", ("median", "mean", "sum")).layers) == ["sum", "mean", "median"]
    assert list(sc.get.aggregate(a, "grp", "var").layers) == ["var"]
    with pytest.raises(ValueError, match=r"func \{'mode'\} is not one of \{"):
        sc.get.aggregate(a, "grp", ["sum", "mode"])
    with pytest.raises(TypeError, match="not iterable"):
        sc.get.aggregate(a, 123, "sum")


def test_dof_warning_and_nans():
    x = np.array([1.0, 2.0, 3.0, 5.0]).reshape(-1, 1)
    obs = pd.DataFrame({"group": pd.Categorical(["a", "b", "a", "a"])}, index=list("wxyz"))
    for dof in (1, 4):
        with pytest.warns(RuntimeWarning, match=r"Group counts matches dof, resulting var for groups \[.*'b'\] will be nan") as rec:
            v = sc.get.aggregate(sc.AnnData(x, obs=obs), "group", "var", dof=dof).layers["var"]
        assert len(rec) == 1 and np.isnan(v[1, 0])
        assert np.isnan(v[0, 0]) if dof == 4 else v[0, 0] == np.var([1.0, 3.0, 5.0], ddof=1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v = sc.get.aggregate(sc.AnnData(x, obs=obs), "group", ["var", "mean"], dof=0).layers
    assert v["var"][1, 0] == 0.0 and v["var"][0, 0] == np.var([1.0, 3.0, 5.0]) and v["mean"][:, 0].tolist() == [3.0, 2.0]


def test_dtypes_per_route(stub):
    a = _small()
    x = a.X
    routes = {"dense f32": x, "dense f64": x.astype(np.float64), "dense i32": x.astype(np.int32), "csr f32": sparse.csr_matrix(x),
              "csc f32": sparse.csc_matrix(x), "coo f32": sparse.coo_matrix(x), "csr i64": sparse.csr_matrix(x.astype(np.int64)),
              "csr f64": sparse.csr_matrix(x.astype(np.float64))}
    base = None
    for name, m in routes.items():
        stub.calls.clear()
        res = sc.get.aggregate(sc.AnnData(m, obs=a.obs, var=a.var), "grp", FUNCS)
        lay = res.layers
        is_sparse, kind = sparse.issparse(m), m.dtype.kind
        assert lay["sum"].dtype == (np.int64 if is_sparse and kind == "i" else np.float64), name
        assert lay["count_nonzero"].dtype == (np.int64 if is_sparse else np.float64), name
        assert lay["mean"].dtype == np.float64 and lay["var"].dtype == np.float64, name
        assert lay["median"].dtype == (np.float32 if name == "dense f32" else np.float64), name
        assert stub.calls[0][0] == ("csr_from_transpose" if name == "csc f32" else "csr"), (name, stub.calls)
        assert stub.calls[-1] == ("aggregate", True, True, m.dtype == np.float32), (name, stub.calls)
        if base is None:
            base = lay
        for f in ("sum", "count_nonzero", "mean", "var"):
            np.testing.assert_array_equal(np.asarray(lay[f], dtype=np.float64), np.asarray(base[f], dtype=np.float64), err_msg=f"{name} {f}")
    # the even-size midpoint: float32 data form the sum in float32, integer and float64 data in float64
    pair = np.array([[2.0 ** 24 - 1], [2.0 ** 24]])
    obs = pd.DataFrame({"k": ["u", "u"]}, index=["p", "q"])
    assert sc.get.aggregate(sc.AnnData(pair.astype(np.int32), obs=obs), "k", "median").layers["median"][0, 0] == 2.0 ** 24 - 0.5
    assert sc.get.aggregate(sc.AnnData(sparse.csr_matrix(pair.astype(np.float32)), obs=obs), "k", "median").layers["median"][0, 0] \
        == np.float64((np.float32(2.0 ** 24 - 1) + np.float32(2.0 ** 24)) / np.float32(2))


def test_axis_and_data_sources():
    a = _small()
    rng = np.random.default_rng(3)
    a.layers["test"] = (a.X * 2).astype(np.float32)
    a.obsm["test"] = rng.integers(0, 5, size=(a.n_obs, 3)).astype(np.float32)
    a.obsm["frame"] = pd.DataFrame(a.obsm["test"], index=a.obs.index, columns=["u", "v", "w"])
    a.varm["test"] = rng.integers(0, 5, size=(a.n_vars, 2)).astype(np.float32)
    for kwargs, match in ((dict(layer="test", obsm="test"), r"Only one of `layer`, or `obsm` can be specified\."),
                          (dict(layer="test", obsm="test", varm="test"), r"Only one of `layer`, `obsm`, or `varm` can be specified\."),
                          (dict(obsm="test", axis=1), r"`obsm` cannot be used when `dim` is `var`"),
                          (dict(varm="test", axis=0), r"`varm` cannot be used when `dim` is `obs`"),
                          (dict(axis="foo"), r"was 'foo'"), (dict(axis=2), r"was 2")):
        with pytest.raises(ValueError, match=match):
            sc.get.aggregate(a, by="grp", func="sum", **kwargs)
    for axis in (0, "obs", None):
        r = sc.get.aggregate(a, "grp", "sum", axis=axis)
        assert r.shape == (4, a.n_vars) and r.var is a.var and r.obs.index.tolist() == list("abcd")
    assert np.array_equal(sc.get.aggregate(a, "grp", "sum", layer="test").layers["sum"], 2 * sc.get.aggregate(a, "grp", "sum").layers["sum"])
    r = sc.get.aggregate(a, "grp", "sum", obsm="test")
    assert r.shape == (4, 3) and r.var.index.tolist() == ["0", "1", "2"]
    named = sc.get.aggregate(a, "grp", "sum", obsm="frame")
    assert named.var.index.tolist() == ["u", "v", "w"] and np.array_equal(named.layers["sum"], r.layers["sum"])
    # axis = 'var': the result is built in the transposed shape, and equals the obs-axis call on the transposed data
    t = sc.AnnData(np.ascontiguousarray(a.X.T), obs=a.var, var=a.obs, layers={"test": np.ascontiguousarray(a.layers["test"].T)})
    for axis in (1, "var"):
        for kw in ({}, {"layer": "test"}):
            r = sc.get.aggregate(a, "vg", FUNCS, axis=axis, **kw)
            want = sc.get.aggregate(t, "vg", FUNCS, **kw)
            assert r.shape == (a.n_obs, 3) and r.obs is a.obs and r.var.index.tolist() == list("xyz")
            assert r.var["n_obs_aggregated"].tolist() == want.obs["n_obs_aggregated"].tolist()
            for f in FUNCS:
                assert r.layers[f].shape == (a.n_obs, 3) and np.array_equal(r.layers[f], want.layers[f].T, equal_nan=True), (axis, kw, f)
    for m in (sparse.csr_matrix(a.X), sparse.csc_matrix(a.X)):
        r = sc.get.aggregate(sc.AnnData(m, obs=a.obs, var=a.var), "vg", "sum", axis="var")
        assert np.array_equal(r.layers["sum"], sc.get.aggregate(a, "vg", "sum", axis=1).layers["sum"])
    r = sc.get.aggregate(a, "vg", "sum", varm="test")       # axis=None with varm: 'var'
    assert r.shape == (2, 3) and r.obs.index.tolist() == ["0", "1"] and r.var.index.tolist() == list("xyz")
    assert np.array_equal(r.layers["sum"], sc.get.aggregate(a, "vg", "sum", varm="test", axis="var").layers["sum"])


def test_every_refusal():
    a = _small()

    def with_x(m):
        return sc.AnnData(m, obs=a.obs, var=a.var)

    with pytest.raises(NotImplementedError, match="only implemented for AnnData input"):
        sc.get.aggregate(a.X, a.obs["grp"], "sum")
    with pytest.raises(NotImplementedError, match="float64 values that float32 does not hold exactly"):
        sc.get.aggregate(with_x(a.X.astype(np.float64) + 1e-9), "grp", "sum")
    with pytest.raises(NotImplementedError, match=r"beyond 2\^24"):
        sc.get.aggregate(with_x(sparse.csr_matrix(a.X.astype(np.int64) * (2 ** 24 + 1))), "grp", "sum")
    with pytest.raises(NotImplementedError, match="anndata.acc"):
        sc.get.aggregate(a, "grp", "sum", acc="X")
    AdRef = type("AdRef", (), dict(__module__="anndata.acc"))
    with pytest.raises(NotImplementedError, match="anndata.acc"):
        sc.get.aggregate(a, AdRef(), "sum")
    with pytest.raises(NotImplementedError, match="anndata.acc"):
        sc.get.aggregate(a, ["grp", AdRef()], "sum")

    class Backed:
        is_backed, shape, T = True, a.X.shape, None

    with pytest.raises(NotImplementedError, match="backed"):
        sc.get.aggregate(with_x(Backed()), "grp", "sum")
    Dask = type("Array", (), dict(__module__="dask.array.core", shape=a.X.shape, T=None))
    b = with_x(a.X)
    b.layers["lazy"] = Dask()
    with pytest.raises(NotImplementedError, match="dask"):
        sc.get.aggregate(b, "grp", "sum", layer="lazy")
    for bad in (np.nan, np.inf):
        x = a.X.copy()
        x[3, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            sc.get.aggregate(with_x(x), "grp", "sum")
        x[3, 2] = 0
        masked = np.ones(a.n_obs, dtype=bool)
        masked[3] = False
        x[3, 2] = bad       # a row that takes no part may hold anything
        sc.get.aggregate(with_x(x), "grp", "sum", mask=masked)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's test_aggregate_vs_pandas on the committed pbmc68k fixture (shared with tests/test_gpu_aggregate.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["raw_csr", "raw_csc", "dense_X"])
@pytest.mark.parametrize("use_mask", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("with_na", [True, False], ids=["na", "no_na"])
def test_pbmc68k_against_pandas(pbmc68k, source, use_mask, with_na):
    A.front_vs_pandas(pbmc68k, source, use_mask, with_na)
