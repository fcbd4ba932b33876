"""Host logic of scanpy_amd.metrics.morans_i / gearys_c on a CPU stand-in for the device passes
(tests/autocorr_cases.CpuStubAutocorrBackend: float64 numpy), and `sc.metrics.confusion_matrix` (host only): the reference's
behavioural tests (tests/test_metrics.py:41-248 of the reference) restated on the committed pbmc68k fixture, the routes by which
values reach a slab, the dtype rules, the errors and the refusals.  The same front end runs on the HIP kernels in
tests/test_gpu_autocorr.py."""
from __future__ import annotations

import sys
import warnings
from pathlib import Path
from string import ascii_letters

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import autocorr_cases as A  # noqa: E402

import scanpy_amd as sc  # noqa: E402
from scanpy_amd.metrics import _autocorr  # noqa: E402

METRICS = [sc.metrics.morans_i, sc.metrics.gearys_c]


@pytest.fixture(autouse=True)
def stub(monkeypatch):
    be = A.CpuStubAutocorrBackend()
    monkeypatch.setattr(_autocorr, "default_backend", lambda: be)
    return be


@pytest.fixture(params=METRICS, ids=["morans_i", "gearys_c"])
def metric(request):
    return request.param


def _graph(n=40, seed=0, dtype=np.float64):
    g = sparse.random(n, n, density=0.2, format="csr", random_state=seed, dtype=np.float64)
    return g.astype(dtype)


def test_exported():
    assert {"morans_i", "gearys_c", "confusion_matrix", "modularity"} <= set(sc.metrics.__all__)
    assert sc.metrics.morans_i is _autocorr.morans_i and sc.metrics.gearys_c is _autocorr.gearys_c


def test_consistency(metric, pbmc68k, stub):
    A.front_consistency(metric, pbmc68k)
    # X_pca travels as float32 and is read in place: one upload of the whole array, ld = 50, float64 graph weights
    assert ("dense_cell_major", "float32", (700, 50)) in stub.calls and ("stats", "float32", "float64", 50, 50, 0) in stub.calls


def test_raw_matrix_inputs_agree_bit_for_bit(metric, pbmc68k, stub):
    A.front_raw_matrix(metric, pbmc68k)
    kinds = {c[0] for c in stub.calls}
    assert {"csr_cell_major", "csr_feature_major", "rows_slab", "dense_cell_major"} <= kinds
    assert ("stats", "float32", "float64", 64, 61, 0) in stub.calls   # 765 = 11 * 64 + 61: the partial last slab


def test_two_cells_and_the_reference_blocks():
    """worked by hand: I == -1.0, C == 1.0; the reference's test_correctness: C == 0.0 exactly (also for a 1 x n sparse `vals`),
    |I - 1| <= 1e-14"""
    (indptr, indices, w), x = A.two_cells()
    g = sparse.csr_matrix((w, indices, indptr), shape=(2, 2))
    assert sc.metrics.morans_i(g, x) == -1.0 and sc.metrics.gearys_c(g, x) == 1.0
    g, x = A.block_graph(30)
    assert sc.metrics.gearys_c(g, x) == 0.0
    via_sparse = sc.metrics.gearys_c(g, sparse.csr_matrix(x))
    assert via_sparse.shape == (1,) and via_sparse[0] == 0.0
    g, x = A.block_graph(50)
    assert abs(sc.metrics.morans_i(g, x) - 1.0) <= 1e-14


@pytest.mark.parametrize("how", ["use_graph", "neighbors_key", "default"])
def test_graph_params(metric, how):
    """`test_metrics_graph_params`: the graph from `obsp[use_graph]`, or from the connectivities of a neighbors entry"""
    rng = np.random.default_rng(0)
    g = _graph(10)
    want = metric(g, rng.normal(size=(20, 10)).astype(np.float64))
    x = np.random.default_rng(0).normal(size=(20, 10)).T.copy()
    if how == "use_graph":
        a, kw = sc.AnnData(x, obsp={"foo_connectivities": g}), dict(use_graph="foo_connectivities")
    elif how == "neighbors_key":
        a = sc.AnnData(x, obsp={"bar_connectivities": g},
                       uns={"bar": {"connectivities_key": "bar_connectivities", "distances_key": "bar_distances"}})
        kw = dict(neighbors_key="bar")
    else:
        a, kw = sc.AnnData(x, obsp={"connectivities": g}, uns={"neighbors": {}}), {}
    assert metric(a, **kw).tobytes() == want.tobytes()


@pytest.mark.parametrize(("params", "err_cls", "pattern"), [
    pytest.param(dict(use_graph="foo", neighbors_key="bar"), TypeError, r"both", id="both"),
    pytest.param(dict(use_graph="foo"), KeyError, r"foo", id="no_graph"),
    pytest.param(dict(neighbors_key="bar"), KeyError, r"bar", id="no_key"),
    pytest.param({}, KeyError, r"neighbors.*uns", id="nothing"),
])
def test_graph_params_errors(metric, params, err_cls, pattern):
    adata = sc.AnnData(np.zeros((10, 20), dtype=np.float32))
    with pytest.raises(err_cls, match=pattern):
        metric(adata, **params)
    with pytest.raises(TypeError, match="Cannot specify both `use_graph` and `neighbors_key`."):
        metric(adata, use_graph="foo", neighbors_key="bar")


def test_other_argument_errors(metric):
    g = _graph(10)
    with pytest.raises(ValueError, match="square"):
        metric(sparse.random(10, 12, density=0.3, format="csr"), np.zeros(10))
    with pytest.raises(ValueError, match="cells"):
        metric(g, np.zeros(11))
    with pytest.raises(TypeError):
        metric(g.toarray(), np.zeros(10))
    with pytest.raises(TypeError):
        metric(g)
    with pytest.raises(TypeError):
        metric(g, np.array(["a"] * 10))
    a = sc.AnnData(np.zeros((10, 3), dtype=np.float32), obsp={"connectivities": g}, uns={"neighbors": {}}, obsm={"X_pca": np.zeros((10, 2))})
    with pytest.raises(ValueError, match="Only one of"):
        metric(a, layer="raw", obsm="X_pca")
    with pytest.raises(ValueError, match="Must run neighbors first"):
        metric(sc.AnnData(np.zeros((10, 3), dtype=np.float32), uns={"neighbors": {}}))


def test_dtype_rules(metric, stub):
    """float32 and integers of at most 16 bits travel as float32, float64 and wider integers as float64; sparse float64 travels
    as float32 when the cast is exact and is densified on the host in float64 when it is not; the graph keeps float32 weights
    and turns every other dtype into float64"""
    g = _graph(50)
    rng = np.random.default_rng(1)
    base = np.round(rng.normal(size=(3, 50)) * 100)

    def travelled(vals, graph=g):
        stub.calls.clear()
        out = metric(graph, vals)
        return out, {(c[1], c[2]) for c in stub.calls if c[0] == "stats"}

    want, seen = travelled(base)
    assert seen == {("float64", "float64")}
    for dt, tag in ((np.float32, "float32"), (np.int8, "float32"), (np.uint16, "float32"), (np.int16, "float32"), (np.float16, "float32"),
                    (np.int32, "float64"), (np.int64, "float64")):
        vals = (base % 100).astype(dt)
        out, seen = travelled(vals)
        assert seen == {(tag, "float64")}, dt
        A.assert_close(out, travelled(vals.astype(np.float64))[0], dt)
    _, seen = travelled(base, g.astype(np.float32))
    assert seen == {("float64", "float32")}
    _, seen = travelled(base, g.astype(np.int32))
    assert seen == {("float64", "float64")}
    # sparse float64: integers are exact in float32 ...
    sp = sparse.csr_matrix(np.where(rng.random((3, 50)) < 0.5, base, 0.0))
    out, seen = travelled(sp)
    assert seen == {("float32", "float64")} and ("csr_feature_major", "float64") in stub.calls
    A.assert_close(out, travelled(sp.toarray())[0])
    # ... thirds are not: the host densifies in float64, and nothing is rounded
    sp3 = sp / 3.0
    out, seen = travelled(sp3.tocsc())
    assert seen == {("float64", "float64")} and not any(c[0].startswith("csr_") for c in stub.calls)
    assert out.tobytes() == travelled(sp3.toarray())[0].tobytes()
    # offset values: centring in float32 would lose them
    off = 1000.0 + rng.normal(size=(2, 50))
    A.assert_close(metric(g, off), A.restate_metric(metric, g, off.T))


def test_wide_cell_major_input_is_uploaded_slab_by_slab(metric, stub):
    """up to 128 features a cell-major array is read in place; beyond, 64 columns at a time"""
    g = _graph(30)
    rng = np.random.default_rng(2)
    for m, in_place in ((128, True), (129, False)):
        cells = rng.normal(size=(30, m))
        stub.calls.clear()
        out = metric(g, cells.T)
        ups = [c for c in stub.calls if c[0] == "dense_cell_major"]
        assert ([u[2] for u in ups] == [(30, m)]) if in_place else ([u[2] for u in ups] == [(30, 64), (30, 64), (30, 1)])
        assert out.tobytes() == metric(g, np.ascontiguousarray(cells.T)).tobytes()


def test_constant_features(metric, pbmc68k):
    """`test_graph_metrics_w_constant_values`: rows that are all zero (nothing stored), all explicit zeros and all 42 return NaN
    at exactly those positions with ONE warning that counts them; the other features keep their bits"""
    g = pbmc68k["connectivities"]
    x_t = pbmc68k["raw_X"].T.tocsr()[:200].copy()
    const = np.random.default_rng(3).choice(200, 10, replace=False)
    full = metric(g, x_t)
    assert not np.isnan(full).any()
    dense = x_t.toarray()
    zero, fortytwo = dense.copy(), dense.copy()
    zero[const], fortytwo[const] = 0.0, 42.0
    explicit = sparse.csr_matrix(zero)
    lil = explicit.tolil()
    lil[const[:5], 3] = 1.0
    explicit = lil.tocsr()
    explicit.data[np.isin(A.coo_rows(explicit.indptr), const[:5])] = 0.0   # stored zeros
    assert explicit.nnz > sparse.csr_matrix(zero).nnz
    other = ~np.isin(np.arange(200), const)
    for vals in (zero, sparse.csr_matrix(zero), sparse.coo_matrix(zero), explicit, fortytwo, sparse.csc_matrix(fortytwo)):
        with pytest.warns(UserWarning, match=r"10 variables were constant, will return nan for these") as rec:
            out = metric(g, vals)
        assert len(rec) == 1
        assert np.isnan(out[const]).all() and out[other].tobytes() == full[other].tobytes()
    # 1-D: NaN without a warning; n = 1: NaN
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.isnan(metric(g, np.full(700, 42.0)))
        assert np.isnan(metric(sparse.csr_matrix(np.ones((1, 1))), np.array([3.0])))
    with pytest.warns(UserWarning, match=r"2 variables were constant"):
        assert np.isnan(metric(sparse.csr_matrix(np.ones((1, 1))), np.array([[3.0], [4.0]]))).all()


def test_nonfinite_values_and_weightless_graphs(metric):
    g = _graph(60)
    rng = np.random.default_rng(4)
    vals = rng.normal(size=(5, 60))
    clean = metric(g, vals)
    dirty = vals.copy()
    dirty[1, 7], dirty[3, 9] = np.nan, -np.inf
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # not constant: no warning
        out = metric(g, dirty)
    assert np.isnan(out[[1, 3]]).all() and out[[0, 2, 4]].tobytes() == clean[[0, 2, 4]].tobytes()
    # W_sum == 0: what IEEE division gives, no exception
    empty = sparse.csr_matrix((60, 60))
    out = metric(empty, vals)
    assert out.shape == (5,) and np.isnan(out).all()                       # n / 0 * 0 / z2
    cancel = sparse.csr_matrix((np.array([1.0, -1.0]), (np.array([0, 5]), np.array([1, 6]))), shape=(60, 60))
    assert not np.isfinite(metric(cancel, vals)).any()


def test_refusals(metric):
    g = _graph(10)

    class Backed:
        is_backed = True
        shape = (3, 10)
        ndim = 2

    fake_dask = type("Array", (), {"shape": (3, 10), "ndim": 2})
    fake_dask.__module__ = "dask.array.core"
    for bad in (Backed(), fake_dask()):
        with pytest.raises(NotImplementedError):
            metric(g, bad)
        with pytest.raises(NotImplementedError):
            metric(bad, np.zeros(10))
    with pytest.raises(NotImplementedError, match="2\\^31"):
        metric(sparse.coo_matrix((2 ** 31, 2 ** 31)), np.zeros(3))
    a = sc.AnnData(np.zeros((10, 3), dtype=np.float32), obsp={"connectivities": g}, uns={"neighbors": {}})
    a.X = Backed()
    with pytest.raises(NotImplementedError, match="backed"):
        metric(a)


# ---- confusion_matrix (tests/test_metrics.py:191-248 of the reference, restated) ---------------------------------------
def test_confusion_matrix():
    mtx = sc.metrics.confusion_matrix(["a", "b"], ["c", "d"], normalize=False)
    assert mtx.loc["a", "c"] == 1 and mtx.loc["a", "d"] == 0 and mtx.loc["b", "d"] == 1 and mtx.loc["b", "c"] == 0
    mtx = sc.metrics.confusion_matrix(["a", "b"], ["c", "d"], normalize=True)
    assert mtx.loc["a", "c"] == 1.0 and mtx.loc["a", "d"] == 0.0 and mtx.loc["b", "d"] == 1.0 and mtx.loc["b", "c"] == 0.0
    mtx = sc.metrics.confusion_matrix(["a", "a", "b", "b"], ["c", "d", "c", "d"], normalize=True)
    assert np.all(mtx == 0.5)
    assert mtx.index.name == "Original labels" and mtx.columns.name == "New Labels"
    assert list(mtx.index) == ["a", "b"] and list(mtx.columns) == ["c", "d"]


def test_confusion_matrix_randomized():
    rng = np.random.default_rng(0)
    chars = np.array(list(ascii_letters))
    pos = rng.choice(len(chars), size=120)
    a = chars[pos]
    b = rng.permutation(chars)[pos]
    df = pd.DataFrame({"a": a, "b": b})
    pd.testing.assert_frame_equal(sc.metrics.confusion_matrix("a", "b", df), sc.metrics.confusion_matrix(df["a"], df["b"]))
    pd.testing.assert_frame_equal(sc.metrics.confusion_matrix(df["a"].values, df["b"].values), sc.metrics.confusion_matrix(a, b))
    counts = sc.metrics.confusion_matrix(a, b, normalize=False)
    assert counts.to_numpy().sum() == 120 and (counts.to_numpy().sum(axis=1) == pd.Series(a).value_counts().loc[counts.index]).all()


def test_confusion_matrix_api():
    rng = np.random.default_rng(0)
    data = pd.DataFrame({"a": rng.integers(5, size=100), "b": rng.integers(5, size=100)})
    expected = sc.metrics.confusion_matrix(data["a"], data["b"])
    pd.testing.assert_frame_equal(expected, sc.metrics.confusion_matrix("a", "b", data))
    pd.testing.assert_frame_equal(expected, sc.metrics.confusion_matrix("a", data["b"], data))
    pd.testing.assert_frame_equal(expected, sc.metrics.confusion_matrix(data["a"], "b", data))
    assert np.allclose(expected.to_numpy().sum(axis=1), 1.0) and list(expected.index) == sorted(set(data["a"]))
    cat = pd.Series(pd.Categorical(["x", "y", "x"], categories=["y", "x"]))   # a categorical keeps the order of its categories
    assert list(sc.metrics.confusion_matrix(cat, ["p", "p", "q"]).index) == ["y", "x"]
