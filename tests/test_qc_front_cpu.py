"""Host logic of scanpy_amd.pp.calculate_qc_metrics / describe_obs / describe_var on a CPU stand-in for the device passes
(tests/qc_cases.CpuStubQcBackend: the numpy restatement of the primitives): column names, order and dtypes, arguments, errors,
matrix selection, write-back and streaming of a backed matrix.  The same front end runs on the HIP kernels in tests/test_gpu_qc.py."""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import qc_cases as Q  # noqa: E402

import scanpy_amd as sc  # noqa: E402
from scanpy_amd.preprocessing import _csr_device, _qc  # noqa: E402


@pytest.fixture(autouse=True)
def _stub(monkeypatch):
    monkeypatch.setattr(_csr_device, "default_backend", lambda: Q.CpuStubQcBackend())


def _counts(n=120, g=90, seed=0, density=0.3):
    x = sparse.random(n, g, density=density, format="csr", dtype=np.float32, random_state=seed)
    x.data = np.ceil(x.data * 30).astype(np.float32)
    x.data[::17] = 0.0   # stored zeros
    lil = x.tolil()
    lil[3] = 0           # an empty cell
    x = lil.tocsr()
    return x


def _adata(x=None, seed=0):
    x = _counts(seed=seed) if x is None else x
    a = sc.AnnData(x)
    rng = np.random.default_rng(seed)
    a.var["mt"] = rng.random(a.n_vars) < 0.2
    a.var["ribo"] = rng.random(a.n_vars) < 0.3
    return a


def _expected(a, x, **kw):
    qc_vars = kw.get("qc_vars", ())
    qc_vars = [qc_vars] if isinstance(qc_vars, str) else list(qc_vars)
    pt = kw.get("percent_top", (50,))
    masks = np.stack([a.var[v].to_numpy() for v in qc_vars]) if qc_vars else np.zeros((0, x.shape[1]), bool)
    prim = Q.ref_primitives(x, masks, pt)
    names = {k: kw[k] for k in ("expr_type", "var_type", "log1p") if k in kw}
    return Q.ref_columns(prim, x.dtype, x.shape[0], qc_vars=qc_vars, percent_top=pt, **names)


def test_exported():
    assert {"calculate_qc_metrics", "describe_obs", "describe_var"} <= set(sc.pp.__all__)
    assert sc.pp.calculate_qc_metrics is _qc.calculate_qc_metrics


def test_columns_names_order_and_dtypes():
    a = _adata()
    obs, var = sc.pp.calculate_qc_metrics(a, qc_vars=["mt", "ribo"], percent_top=(50, 10))
    assert list(obs.columns) == [
        "n_genes_by_counts", "log1p_n_genes_by_counts", "total_counts", "log1p_total_counts", "pct_counts_in_top_10_genes",
        "pct_counts_in_top_50_genes", "total_counts_mt", "log1p_total_counts_mt", "pct_counts_mt", "total_counts_ribo",
        "log1p_total_counts_ribo", "pct_counts_ribo"]
    assert list(var.columns) == ["n_cells_by_counts", "mean_counts", "log1p_mean_counts", "pct_dropout_by_counts", "total_counts",
                                 "log1p_total_counts"]
    assert obs.index.equals(a.obs_names) and var.index.equals(a.var_names)
    assert obs["n_genes_by_counts"].dtype == np.int64 and var["n_cells_by_counts"].dtype == np.int64
    assert obs["total_counts"].dtype == np.float32 and var["total_counts"].dtype == np.float32
    assert var["mean_counts"].dtype == np.float64 and obs["pct_counts_in_top_10_genes"].dtype == np.float64
    want_obs, want_var = _expected(a, a.X, qc_vars=["mt", "ribo"], percent_top=(50, 10))
    Q.assert_frames_equal_columns(obs, want_obs, "obs")
    Q.assert_frames_equal_columns(var, want_var, "var")
    assert "mt" not in obs.columns and list(a.obs.columns) == []   # inplace=False writes nothing


def test_other_names_and_no_log1p():
    a = _adata()
    kw = dict(expr_type="umis", var_type="features", qc_vars="mt", percent_top=[1], log1p=False)
    obs, var = sc.pp.calculate_qc_metrics(a, **kw)
    assert list(obs.columns) == ["n_features_by_umis", "total_umis", "pct_umis_in_top_1_features", "total_umis_mt", "pct_umis_mt"]
    assert list(var.columns) == ["n_cells_by_umis", "mean_umis", "pct_dropout_by_umis", "total_umis"]
    want_obs, want_var = _expected(a, a.X, **kw)
    Q.assert_frames_equal_columns(obs, want_obs)
    Q.assert_frames_equal_columns(var, want_var)


def test_qc_vars_as_string_and_as_list():
    a = _adata()
    o1, _ = sc.pp.calculate_qc_metrics(a, qc_vars="mt", percent_top=None)
    o2, _ = sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=None)
    assert o1.equals(o2) and "pct_counts_mt" in o1.columns


@pytest.mark.parametrize("percent_top", [None, (), []])
def test_no_top_columns(percent_top):
    obs, _ = sc.pp.calculate_qc_metrics(_adata(), percent_top=percent_top)
    assert not [c for c in obs.columns if "_in_top_" in c]


def test_positions_outside_the_features():
    a = _adata()
    for bad in ((0, 5), (5, a.n_vars + 1), (-1,)):
        with pytest.raises(IndexError, match="Positions outside range of features."):
            sc.pp.calculate_qc_metrics(a, percent_top=bad)
    obs, _ = sc.pp.calculate_qc_metrics(a, percent_top=[a.n_vars])   # the last position is inside
    total = obs["total_counts"].to_numpy()
    assert np.array_equal(obs[f"pct_counts_in_top_{a.n_vars}_genes"].to_numpy()[total > 0], np.full((total > 0).sum(), 100.0))


def test_parallel_warns():
    a = _adata()
    with pytest.warns(FutureWarning, match="Argument `parallel` is deprecated, and currently has no effect."):
        sc.pp.calculate_qc_metrics(a, percent_top=None, parallel=True)
    with pytest.warns(FutureWarning, match="`parallel` is deprecated"):
        sc.pp.describe_obs(a, percent_top=None, parallel=False)


def test_inplace_twice_overwrites_and_adds_nothing():
    a = _adata()
    obs, var = sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(20,))
    assert sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(20,), inplace=True) is None
    obs_cols, var_cols = list(a.obs.columns), list(a.var.columns)
    assert obs_cols == list(obs.columns) and var_cols == ["mt", "ribo", *var.columns]
    a.obs["total_counts"] = -1.0
    sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(20,), inplace=True)
    assert list(a.obs.columns) == obs_cols and list(a.var.columns) == var_cols
    for col in obs.columns:
        assert np.array_equal(a.obs[col].to_numpy(), obs[col].to_numpy(), equal_nan=True), col
    for col in var.columns:
        assert np.array_equal(a.var[col].to_numpy(), var[col].to_numpy(), equal_nan=True), col


def test_layer_and_use_raw_select_the_matrix():
    a = _adata()
    counts = a.X.copy()
    a.layers["counts"] = counts.copy()
    a.raw = sc.AnnData(counts.copy(), a.obs, a.var.copy())
    want = sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(20,))
    sc.pp.log1p(a)
    assert abs(a.X - counts).max() > 0
    changed = sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(20,))
    assert not changed[0]["total_counts"].equals(want[0]["total_counts"])
    for kw in (dict(layer="counts"), dict(use_raw=True)):
        got = sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(20,), **kw)
        assert got[0].equals(want[0]) and got[1].equals(want[1]), kw
    with pytest.raises(ValueError, match="Only one of `layer`, or `use_raw` can be specified."):
        sc.pp.calculate_qc_metrics(a, layer="counts", use_raw=True)
    a.raw = None
    with pytest.raises(AttributeError, match="'NoneType' object has no attribute 'X'"):
        sc.pp.calculate_qc_metrics(a, use_raw=True)
    with pytest.raises(KeyError):
        sc.pp.calculate_qc_metrics(a, layer="nope")


def test_describe_obs_and_var_together_equal_calculate():
    a = _adata()
    obs, var = sc.pp.calculate_qc_metrics(a, qc_vars=["mt", "ribo"], percent_top=(5, 50))
    assert sc.pp.describe_obs(a, qc_vars=["mt", "ribo"], percent_top=(5, 50)).equals(obs)
    assert sc.pp.describe_var(a).equals(var)
    assert sc.pp.describe_obs(a, qc_vars="mt", percent_top=None, inplace=True) is None and "pct_counts_mt" in a.obs.columns
    assert sc.pp.describe_var(a, inplace=True) is None and "pct_dropout_by_counts" in a.var.columns


def test_formats_and_integer_input_agree():
    x = _counts()
    base = _adata(x)
    want_obs, want_var = sc.pp.calculate_qc_metrics(base, qc_vars=["mt"], percent_top=(1, 20))
    for typ in (sparse.csc_matrix, lambda m: m.toarray(), sparse.csr_matrix):
        a = _adata(typ(x))
        obs, var = sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(1, 20))
        assert obs.equals(want_obs) and var.equals(want_var)
    a = _adata(x.astype(np.int32))
    obs, var = sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(1, 20))
    assert obs["total_counts"].dtype == np.int64 and var["total_counts"].dtype == np.int64 and obs["total_counts_mt"].dtype == np.int64
    want_i_obs, want_i_var = _expected(a, a.X, qc_vars=["mt"], percent_top=(1, 20))
    Q.assert_frames_equal_columns(obs, want_i_obs)
    Q.assert_frames_equal_columns(var, want_i_var)
    for col in want_obs.columns:   # the same numbers, whatever numpy's dtype for the formula
        np.testing.assert_allclose(obs[col].to_numpy().astype(np.float64), want_obs[col].to_numpy().astype(np.float64), rtol=1e-6,
                                   equal_nan=True, err_msg=col)
    assert (x != _counts()).nnz == 0   # the user's matrix is not rewritten


def test_empty_cells_give_nan_without_a_warning():
    a = _adata()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        obs, _ = sc.pp.calculate_qc_metrics(a, qc_vars=["mt"], percent_top=(1, 20))
    assert obs["total_counts"].iloc[3] == 0 and obs["n_genes_by_counts"].iloc[3] == 0
    for col in ("pct_counts_in_top_1_genes", "pct_counts_in_top_20_genes", "pct_counts_mt"):
        assert np.isnan(obs[col].iloc[3]) and not np.isnan(np.delete(obs[col].to_numpy(), 3)).any(), col


def test_stored_zeros_do_not_count():
    x = sparse.csr_matrix(np.array([[3, 0, 5, 0], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=np.float32))
    x.data[0] = 0.0   # the 3 becomes a stored zero
    a = sc.AnnData(x)
    obs, var = sc.pp.calculate_qc_metrics(a, percent_top=(1, 2))
    assert obs["n_genes_by_counts"].tolist() == [1, 0, 4] and var["n_cells_by_counts"].tolist() == [1, 1, 2, 1]
    assert obs["pct_counts_in_top_2_genes"].tolist()[::2] == [100.0, 50.0] and x.nnz == 6


def test_refusals():
    a = _adata(_counts().astype(np.float64))
    with pytest.raises(NotImplementedError, match="float32"):
        sc.pp.calculate_qc_metrics(a, percent_top=(5,))
    d = _counts().toarray()
    d[5, 7] = -2.0
    with pytest.raises(NotImplementedError, match="dense matrix with a negative entry"):
        sc.pp.calculate_qc_metrics(_adata(d), percent_top=(5,))
    sc.pp.calculate_qc_metrics(_adata(sparse.csr_matrix(d)), percent_top=(5,))   # CSR: the padded-multiset rule applies
    wide = sc.AnnData(sparse.random(6, 5000, density=0.01, format="csr", dtype=np.float32, random_state=1))
    with pytest.raises(NotImplementedError, match="at most 16 positions, each <= 4096"):
        sc.pp.calculate_qc_metrics(wide, percent_top=(4097,))
    with pytest.raises(NotImplementedError, match="at most 16 positions"):
        sc.pp.calculate_qc_metrics(wide, percent_top=tuple(range(1, 18)))
    many = _adata()
    names = []
    for k in range(33):
        many.var[f"v{k}"] = np.arange(many.n_vars) % (k + 2) == 0
        names.append(f"v{k}")
    with pytest.raises(NotImplementedError, match="at most 32"):
        sc.pp.calculate_qc_metrics(many, qc_vars=names, percent_top=None)
    obs, _ = sc.pp.calculate_qc_metrics(many, qc_vars=names[:32], percent_top=None)
    want, _ = _expected(many, many.X, qc_vars=names[:32], percent_top=None)
    Q.assert_frames_equal_columns(obs, want)


def test_no_cpu_fallback(monkeypatch):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scanpy_amd import _lib

    monkeypatch.setattr(_csr_device, "default_backend", lambda: _csr_device.GpuPPBackend())
    with pytest.raises(_lib.ScamdError, match="no CPU fallback"):
        sc.pp.calculate_qc_metrics(_adata(), percent_top=(5,))


@pytest.mark.parametrize("fmt", ["h5ad", "zarr"])
def test_backed_matrix_streams_in_chunks(tmp_path, monkeypatch, fmt):
    a = _adata(_counts(n=400, g=120, seed=3))
    if fmt == "h5ad":
        sc.write_h5ad(tmp_path / "a.h5ad", a)
        b = sc.read_h5ad(tmp_path / "a.h5ad", backed="r")
    else:
        sc.write_zarr(tmp_path / "a.zarr", a)
        b = sc.read_zarr(tmp_path / "a.zarr", backed="r")
    assert b.X.is_backed
    orig = _qc._StreamedQc.__init__
    seen = []

    def init(self, be, x, step=97):
        seen.append(step)
        orig(self, be, x, step)

    monkeypatch.setattr(_qc._StreamedQc, "__init__", init)
    kw = dict(qc_vars=["mt", "ribo"], percent_top=(1, 10, 100))
    want = sc.pp.calculate_qc_metrics(a, **kw)
    got = sc.pp.calculate_qc_metrics(b, **kw)
    assert seen == [97] and b.X.is_backed
    for g_, w_ in zip(got, want):
        assert list(g_.columns) == list(w_.columns)
        for col in w_.columns:
            assert g_[col].dtype == w_[col].dtype and g_[col].to_numpy().tobytes() == w_[col].to_numpy().tobytes(), col
    # pending transforms of the backed matrix run on every chunk
    sc.pp.normalize_total(a, target_sum=1e4)
    sc.pp.normalize_total(b, target_sum=1e4)
    o_a, v_a = sc.pp.calculate_qc_metrics(a, percent_top=(10,))
    o_b, v_b = sc.pp.calculate_qc_metrics(b, percent_top=(10,))
    assert b.X.is_backed and o_b["total_counts"].dtype == np.float32
    np.testing.assert_allclose(o_b["total_counts"].to_numpy(), o_a["total_counts"].to_numpy(), rtol=1e-6)
    np.testing.assert_allclose(v_b["mean_counts"].to_numpy(), v_a["mean_counts"].to_numpy(), rtol=1e-12)
