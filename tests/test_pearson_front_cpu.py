"""Host logic of `scanpy_amd.experimental.pp` on a CPU stand-in for the device passes (tests/pearson_cases.CpuStubPearsonBackend:
the float64 restatement; tests/stub_backend.CpuStubBackend for the data passes of `pp.pca`): the reference's
`test_pearson_residuals_general`, `_batch`, `_inputchecks`, the normalisation and the recipe tests
(tests/test_highly_variable_genes.py, tests/test_normalization.py of the reference) restated -- signatures, slots, dtypes,
messages, the ranking and the merge over batches, the first-batch clip rule, the refusals.  The `check_*` bodies run again on
the HIP kernels in tests/test_gpu_pearson.py."""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch
from scipy import sparse

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import pearson_cases as P  # noqa: E402

import scanpy_amd as sc  # noqa: E402
from scanpy_amd.preprocessing import _csr_device  # noqa: E402

N_OBS, N_VARS, N_TOP, SEED = 700, 300, 100, 0
# the selected set is compared with the restatement's: the relative gap in residual variance across the cut must exceed this
# (the derived bound of the kernel is below 1e-12 at this shape; the seed is picked so that the gap is far above it)
SET_RTOL = 1e-9


@pytest.fixture(autouse=True)
def _stub(monkeypatch):
    from stub_backend import CpuStubBackend

    from scanpy_amd import _device
    from scanpy_amd.preprocessing import _pca_solver

    monkeypatch.setattr(_csr_device, "default_backend", lambda: P.CpuStubPearsonBackend())
    monkeypatch.setattr(_device, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(_pca_solver, "GpuBackend", CpuStubBackend)


def counts(dtype=np.float32, fmt="csr", seed=SEED):
    """negative-binomial counts, 700 x 300: gene means over three decades, a third of the genes differ between two cell types"""
    rng = np.random.default_rng(seed)
    mean = 10.0 ** rng.uniform(-1.5, 1.0, N_VARS)
    kind = rng.integers(0, 2, N_OBS)
    fold = np.where(rng.random(N_VARS) < 0.33, 2.0 ** rng.normal(0, 1.5, N_VARS), 1.0)
    depth = rng.lognormal(0, 0.4, N_OBS)
    lam = depth[:, None] * mean[None, :] * np.where(kind[:, None] == 1, fold[None, :], 1.0)
    x = rng.poisson(lam * rng.gamma(5.0, 1 / 5.0, lam.shape))
    x[:, 0] = np.maximum(x[:, 0], 1)   # no cell with total 0
    x[3, 5] += 400                     # one residual far beyond sqrt(n) (cell 3 is of the second batch of `adata_of`)
    x = x.astype(dtype)
    return x if fmt == "dense" else (sparse.csr_matrix(x) if fmt == "csr" else sparse.csc_matrix(x))


def adata_of(x, batches=False):
    a = sc.AnnData(x)
    a.var.index = pd.Index([f"gene{j}" for j in range(x.shape[1])])
    if batches:
        a.obs["batch"] = np.where(np.arange(x.shape[0]) % 3 == 0, "b", "a")   # 'a': 466 cells (first in np.unique order), 'b': 234
    return a


def _dense(x):
    return x.toarray() if sparse.issparse(x) else np.asarray(x)


def restated_table(dense, theta, clip, batch=None):
    """the residual variances per batch by the restatement, with the reference's clip rule"""
    labels = np.zeros(len(dense), int) if batch is None else np.unique(batch, return_inverse=True)[1]
    if clip is None:
        clip = np.sqrt((labels == 0).sum())
    return np.array([P.restate_gene_var(dense, theta, clip, labels, b) for b in range(labels.max() + 1)])


def check_general(theta, clip, fmt="csr", dtype=np.float32):
    """`test_pearson_residuals_general`: columns, dtypes, order, counts, the rank bound, the selected set, X untouched"""
    x = counts(dtype, fmt)
    a = adata_of(x)
    before = _dense(a.X).copy()
    assert sc.experimental.pp.highly_variable_genes(a, theta=theta, clip=clip, n_top_genes=N_TOP) is None
    assert np.array_equal(_dense(a.X), before) and type(a.X) is type(x)
    assert a.uns["hvg"] == {"flavor": "pearson_residuals", "computed_on": "adata.X"}
    assert list(a.var.columns) == ["means", "variances", "residual_variances", "highly_variable_rank", "highly_variable"]
    assert a.var["highly_variable"].dtype == bool and a.var["highly_variable_rank"].dtype == np.float32
    for c in ("means", "variances", "residual_variances"):
        assert a.var[c].dtype == np.float64, c
    assert a.var["highly_variable"].sum() == N_TOP
    assert np.nanmax(a.var["highly_variable_rank"].to_numpy()) <= N_TOP - 1
    dense = before.astype(np.float64)
    assert np.allclose(a.var["means"], dense.mean(axis=0), rtol=1e-12) and np.allclose(a.var["variances"], dense.var(axis=0, ddof=1), rtol=1e-9)
    want = restated_table(dense, theta, clip)[0]
    order = np.sort(want)[::-1]
    gap = (order[N_TOP - 1] - order[N_TOP]) / order[N_TOP - 1]
    assert gap > SET_RTOL, ("pick another seed: the cut falls into a tie of the restatement", gap)
    assert np.allclose(a.var["residual_variances"], want, rtol=SET_RTOL, atol=0)
    assert set(np.flatnonzero(a.var["highly_variable"])) == set(np.argsort(-want)[:N_TOP])
    sel = a.var["highly_variable"].to_numpy()
    assert np.array_equal(np.sort(a.var["highly_variable_rank"].to_numpy()[sel]), np.arange(N_TOP))
    assert np.isnan(a.var["highly_variable_rank"].to_numpy()[~sel]).all()
    return a


def check_batch(theta=100, clip=None):
    """`test_pearson_residuals_batch`: the two extra columns, the mean over batches, and the reference's rule that clip=None
    is the FIRST batch's sqrt(n) for every batch"""
    x = counts()
    a = adata_of(x, batches=True)
    df = sc.experimental.pp.highly_variable_genes(a, theta=theta, clip=clip, n_top_genes=N_TOP, batch_key="batch", inplace=False)
    assert list(df.columns) == ["means", "variances", "residual_variances", "highly_variable_rank", "highly_variable_nbatches",
                                "highly_variable_intersection", "highly_variable"]
    assert df["highly_variable_nbatches"].dtype == np.int64 and df["highly_variable_intersection"].dtype == bool
    assert df["highly_variable"].sum() == N_TOP and np.nanmax(df["highly_variable_rank"].to_numpy()) <= N_TOP - 1
    dense = _dense(x).astype(np.float64)
    per_batch = restated_table(dense, theta, clip, a.obs["batch"].to_numpy())
    assert np.allclose(df["residual_variances"], per_batch.mean(axis=0), rtol=SET_RTOL, atol=0)
    if clip is None:   # with each batch's own sqrt(n) the second batch (234 cells) would be clipped lower
        labels = np.unique(a.obs["batch"].to_numpy(), return_inverse=True)[1]
        own = np.array([P.restate_gene_var(dense, theta, np.sqrt((labels == b).sum()), labels, b) for b in range(2)])
        assert not np.allclose(own.mean(axis=0), per_batch.mean(axis=0), rtol=1e-6, atol=0)
    ranks = np.argsort(np.argsort(-per_batch, axis=1), axis=1)
    nb = (ranks < N_TOP).sum(axis=0)
    assert np.array_equal(df["highly_variable_nbatches"].to_numpy(), nb)
    assert np.array_equal(df["highly_variable_intersection"].to_numpy(), nb == 2)
    assert df["highly_variable"].to_numpy()[nb == 2].all() and not df["highly_variable"].to_numpy()[nb == 0].any()
    b = adata_of(x, batches=True)
    sc.experimental.pp.highly_variable_genes(b, theta=theta, clip=clip, n_top_genes=N_TOP, batch_key="batch")
    assert list(b.var.columns) == ["means", "variances", "residual_variances", "highly_variable_rank", "highly_variable_nbatches",
                                   "highly_variable_intersection", "highly_variable"]
    assert np.array_equal(b.var["highly_variable"].to_numpy(), df["highly_variable"].to_numpy())


def check_subset_inplace_layer():
    x = counts()
    a = adata_of(x)
    df = sc.experimental.pp.highly_variable_genes(a, n_top_genes=N_TOP, inplace=False)
    assert list(df.columns) == ["means", "variances", "residual_variances", "highly_variable_rank", "highly_variable"]
    assert "highly_variable" not in a.var and "hvg" not in a.uns and list(df.index) == list(a.var_names)
    sub = sc.experimental.pp.highly_variable_genes(a, n_top_genes=N_TOP, inplace=False, subset=True)
    assert len(sub) == N_TOP and sub["highly_variable"].all() and list(sub.index) == list(df.index[df["highly_variable"]])
    b = adata_of(x)
    sc.experimental.pp.highly_variable_genes(b, n_top_genes=N_TOP, subset=True, chunksize=7)
    assert b.shape == (N_OBS, N_TOP) and list(b.var_names) == list(sub.index) and b.var["highly_variable"].all()
    c = adata_of(sparse.csr_matrix(x.shape, dtype=np.float32))
    c.layers["counts"] = x
    c.X = sparse.csr_matrix(np.ones(x.shape, dtype=np.float32))
    sc.experimental.pp.highly_variable_genes(c, n_top_genes=N_TOP, layer="counts")
    assert c.uns["hvg"]["computed_on"] == "counts"
    assert np.array_equal(c.var["highly_variable"].to_numpy(), df["highly_variable"].to_numpy())
    assert np.array_equal(c.var["residual_variances"].to_numpy(), df["residual_variances"].to_numpy())


def check_formats_give_the_same_bits():
    runs = {fmt: sc.experimental.pp.highly_variable_genes(adata_of(counts(fmt=fmt)), n_top_genes=N_TOP, inplace=False)
            for fmt in ("csr", "csc", "dense")}
    norm = {fmt: sc.experimental.pp.normalize_pearson_residuals(adata_of(counts(fmt=fmt)), inplace=False)["X"]
            for fmt in ("csr", "csc", "dense")}
    for fmt in ("csc", "dense"):
        assert runs[fmt]["residual_variances"].to_numpy().tobytes() == runs["csr"]["residual_variances"].to_numpy().tobytes(), fmt
        assert runs[fmt].equals(runs["csr"]), fmt
        assert norm[fmt].tobytes() == norm["csr"].tobytes(), fmt
    ints = sc.experimental.pp.highly_variable_genes(adata_of(counts(np.int64)), n_top_genes=N_TOP, inplace=False)
    f64 = sc.experimental.pp.highly_variable_genes(adata_of(counts(np.float64)), n_top_genes=N_TOP, inplace=False)
    assert ints.equals(runs["csr"]) and f64.equals(runs["csr"])


def check_normalize(theta, clip, dtype, out_dtype):
    """X, layer and obsm routes, the dict, `copy`, the dtype rule, against the restatement"""
    x = counts(dtype)
    dense = _dense(x).astype(np.float64)
    want = P.restate_residuals(dense, theta, np.sqrt(N_OBS) if clip is None else clip)
    tol = P.residual_tolerance(dense, theta) if out_dtype == np.float64 else np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    a = adata_of(x)
    assert sc.experimental.pp.normalize_pearson_residuals(a, theta=theta, clip=clip) is None
    assert isinstance(a.X, np.ndarray) and a.X.dtype == out_dtype and a.X.shape == x.shape
    assert np.all(np.abs(a.X.astype(np.float64) - want) <= tol)
    assert a.uns["pearson_residuals_normalization"] == dict(theta=theta, clip=clip, computed_on="adata.X")
    if clip is not None and np.isfinite(clip):
        assert a.X.max() <= clip and a.X.min() >= -clip and (np.abs(a.X) == clip).any()
    b = adata_of(sparse.csr_matrix(np.ones(x.shape, dtype=np.float32)))
    b.layers["counts"], b.obsm["prot"] = x, x[:, :40]
    keep = b.X.copy()
    out = sc.experimental.pp.normalize_pearson_residuals(b, theta=theta, clip=clip, layer="counts", inplace=False)
    assert set(out) == {"X", "theta", "clip", "computed_on"} and out["computed_on"] == "counts" and out["X"].tobytes() == a.X.tobytes()
    assert b.layers["counts"] is x and "pearson_residuals_normalization" not in b.uns
    sc.experimental.pp.normalize_pearson_residuals(b, theta=theta, clip=clip, layer="counts")
    assert b.layers["counts"].tobytes() == a.X.tobytes() and (b.X != keep).nnz == 0
    sc.experimental.pp.normalize_pearson_residuals(b, theta=theta, clip=clip, obsm="prot")
    assert b.obsm["prot"].shape == (N_OBS, 40) and b.uns["pearson_residuals_normalization"]["computed_on"] == "prot"
    assert np.all(np.abs(b.obsm["prot"].astype(np.float64) - P.restate_residuals(dense[:, :40], theta, np.sqrt(N_OBS) if clip is None else clip))
                  <= 2 * P.residual_tolerance(dense[:, :40], theta) + (out_dtype == np.float32) * 1e-6 * np.abs(b.obsm["prot"]))
    c = adata_of(x)
    d = sc.experimental.pp.normalize_pearson_residuals(c, theta=theta, clip=clip, copy=True)
    assert d is not c and c.X is x and d.X.tobytes() == a.X.tobytes() and "pearson_residuals_normalization" in d.uns


def _abs_close(got, want, atol):
    return np.abs(np.abs(got) - np.abs(want)).max() <= atol


def check_pca_and_recipe():
    """`test_normalize_pearson_residuals_pca` / `test_pearson_residuals_recipe`: slots, shapes, `mask_var`, zero rows, the
    residual table, and the PCA equal to `pp.pca` on the restated residuals (|loadings| within 1e-4, the tolerance the
    project's PCA is held to against its oracle)"""
    x = counts()
    dense = _dense(x).astype(np.float64)
    a = adata_of(x)
    sc.experimental.pp.highly_variable_genes(a, n_top_genes=N_TOP)
    mask = a.var["highly_variable"].to_numpy()
    ref = adata_of(P.restate_residuals(dense[:, mask], 100, np.sqrt(N_OBS)).astype(np.float32))
    sc.pp.pca(ref, n_comps=20)
    # inplace, the default mask
    assert sc.experimental.pp.normalize_pearson_residuals_pca(a, n_comps=20) is None
    assert a.obsm["X_pca"].shape == (N_OBS, 20) and a.varm["PCs"].shape == (N_VARS, 20)
    assert (a.varm["PCs"][~mask] == 0).all() and (np.abs(a.varm["PCs"][mask]).sum(axis=1) > 0).all()
    assert {"variance", "variance_ratio"} <= set(a.uns["pca"])
    norm = a.uns["pearson_residuals_normalization"]
    assert set(norm) == {"theta", "clip", "computed_on", "pearson_residuals_df"} and norm["theta"] == 100 and norm["clip"] is None
    df = norm["pearson_residuals_df"]
    assert df.shape == (N_OBS, N_TOP) and list(df.columns) == list(a.var_names[mask]) and list(df.index) == list(a.obs_names)
    assert type(a.X) is type(x) and (a.X != x).nnz == 0
    assert _abs_close(a.varm["PCs"][mask], ref.varm["PCs"], 1e-4) and np.allclose(a.uns["pca"]["variance"], ref.uns["pca"]["variance"], rtol=1e-4)
    # not inplace, an explicit mask, no mask at all, key_added
    first = np.arange(N_VARS) < 50
    b = adata_of(x)
    out = sc.experimental.pp.normalize_pearson_residuals_pca(b, n_comps=10, mask_var=first, inplace=False)
    assert out.shape == (N_OBS, 50) and out.obsm["X_pca"].shape == (N_OBS, 10) and out.varm["PCs"].shape == (50, 10)
    assert "X_pca" not in b.obsm and "pearson_residuals_normalization" in out.uns and list(out.var_names) == list(b.var_names[first])
    sc.experimental.pp.normalize_pearson_residuals_pca(b, n_comps=10, mask_var=None, kwargs_pca=dict(key_added="pr"), random_state=0)
    assert b.obsm["pr"].shape == (N_OBS, 10) and b.varm["pr"].shape == (N_VARS, 10) and "pr" in b.uns
    assert b.uns["pearson_residuals_normalization"]["pearson_residuals_df"].shape == (N_OBS, N_VARS)
    # the recipe
    c = adata_of(x)
    assert sc.experimental.pp.recipe_pearson_residuals(c, n_top_genes=N_TOP, n_comps=20) is None
    assert np.array_equal(c.var["highly_variable"].to_numpy(), mask) and c.uns["hvg"]["flavor"] == "pearson_residuals"
    assert c.obsm["X_pca"].shape == (N_OBS, 20) and (c.varm["PCs"][~mask] == 0).all()
    assert c.obsm["X_pca"].tobytes() == a.obsm["X_pca"].tobytes() and c.varm["PCs"].tobytes() == a.varm["PCs"].tobytes()
    assert c.uns["pearson_residuals_normalization"]["pearson_residuals_df"].equals(df)
    d = adata_of(x)
    adata_pca, hvg = sc.experimental.pp.recipe_pearson_residuals(d, n_top_genes=N_TOP, n_comps=20, inplace=False)
    assert "highly_variable" not in d.var and "X_pca" not in d.obsm and np.array_equal(hvg["highly_variable"].to_numpy(), mask)
    assert adata_pca.shape == (N_OBS, N_TOP) and adata_pca.obsm["X_pca"].tobytes() == a.obsm["X_pca"].tobytes()
    assert adata_pca.X.dtype == np.float32 and np.array_equal(adata_pca.X, df.to_numpy())


def check_pbmc68k_warns(pbmc68k):
    """`raw_X` is log-normalised: the warning path of `check_values`, silence without it, and the result at the reference's own
    ceiling (np.allclose defaults) against the restatement"""
    raw = pbmc68k["raw_X"]
    a = adata_of(raw)
    with pytest.warns(UserWarning, match="`flavor='pearson_residuals'` expects raw count data, but non-integers were found."):
        df = sc.experimental.pp.highly_variable_genes(a, n_top_genes=100, inplace=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sc.experimental.pp.highly_variable_genes(a, n_top_genes=100, inplace=False, check_values=False)
        out = sc.experimental.pp.normalize_pearson_residuals(a, check_values=False, inplace=False)
    with pytest.warns(UserWarning, match=r"`normalize_pearson_residuals\(\)` expects raw count data, but non-integers were found."):
        sc.experimental.pp.normalize_pearson_residuals(a, inplace=False)
    dense = raw.toarray().astype(np.float64)
    assert np.allclose(df["residual_variances"], P.restate_gene_var(dense, 100, np.sqrt(raw.shape[0])))
    assert np.allclose(df["residual_variances"], np.var(out["X"].astype(np.float64), axis=0), rtol=1e-4)   # (float32 matrix)
    assert df["highly_variable"].sum() == 100


# ---- the tests ---------------------------------------------------------------------------------------------------------
def test_exported():
    from scanpy_amd.experimental import pp as epp

    assert "experimental" in sc.__all__ and sc.experimental.pp is epp
    assert epp.__all__ == ["highly_variable_genes", "normalize_pearson_residuals", "normalize_pearson_residuals_pca",
                           "recipe_pearson_residuals"]


@pytest.mark.parametrize("theta", [100, np.inf])
@pytest.mark.parametrize("clip", [None, np.inf, 30])
def test_general(theta, clip):
    check_general(theta, clip)


def test_batch():
    check_batch()
    check_batch(theta=np.inf, clip=30)


def test_subset_inplace_layer():
    check_subset_inplace_layer()


def test_formats_and_dtypes_give_the_same_bits():
    check_formats_give_the_same_bits()


@pytest.mark.parametrize(("dtype", "out_dtype"), [(np.float32, np.float32), (np.int64, np.float64), (np.float64, np.float64),
                                                  (np.uint16, np.float64)])
def test_normalize_dtype_rule(dtype, out_dtype):
    check_normalize(100, None, dtype, out_dtype)


@pytest.mark.parametrize(("theta", "clip"), [(np.inf, np.inf), (100, 30), (np.inf, 3.0)])
def test_normalize_parameters(theta, clip):
    check_normalize(theta, clip, np.float32, np.float32)


def test_pca_and_recipe():
    check_pca_and_recipe()


def test_pbmc68k_noninteger_warning(pbmc68k):
    check_pbmc68k_warns(pbmc68k)


def test_ranking_and_merge_on_given_variances():
    """three batches, five genes, worked by hand: ranks 0 = most variable; top 2 per batch; sort by (nbatches desc, median rank)"""
    from scanpy_amd.experimental.pp._highly_variable_genes import _rank_and_select

    v = np.array([[9.0, 8.0, 1.0, 0.0, 0.5], [9.0, 1.0, 8.0, 0.0, 0.5], [1.0, 9.0, 8.0, 0.0, 0.5]])
    names = pd.Index(list("abcde"))
    df = _rank_and_select(v, 2, names, np.zeros(5), np.ones(5))
    assert list(df.index) == list("abcde")
    assert df["highly_variable_nbatches"].tolist() == [2, 2, 2, 0, 0] and not df["highly_variable_intersection"].any()
    rank = df["highly_variable_rank"].to_numpy()
    assert rank[:3].tolist() == [0.0, 0.5, 1.0] and np.isnan(rank[3:]).all() and rank.dtype == np.float32
    assert df["highly_variable"].tolist() == [True, True, False, False, False]
    assert np.allclose(df["residual_variances"], v.mean(axis=0))


def test_input_checks_and_messages():
    """`test_pearson_residuals_inputchecks` and the messages of both modules"""
    x = counts()
    a = adata_of(x)
    hvg, norm = sc.experimental.pp.highly_variable_genes, sc.experimental.pp.normalize_pearson_residuals
    with pytest.raises(ValueError, match="Pearson residuals require theta > 0"):
        hvg(a, theta=0, n_top_genes=10)
    with pytest.raises(ValueError, match="Pearson residuals require theta > 0"):
        norm(a, theta=-1)
    with pytest.raises(ValueError, match="Pearson residuals require `clip>=0` or `clip=None`."):
        hvg(a, clip=-1, n_top_genes=10)
    with pytest.raises(ValueError, match="Pearson residuals require `clip>=0` or `clip=None`."):
        norm(a, clip=-1)
    with pytest.raises(ValueError, match="requires the argument `n_top_genes` for `flavor='pearson_residuals'`"):
        hvg(a)
    with pytest.raises(ValueError, match="This is an experimental API and only `flavor=pearson_residuals` is available."):
        hvg(a, flavor="seurat", n_top_genes=10)
    with pytest.raises(ValueError, match="expects an `AnnData` argument, pass `inplace=False` if you want to return a `pd.DataFrame`."):
        hvg(x, n_top_genes=10)
    with pytest.raises(ValueError, match="`copy=True` cannot be used with `inplace=False`."):
        norm(a, copy=True, inplace=False)
    frac = x.copy()
    frac.data = frac.data + np.float32(0.5)
    with pytest.warns(UserWarning, match="`flavor='pearson_residuals'` expects raw count data, but non-integers were found."):
        hvg(adata_of(frac), n_top_genes=10)
    with pytest.warns(UserWarning, match=r"`normalize_pearson_residuals\(\)` expects raw count data, but non-integers were found."):
        sc.experimental.pp.normalize_pearson_residuals_pca(adata_of(frac), n_comps=5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hvg(adata_of(frac), n_top_genes=10, check_values=False)
        sc.experimental.pp.recipe_pearson_residuals(adata_of(frac), n_top_genes=50, n_comps=5, check_values=False)
        hvg(a, n_top_genes=10)
    assert (a.X != x).nnz == 0


def test_refusals():
    x = counts()
    hvg, norm = sc.experimental.pp.highly_variable_genes, sc.experimental.pp.normalize_pearson_residuals
    wide = x.astype(np.float64)
    wide.data[5] = 1.0 + 2.0 ** -40
    with pytest.raises(NotImplementedError, match="float64 values that float32 does not hold exactly"):
        hvg(adata_of(wide), n_top_genes=10)
    big = x.astype(np.int64)
    big.data[5] = 2 ** 24 + 1
    with pytest.raises(NotImplementedError, match="beyond 2\\^24"):
        norm(adata_of(big))
    for bad_value in (np.nan, np.inf):
        bad = x.copy()
        bad.data[9] = bad_value
        with pytest.raises(ValueError, match="not finite"):
            hvg(adata_of(bad), n_top_genes=10)
        with pytest.raises(ValueError, match="not finite"):
            norm(adata_of(bad.toarray()))

    class Backed:
        is_backed, shape, dtype = True, x.shape, np.float32

    a = adata_of(x)
    a.X = Backed()
    with pytest.raises(NotImplementedError, match="backed"):
        hvg(a, n_top_genes=10)
    with pytest.raises(NotImplementedError, match="backed"):
        norm(a)
    DaskArray = type("Array", (), {"__module__": "dask.array.core", "shape": x.shape, "dtype": np.float32})
    a.X = DaskArray()
    with pytest.raises(NotImplementedError, match="dask"):
        hvg(a, n_top_genes=10)
