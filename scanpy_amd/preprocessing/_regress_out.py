"""`sc.pp.regress_out` on MI355X (reference: src/scanpy/preprocessing/_simple.py:468-681).

The reference fits one linear model per gene (a normal-equations shortcut, `numpy_regress_out` `:496-507`, or one statsmodels
GLM per gene, `_regress_out_chunk` `:646-681`).  Both branches are closed forms of ONE model, out = X - W T:

* a categorical key: the reference regresses each gene on [1, m] with m_i the gene's mean in the category of cell i
  (`_create_regressor_categorical`, `:468-482`); the least-squares slope is exactly 1 and the intercept exactly 0, so the
  residual is x_ij - mean_j(category of i).  W = one-hot of the category code, T = the category means.
* numeric keys: the residual of projecting each gene on span[1, keys...] does not depend on how the span is parametrised, so
  the raw regressors (badly conditioned: counts next to fractions) are replaced ON THE HOST by an orthonormal basis Q of the
  centred, unit-scaled key columns.  W = [1, Q], T = [mean; Q^T X].

The device does the two passes over the matrix (csrc/regress.hip): `scamd_pp_regress_sums_f32` gives W^T X (order-independent
fixed-point sums) with every gene's minimum and maximum, `scamd_pp_regress_resid_f32` writes the dense residual.  The host
handles the n x (p + 1) regressors and the (r + 1) x g or K x g table only."""
from __future__ import annotations

import numpy as np
import pandas as pd

from .._utils import view_to_actual
from . import _csr_device
from ._normalization import _set_obs_rep
from ._pca import _get_arr

MAX_NUMERIC_KEYS = 16
MAX_CATEGORIES = 65536


def _numeric_basis(regressors: np.ndarray) -> np.ndarray:
    """regressors float64 [n, p] -> Q float64 [n, r]: an orthonormal basis of the centred columns, r <= p (0: all constant).
    Columns are centred and scaled to unit norm; directions below max(n, p) * eps relative to the largest are dropped."""
    n, p = regressors.shape
    if n == 0 or p == 0:
        return np.zeros((n, 0))
    eps = np.finfo(np.float64).eps
    centred = regressors - regressors.mean(axis=0)
    centred[:, regressors.max(axis=0) == regressors.min(axis=0)] = 0.0  # (the mean of n equal values need not be the value)
    norm = np.sqrt((centred * centred).sum(axis=0))
    live = norm > max(n, p) * eps * np.abs(regressors).max(axis=0)
    if not live.any():
        return np.zeros((n, 0))
    unit = centred[:, live] / norm[live]
    u, s, _ = np.linalg.svd(unit, full_matrices=False)
    return np.ascontiguousarray(u[:, s > max(n, p) * eps * s[0]])


def _out_is_f64(dtype, *, glm_route: bool) -> bool:
    """`:603-609`: the shortcut keeps float32 and turns integers of up to 4 bytes into float32, wider ones into float64; the GLM
    route (`:639`: categorical key or singular design) returns float64"""
    if glm_route:
        return True
    dt = np.dtype(dtype)
    return dt != np.float32 and dt.itemsize > 4


def _regress_matrix(x, obs: pd.DataFrame, keys: list):
    x = _csr_device.in_memory(x)
    n, g = x.shape
    first = obs[keys[0]] if keys and keys[0] in obs else None
    if first is not None and isinstance(first.dtype, pd.CategoricalDtype):
        if len(keys) > 1:
            msg = ("If providing categorical variable, only a single one is allowed. For this one we regress on the mean for "
                   "each category.")
            raise ValueError(msg)
        codes = first.cat.codes.to_numpy().astype(np.int32)
        n_cat = len(first.cat.categories)
        if (codes < 0).any():
            raise NotImplementedError(f"obs[{keys[0]!r}] has missing values: the reference would regress such cells on 0, which "
                                      "is another model; drop them or give them a category of their own")
        if n_cat > MAX_CATEGORIES:
            raise NotImplementedError(f"obs[{keys[0]!r}] has {n_cat} categories, at most {MAX_CATEGORIES} are offered")
        n_cat = max(n_cat, 1)
        size = np.bincount(codes, minlength=n_cat).astype(np.float64)
        model, n_table, wbound, glm_route = {"codes": codes}, n_cat, size, True
    else:
        frame = obs[keys]
        if frame.shape[1] > MAX_NUMERIC_KEYS:
            raise NotImplementedError(f"{frame.shape[1]} keys, at most {MAX_NUMERIC_KEYS} numeric keys are offered")
        try:
            cols = frame.to_numpy(dtype=np.float64, na_value=np.nan).reshape(n, -1)
        except (TypeError, ValueError) as e:
            raise ValueError(f"the keys {keys} must be numeric columns of `obs` (or one categorical column): {e}") from None
        if not np.isfinite(cols).all():
            raise ValueError(f"non-finite values in obs[{keys}]: the regression is not defined")
        design = np.concatenate([np.ones((n, 1)), cols], axis=1)
        glm_route = bool(np.linalg.det(design.T @ design) == 0)  # `:600`
        w = np.ascontiguousarray(np.concatenate([np.ones((n, 1)), _numeric_basis(cols)], axis=1))
        model, n_table, wbound = {"w": w}, w.shape[1], np.abs(w).sum(axis=0) * (1 + 1e-6)
    be = _csr_device.default_backend()
    m = be.upload(x)
    sums = be.regress_sums(m, n_table=n_table, wbound=wbound, **model)
    if sums["nonfinite"]:
        raise ValueError("the matrix holds non-finite values (NaN or infinity): the regression is not defined")
    # the table T: the category means, or [mean; Q^T X] (Q is centred: Q^T X = Q^T (X - mean))
    table = sums["sums"] / np.maximum(wbound if "codes" in model else np.r_[float(max(n, 1)), np.ones(n_table - 1)], 1.0)[:, None]
    # `:657-661`: the GLM route returns a gene whose values are all identical as it is
    keep = np.ones(g, dtype=np.uint8) if not glm_route else (sums["col_min"] != sums["col_max"]).astype(np.uint8)
    return be.regress_resid(m, table, keep, out_f64=_out_is_f64(x.dtype, glm_route=glm_route), **model)


def regress_out(adata, keys, *, layer: str | None = None, n_jobs: int | None = None, copy: bool = False):
    """Regress out (mostly) unwanted sources of variation (drop-in for `scanpy.pp.regress_out`, `_simple.py:510-643`).

    keys: one key or a sequence of keys of `adata.obs`; an empty sequence takes every column (`:592`).  A categorical (or
    string) first key must be the only one: the per-gene mean of every category is removed (`:568-588`).  Numeric keys (at
    most 16): the residual of the least-squares fit on [1, keys...] (`:496-507`).  `n_jobs` is accepted and ignored.
    X / `layers[layer]` becomes a dense matrix: float32 for float32 or integer (<= 4 bytes) input on the non-singular numeric
    route (`:603-609`), float64 otherwise; on the float64 routes a gene whose values are all identical is returned unchanged
    (`:657-661`).  Returns `adata` if `copy` else None."""
    del n_jobs
    adata = adata.copy() if copy else adata
    view_to_actual(adata)  # `:555`
    keys = [keys] if isinstance(keys, str) else list(keys)
    if not keys:
        keys = list(adata.obs.columns)
    for k in keys:  # the part of `sanitize_anndata` (`:553`) that matters here: strings become categoricals
        if k in adata.obs and (adata.obs[k].dtype == object or pd.api.types.is_string_dtype(adata.obs[k].dtype)):
            adata.obs[k] = adata.obs[k].astype("category")
    x = _get_arr(adata, layer=layer)
    out = _regress_matrix(x, adata.obs, keys)
    _set_obs_rep(adata, out, layer=layer)
    return adata if copy else None
