"""`sc.experimental.pp.normalize_pearson_residuals` and `normalize_pearson_residuals_pca` on MI355X (reference:
src/scanpy/experimental/pp/_normalization.py).

The reference forms the dense n x g matrix mu on the host and divides; here `scamd_pp_pearson_residuals_f32` writes the clipped
residuals from the CSR matrix in one pass (csrc/pearson.hip).  The arithmetic is float64 whatever the input; a float32 result is
that value rounded once, so it is closer to the exact residual than the reference's, whose float32 input makes mu float32."""
from __future__ import annotations

import warnings
from types import MappingProxyType

import numpy as np
import pandas as pd

from ..._anndata import AnnData
from ..._utils import _UNSET, view_to_actual
from ...preprocessing._normalization import _set_obs_rep
from ...preprocessing._pca import _DEFAULT_MASK, _check_mask, _get_arr, pca
from . import _pearson

_WHAT = "experimental.pp.normalize_pearson_residuals"


def _pearson_residuals(x, theta, clip, check_values) -> np.ndarray:
    """the clipped residuals of x as a dense matrix: float32 for float32 input, float64 otherwise (`:36-75`)"""
    if theta <= 0:
        msg = "Pearson residuals require theta > 0"
        raise ValueError(msg)
    if clip is None:
        clip = np.sqrt(x.shape[0])
    if clip < 0:
        msg = "Pearson residuals require `clip>=0` or `clip=None`."
        raise ValueError(msg)
    be, m, dtype = _pearson.upload(x, _WHAT)
    if check_values and not be.nonnegative_integers(m):
        warnings.warn("`normalize_pearson_residuals()` expects raw count data, but non-integers were found.", UserWarning, stacklevel=4)
    gene_sum = be.col_stats(m)[0]
    return be.pearson_residuals(m, gene_sum, be.row_totals64(m), float(np.sum(gene_sum)), inv_theta=1.0 / float(theta),
                                clip=float(clip), out_f64=np.dtype(dtype) != np.float32)


def normalize_pearson_residuals(adata, *, theta: float = 100, clip: float | None = None, check_values: bool = True,
                                layer: str | None = None, obsm: str | None = None, inplace: bool = True, copy: bool = False):
    """Analytic Pearson residual normalisation (drop-in for `scanpy.experimental.pp.normalize_pearson_residuals`, `:86-156`).

    `theta`: the overdispersion shared by all genes (`np.inf`: Poisson); `clip`: residuals are clipped to +-clip (None:
    sqrt(n_obs), `np.inf`: not at all).  `X`, `layers[layer]` or `obsm[obsm]` becomes the dense residual matrix -- float32 for
    float32 input, float64 for integer and float64 input; the arithmetic is float64 in both cases -- and
    `uns['pearson_residuals_normalization']` holds `theta`, `clip` and `computed_on`.  With `inplace=False` that dict is
    returned with the matrix as `'X'`; `copy=True` works on and returns a copy.  Expects raw counts."""
    if copy:
        if not inplace:
            msg = "`copy=True` cannot be used with `inplace=False`."
            raise ValueError(msg)
        adata = adata.copy()
    view_to_actual(adata)
    x = _get_arr(adata, layer=layer, obsm=obsm)
    computed_on = layer or obsm or "adata.X"
    residuals = _pearson_residuals(x, theta, clip, check_values)
    settings_dict = dict(theta=theta, clip=clip, computed_on=computed_on)
    if inplace:
        _set_obs_rep(adata, residuals, layer=layer, obsm=obsm)
        adata.uns["pearson_residuals_normalization"] = settings_dict
    if copy:
        return adata
    if not inplace:
        return dict(X=residuals, **settings_dict)
    return None


def _pca_keys(kwargs_pca) -> tuple:
    key_added = kwargs_pca.get("key_added")
    return ("X_pca", "PCs", "pca") if key_added is None else (key_added,) * 3


def _to_df(adata) -> pd.DataFrame:
    return pd.DataFrame(np.asarray(adata.X), index=adata.obs_names, columns=adata.var_names)


def normalize_pearson_residuals_pca(adata, *, theta: float = 100, clip: float | None = None, n_comps: int | None = 50, rng=None,
                                    random_state=_UNSET, kwargs_pca=MappingProxyType({}), mask_var=_DEFAULT_MASK,
                                    check_values: bool = True, inplace: bool = True):
    """Pearson residual normalisation of the selected genes, then `sc.pp.pca` (drop-in for
    `scanpy.experimental.pp.normalize_pearson_residuals_pca`, `:168-258`).

    `mask_var`: the genes to use (default: `var['highly_variable']` if present, else all).  The residual matrix comes back to
    the host and goes to `pp.pca` through its public door.  With `inplace`, `obsm`, `varm` (zero rows for the genes that were
    not selected), `uns[pca key]` and `uns['pearson_residuals_normalization']` (with `pearson_residuals_df`) are written;
    otherwise the AnnData of the selected genes with the PCA is returned."""
    k_obsm, k_varm, k_uns = _pca_keys(kwargs_pca)
    if mask_var is _DEFAULT_MASK:
        mask_var = "highly_variable" if "highly_variable" in adata.var else None
    mask_var = _check_mask(adata, mask_var, "var")
    sub = adata if mask_var is None else adata[:, mask_var]
    adata_pca = AnnData(sub.X.copy(), obs=sub.obs[[]].copy(), var=sub.var[[]].copy())
    normalize_pearson_residuals(adata_pca, theta=theta, clip=clip, check_values=check_values)
    pca(adata_pca, n_comps=n_comps, rng=rng, random_state=random_state, **kwargs_pca)
    n_comps = adata_pca.obsm[k_obsm].shape[1]  # (None was resolved by pca)
    if not inplace:
        return adata_pca
    norm_dict = dict(**adata_pca.uns["pearson_residuals_normalization"], pearson_residuals_df=_to_df(adata_pca))
    if mask_var is not None:
        adata.varm[k_varm] = np.zeros(shape=(adata.n_vars, n_comps))
        adata.varm[k_varm][mask_var] = adata_pca.varm[k_varm]
    else:
        adata.varm[k_varm] = adata_pca.varm[k_varm]
    adata.uns[k_uns] = adata_pca.uns[k_uns]
    adata.uns["pearson_residuals_normalization"] = norm_dict
    adata.obsm[k_obsm] = adata_pca.obsm[k_obsm]
    return None
