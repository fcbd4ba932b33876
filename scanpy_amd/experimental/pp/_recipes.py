"""`sc.experimental.pp.recipe_pearson_residuals` (reference: src/scanpy/experimental/pp/_recipes.py): gene selection,
normalisation and PCA by Pearson residuals, a host composition of the calls of this package with `sc.pp.pca`."""
from __future__ import annotations

from types import MappingProxyType

import numpy as np

from ..._utils import _UNSET
from ...preprocessing._pca import pca
from ._highly_variable_genes import highly_variable_genes
from ._normalization import _pca_keys, _to_df, normalize_pearson_residuals


def recipe_pearson_residuals(adata, *, theta: float = 100, clip: float | None = None, n_top_genes: int = 1000,
                             batch_key: str | None = None, chunksize: int = 1000, n_comps: int | None = 50, rng=None,
                             random_state=_UNSET, kwargs_pca=MappingProxyType({}), check_values: bool = True, inplace: bool = True):
    """Full preprocessing by analytic Pearson residuals (drop-in for `scanpy.experimental.pp.recipe_pearson_residuals`):
    `highly_variable_genes(flavor='pearson_residuals')`, `normalize_pearson_residuals` of the selected genes, `sc.pp.pca`.

    With `inplace`, `adata.var` gets the gene selection and `obsm`, `varm` (zero rows for the genes that were not selected),
    `uns[pca key]` and `uns['pearson_residuals_normalization']` (with `pearson_residuals_df`) the rest; otherwise the pair
    (AnnData of the selected genes with the PCA, the selection table) is returned.  `chunksize` is accepted and ignored."""
    k_obsm, k_varm, k_uns = _pca_keys(kwargs_pca)
    hvg_args = dict(flavor="pearson_residuals", n_top_genes=n_top_genes, batch_key=batch_key, theta=theta, clip=clip,
                    chunksize=chunksize, check_values=check_values)
    hvg = None
    if inplace:
        highly_variable_genes(adata, **hvg_args, inplace=True)
        selected = adata.var["highly_variable"].to_numpy()
    else:
        hvg = highly_variable_genes(adata, **hvg_args, inplace=False)
        selected = hvg["highly_variable"].to_numpy()
    adata_pca = adata[:, selected].copy()
    normalize_pearson_residuals(adata_pca, theta=theta, clip=clip, check_values=check_values)
    pca(adata_pca, n_comps=n_comps, rng=rng, random_state=random_state, **kwargs_pca)
    if not inplace:
        return adata_pca, hvg
    norm_dict = dict(**adata_pca.uns["pearson_residuals_normalization"], pearson_residuals_df=_to_df(adata_pca))
    adata.uns[k_uns] = adata_pca.uns[k_uns]
    adata.varm[k_varm] = np.zeros(shape=(adata.n_vars, adata_pca.obsm[k_obsm].shape[1]))
    adata.varm[k_varm][selected] = adata_pca.varm[k_varm]
    adata.uns["pearson_residuals_normalization"] = norm_dict
    adata.obsm[k_obsm] = adata_pca.obsm[k_obsm]
    return None
