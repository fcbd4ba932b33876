"""`sc.experimental.pp.highly_variable_genes` on MI355X (reference: src/scanpy/experimental/pp/_highly_variable_genes.py).

The reference evaluates a clipped Pearson residual for every (cell, gene) pair, twice, in a numba loop over the CSC matrix.
Here `scamd_pp_pearson_gene_var_f32` gives the same per-gene variance from the stored entries and the DISTINCT cell totals
(csrc/pearson.hip); the ranking across batches, the masked median and the sort stay on the host, with the reference's numpy and
pandas calls, so ties fall as they do there."""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd

from ..._anndata import is_anndata
from ..._utils import view_to_actual
from ...preprocessing._csr_device import mean_var_from_sums
from ...preprocessing._pca import _get_arr
from . import _pearson

_WHAT = "experimental.pp.highly_variable_genes"


def _rank_and_select(residual_gene_vars: np.ndarray, n_top_genes: int, var_names, means, variances) -> pd.DataFrame:
    """residual_gene_vars [n_batches, g] -> the reference's table (`:211-251`), indexed and ordered by var_names"""
    n_batches = residual_gene_vars.shape[0]
    ranks = np.argsort(np.argsort(-residual_gene_vars, axis=1), axis=1).astype(np.float32)  # small rank: most variable
    nbatches = np.sum((ranks < n_top_genes).astype(int), axis=0)
    ranks[ranks >= n_top_genes] = np.nan
    median_rank = np.ma.median(np.ma.masked_invalid(ranks), axis=0).filled(np.nan)
    df = pd.DataFrame.from_dict(dict(means=means, variances=variances, residual_variances=np.mean(residual_gene_vars, axis=0),
                                     highly_variable_rank=median_rank, highly_variable_nbatches=nbatches.astype(np.int64),
                                     highly_variable_intersection=nbatches == n_batches))
    df = df.set_index(var_names)
    df = df.sort_values(["highly_variable_nbatches", "highly_variable_rank"], ascending=[False, True], na_position="last")
    high_var = np.zeros(df.shape[0], dtype=bool)
    high_var[:n_top_genes] = True
    df["highly_variable"] = high_var
    return df.loc[var_names, :]


def _residual_variances(adata, x, *, theta, clip, batch_key, check_values) -> tuple:
    """-> (residual variances [n_batches, g], means, variances); the checks in the reference's order (`:146-182`)"""
    be, m, _ = _pearson.upload(x, _WHAT)
    if check_values and not be.nonnegative_integers(m):
        warnings.warn("`flavor='pearson_residuals'` expects raw count data, but non-integers were found.", UserWarning, stacklevel=4)
    if theta <= 0:
        msg = "Pearson residuals require theta > 0"
        raise ValueError(msg)
    n = adata.shape[0]
    if batch_key is None:
        batches, codes = np.zeros(1, dtype=int), None
    else:
        batches, codes = np.unique(adata.obs[batch_key].to_numpy(), return_inverse=True)
        codes = np.asarray(codes, dtype=np.int32).reshape(-1)
    cell_total = be.row_totals64(m)
    s_all, sq_all, _ = be.col_stats(m)
    out = []
    for k in range(len(batches)):
        in_batch = None if codes is None else codes == k
        n_batch = n if codes is None else int(in_batch.sum())
        if clip is None:  # (`:177-179`: set once, so every later batch is clipped at the FIRST batch's sqrt(n))
            clip = np.sqrt(n_batch)
        if clip < 0:
            msg = "Pearson residuals require `clip>=0` or `clip=None`."
            raise ValueError(msg)
        gene_sum = s_all if codes is None else be.col_stats(m, row_mask=in_batch.astype(np.uint8))[0]
        out.append(be.pearson_gene_var(m, gene_sum, cell_total, float(np.sum(gene_sum)), inv_theta=1.0 / float(theta), clip=float(clip),
                                       batch_codes=codes, batch_id=k, n_batch=n_batch).reshape(1, -1))
    means, variances = mean_var_from_sums(s_all, sq_all, n, correction=1)
    return np.concatenate(out, axis=0), np.asarray(means), np.asarray(variances)


def highly_variable_genes(adata, *, theta: float = 100, clip: float | None = None, n_top_genes: int | None = None,
                          batch_key: str | None = None, chunksize: int = 1000, flavor: str = "pearson_residuals",
                          check_values: bool = True, layer: str | None = None, subset: bool = False, inplace: bool = True):
    """Select highly variable genes by the variance of their analytic Pearson residuals (drop-in for
    `scanpy.experimental.pp.highly_variable_genes`, `:298-395`).

    The residuals are those of a negative binomial offset model with the overdispersion `theta` shared by all genes
    (`np.inf`: Poisson), clipped to +-`clip` (None: sqrt of the number of cells; with `batch_key`, of the first batch in
    `np.unique` order for every batch, as in the reference).  Genes are ranked by residual variance within each batch and then
    by the number of batches in which they are among the `n_top_genes` and the median of those ranks.  `chunksize` is accepted
    and ignored: nothing is densified here.  Expects raw counts (`check_values` warns otherwise).

    With `inplace`, `adata.var` gets `means`, `variances` (`correction=1`), `residual_variances` (the mean over batches),
    `highly_variable_rank`, with `batch_key` also `highly_variable_nbatches` and `highly_variable_intersection`, and
    `highly_variable`; `adata.uns['hvg']` names the flavor; `subset` keeps the selected genes only.  Otherwise the table is
    returned."""
    del chunksize
    if not is_anndata(adata):
        msg = "`pp.highly_variable_genes` expects an `AnnData` argument, pass `inplace=False` if you want to return a `pd.DataFrame`."
        raise ValueError(msg)
    if flavor != "pearson_residuals":
        msg = "This is an experimental API and only `flavor=pearson_residuals` is available."
        raise ValueError(msg)
    if n_top_genes is None:
        msg = "`pp.highly_variable_genes` requires the argument `n_top_genes` for `flavor='pearson_residuals'`"
        raise ValueError(msg)
    view_to_actual(adata)
    x = _get_arr(adata, layer=layer)
    computed_on = layer if layer else "adata.X"
    residual_gene_vars, means, variances = _residual_variances(adata, x, theta=theta, clip=clip, batch_key=batch_key,
                                                               check_values=check_values)
    df = _rank_and_select(residual_gene_vars, n_top_genes, adata.var_names, means, variances)
    if inplace:
        adata.uns["hvg"] = {"flavor": "pearson_residuals", "computed_on": computed_on}
        cols = ["means", "variances", "residual_variances", "highly_variable_rank"]
        if batch_key is not None:
            cols += ["highly_variable_nbatches", "highly_variable_intersection"]
        for c in [*cols, "highly_variable"]:
            adata.var[c] = df[c].array
        if subset:
            adata._inplace_subset_var(df["highly_variable"].to_numpy())
        return None
    if batch_key is None:
        df = df.drop(["highly_variable_nbatches", "highly_variable_intersection"], axis=1)
    if subset:
        df = df.iloc[df["highly_variable"].to_numpy(), :]
    return df
