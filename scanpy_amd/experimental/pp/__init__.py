"""`sc.experimental.pp`: analytic Pearson residuals (Lause et al. 2021) on the device -- gene selection, normalisation, and the
two host compositions with `sc.pp.pca` (reference: src/scanpy/experimental/pp/; csrc/pearson.hip)."""
from __future__ import annotations

from ._highly_variable_genes import highly_variable_genes
from ._normalization import normalize_pearson_residuals, normalize_pearson_residuals_pca
from ._recipes import recipe_pearson_residuals

__all__ = ["highly_variable_genes", "normalize_pearson_residuals", "normalize_pearson_residuals_pca", "recipe_pearson_residuals"]
