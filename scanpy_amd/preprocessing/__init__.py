from ..neighbors import neighbors
from ._filter import filter_cells, filter_genes
from ._harmony import harmony_integrate
from ._highly_variable_genes import highly_variable_genes
from ._normalization import normalize_total
from ._pca import pca
from ._regress_out import regress_out
from ._qc import calculate_qc_metrics, describe_obs, describe_var
from ._scale import scale
from ._scrublet import scrublet, scrublet_simulate_doublets
from ._simple import log1p

__all__ = ["pca", "neighbors", "filter_cells", "filter_genes", "normalize_total", "log1p", "highly_variable_genes", "scale", "harmony_integrate",
           "calculate_qc_metrics", "describe_obs", "describe_var", "regress_out", "scrublet", "scrublet_simulate_doublets"]
