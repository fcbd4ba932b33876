"""`sc.metrics` on MI355X: `modularity` and `confusion_matrix` (src/scanpy/metrics/_metrics.py), `morans_i` and `gearys_c`
(metrics/_morans_i.py, metrics/_gearys_c.py of the reference)."""
from ._autocorr import gearys_c, morans_i
from ._metrics import confusion_matrix, modularity, modularity_adata

__all__ = ["confusion_matrix", "gearys_c", "modularity", "modularity_adata", "morans_i"]
