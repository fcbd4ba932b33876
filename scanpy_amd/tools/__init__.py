from ._diffmap import diffmap
from ._dpt import dpt
from ._leiden import leiden
from ._leiden_multires import leiden_multires
from ._rank_genes_groups import rank_genes_groups
from ._umap import umap

__all__ = ["diffmap", "dpt", "leiden", "leiden_multires", "rank_genes_groups", "umap"]
