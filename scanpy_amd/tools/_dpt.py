"""`sc.tl.dpt` on MI355X (src/scanpy/tools/_dpt.py:24-191), pseudotime only: the DPT distances from the root cell and their
scaling run in scamd_dpt_pseudotime_f32; the root cell, the fall-back to `tl.diffmap`, slots and messages follow the
reference.  The branching search (`n_branchings > 0`) is not offered."""
from __future__ import annotations

import warnings

from ..neighbors import Neighbors, existing_diffmap_keys

__all__ = ["dpt"]


def dpt(adata, n_dcs: int = 10, *, n_branchings: int = 0, min_group_size: float = 0.01, allow_kendall_tau_shift: bool = True,
        neighbors_key: str | None = None, diffmap_key: str | None = None, copy: bool = False):
    """Diffusion pseudotime (drop-in for `scanpy.tl.dpt` with `n_branchings=0`).  Writes `.obs['dpt_pseudotime']` when a root
    cell is given by `.uns['iroot']` or `.var['xroot']` / `.uns['xroot']`, and re-writes `.uns['iroot']`."""
    if n_branchings > 0:
        msg = (f"tl.dpt: n_branchings={n_branchings}: the branching search walks O(n^2) DPT distance rows on the host and is a "
               "separate piece of work; only the pseudotime (n_branchings=0) runs on the MI355X path (see tl.paga in scanpy "
               "for branchings).")
        raise NotImplementedError(msg)
    adata = adata.copy() if copy else adata
    if neighbors_key is None:
        neighbors_key = "neighbors"
    if neighbors_key not in adata.uns:
        msg = "You need to run `pp.neighbors` and `tl.diffmap` first."
        raise ValueError(msg)
    if "iroot" not in adata.uns and "xroot" not in adata.var:
        warnings.warn("No root cell found. To compute pseudotime, pass the index or expression vector of a root cell, one of:\n"
                      "    adata.uns['iroot'] = root_cell_index\n"
                      "    adata.var['xroot'] = adata[root_cell_name, :].X", UserWarning, stacklevel=2)
    if not diffmap_key and not existing_diffmap_keys(adata):
        warnings.warn("Trying to run `tl.dpt` without prior call of `tl.diffmap`. Falling back to `tl.diffmap` with default "
                      "parameters.", UserWarning, stacklevel=2)
        from ._diffmap import diffmap

        diffmap(adata, neighbors_key=neighbors_key, random_state=0)
    neighbors = Neighbors(adata, n_dcs=n_dcs, neighbors_key=neighbors_key, diffmap_key=diffmap_key)
    if neighbors.iroot is not None:
        neighbors._set_pseudotime()  # pseudotimes are distances from the root cell
        adata.uns["iroot"] = neighbors.iroot
        adata.obs["dpt_pseudotime"] = neighbors.pseudotime
    return adata if copy else None
