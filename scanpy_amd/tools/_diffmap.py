"""`sc.tl.diffmap` on MI355X (src/scanpy/tools/_diffmap.py): the transition matrix and its leading eigenpairs come from
`Neighbors.compute_transitions` / `.compute_eigen` (scamd_transitions_sym_f32, scamd_diffmap_f32); slots, messages and `copy`
semantics follow the reference."""
from __future__ import annotations

from .._settings import settings
from .._utils import _UNSET, resolve_seed
from ..neighbors import Neighbors, check_eigen_arguments, diffmap_keys

__all__ = ["diffmap"]


def _preset_key_added():
    """`settings.preset.diffmap.key_added` (src/scanpy/_settings/presets.py:224-229)"""
    return "diffmap" if settings.preset == "ScanpyV2Preview" else None


def diffmap(adata, n_comps: int = 15, *, neighbors_key: str | None = None, key_added=_UNSET, rng=None, random_state=_UNSET,
            copy: bool = False):
    """Diffusion maps (drop-in for `scanpy.tl.diffmap`).  Writes `.obsm['X_diffmap']` and `.uns['diffmap_evals']`, or
    `.obsm[key_added]` and `.uns[key_added]['evals']`; column 0 is the stationary state.  At most 26 components; a graph whose
    transition matrix has a negative eigenvalue of larger magnitude than the last requested one raises NotImplementedError."""
    seed, _ = resolve_seed(rng, random_state)
    if neighbors_key is None:
        neighbors_key = "neighbors"
    if neighbors_key not in adata.uns:
        msg = "You need to run `pp.neighbors` first to compute a neighborhood graph."
        raise ValueError(msg)
    if n_comps <= 2:
        msg = "Provide any value greater than 2 for `n_comps`. "
        raise ValueError(msg)
    check_eigen_arguments(n_comps)
    if key_added is _UNSET:
        key_added = _preset_key_added()
    adata = adata.copy() if copy else adata
    uns_key, obsm_key = diffmap_keys(key_added)
    dpt = Neighbors(adata, neighbors_key=neighbors_key)
    dpt.compute_transitions()
    dpt.compute_eigen(n_comps=n_comps, rng=seed)
    adata.obsm[obsm_key] = dpt.eigen_basis
    adata.uns[uns_key] = dpt.eigen_values if key_added is None else dict(evals=dpt.eigen_values)
    return adata if copy else None
