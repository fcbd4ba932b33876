"""`sc.pp.neighbors` on MI355X (src/scanpy/neighbors/__init__.py:88-299, 399-710).

kNN search and the umap connectivities run in HIP kernels (`scamd_knn_l2_f32`,
`scamd_fuzzy_simplicial_set_f32`); slot names, `uns[...]['params']`, the self-column conventions of
src/scanpy/neighbors/_common.py and the error behaviour follow the reference.  The search is EXACT
(the reference's `transformer='sklearn'` semantics) for every n -- where the reference would switch to
approximate NN-descent at n >= 8192 (neighbors/__init__.py:734-739) this path stays exact, also for
`transformer='pynndescent'`.  The approximate search is opt-in: `transformer='ivf'` (probes
`settings.knn_nprobe` cells of the k-means quantiser, `scamd_knn_l2_ivf_f32`) or an
`MI355XKNNTransformer(nprobe=...)` instance.
"""
from __future__ import annotations

import warnings
from types import MappingProxyType

import numpy as np
from scipy import sparse

from .._anndata import is_anndata
from .._utils import _UNSET, choose_representation, resolve_seed
from ._common import (
    get_indices_distances_from_dense_matrix,
    get_indices_distances_from_sparse_matrix,
    graph_from_device,
    sparse_distances_from_device,
)
from ._transformer import METRICS, MI355XKNNTransformer, knn_search_device

__all__ = ["neighbors", "Neighbors", "MI355XKNNTransformer"]

_METHODS = ("umap", "gauss", "jaccard")


def _to_device(a, dtype):
    """host array or torch tensor (already on the device: the built-in search hands its lists over without a round
    trip through the host) -> contiguous device tensor of `dtype`"""
    import torch

    from .._device import require_gpu

    if isinstance(a, torch.Tensor):
        return a.to(dtype).contiguous()
    np_dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32}[dtype]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(require_gpu())


def _connectivities_umap(knn_indices, knn_dists, n_obs: int) -> sparse.csr_matrix:
    """neighbors/_connectivity.py:103-138 -> scamd_fuzzy_simplicial_set_f32."""
    import torch

    from .. import _kernels

    indptr, indices, data, _, _ = _kernels.fuzzy_simplicial_set(_to_device(knn_indices, torch.int32),
                                                                _to_device(knn_dists, torch.float32))
    return graph_from_device(indptr, indices, data, n_obs)


def _connectivities_kernel(method: str, knn_indices, knn_dists, n_obs: int) -> sparse.csr_matrix:
    """neighbors/_connectivity.py:21-100 ('gauss', sparse branch) / :141-186 ('jaccard') ->
    scamd_gauss_connectivities_f32 / scamd_jaccard_connectivities_f32."""
    import torch

    from .. import _kernels

    idx = _to_device(knn_indices, torch.int32)
    if method == "gauss":
        indptr, indices, data = _kernels.gauss_connectivities(idx, _to_device(knn_dists, torch.float32))
    else:
        indptr, indices, data = _kernels.jaccard_connectivities(idx)
    return graph_from_device(indptr, indices, data, n_obs)


class Neighbors:
    """Data represented as graph of nearest neighbors (the slice of the reference class the path needs)."""

    def __init__(self, adata, *, n_dcs=None, neighbors_key=None, diffmap_key=None):
        self._adata = adata
        self._iroot = _UNSET  # the root cell is looked for when `.iroot` is first read (`tl.dpt`), never by `pp.neighbors`
        self._transitions_sym = None
        self.Z = None
        self._eigen_info = None
        self._distances = None
        self._connectivities = None
        self.n_neighbors = None
        self.knn = None
        self.rp_forest = None
        self._cc = None
        key = "neighbors" if neighbors_key is None else neighbors_key
        if key in adata.uns:  # restore an existing graph (neighbors/__init__.py:437-474)
            info = adata.uns[key]
            ck, dk = info.get("connectivities_key", "connectivities"), info.get("distances_key", "distances")
            if ck in adata.obsp:
                self._connectivities = adata.obsp[ck]
            if dk in adata.obsp:
                self._distances = adata.obsp[dk]
            self.knn = sparse.issparse(self._distances) or sparse.issparse(self._connectivities)
            if "params" in info:
                self.n_neighbors = info["params"]["n_neighbors"]
            else:  # estimate from the stored graph (neighbors/__init__.py:446-464)

                def count_nonzero(a) -> int:
                    return a.count_nonzero() if sparse.issparse(a) else int(np.count_nonzero(a))

                if self._connectivities is None:
                    self.n_neighbors = int(count_nonzero(self._distances) / self._distances.shape[0])
                else:
                    self.n_neighbors = int(count_nonzero(self._connectivities) / self._connectivities.shape[0] / 2)
            self._cc = None  # `:466-472`, lazily (see `_connected_components`)
        # a stored diffusion map (neighbors/__init__.py:476-497)
        keys = (diffmap_key, diffmap_key) if diffmap_key else existing_diffmap_keys(adata)
        if keys:
            evals = adata.uns[keys[0]]
            self._eigen_values = np.asarray(evals["evals"] if isinstance(evals, dict) else evals)  # (`uns[key_added]['evals']`)
            self._eigen_basis = adata.obsm[keys[1]]
            if n_dcs is not None:
                if n_dcs > len(self._eigen_values):
                    msg = f"Cannot instantiate using `n_dcs`={n_dcs}. Compute diffmap/spectrum with more components first."
                    raise ValueError(msg)
                self._eigen_values = self._eigen_values[:n_dcs]
                self._eigen_basis = self._eigen_basis[:, :n_dcs]
            self.n_dcs = len(self._eigen_values)
        else:
            self._eigen_values = None
            self._eigen_basis = None
            self.n_dcs = None

    @property
    def _connected_components(self):
        """(n_components, labels) of the connectivity graph.  The reference computes it eagerly at the end of
        `compute_neighbors` / on restore (scipy `connected_components`: ~0.3-3 s at 1M cells, more than the GPU spends
        on the whole path); nothing on this path reads it, so it is computed when first asked for."""
        if self._cc is None and sparse.issparse(self._connectivities):
            from scipy.sparse.csgraph import connected_components

            self._cc = connected_components(self._connectivities)
        return self._cc

    @property
    def _number_connected_components(self):
        if self._connectivities is None:
            return None
        cc = self._connected_components
        return 1 if cc is None else cc[0]

    @property
    def distances(self):
        return self._distances

    @property
    def connectivities(self):
        return self._connectivities

    # ---- diffusion maps and pseudotime (neighbors/__init__.py:516-575, 791-985) --------------------------------------------
    @property
    def transitions_sym(self):
        """Symmetrised transition matrix (scipy CSR, float32)."""
        return self._transitions_sym

    @property
    def transitions(self):
        """Transition matrix `Z T_sym Z^-1` (neighbors/__init__.py:516-537)."""
        return self.Z @ self.transitions_sym @ self.Z.power(-1)

    @property
    def eigen_values(self):
        return self._eigen_values

    @property
    def eigen_basis(self):
        return self._eigen_basis

    @property
    def distances_dpt(self):
        return _DptRows(self)

    def compute_transitions(self, *, density_normalize: bool = True) -> None:
        """neighbors/__init__.py:791-828 -> scamd_transitions_sym_f32.  Makes `.transitions_sym`, `.transitions` and `.Z`
        available (scipy matrices on the host, as the reference returns them)."""
        import torch

        from .. import _kernels

        conn = self._connectivities
        if not sparse.issparse(conn):
            msg = "compute_transitions: a dense connectivity matrix is outside the MI355X path (pp.neighbors stores a sparse one)."
            raise NotImplementedError(msg)
        conn = sparse.csr_matrix(conn)
        conn.sort_indices()
        n = conn.shape[0]
        if np.any(np.diff(conn.indptr) == 0):
            msg = "compute_transitions: the graph has a cell without neighbours (an empty row)."
            raise ValueError(msg)
        t, z = _kernels.transitions_sym(_to_device(conn.indptr, torch.int64), _to_device(conn.indices, torch.int32),
                                        _to_device(conn.data, torch.float32), n, density_normalize=density_normalize)
        self._transitions_sym = sparse.csr_matrix((t.cpu().numpy(), conn.indices.copy(), conn.indptr.copy()), shape=conn.shape)
        self.Z = sparse.diags(1.0 / z.cpu().numpy()).tocsr()

    def compute_eigen(self, *, n_comps: int = 15, sort: str = "decrease", rng=None, random_state=_UNSET, sym=None) -> None:
        """neighbors/__init__.py:830-895 -> scamd_diffmap_f32: the `n_comps` leading eigenpairs of `.transitions_sym`
        (`eigsh(which='LM')` there), float32 as the reference casts them.  `rng` / `random_state` seed the start block."""
        import torch

        from .. import _kernels

        if self._transitions_sym is None:
            msg = "Run `.compute_transitions` first."
            raise ValueError(msg)
        check_eigen_arguments(n_comps, sort)
        seed, _ = resolve_seed(rng, random_state)
        t = self._transitions_sym
        n = t.shape[0]
        n_comps = min(n - 1, n_comps)
        if np.any(np.diff(t.indptr) == 0):
            msg = "compute_eigen: the transition matrix has an empty row."
            raise ValueError(msg)
        evals, evecs, info = _kernels.diffmap(_to_device(t.indptr, torch.int64), _to_device(t.indices, torch.int32),
                                              _to_device(t.data, torch.float32), n, n_comps, seed=seed)
        if not info["converged"]:
            from .._lib import ScamdError

            raise ScamdError(f"compute_eigen: the subspace iteration did not converge ({info})")
        self._eigen_info = info
        self._eigen_values = evals.to(torch.float32).cpu().numpy()
        self._eigen_basis = evecs.to(torch.float32).cpu().numpy()
        # (the reference counts the connected components of the graph, :892; every component owns one eigenvalue 1, so the
        # eigenvalues just computed say the same without a pass over the graph on the host)
        if int(np.sum(self._eigen_values > 1.0 - 1e-5)) > len(self._eigen_values) / 2:
            warnings.warn("Transition matrix has many disconnected components!", UserWarning, stacklevel=2)

    @property
    def iroot(self):
        """index of the root cell, from `uns['iroot']` or `uns['xroot']` / `var['xroot']` (neighbors/__init__.py:897-918); the
        reference looks for it when the object is built, here the first read does"""
        if self._iroot is _UNSET:
            self._init_iroot()
        return self._iroot

    @iroot.setter
    def iroot(self, value):
        self._iroot = value

    def _init_iroot(self):
        """neighbors/__init__.py:897-918."""
        self._iroot = None
        adata = self._adata
        uns, var = getattr(adata, "uns", {}), getattr(adata, "var", None)
        if "iroot" in uns:
            if uns["iroot"] >= adata.n_obs:
                warnings.warn(f"Root cell index {uns['iroot']} does not exist for {adata.n_obs} samples. It’s ignored.",
                              UserWarning, stacklevel=3)
            else:
                self.iroot = uns["iroot"]
            return
        xroot = None
        if "xroot" in uns:
            xroot = uns["xroot"]
        elif var is not None and "xroot" in var:
            xroot = var["xroot"]
        if xroot is not None and np.size(xroot) == adata.shape[1]:
            self._set_iroot_via_xroot(np.asarray(xroot))

    def _set_iroot_via_xroot(self, xroot):
        """neighbors/__init__.py:955-985: the cell nearest to `xroot` in X -- the first within 1e-10, else the first of the
        nearest; a host loop over the rows there, row blocks here."""
        if self._adata.shape[1] != xroot.size:
            msg = "The root vector you provided does not have the correct dimension."
            raise ValueError(msg)
        x = self._adata.X
        xroot = np.asarray(xroot).ravel()
        dsq = np.empty(x.shape[0])
        for i0 in range(0, x.shape[0], 4096):
            blk = x[i0:i0 + 4096]
            diff = (blk.toarray() if sparse.issparse(blk) else np.asarray(blk)) - xroot
            dsq[i0:i0 + 4096] = np.einsum("ij,ij->i", diff, diff)
        exact = np.flatnonzero(np.sqrt(dsq) < 1e-10)
        iroot = int(exact[0]) if exact.size else (int(np.argmin(dsq)) if dsq.min() < 1e10 else 0)
        if self.iroot is not None and iroot != self.iroot:
            warnings.warn(f"Changing index of iroot from {self.iroot} to {iroot}.", UserWarning, stacklevel=3)
        self.iroot = iroot

    def _get_dpt_row(self, i: int, *, scale: bool = False) -> np.ndarray:
        """One row of the DPT distance matrix (neighbors/__init__.py:920-948); scale: divided by its largest finite entry, as
        `_set_pseudotime` does (:950-953), in the same call of scamd_dpt_pseudotime_f32."""
        import torch

        from .. import _kernels

        labels = None
        if self._number_connected_components is not None and self._number_connected_components > 1:
            labels = _to_device(self._connected_components[1], torch.int32)
        evals = _to_device(np.asarray(self.eigen_values, dtype=np.float32), torch.float32)
        basis = _to_device(np.asarray(self.eigen_basis, dtype=np.float32), torch.float32)
        return _kernels.dpt_pseudotime(evals, basis, int(i), labels, scale=scale).cpu().numpy()

    def _set_pseudotime(self):
        """Pseudotime with respect to the root cell (neighbors/__init__.py:950-953)."""
        self.pseudotime = self._get_dpt_row(self.iroot, scale=True)

    def compute_neighbors(self, n_neighbors: int = 30, n_pcs: int | None = None, *, use_rep: str | None = None,
                          knn: bool = True, method: str | None = "umap", transformer=None,
                          metric="euclidean", metric_kwds=MappingProxyType({}), rng=None, random_state=_UNSET):
        """neighbors/__init__.py:578-673."""
        if transformer is not None and not isinstance(transformer, str):
            n_neighbors = transformer.get_params()["n_neighbors"]
        elif n_neighbors > self._adata.shape[0]:  # very small datasets
            n_neighbors = 1 + int(0.5 * self._adata.shape[0])
            warnings.warn(f"n_obs too small: adjusting to `n_neighbors = {n_neighbors}`", UserWarning, stacklevel=2)
        if method not in _METHODS and method is not None:
            msg = f"`method` needs to be one of {set(_METHODS)}."
            raise ValueError(msg)
        conn_method = method if method in {"gauss", "jaccard", None} else "umap"
        if not knn and not (conn_method == "gauss" and transformer is None):
            msg = f"`method = {method!r} only with `knn = True`."
            raise ValueError(msg)
        if conn_method == "gauss" and not knn:
            msg = "method='gauss' with knn=False builds a dense n x n kernel matrix: not offered on the MI355X path."
            raise NotImplementedError(msg)
        if isinstance(transformer, str) and transformer not in {"sklearn", "pynndescent", "mi355x", "ivf"}:
            msg = f"Unknown transformer: {transformer}. Try passing a class or one of {{'pynndescent', 'sklearn'}}"
            raise ValueError(msg)
        self.n_neighbors = n_neighbors
        self.knn = knn
        x = choose_representation(self._adata, use_rep=use_rep, n_pcs=n_pcs)
        if transformer is None or isinstance(transformer, str):
            if callable(metric) or metric not in METRICS:
                msg = (f"metric={metric!r}: the MI355X kNN kernel offers {METRICS}; pass a `transformer` for other "
                       "metrics.")
                raise NotImplementedError(msg)
            # built-in exact search: (n, k) arrays straight from the device, self column first with an
            # exact 0 (what the reference gets after zeroing the diagonal, neighbors/__init__.py:639-648)
            k = min(n_neighbors, self._adata.n_obs)
            # (the lists stay on the device: they feed the connectivity kernel as they are)
            nprobe = None
            if transformer == "ivf":  # approximate: the cells of the quantiser nearest to the query's own
                from .._settings import settings

                nprobe = int(settings.knn_nprobe)
            knn_indices, knn_distances = knn_search_device(x, k, metric=metric, nprobe=nprobe)
            # (the download of the distances runs on a side stream under the connectivity kernels below)
            pending_distances = sparse_distances_from_device(knn_indices, knn_distances, deferred=True)
        else:  # user-supplied estimator instance: the reference's plug-in route, used as-is (:788, :638)
            self._distances = transformer.fit_transform(x)
            knn_indices, knn_distances = get_indices_distances_from_sparse_matrix(self._distances, n_neighbors)
            pending_distances = None
        self._connectivities = None
        try:
            if conn_method == "umap":
                self._connectivities = _connectivities_umap(knn_indices, knn_distances, self._adata.n_obs)
            elif conn_method in {"gauss", "jaccard"}:  # neighbors/__init__.py:694-708
                self._connectivities = _connectivities_kernel(conn_method, knn_indices, knn_distances, self._adata.n_obs)
        finally:
            if pending_distances is not None:
                self._distances = pending_distances()
        self._cc = None  # connected components (neighbors/__init__.py:666-671) are computed on first use


class _DptRows:
    """`Neighbors.distances_dpt`: row i of the DPT distances on demand (the reference's OnFlySymMatrix,
    neighbors/__init__.py:547-575)"""

    def __init__(self, neighbors):
        self._neighbors = neighbors

    def __getitem__(self, i):
        return self._neighbors._get_dpt_row(int(i))


MAX_DIFFMAP_COMPS = 26  # the block of scamd_diffmap_f32 holds n_comps + 6 <= 32 columns


def check_eigen_arguments(n_comps: int, sort: str = "decrease") -> None:
    """what `compute_eigen` refuses, before anything touches the library"""
    if sort != "decrease":
        msg = f"compute_eigen: sort={sort!r} (the smallest eigenvalues, eigsh(which='SM')) is not offered on the MI355X path."
        raise NotImplementedError(msg)
    if n_comps == 0:
        msg = "compute_eigen: n_comps=0 (the full dense eigendecomposition of an n x n matrix) is not offered on the MI355X path."
        raise NotImplementedError(msg)
    if n_comps > MAX_DIFFMAP_COMPS:
        msg = (f"compute_eigen: n_comps={n_comps}: the device eigensolver holds a block of n_comps + 6 <= 32 columns, "
               f"at most {MAX_DIFFMAP_COMPS} components.")
        raise NotImplementedError(msg)


def diffmap_keys(key_added) -> tuple:
    """(uns key, obsm key) of a diffusion map (src/scanpy/_keys.py:76-79)"""
    return ("diffmap_evals", "X_diffmap") if key_added is None else (key_added, key_added)


def existing_diffmap_keys(adata):
    """the keys of a stored diffusion map under either preset, V1 first (src/scanpy/_keys.py:113-126), or None"""
    obsm = getattr(adata, "obsm", None)
    if obsm is None:
        return None
    for key_added in (None, "diffmap"):
        keys = diffmap_keys(key_added)
        if keys[1] in obsm and keys[0] in adata.uns:
            return keys
    return None


def _get_metadata(key_added, **params):
    """neighbors/__init__.py:302-316."""
    if key_added is None:
        return "neighbors", dict(connectivities_key="connectivities", distances_key="distances", params=params)
    return key_added, dict(connectivities_key=f"{key_added}_connectivities", distances_key=f"{key_added}_distances",
                           params=params)


def neighbors(  # noqa: PLR0913
    adata,
    n_neighbors: int = 15,
    n_pcs: int | None = None,
    *,
    distances=None,
    use_rep: str | None = None,
    knn: bool = True,
    method: str = "umap",
    transformer=None,
    metric=None,
    metric_kwds=MappingProxyType({}),
    rng=None,
    random_state=_UNSET,
    key_added: str | None = None,
    copy: bool = False,
):
    """Nearest-neighbour distance matrix and neighbourhood graph (drop-in for `scanpy.pp.neighbors`,
    src/scanpy/neighbors/__init__.py:88-299).  Writes `.obsp['distances']` (n_neighbors-1 stored entries
    per row), `.obsp['connectivities']` and `.uns['neighbors']`."""
    if not is_anndata(adata):
        raise TypeError("neighbors() expects an AnnData-like object")
    _, meta_random_state = resolve_seed(rng, random_state)
    if distances is None:
        if metric is None:
            metric = "euclidean"
        adata = adata.copy() if copy else adata
        neighbors_ = Neighbors(adata)
        neighbors_.compute_neighbors(n_neighbors, n_pcs=n_pcs, use_rep=use_rep, knn=knn, method=method,
                                     transformer=transformer, metric=metric, metric_kwds=metric_kwds)
    else:  # neighbors/__init__.py:232-270: precomputed distances, connectivities only
        ignored = set()
        if use_rep is not None:
            ignored.add("use_rep")
        if knn is not True:
            ignored.add("knn")
        if n_pcs is not None:
            ignored.add("n_pcs")
        if metric_kwds:
            ignored.add("metric_kwds")
        if meta_random_state.get("random_state", None) != 0 or rng is not None:
            ignored.add("rng/random_state")
            meta_random_state.pop("random_state", None)
        if ignored:
            warnings.warn(f"Parameter(s) ignored if `distances` is given: {ignored}", UserWarning, stacklevel=2)
        if callable(metric):
            msg = "`metric` must be a string if `distances` is given."
            raise TypeError(msg)
        adata = adata.copy() if copy else adata
        if sparse.issparse(distances):
            distances = sparse.csr_matrix(distances, copy=True)
            distances.setdiag(0)
            distances.eliminate_zeros()
        else:
            distances = np.asarray(distances).copy()
            np.fill_diagonal(distances, 0)
        if method != "umap":
            raise NotImplementedError(f"method={method!r} is outside the MI355X hot path")
        neighbors_ = Neighbors(adata)
        neighbors_.n_neighbors = n_neighbors
        neighbors_.knn = True
        neighbors_._distances = distances
        if sparse.issparse(distances):
            knn_indices, knn_distances = get_indices_distances_from_sparse_matrix(distances, n_neighbors)
        else:
            knn_indices, knn_distances = get_indices_distances_from_dense_matrix(distances, n_neighbors)
        neighbors_._connectivities = _connectivities_umap(knn_indices, knn_distances, adata.n_obs)

    key_added, neighbors_dict = _get_metadata(
        key_added,
        n_neighbors=neighbors_.n_neighbors,
        method=method,
        metric=metric,
        **meta_random_state,
        **({} if not metric_kwds else dict(metric_kwds=metric_kwds)),
        **({} if use_rep is None else dict(use_rep=use_rep)),
        **({} if n_pcs is None else dict(n_pcs=n_pcs)),
    )
    adata.uns[key_added] = neighbors_dict
    adata.obsp[neighbors_dict["distances_key"]] = neighbors_.distances
    adata.obsp[neighbors_dict["connectivities_key"]] = neighbors_.connectivities
    return adata if copy else None
