"""`sc.metrics.morans_i` and `sc.metrics.gearys_c` on MI355X (reference: metrics/_morans_i.py, metrics/_gearys_c.py and
metrics/_common.py of src/scanpy).

With W the graph (every stored entry w_ij counts as it is), x a feature over the n cells and z = x - mean(x):

    I = n / W_sum * sum_ij w_ij z_i z_j / sum_i z_i^2          C = (n - 1) / (2 W_sum) * sum_ij w_ij (x_i - x_j)^2 / sum_i z_i^2

The reference walks the graph once per feature on the CPU.  Here the features travel in cell-major slabs of 64 and one sweep of
the graph serves a whole slab (csrc/graph_autocorr.hip: `scamd_graph_autocorr_slab_{f32,f64}`, float64 arithmetic, fixed
summation order, both numerators from the same sweep); the host does the two divisions.  How the values reach a slab:

* dense, cell-major in memory (`obsm['X_pca']`, whose `.T` the reference passes): read in place, up to 128 features uploaded
  whole, wider arrays 64 columns at a time;
* dense, feature-major: 64 rows uploaded at a time and transposed on the device (`scamd_transpose_slab_*`);
* sparse: the cell-major CSR is resident as float32 and densified 64 features at a time (`scamd_csr_dense_slab_f32`); a CSC
  `vals` (features x cells) IS that CSR, a CSR `vals` goes through the device transpose; float64 data that float32 cannot hold
  exactly is densified on the host instead, slab by slab in float64 (slower: the host touches every stored entry per slab)."""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd
from scipy import sparse

from .._anndata import is_anndata

SLAB = 64
IN_PLACE_MAX = 2 * SLAB  # a dense cell-major array of up to two slabs is uploaded whole and read in place


class GpuAutocorrBackend:
    """The only product backend: every pass runs through libscanpy_amd.so (raises without a GPU)."""

    def __init__(self):
        from .. import _kernels
        from .._device import require_gpu

        self.K = _kernels
        self.device = require_gpu()

    def _up(self, a, dtype):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def open_graph(self, indptr, indices, weights, n: int) -> dict:
        return {"indptr": self._up(indptr, np.int64), "indices": self._up(indices, np.int32),
                "weights": self._up(weights, weights.dtype), "n": int(n)}

    def weight_sum(self, g: dict) -> float:
        return self.K.graph_weight_sum(g["weights"])

    def stats(self, g: dict, slab, ld: int, ncols: int, offset: int = 0) -> dict:
        """-> mean, z2, moran, geary, min, max: numpy float64 [ncols] for the features at slab[offset + j * ld + l]"""
        out = self.K.graph_autocorr_slab(g["indptr"], g["indices"], g["weights"], g["n"], slab, ld, ncols, offset=offset)
        return dict(zip(("mean", "z2", "moran", "geary", "min", "max"), (o.cpu().numpy() for o in out)))

    def dense_cell_major(self, block: np.ndarray):
        """a host [n, b] block as it is (C order) -> the device array, ld = b"""
        return self._up(block, block.dtype).reshape(-1)

    def rows_slab(self, rows: np.ndarray):
        """host feature-major rows [b <= 64, n] -> the cell-major device slab, ld = 64"""
        return self.K.transpose_slab(self._up(rows, rows.dtype)).reshape(-1)

    def csr_cell_major(self, indptr, indices, data, n: int, m: int) -> dict:
        """canonical CSR cells x features (float32 values) -> resident handle"""
        return {"indptr": self._up(indptr, np.int64), "indices": self._up(indices, np.int32), "data": self._up(data, np.float32),
                "n": int(n), "m": int(m)}

    def csr_feature_major(self, indptr, indices, data, n: int, m: int) -> dict:
        """canonical CSR features x cells -> the resident cell-major CSR, by the device transpose"""
        t_indptr, t_indices, t_data = self.K.csr_transpose(self._up(indptr, np.int64), self._up(indices, np.int32),
                                                           self._up(data, np.float32), int(m), int(n))
        return {"indptr": t_indptr, "indices": t_indices, "data": t_data, "n": int(n), "m": int(m)}

    def csr_slab(self, h: dict, c0: int, ncols: int):
        return self.K.csr_dense_slab(h["indptr"], h["indices"], h["data"], h["n"], h["m"], c0, ncols).reshape(-1)


def default_backend():
    return GpuAutocorrBackend()


# ---------------------------------------------------------------------------------------------------------------------
# the graph argument
# ---------------------------------------------------------------------------------------------------------------------
def _get_graph(adata, *, use_graph=None, neighbors_key=None):
    """metrics/_common.py `_get_graph` with the `NeighborsView` lookup it does (src/scanpy/_utils/__init__.py:902-924)"""
    if use_graph is not None:
        if neighbors_key is not None:
            msg = "Cannot specify both `use_graph` and `neighbors_key`."
            raise TypeError(msg)
        return adata.obsp[use_graph]
    if neighbors_key is None or neighbors_key == "neighbors":
        if "neighbors" not in adata.uns:
            msg = 'No "neighbors" in .uns'
            raise KeyError(msg)
        conn_key = "connectivities"
    else:
        if neighbors_key not in adata.uns:
            msg = f"No {neighbors_key!r} in .uns"
            raise KeyError(msg)
        conn_key = adata.uns[neighbors_key]["connectivities_key"]
    if conn_key not in adata.obsp:
        msg = "Must run neighbors first."
        raise ValueError(msg)
    return adata.obsp[conn_key]


def _refuse_lazy(x, what: str) -> None:
    if getattr(x, "is_backed", False):
        raise NotImplementedError(f"{what} is an on-disk (backed) matrix: graph autocorrelation needs it in memory "
                                  "(`.to_memory()`, or read without backed='r')")
    if type(x).__module__.split(".")[0] == "dask":
        raise NotImplementedError(f"{what} is a dask array: graph autocorrelation is offered for in-memory arrays only "
                                  "(`.compute()` first)")


def _host_graph(graph):
    _refuse_lazy(graph, "the graph")
    if not sparse.issparse(graph):
        raise TypeError(f"the graph must be a scipy sparse matrix (or an AnnData that holds one), got {type(graph)}")
    if graph.shape[0] != graph.shape[1]:
        raise ValueError(f"`g` should be a square adjacency matrix, got shape {graph.shape}")
    n = graph.shape[0]
    if n >= 2 ** 31:
        raise NotImplementedError(f"{n} cells: graph autocorrelation is offered below 2^31 cells")
    g = graph if graph.format == "csr" else graph.tocsr()
    weights = g.data if g.data.dtype == np.float32 else g.data.astype(np.float64, copy=False)
    if g.nnz and (int(g.indices.min()) < 0 or int(g.indices.max()) >= n):
        raise ValueError("the graph holds a column index outside [0, n)")
    return g.indptr, g.indices, weights, n


# ---------------------------------------------------------------------------------------------------------------------
# the values: which dtype travels, and the slabs
# ---------------------------------------------------------------------------------------------------------------------
def _travel_dtype(dt) -> np.dtype:
    """float32 and integers of at most 16 bits are exact in float32; everything wider travels as float64"""
    dt = np.dtype(dt)
    if dt.kind == "b" or dt == np.float32 or dt == np.float16 or (dt.kind in "iu" and dt.itemsize <= 2):
        return np.dtype(np.float32)
    if dt.kind in "iuf":
        return np.dtype(np.float64)
    raise TypeError(f"graph autocorrelation needs numeric values, got dtype {dt}")


def _canonical(x):
    if not x.has_canonical_format:
        x = x.copy()
        x.sum_duplicates()
    return x


def _sparse_slabs(be, vals, n: int):
    """vals: scipy sparse, features x cells -> generator of (slab, ld, ncols, offset)"""
    m = vals.shape[0]
    travel = _travel_dtype(vals.dtype)
    if vals.format not in ("csr", "csc"):
        vals = vals.tocsr()
    if travel == np.float64:
        data64 = vals.data.astype(np.float64, copy=False)
        with np.errstate(over="ignore", invalid="ignore"):
            back = data64.astype(np.float32).astype(np.float64)
        if not np.all((back == data64) | np.isnan(data64)):
            # float32 would round: densify on the host, 64 features at a time, in float64
            cells = _canonical(vals.T.tocsr())
            for c0 in range(0, m, SLAB):
                b = min(SLAB, m - c0)
                block = np.ascontiguousarray(cells[:, c0:c0 + b].toarray(), dtype=np.float64)
                yield be.dense_cell_major(block), b, b, 0
            return
    vals = _canonical(vals)
    if vals.format == "csc":  # features x cells by columns: the arrays ARE the cell-major CSR
        h = be.csr_cell_major(vals.indptr, vals.indices, vals.data, n, m)
    else:
        h = be.csr_feature_major(vals.indptr, vals.indices, vals.data, n, m)
    for c0 in range(0, m, SLAB):
        b = min(SLAB, m - c0)
        yield be.csr_slab(h, c0, b), SLAB, b, 0


def _dense_slabs(be, vals: np.ndarray, n: int):
    """vals: numpy [m, n] -> generator of (slab, ld, ncols, offset)"""
    m = vals.shape[0]
    travel = _travel_dtype(vals.dtype)
    cells = vals.T
    if m > 1 and cells.flags.c_contiguous:  # cell-major in memory: no transpose anywhere
        if m <= IN_PLACE_MAX:
            whole = be.dense_cell_major(np.ascontiguousarray(cells, dtype=travel))
            for c0 in range(0, m, SLAB):
                yield whole, m, min(SLAB, m - c0), c0
            return
        for c0 in range(0, m, SLAB):
            b = min(SLAB, m - c0)
            yield be.dense_cell_major(np.ascontiguousarray(cells[:, c0:c0 + b], dtype=travel)), b, b, 0
        return
    for f0 in range(0, m, SLAB):
        b = min(SLAB, m - f0)
        yield be.rows_slab(np.ascontiguousarray(vals[f0:f0 + b], dtype=travel)), SLAB, b, 0


def _autocorr(graph, vals, which: str, name: str):
    indptr, indices, weights, n = _host_graph(graph)
    _refuse_lazy(vals, "`vals`")
    if isinstance(vals, (pd.DataFrame, pd.Series)):
        vals = vals.to_numpy()
    scalar = False
    if sparse.issparse(vals):
        if vals.ndim != 2:
            vals = sparse.csr_matrix(vals)
    else:
        if not isinstance(vals, np.ndarray):
            raise TypeError(f"Unsupported type {type(vals)}")
        if vals.ndim == 1:
            scalar, vals = True, vals.reshape(1, -1)
        elif vals.ndim != 2:
            raise NotImplementedError(f"{name} metric not implemented for vals of type {type(vals).__name__} and ndim {vals.ndim}.")
    if vals.shape[1] != n:
        raise ValueError(f"`vals` has {vals.shape[1]} cells, the graph has {n}")
    m = vals.shape[0]
    _travel_dtype(vals.dtype)
    res = {key: np.full(m, np.nan) for key in ("mean", "z2", "moran", "geary", "min", "max")}
    w_sum = np.float64(0.0)
    if n > 0 and m > 0:
        be = default_backend()
        g = be.open_graph(indptr, indices, weights, n)
        w_sum = np.float64(be.weight_sum(g))
        slabs = _sparse_slabs(be, vals, n) if sparse.issparse(vals) else _dense_slabs(be, vals, n)
        f0 = 0
        for slab, ld, ncols, offset in slabs:
            part = be.stats(g, slab, ld, ncols, offset)
            for key in res:
                res[key][f0:f0 + ncols] = part[key]
            f0 += ncols
        assert f0 == m
    finite = np.isfinite(res["mean"])
    constant = (res["min"] == res["max"]) & finite if n > 0 else np.ones(m, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if which == "moran":
            out = np.float64(n) / w_sum * res["moran"] / res["z2"]
        else:
            out = np.float64(n - 1) / (2 * w_sum) * res["geary"] / res["z2"]
    out[constant | ~finite] = np.nan
    if scalar:
        return np.float64(out[0])
    if constant.any():
        warnings.warn(f"{int(constant.sum())} variables were constant, will return nan for these.", UserWarning, stacklevel=3)
    return out


def _get_vals(adata, *, use_raw, layer, obsm, obsp):
    """`scanpy.get._get_arr(adata, use_raw=, layer=, obsm=, obsp=)`: cells x features"""
    if not isinstance(use_raw, bool):
        raise TypeError(f"use_raw expected to be bool, was {type(use_raw)}.")
    given = [k for k, v in (("layer", layer), ("use_raw", use_raw), ("obsm", obsm), ("obsp", obsp)) if v]
    if len(given) > 1:
        raise ValueError(f"Only one of {', '.join(given)} can be specified.")
    if layer is not None:
        return adata.layers[layer]
    if use_raw:
        return adata.raw.X
    if obsm is not None:
        return adata.obsm[obsm]
    if obsp is not None:
        return adata.obsp[obsp]
    return adata.X


def _metric(which, name, adata_or_graph, vals, use_graph, neighbors_key, layer, obsm, obsp, use_raw):
    if is_anndata(adata_or_graph):
        adata = adata_or_graph
        graph = _get_graph(adata, use_graph=use_graph, neighbors_key=neighbors_key)
        if vals is None:
            arr = _get_vals(adata, use_raw=use_raw, layer=layer, obsm=obsm, obsp=obsp)
            _refuse_lazy(arr, "the selected matrix")
            if isinstance(arr, pd.DataFrame):
                arr = arr.to_numpy()
            vals = arr.T
        return _autocorr(graph, vals, which, name)
    if vals is None:
        raise TypeError("`vals` must be given when the first argument is the graph itself")
    return _autocorr(adata_or_graph, vals, which, name)


def morans_i(adata_or_graph, /, vals=None, *, use_graph=None, neighbors_key=None, layer=None, obsm=None, obsp=None,
             use_raw=False):
    """Moran's I global autocorrelation statistic (same signature as the reference).

    adata_or_graph: an AnnData (the graph is `obsp[use_graph]`, or the connectivities of `uns[neighbors_key or 'neighbors']`)
    or the graph itself as a scipy sparse matrix.  vals: `(n_cells,)` -> a float64 scalar, or `(n_features, n_cells)` (numpy,
    DataFrame, any scipy sparse format) -> a float64 array; left out, `layer` / `obsm` / `obsp` / `use_raw` select cells x
    features from the AnnData.  Constant features return NaN (with one UserWarning for 2-D input), as does a feature holding a
    non-finite value."""
    return _metric("moran", "Moran’s I", adata_or_graph, vals, use_graph, neighbors_key, layer, obsm, obsp, use_raw)


def gearys_c(adata_or_graph, /, vals=None, *, use_graph=None, neighbors_key=None, layer=None, obsm=None, obsp=None,
             use_raw=False):
    """Geary's C autocorrelation statistic (same signature as the reference; see `morans_i` for the arguments).  The numerator
    is summed from the differences x_i - x_j themselves: a signal constant on every connected component gives exactly 0."""
    return _metric("geary", "Geary’s C", adata_or_graph, vals, use_graph, neighbors_key, layer, obsm, obsp, use_raw)
