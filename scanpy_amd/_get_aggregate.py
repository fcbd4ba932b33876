"""`sc.get.aggregate` on MI355X (reference: src/scanpy/get/_aggregated.py, `_get_arr` / `_check_mask` of src/scanpy/get/get.py).

Cells (or, with axis='var', genes) are collapsed into groups: per group and variable the sum, mean, variance, number of
non-zero values and median, one layer each.  The host does the bookkeeping -- which axis, which matrix, the combined categories,
the mask, the row order by group -- and every number comes from two entry points of csrc/aggregate.hip through a backend object
(`default_backend()`; the tests put a numpy stand-in there).  Every route ends as canonical float32 CSR of (grouped axis x other
axis) on the device: a CSR matrix as it is, a CSC matrix (or the other axis of a CSR one) through the device transpose, a dense
one as the full pattern.

Where this differs from the reference:
* values travel as float32: float32, integers of magnitude <= 2^24 (their sums are exact) and float64 data that float32 holds
  exactly are accepted; other float64 and wider integers raise NotImplementedError;
* a stored value that is not finite raises ValueError (the reference lets NaN spread through the sums of its group);
* `acc=` / `AdRef` arguments (anndata.acc), backed matrices and dask arrays raise NotImplementedError."""
from __future__ import annotations

import warnings
from itertools import product

import numpy as np
import pandas as pd
from scipy import sparse

from ._anndata import AnnData, is_anndata

AGG_FUNCS = ("count_nonzero", "sum", "median", "mean", "var")
TRANSPOSE_MAX_COLUMNS = 40944   # scamd_csr_transpose_f32 keeps one counter per column in LDS
FLAG_NONFINITE = 1


class GpuAggregateBackend:
    """The only product backend: every number comes from libscanpy_amd.so (raises without a GPU)."""

    def __init__(self):
        from . import _kernels
        from ._device import require_gpu

        self.K = _kernels
        self.device = require_gpu()

    def _up(self, a, dtype):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def csr(self, indptr, indices, data, n: int, g: int) -> dict:
        """canonical CSR [n, g], float32 values -> resident handle"""
        return {"indptr": self._up(indptr, np.int64), "indices": self._up(indices, np.int32), "data": self._up(data, np.float32),
                "n": int(n), "g": int(g)}

    def csr_from_transpose(self, indptr, indices, data, n: int, g: int) -> dict:
        """the arrays are the canonical CSR of the [g, n] transpose -> the resident CSR [n, g], by the device transpose"""
        t = self.K.csr_transpose(self._up(indptr, np.int64), self._up(indices, np.int32), self._up(data, np.float32), int(g), int(n))
        return {"indptr": t[0], "indices": t[1], "data": t[2], "n": int(n), "g": int(g)}

    def aggregate(self, h: dict, codes, order, group_sizes, *, want_m2: bool, want_median: bool, mid_in_f32: bool) -> dict:
        """-> numpy [n_groups, g]: sum (float64), count_nonzero (int64), on request m2 and median (float64); flags (int)"""
        out = self.K.aggregate(h["indptr"], h["indices"], h["data"], h["n"], h["g"], self._up(codes, np.int32), self._up(order, np.int32),
                               self._up(group_sizes, np.int64), want_m2=want_m2, want_median=want_median, mid_in_f32=mid_in_f32)
        return {k: (v if isinstance(v, (int, list)) else v.cpu().numpy()) for k, v in out.items()}


def default_backend():
    return GpuAggregateBackend()


# ---------------------------------------------------------------------------------------------------------------------
# which axis, which matrix
# ---------------------------------------------------------------------------------------------------------------------
def _resolve_axis(axis) -> str:
    if isinstance(axis, (int, str)) and not isinstance(axis, bool):
        if axis in (0, "obs"):
            return "obs"
        if axis in (1, "var"):
            return "var"
    msg = f"`axis` must be either 0, 1, 'obs', or 'var', was {axis!r}"
    raise ValueError(msg)


def _is_ref(x) -> bool:
    return type(x).__module__.split(".")[0] == "anndata" and type(x).__name__ in ("AdRef", "LayerAcc", "MultiAcc", "GraphAcc")


def _get_arr(adata, dim: str, *, layer, obsm, varm):
    """the reference's `_get_arr(adata, None, dim=, layer=, obsm=, varm=)`: the matrix of (grouped axis x other axis)"""
    picked = [(k, v) for k, v in (("layer", layer), ("obsm", obsm), ("varm", varm)) if v is not None]
    if not picked:
        return adata.X.T if dim == "var" else adata.X
    if len(picked) > 1:
        names = [f"`{k}`" for k, _ in picked]
        names[-1] = f"or {names[-1]}"
        msg = f"Only one of {', '.join(names)} can be specified."
        raise ValueError(msg)
    k, v = picked[0]
    if k == "layer":
        return adata.layers[v].T if dim == "var" else adata.layers[v]
    if k == "obsm":
        if dim == "var":
            msg = "`obsm` cannot be used when `dim` is `var`"
            raise ValueError(msg)
        return adata.obsm[v]
    if dim == "obs":
        msg = "`varm` cannot be used when `dim` is `obs`"
        raise ValueError(msg)
    return adata.varm[v]


def _check_mask(adata, mask, dim: str):
    if mask is None:
        return None
    if isinstance(mask, str):
        try:
            arr = np.asarray(getattr(adata, dim)[mask])
        except KeyError:
            msg = f"Did not find `adata.{dim}[{mask!r}]`. "
            raise ValueError(msg) from None
    else:
        if len(mask) != adata.shape[0 if dim == "obs" else 1]:
            msg = "The shape of the mask do not match the data."
            raise ValueError(msg)
        arr = np.asarray(mask)
    if not pd.api.types.is_bool_dtype(arr.dtype):
        msg = "Mask array must be boolean."
        raise ValueError(msg)
    return arr.astype(bool)


def _combine_categories(label_df: pd.DataFrame):
    """-> (the combined categorical of every row, the table labelling the result's rows): categories `a_b_c` in product order,
    unused combinations dropped, a missing value in any key gives code -1"""
    cols = list(label_df.columns)
    df = pd.DataFrame({c: pd.Categorical(label_df[c]).remove_unused_categories() for c in cols}, index=label_df.index)
    cats = [df[c].cat.categories for c in cols]
    counts = [len(c) for c in cats]
    names = pd.Index(["_".join(map(str, combo)) for combo in product(*cats)])
    combos = np.indices(counts).reshape(len(counts), -1) if counts else np.zeros((0, 1), dtype=np.int64)
    table = pd.DataFrame({c: pd.Categorical.from_codes(combos[i], cats[i]) for i, c in enumerate(cols)}, index=names)
    codes = np.zeros(len(df), dtype=np.int64)
    missing = np.zeros(len(df), dtype=bool)
    for i, c in enumerate(cols):
        own = df[c].cat.codes.to_numpy().astype(np.int64)
        missing |= own < 0
        codes = codes * counts[i] + np.where(own < 0, 0, own)
    codes[missing] = -1
    combined = pd.Categorical.from_codes(codes, categories=names).remove_unused_categories()
    return combined, table.loc[combined.categories]


# ---------------------------------------------------------------------------------------------------------------------
# the values: what may travel as float32, and the CSR of (grouped axis x other axis) on the device
# ---------------------------------------------------------------------------------------------------------------------
def _refuse_lazy(x) -> None:
    if getattr(x, "is_backed", False) or type(x).__module__.split(".")[0] == "h5py":
        raise NotImplementedError("sc.get.aggregate: the matrix is on disk (backed): streaming a backed matrix is not offered, "
                                  "load it first (`.to_memory()`, or read without backed='r')")
    if type(x).__module__.split(".")[0] == "dask":
        raise NotImplementedError("sc.get.aggregate: dask arrays are not offered, `.compute()` first")


def _as_float32(values: np.ndarray) -> np.ndarray:
    dt = values.dtype
    if dt == np.float32:
        return values
    if dt.kind == "b" or dt == np.float16:
        return values.astype(np.float32)
    if dt.kind in "iu":
        if values.size and max(int(values.max()), -int(values.min())) > 2 ** 24:
            raise NotImplementedError(f"sc.get.aggregate: {dt} values beyond 2^24 in magnitude do not travel as float32 exactly")
        return values.astype(np.float32)
    if dt == np.float64:
        with np.errstate(over="ignore", invalid="ignore"):
            narrow = values.astype(np.float32)
        if not np.all((narrow == values) | np.isnan(values)):
            raise NotImplementedError("sc.get.aggregate: float64 values that float32 does not hold exactly are not offered "
                                      "(the matrix travels as float32)")
        return narrow
    raise NotImplementedError(f"sc.get.aggregate: values of dtype {dt}")


def _to_device(be, data):
    """data: scipy sparse or numpy [n, g] -> (handle, is_sparse, dtype of the input)"""
    n, g = data.shape
    if max(n, g) >= 2 ** 31:
        raise NotImplementedError("sc.get.aggregate is offered below 2^31 rows and columns")
    if sparse.issparse(data):
        if data.format not in ("csr", "csc"):
            data = data.tocsr()
        if data.format == "csc" and n > TRANSPOSE_MAX_COLUMNS:  # (beyond the device transpose: one pass on the host)
            data = data.tocsr()
        if not data.has_canonical_format:
            data = data.copy()
            data.sum_duplicates()
        values = _as_float32(np.asarray(data.data))
        make = be.csr if data.format == "csr" else be.csr_from_transpose
        return make(np.asarray(data.indptr, dtype=np.int64), np.asarray(data.indices, dtype=np.int32), values, n, g), True, data.dtype
    dense = np.asarray(data)
    if dense.ndim != 2:
        raise ValueError(f"sc.get.aggregate needs a 2-d matrix, got {dense.ndim} dimensions")
    values = _as_float32(np.ascontiguousarray(dense)).reshape(-1)
    indptr = np.arange(n + 1, dtype=np.int64) * g
    indices = np.tile(np.arange(g, dtype=np.int32), n)
    return be.csr(indptr, indices, values, n, g), False, dense.dtype


def _grouping(codes: np.ndarray, n_groups: int):
    """-> (order: the rows with a group, sorted by group; group_sizes)"""
    keep = np.flatnonzero(codes >= 0)
    order = keep[np.argsort(codes[keep], kind="stable")].astype(np.int32)
    return order, np.bincount(codes[keep], minlength=n_groups).astype(np.int64)


def _aggregate(be, data, by: pd.Categorical, funcs: set, *, mask, dof: int) -> dict:
    n_groups = len(by.categories)
    codes = np.asarray(by.codes).astype(np.int32)
    if mask is not None:
        codes = np.where(mask, codes, np.int32(-1)).astype(np.int32)
    order, sizes = _grouping(codes, n_groups)
    h, is_sparse, dtype = _to_device(be, data)
    is_f32 = dtype == np.float32 or dtype == np.float16
    res = be.aggregate(h, codes, order, sizes, want_m2="var" in funcs, want_median="median" in funcs, mid_in_f32=bool(is_f32))
    if res["flags"] & FLAG_NONFINITE:
        raise ValueError("sc.get.aggregate: the matrix holds a value that is not finite (NaN or infinity) in a row that is aggregated")
    if res["flags"]:
        raise RuntimeError(f"sc.get.aggregate: the aggregation kernels report inconsistent input (flags {res['flags']})")
    size_col = sizes.astype(np.float64)[:, None]
    layers = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        if "sum" in funcs:
            layers["sum"] = np.rint(res["sum"]).astype(np.int64) if is_sparse and dtype.kind in "iub" else res["sum"]
        if "mean" in funcs and "var" not in funcs:
            layers["mean"] = res["sum"] / size_col
        if "count_nonzero" in funcs:
            layers["count_nonzero"] = res["count_nonzero"] if is_sparse else res["count_nonzero"].astype(np.float64)
        if "var" in funcs:
            assert dof >= 0
            if dof != 0:
                denom = np.where(sizes > dof, sizes - dof, np.nan)
                which_nan = np.isnan(denom)
                if which_nan.any():
                    msg = f"Group counts matches dof, resulting var for groups {by.categories[which_nan].to_list()} will be nan"
                    warnings.warn(msg, RuntimeWarning, stacklevel=3)
                layers["var"] = res["m2"] / denom[:, None]
            else:
                layers["var"] = np.where(size_col > 0, res["m2"] / size_col, 0.0)
            if "mean" in funcs:
                layers["mean"] = res["sum"] / size_col
        if "median" in funcs:
            layers["median"] = res["median"].astype(np.float32) if (not is_sparse and dtype == np.float32) else res["median"]
    return layers


def aggregate(adata, by, func, *, acc=None, mask=None, dof: int = 1, axis=None, layer=None, obsm=None, varm=None):
    """Aggregate the data matrix over a categorical grouping (same signature as the reference).

    by: a column name, or a sequence of them, of `adata.obs` (axis 0 / 'obs') or `adata.var` (axis 1 / 'var'; axis=None means
    'var' when `varm` is given, else 'obs').  Several keys combine into categories `a_b_c`; combinations that do not occur are
    dropped, and a missing value in any key drops the row.  func: one of, or an iterable of, 'sum', 'mean', 'var',
    'count_nonzero', 'median'; each becomes a layer of the result.  mask: a boolean array or a column name; rows outside it take
    no part.  dof: var = m2 / (size - dof); groups of at most dof rows give NaN and one RuntimeWarning.  layer / obsm / varm pick
    the matrix (default X); a DataFrame there names the result's variables.

    Returns an AnnData: one row per group (axis='var': one column per group) with one categorical column per key and
    `n_obs_aggregated`, which respects the mask.  'sum' is float64 (int64 for an integer sparse matrix), 'count_nonzero' int64
    (float64 for a dense matrix), 'mean' and 'var' float64, 'median' float64 (float32 for a dense float32 matrix).  A group
    without rows gives sum 0, count 0, mean NaN and median NaN.  Non-finite values raise ValueError."""
    if not is_anndata(adata):
        msg = f"sc.get.aggregate is currently only implemented for AnnData input, was passed {type(adata)}."
        raise NotImplementedError(msg)
    if acc is not None or _is_ref(by) or _is_ref(mask):
        raise NotImplementedError("sc.get.aggregate: `acc=` accessors and `AdRef` references (anndata.acc) are not part of this "
                                  "package; use `by` column names with `axis`, `layer`, `obsm` or `varm`")
    by_list = [by] if isinstance(by, str) else list(by)
    if any(_is_ref(b) for b in by_list):
        raise NotImplementedError("sc.get.aggregate: `AdRef` references (anndata.acc) are not part of this package")
    dim = _resolve_axis(axis) if axis is not None else ("var" if varm else "obs")
    data = _get_arr(adata, dim, layer=layer, obsm=obsm, varm=varm)
    _refuse_lazy(data)
    funcs = {func} if isinstance(func, str) else set(func)
    if unknown := funcs - set(AGG_FUNCS):
        msg = f"func {unknown} is not one of {set(AGG_FUNCS)}"
        raise ValueError(msg)
    names = None
    if isinstance(data, pd.DataFrame):
        names, data = data.columns, data.to_numpy()
    if "median" in funcs and data.shape[1] > TRANSPOSE_MAX_COLUMNS:
        raise NotImplementedError(f"sc.get.aggregate: the median is offered up to {TRANSPOSE_MAX_COLUMNS} variables")
    dim_df = getattr(adata, dim)
    label_df = pd.DataFrame({key: dim_df[key].to_numpy() for key in by_list}, index=dim_df.index)
    mask_arr = _check_mask(adata, mask, dim)
    categorical, new_label_df = _combine_categories(label_df)
    kept = categorical.codes >= 0 if mask_arr is None else (categorical.codes >= 0) & mask_arr
    new_label_df["n_obs_aggregated"] = np.bincount(categorical.codes[kept], minlength=len(categorical.categories))
    layers = _aggregate(default_backend(), data, categorical, funcs, mask=mask_arr, dof=dof)
    if obsm is not None or varm is not None:
        other = pd.DataFrame(index=names if names is not None else pd.RangeIndex(data.shape[1]).astype(str))
    else:
        other = getattr(adata, "var" if dim == "obs" else "obs")
    if dim == "obs":
        return AnnData(None, obs=new_label_df, var=other, layers=layers)
    return AnnData(None, obs=other, var=new_label_df, layers={k: np.ascontiguousarray(v.T) for k, v in layers.items()})
