"""`sc.pp.calculate_qc_metrics` / `describe_obs` / `describe_var` on MI355X (reference:
src/scanpy/preprocessing/_qc.py -- `calculate_qc_metrics`, `describe_obs`, `describe_var`, `top_segment_proportions`).

The device gives the primitives in one sweep over the matrix plus one selection pass (csrc/qc.hip, `scamd_pp_qc_sweep_f32`
and `scamd_pp_qc_top_f32`): per cell the number of non-zero entries, the total, the totals inside every `qc_var` and the sum
of the n largest entries for every `percent_top` position; per gene the number of non-zero entries and the sum over cells.
The derived columns (`log1p_*`, `pct_*`, `pct_dropout_*`, `mean_*`) are numpy on those small vectors, with the reference's
formulas.  A backed matrix is streamed by row chunks: per-cell columns concatenate, per-gene counts and sums add up.

Dtypes.  `fast_array_utils` (which the reference sums with) is not a dependency, so the dtypes follow numpy's `sum` / `mean`
conventions: counts of non-zero entries are int64; row and column totals have the matrix' dtype for float32 input and are
int64 for integer input; `mean_*` is float64; every derived column has the dtype numpy gives the formula.

The top-n rule.  For one cell: the stored non-zero values, padded with zeros up to max(percent_top) elements; top(n) is the
sum of the n largest elements of that multiset, `pct_*_in_top_n_*` = top(n) / total * 100.  This is what the reference's
CSR routine computes.  Its dense routine ranks the implicit zeros of ALL genes, which differs once a value is negative: a
dense matrix with a negative entry is refused."""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd

from . import _csr_device

MAX_POSITIONS = 16   # csrc/qc.hip: QC_MAX_POSITIONS
MAX_TOP = 4096       # csrc/qc.hip: QC_MAX_TOP
MAX_QC_VARS = 32     # csrc/qc.hip: QC_MAX_MASKS
STREAM_ROWS = 1_000_000


class _StreamedQc:
    """`qc_sweep` of a backed CSR matrix (`_backed.BackedCsr`): row chunks are read, uploaded, brought up to date with the
    matrix' pending transforms and swept one after the other; per-cell results concatenate, per-gene ones add up."""

    def __init__(self, be, x, step: int = STREAM_ROWS):
        self.be, self.x, self.step = be, x, step

    def qc_sweep(self, m, *, gene_masks=None, positions=(), per_gene: bool = True) -> dict:
        from .._backed import apply_ops_pp

        n, g = self.x.shape
        n_masks = 0 if gene_masks is None else len(gene_masks)
        parts = []
        for c in self.x.row_chunks(self.step):
            rows = c.load()
            dm = self.be.upload(rows.to_scipy())
            apply_ops_pp(self.be, dm, rows.ops)
            parts.append(self.be.qc_sweep(dm, gene_masks=gene_masks, positions=positions, per_gene=per_gene))
        if not parts:
            return {"row_nnz": np.zeros(0, np.int64), "row_total": np.zeros(0), "row_masked": np.zeros((n_masks, 0)),
                    "col_nnz": np.zeros(g, np.int64) if per_gene else None, "col_sum": np.zeros(g) if per_gene else None,
                    "negative": False, "top": np.zeros((0, len(positions))) if len(positions) else None}
        return {"row_nnz": np.concatenate([p["row_nnz"] for p in parts]),
                "row_total": np.concatenate([p["row_total"] for p in parts]),
                "row_masked": np.concatenate([p["row_masked"] for p in parts], axis=1),
                "col_nnz": sum(p["col_nnz"] for p in parts) if per_gene else None,
                "col_sum": sum(p["col_sum"] for p in parts) if per_gene else None,
                "negative": any(p["negative"] for p in parts),
                "top": np.concatenate([p["top"] for p in parts], axis=0) if len(positions) else None}


def _warn_parallel(parallel) -> None:
    if parallel is not None:
        warnings.warn("Argument `parallel` is deprecated, and currently has no effect.", FutureWarning, stacklevel=3)


def _get_arr(adata, *, use_raw: bool, layer):
    """`scanpy.get._get_arr(adata, use_raw=, layer=)` (src/scanpy/get/get.py)"""
    if not isinstance(use_raw, bool):
        raise TypeError(f"use_raw expected to be bool, was {type(use_raw)}.")
    if layer is not None and use_raw:
        raise ValueError("Only one of `layer`, or `use_raw` can be specified.")
    if layer is not None:
        return adata.layers[layer]
    if use_raw:
        return adata.raw.X  # (`adata.raw` is None: the AttributeError of the reference)
    return adata.X


def _total_dtype(x):
    """numpy's `sum` convention: float32 stays, every integer (and bool) matrix sums to int64"""
    if getattr(x, "is_backed", False) and getattr(x, "_ops", ()):
        return np.dtype(np.float32)  # pending normalize_total / log1p produce float32 values
    dt = np.dtype(x.dtype)
    return np.dtype(np.float32) if dt == np.float32 else (np.dtype(np.int64) if dt.kind in "iub" else dt)


def _as_total(v: np.ndarray, dtype) -> np.ndarray:
    return np.rint(v).astype(np.int64) if dtype.kind == "i" else v.astype(dtype)


def _sweep(x, *, gene_masks=None, positions=(), per_gene: bool = True) -> dict:
    be = _csr_device.default_backend()
    if getattr(x, "is_backed", False):
        res = _StreamedQc(be, x).qc_sweep(x, gene_masks=gene_masks, positions=positions, per_gene=per_gene)
        kind = "csr"
    else:
        m = be.upload(x)
        res = be.qc_sweep(m, gene_masks=gene_masks, positions=positions, per_gene=per_gene)
        kind = m.kind
    if kind == "dense" and res["negative"] and len(positions):
        raise NotImplementedError(
            "calculate_qc_metrics: a dense matrix with a negative entry: the reference's dense and sparse routines rank the "
            "implicit zeros differently there; pass a scipy CSR matrix (the padded-multiset rule) or percent_top=None")
    res["dtype"] = _total_dtype(x)
    return res


def _positions(percent_top, n_vars: int) -> list:
    """sorted positions; `check_ns` of the reference, then the limits of the device pass"""
    if percent_top is None or len(percent_top) == 0:
        return []
    ns = sorted(int(p) for p in percent_top)
    if not (ns[-1] <= n_vars and ns[0] > 0):
        raise IndexError("Positions outside range of features.")
    uniq = sorted(set(ns))
    if len(uniq) > MAX_POSITIONS or uniq[-1] > MAX_TOP:
        raise NotImplementedError(f"calculate_qc_metrics: percent_top holds {len(uniq)} positions up to {uniq[-1]}; the "
                                  f"device pass takes at most {MAX_POSITIONS} positions, each <= {MAX_TOP}")
    return ns


def _gene_masks(adata, qc_vars, g: int):
    if len(qc_vars) > MAX_QC_VARS:
        raise NotImplementedError(f"calculate_qc_metrics: {len(qc_vars)} qc_vars, the device pass takes at most {MAX_QC_VARS}")
    masks = np.zeros((len(qc_vars), g), dtype=bool)
    for k, qc_var in enumerate(qc_vars):
        mask = np.asarray(adata.var[qc_var].to_numpy(), dtype=bool)
        if mask.shape != (g,):
            raise ValueError(f"adata.var[{qc_var!r}] has {mask.shape[0]} entries for a matrix of {g} variables")
        masks[k] = mask
    return masks


def _obs_metrics(adata, res, *, expr_type, var_type, qc_vars, ns, log1p) -> pd.DataFrame:
    dtype = res["dtype"]
    out = pd.DataFrame(index=adata.obs_names)
    with np.errstate(invalid="ignore", divide="ignore"):  # a cell without counts: 0 / 0 = NaN, as the reference's numba code
        out[f"n_{var_type}_by_{expr_type}"] = res["row_nnz"]
        if log1p:
            out[f"log1p_n_{var_type}_by_{expr_type}"] = np.log1p(res["row_nnz"])
        total = _as_total(res["row_total"], dtype)
        out[f"total_{expr_type}"] = total
        if log1p:
            out[f"log1p_total_{expr_type}"] = np.log1p(total)
        if ns:
            uniq = sorted(set(ns))
            proportions = res["top"] / total.astype(np.float64)[:, None]
            for n in ns:
                out[f"pct_{expr_type}_in_top_{n}_{var_type}"] = proportions[:, uniq.index(n)] * 100
        for k, qc_var in enumerate(qc_vars):
            part = _as_total(res["row_masked"][k], dtype)
            out[f"total_{expr_type}_{qc_var}"] = part
            if log1p:
                out[f"log1p_total_{expr_type}_{qc_var}"] = np.log1p(part)
            out[f"pct_{expr_type}_{qc_var}"] = part / total * 100
    return out


def _var_metrics(adata, res, n_obs: int, *, expr_type, log1p) -> pd.DataFrame:
    dtype = res["dtype"]
    out = pd.DataFrame(index=adata.var_names)
    with np.errstate(invalid="ignore", divide="ignore"):
        n_cells = res["col_nnz"].astype(np.int64)
        mean = res["col_sum"] / np.float64(n_obs)
        out[f"n_cells_by_{expr_type}"] = n_cells
        out[f"mean_{expr_type}"] = mean
        if log1p:
            out[f"log1p_mean_{expr_type}"] = np.log1p(mean)
        out[f"pct_dropout_by_{expr_type}"] = (1 - n_cells / n_obs) * 100
        total = _as_total(res["col_sum"], dtype)
        out[f"total_{expr_type}"] = total
        if log1p:
            out[f"log1p_total_{expr_type}"] = np.log1p(total)
    return out


def _n_vars(x) -> int:
    return int(x.shape[1])


def describe_obs(adata, *, expr_type: str = "counts", var_type: str = "genes", qc_vars=(),  # noqa: PLR0913
                 percent_top=(50, 100, 200, 500), layer=None, use_raw: bool = False, log1p: bool = True, inplace: bool = False,
                 x=None, parallel=None, _res=None):
    """Per-cell QC metrics (drop-in for `scanpy.pp.describe_obs`): `n_{var_type}_by_{expr_type}`, `total_{expr_type}`,
    `pct_{expr_type}_in_top_{n}_{var_type}` for every `percent_top` position and, per `qc_var`, `total_{expr_type}_{qc_var}`
    and `pct_{expr_type}_{qc_var}`, plus the `log1p_` columns.  Dtypes follow numpy's conventions (module docstring)."""
    _warn_parallel(parallel)
    if x is None:
        x = _get_arr(adata, use_raw=use_raw, layer=layer)
    qc_vars = [qc_vars] if isinstance(qc_vars, str) else list(qc_vars)
    ns = _positions(percent_top, _n_vars(x))
    if _res is None:
        _res = _sweep(x, gene_masks=_gene_masks(adata, qc_vars, _n_vars(x)), positions=sorted(set(ns)), per_gene=False)
    obs_metrics = _obs_metrics(adata, _res, expr_type=expr_type, var_type=var_type, qc_vars=qc_vars, ns=ns, log1p=log1p)
    if inplace:
        adata.obs[obs_metrics.columns] = obs_metrics
        return None
    return obs_metrics


def describe_var(adata, *, expr_type: str = "counts", var_type: str = "genes", layer=None, use_raw: bool = False,
                 inplace: bool = False, log1p: bool = True, x=None, _res=None):
    """Per-gene QC metrics (drop-in for `scanpy.pp.describe_var`): `n_cells_by_{expr_type}`, `mean_{expr_type}`,
    `pct_dropout_by_{expr_type}`, `total_{expr_type}`, plus the `log1p_` columns."""
    if x is None:
        x = _get_arr(adata, use_raw=use_raw, layer=layer)
    if _res is None:
        _res = _sweep(x)
    var_metrics = _var_metrics(adata, _res, int(x.shape[0]), expr_type=expr_type, log1p=log1p)
    if inplace:
        adata.var[var_metrics.columns] = var_metrics
        return None
    return var_metrics


def calculate_qc_metrics(adata, *, expr_type: str = "counts", var_type: str = "genes", qc_vars=(),  # noqa: PLR0913
                         percent_top=(50, 100, 200, 500), layer=None, use_raw: bool = False, inplace: bool = False,
                         log1p: bool = True, parallel=None):
    """Calculate quality control metrics (drop-in for `scanpy.pp.calculate_qc_metrics`).

    Returns `(obs_metrics, var_metrics)` as DataFrames, or writes the same columns into `adata.obs` / `adata.var` with
    `inplace=True`.  CSR, CSC or dense input, float32 or integer; a backed matrix (`read_h5ad` / `read_zarr(..., backed='r')`)
    is streamed.  Stored zeros do not count and the matrix is not rewritten.  `fast_array_utils` is not a dependency: the
    dtypes follow numpy's `sum` / `mean` conventions (non-zero counts int64; totals in the matrix' dtype for float32 input,
    int64 for integer input; `mean_*` float64).  At most 16 `percent_top` positions, each <= 4096, and 32 `qc_vars`; a dense
    matrix with a negative entry is refused when `percent_top` is asked for (module docstring)."""
    _warn_parallel(parallel)
    x = _get_arr(adata, use_raw=use_raw, layer=layer)
    qc_vars = [qc_vars] if isinstance(qc_vars, str) else list(qc_vars)
    ns = _positions(percent_top, _n_vars(x))
    res = _sweep(x, gene_masks=_gene_masks(adata, qc_vars, _n_vars(x)), positions=sorted(set(ns)))
    obs_metrics = describe_obs(adata, expr_type=expr_type, var_type=var_type, qc_vars=qc_vars, percent_top=percent_top,
                               inplace=inplace, x=x, log1p=log1p, _res=res)
    var_metrics = describe_var(adata, expr_type=expr_type, var_type=var_type, inplace=inplace, x=x, log1p=log1p, _res=res)
    if not inplace:
        return obs_metrics, var_metrics
    return None
