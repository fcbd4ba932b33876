"""`sc.tl.rank_genes_groups`: t-test, t-test_overestim_var and Wilcoxon marker genes (reference: `rank_genes_groups`,
`_RankGenes` and `_build_stats_dataframe` in src/scanpy/tools/_rank_genes_groups.py).

Everything that touches the matrix runs on the device (csrc/rank_genes.hip behind `scamd_rank_genes_*`): the per-group sums,
sums of squares and non-zero counts, and twice the Wilcoxon rank sums with their tie terms, all as exact integers or
fixed-point sums, so that two runs give the same bits.  What is left for the host is arithmetic on the K x genes tables:
Welch's t, the normal approximation, the multiple-testing correction, the sort.  The device is reached through a backend
object (`default_backend()`), as in preprocessing/_csr_device.py, so the host logic runs under a numpy stand-in."""
from __future__ import annotations

import logging
import warnings

import numpy as np
import pandas as pd
from scipy import sparse

from .._settings import settings
from ..preprocessing import _csr_device

log = logging.getLogger("scanpy_amd")

METHODS = ("logreg", "t-test", "wilcoxon", "wilcoxon_illico", "t-test_overestim_var")
CORR_METHODS = {"benjamini-hochberg", "bonferroni"}
TRANSPOSE_MAX_GENES = 40944  # scamd_csr_transpose_f32's bound on the number of columns
_SLOT_DTYPES = {"names": "O", "scores": "float32", "logfoldchanges": "float32", "pvals": "float64", "pvals_adj": "float64"}


class CscOnDevice:
    """The CSC copy of the cells x genes matrix on the device (rows ascending within a column)."""

    def __init__(self, shape, t_indptr, t_indices, t_data):
        self.shape, self.t_indptr, self.t_indices, self.t_data = shape, t_indptr, t_indices, t_data


class GpuRankGenesBackend:
    """The only product backend: libscanpy_amd.so (raises without a GPU)."""

    def __init__(self):
        self.pp = _csr_device.GpuPPBackend()
        self.K = self.pp.K
        self.max_groups = None

    def upload(self, x):
        return self.pp.upload(x)

    def nonnegative_integers(self, m) -> bool:
        return self.pp.nonnegative_integers(m)

    def transpose(self, m) -> CscOnDevice:
        n, g = m.shape
        return CscOnDevice((n, g), *self.K.csr_transpose(m.indptr, m.indices, m.data, n, g))

    def _codes(self, codes):
        import torch

        return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).to(self.pp.device)

    def group_stats(self, c: CscOnDevice, codes, n_groups: int, *, expm1_scale=None):
        """-> (sum, sumsq, nnz), each [n_groups, g] (float64, float64, int64), of the cells with code k"""
        n, g = c.shape
        s, sq, nz = self.K.rank_genes_group_stats(c.t_indptr, c.t_indices, c.t_data, n, g, self._codes(codes), n_groups,
                                                  expm1_scale=expm1_scale)
        return s.cpu().numpy(), sq.cpu().numpy(), nz.cpu().numpy()

    def wilcoxon_ranksums(self, c: CscOnDevice, codes, n_groups: int, group_sizes, reference: int, *, tie_term: bool):
        """-> (twice the rank sums int64 [n_groups, g], tie term float64 or None): scamd_rank_genes_wilcoxon_f32"""
        import torch

        n, g = c.shape
        sizes = torch.from_numpy(np.ascontiguousarray(group_sizes, dtype=np.int64)).to(self.pp.device)
        rs, tie = self.K.rank_genes_wilcoxon(c.t_indptr, c.t_indices, c.t_data, n, g, self._codes(codes), n_groups, sizes,
                                             reference, tie_term=tie_term)
        return rs.cpu().numpy(), None if tie is None else tie.cpu().numpy()


def default_backend():
    return GpuRankGenesBackend()


def max_groups() -> int:
    """Group count (the remainder group of reference='rest' included) the LDS tables of the kernels hold
    (SCAMD_RANK_GENES_MAX_GROUPS of include/scanpy_amd.h)."""
    return 2000


# ---- small host pieces -----------------------------------------------------------------------------------------------
def _sanitize_groupby(adata, groupby: str) -> None:
    """what `sanitize_anndata` does to the one column the function reads: a string column becomes categorical"""
    col = adata.obs[groupby]
    if isinstance(col.dtype, pd.CategoricalDtype):
        return
    if col.dtype == object or pd.api.types.is_string_dtype(col.dtype):
        adata.obs[groupby] = pd.Categorical(col.astype(str), categories=sorted(pd.unique(col.astype(str))))
        log.info("... storing %r as categorical", groupby)


def _check_mask_var(adata, mask_var):
    if mask_var is None:
        return None
    if isinstance(mask_var, str):
        if mask_var not in adata.var.columns:
            msg = f"Did not find `adata.var[{mask_var!r}]`. Either add the mask first to `adata.var` or consider using the mask argument with an array."
            raise ValueError(msg)
        mask = np.asarray(adata.var[mask_var])
    else:
        mask = np.asarray(mask_var)
        if mask.shape != (adata.n_vars,):
            raise ValueError("The shape of the mask do not match the data.")
    if mask.dtype != bool:
        raise ValueError("Mask array must be boolean.")
    return mask


def _select_groups(adata, groups, groupby: str):
    """-> (names of the selected groups in the order given, index of each among the categories)"""
    cats = adata.obs[groupby].cat.categories
    if isinstance(groups, str) and groups == "all":
        return cats.to_numpy(), np.arange(len(cats))
    ids = []
    for name in groups:
        hit = np.flatnonzero(cats.to_numpy() == name)
        if hit.size == 0:
            raise IndexError(f"group {name!r} is not among the categories of adata.obs[{groupby!r}]: {cats.tolist()}")
        ids.append(int(hit[0]))
    if not ids:
        raise RuntimeError(f"{np.array(groups)} invalid! specify valid groups_order (or indices) from {cats}")
    ids = np.asarray(ids)
    return cats[ids].to_numpy(), ids


def _fdr_bh(p: np.ndarray) -> np.ndarray:
    """Benjamini-Hochberg adjusted p-values (what statsmodels' multipletests(method='fdr_bh') returns)"""
    m = p.size
    order = np.argsort(p)
    adj = p[order] * (m / np.arange(1, m + 1))
    adj = np.minimum.accumulate(adj[::-1])[::-1]
    out = np.empty(m)
    out[order] = np.minimum(adj, 1.0)
    return out


def _mean_var(s, sq, count):
    """mean and variance (ddof 1) per row of the [K, g] sums; a group of one cell has variance NaN, an empty one 0 / 0"""
    count = np.asarray(count, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count > 0, s / np.where(count > 0, count, 1), 0.0)
        var = (sq - count * mean * mean) / (count - 1)
    return mean, np.where(count > 0, np.maximum(var, 0.0), 0.0)


def _top_indices(scores: np.ndarray, n_top: int, rankby_abs: bool) -> np.ndarray:
    key = np.abs(scores) if rankby_abs else scores
    # descending score, ties by ascending gene index (np.lexsort: last key is the primary one)
    return np.lexsort((np.arange(key.size), -key))[:n_top]


def rank_genes_groups(adata, groupby: str, *, mask_var=None, use_raw: bool | None = None, groups="all", reference: str = "rest",
                      n_genes: int | None = None, rankby_abs: bool = False, pts: bool = False, key_added: str | None = None,
                      copy: bool = False, method: str | None = None, corr_method: str = "benjamini-hochberg",
                      tie_correct: bool = False, layer: str | None = None, mean_in_log_space: bool | None = None, **kwds):
    """Rank genes for characterizing groups (the reference's `sc.tl.rank_genes_groups`; expects logarithmized data).

    Signature, slots (`uns[key_added]`: params, names, scores, pvals, pvals_adj, logfoldchanges, pts, pts_rest), dtypes,
    warnings and errors are the reference's.  `method`: 't-test', 't-test_overestim_var', 'wilcoxon' (`tie_correct`);
    'wilcoxon_illico' runs the same Wilcoxon engine; 'logreg' is outside the MI355X path (NotImplementedError).  `method`
    and `mean_in_log_space` left as None follow `sc.settings.preset`: ScanpyV1 -> 't-test' and True, ScanpyV2Preview ->
    Wilcoxon and False.

    Order of the tables: descending score (|score| with `rankby_abs`), genes of EQUAL score by ascending position in
    `var_names`.  (The reference selects with `argpartition`, which leaves the order of tied scores unspecified.)

    Limits of the device path: at most 40944 genes (after `mask_var`), at most 2000 groups (the remainder group of
    reference='rest' included), Wilcoxon up to 2^21 cells, a matrix in memory, finite values; NotImplementedError beyond.
    """
    v2 = settings.preset == "ScanpyV2Preview"
    if mean_in_log_space is None:
        mean_in_log_space = not v2
    if method is None:
        method = "wilcoxon_illico" if v2 else "t-test"
    elif "illico" in method:
        msg = ("`wilcoxon_illico` flavor will be removed in scanpy 2.0 and be simply the new `wilcoxon` implementation."
               "To remove theis warning, you can locally do `with sc.settings.override(preset=sc.Preset.ScanpyV2Preview)`.")
        warnings.warn(msg, DeprecationWarning, stacklevel=2)

    if use_raw is None:
        use_raw = adata.raw is not None
    elif use_raw is True and adata.raw is None:
        raise ValueError("Received `use_raw=True`, but `adata.raw` is empty.")
    if "only_positive" in kwds:
        rankby_abs = not kwds.pop("only_positive")  # backwards compat

    if method not in METHODS:
        raise ValueError(f"Method must be one of {METHODS}.")
    if corr_method not in CORR_METHODS:
        raise ValueError(f"Correction method must be one of {CORR_METHODS}.")
    if method == "logreg":
        raise NotImplementedError("method='logreg' is outside the MI355X path of scanpy_amd (it needs scikit-learn's "
                                  "LogisticRegression on the host); use 't-test', 't-test_overestim_var' or 'wilcoxon'")
    mask_var = _check_mask_var(adata, mask_var)

    adata = adata.copy() if copy else adata
    _sanitize_groupby(adata, groupby)
    if isinstance(groups, str) and groups == "all":
        groups_order = "all"
    elif isinstance(groups, (str, int)):
        raise ValueError("Specify a sequence of groups")
    else:
        groups_order = list(groups)
        if isinstance(groups_order[0], int):
            groups_order = [str(n) for n in groups_order]
        if reference != "rest" and reference not in set(groups_order):
            groups_order += [reference]
    cats = adata.obs[groupby].cat.categories
    if reference != "rest" and reference not in cats:
        raise ValueError(f"reference = {reference} needs to be one of groupby = {cats.tolist()}.")

    if key_added is None:
        key_added = "rank_genes_groups"
    adata.uns[key_added] = {}
    adata.uns[key_added]["params"] = dict(groupby=groupby, reference=reference, method=method, use_raw=use_raw, layer=layer,
                                          corr_method=corr_method)

    # ---- groups and the matrix (`_RankGenes.__init__`)
    group_names, group_ids = _select_groups(adata, groups_order, groupby)
    cat_codes = np.asarray(adata.obs[groupby].cat.codes)
    cat_counts = np.bincount(cat_codes[cat_codes >= 0], minlength=len(cats))
    singlets = [str(nm) for nm, i in zip(group_names, group_ids) if cat_counts[i] < 2]
    if singlets:
        raise ValueError(f"Could not calculate statistics for groups {', '.join(singlets)} since they only contain one sample.")
    comp = adata
    if layer is not None:
        if use_raw:
            raise ValueError("Cannot specify `layer` and have `use_raw=True`.")
        x = adata.layers[layer]
    else:
        if use_raw and adata.raw is not None:
            comp = adata.raw
        x = comp.X
    x = _csr_device.in_memory(x)
    var_names = comp.var_names
    if mask_var is not None:
        x = x[:, mask_var]
        var_names = var_names[mask_var]
    n_cells, g = x.shape
    if g > TRANSPOSE_MAX_GENES:
        raise NotImplementedError(f"rank_genes_groups on the MI355X takes at most {TRANSPOSE_MAX_GENES} genes (the CSR -> CSC "
                                  f"transpose); got {g}. Select genes with `mask_var`.")
    k = len(group_names)
    ireference = None if reference == "rest" else int(np.flatnonzero(group_names == reference)[0])
    sel = np.full(len(cats), -1, dtype=np.int64)
    sel[group_ids] = np.arange(k)
    cell_sel = np.where(cat_codes >= 0, sel[np.maximum(cat_codes, 0)], -1)
    n_table = k + 1 if ireference is None else k  # 'rest': group k is the remainder
    if n_table > max_groups():
        raise NotImplementedError(f"rank_genes_groups on the MI355X holds at most {max_groups()} groups (the remainder group of "
                                  f"reference='rest' included) in its LDS tables; got {n_table}")
    codes = (np.where(cell_sel >= 0, cell_sel, k) if ireference is None else cell_sel).astype(np.int32)
    sizes = np.bincount(codes[codes >= 0], minlength=n_table).astype(np.int64)

    be = default_backend()
    m = be.upload(x if sparse.issparse(x) else np.asarray(x))
    if be.nonnegative_integers(m):
        log.warning("It seems you use rank_genes_groups on the raw count data. "
                    "Please logarithmize your data before calling rank_genes_groups.")
    csc = be.transpose(m)

    base = adata.uns.get("log1p", {}).get("base")
    log_scale = 1.0 if base is None else float(np.log(base))

    def expm1_func(v):
        return np.expm1(v * log_scale)

    # ---- per-group statistics (`_basic_stats`)
    ttest = method in ("t-test", "t-test_overestim_var")
    s, sq, nnz = be.group_stats(csc, codes, n_table, expm1_scale=None if mean_in_log_space else log_scale)
    mean, var = _mean_var(s, sq, sizes)
    means, vars_ = mean[:k], var[:k]
    n_sel = sizes[:k].astype(np.float64)
    pts_tab = nnz[:k] / n_sel[:, None] if pts else None
    means_rest = vars_rest = pts_rest = None
    if ireference is None:
        n_rest = (n_cells - n_sel)[:, None]
        tot_s, tot_sq = s.sum(axis=0), sq.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            means_rest = (tot_s - s[:k]) / n_rest
            if ttest:
                vars_rest = np.maximum((tot_sq - sq[:k]) - n_rest * means_rest * means_rest, 0.0) / (n_rest - 1.0)
            if pts:
                pts_rest = (nnz.sum(axis=0) - nnz[:k]) / n_rest

    # ---- the tests: (group index, scores, p-values)
    from scipy import stats

    results = []
    if ttest:
        for gi in range(k):
            if gi == ireference:
                continue
            ns_group = float(n_sel[gi])
            if ireference is not None:
                mean_o, var_o, ns_other = means[ireference], vars_[ireference], float(n_sel[ireference])
            else:
                mean_o, var_o, ns_other = means_rest[gi], vars_rest[gi], float(n_cells - ns_group)
            ns_o = ns_other if method == "t-test" else ns_group  # overestim_var: the group's size for both variances
            with np.errstate(invalid="ignore", divide="ignore"):
                sc_, pv = stats.ttest_ind_from_stats(mean1=means[gi], std1=np.sqrt(vars_[gi]), nobs1=ns_group, mean2=mean_o,
                                                     std2=np.sqrt(var_o), nobs2=ns_o, equal_var=False)
            sc_ = np.array(sc_, dtype=np.float64)
            pv = np.array(pv, dtype=np.float64)
            sc_[np.isnan(sc_)] = 0
            pv[np.isnan(pv)] = 1
            results.append((gi, sc_, pv))
    else:
        rs2, tie = be.wilcoxon_ranksums(csc, codes, n_table, sizes, -1 if ireference is None else ireference, tie_term=bool(tie_correct))
        for gi in range(k):
            if gi == ireference:
                continue
            n_a = float(n_sel[gi])
            if ireference is None:
                n_b, big_n = float(n_cells) - n_a, float(n_cells)
                t_j = tie if tie_correct else None
            else:
                n_b = float(n_sel[ireference])
                big_n = n_a + n_b
                if n_a <= 25 or n_b <= 25:
                    log.info("Few observations in a group for normal approximation (<=25). Lower test accuracy.")
                t_j = tie[gi] if tie_correct else None
            with np.errstate(invalid="ignore", divide="ignore"):
                tc = 1.0 if t_j is None else (1.0 - t_j / (big_n**3 - big_n) if big_n >= 2 else np.ones(g))
                std_dev = np.sqrt(tc * n_a * n_b * (big_n + 1) / 12.0)
                sc_ = (rs2[gi].astype(np.float64) / 2.0 - n_a * (big_n + 1) / 2.0) / std_dev
            sc_[np.isnan(sc_)] = 0
            results.append((gi, sc_, 2 * stats.distributions.norm.sf(np.abs(sc_))))

    # ---- tables (`_build_stats_dataframe`)
    n_top = g if n_genes is None or n_genes > g else n_genes
    cols = {slot: {} for slot in _SLOT_DTYPES}
    for gi, sc_, pv in results:
        name = str(group_names[gi])
        top = _top_indices(sc_, n_top, rankby_abs)
        cols["names"][name] = np.asarray(var_names)[top]
        cols["scores"][name] = sc_[top]
        cols["pvals"][name] = pv[top]
        if corr_method == "benjamini-hochberg":
            adj = _fdr_bh(np.where(np.isnan(pv), 1.0, pv))
        else:
            adj = np.minimum(pv * g, 1.0)
        cols["pvals_adj"][name] = adj[top]
        mean_o = means_rest[gi] if ireference is None else means[ireference]
        with np.errstate(invalid="ignore", divide="ignore"):
            if mean_in_log_space:
                fold = (expm1_func(means[gi]) + 1e-9) / (expm1_func(mean_o) + 1e-9)
            else:
                fold = (means[gi] + 1e-9) / (mean_o + 1e-9)
            cols["logfoldchanges"][name] = np.log2(fold[top])

    shown = [str(nm) for nm in group_names]
    if pts_tab is not None:
        adata.uns[key_added]["pts"] = pd.DataFrame(pts_tab.T, index=var_names, columns=shown)
    if pts_rest is not None:
        adata.uns[key_added]["pts_rest"] = pd.DataFrame(pts_rest.T, index=var_names, columns=shown)
    for slot, dt in _SLOT_DTYPES.items():
        if not cols[slot]:
            continue
        rec = np.empty(n_top, dtype=[(name, dt) for name in cols[slot]])
        for name, vals in cols[slot].items():
            rec[name] = vals
        adata.uns[key_added][slot] = rec.view(np.recarray)
    return adata if copy else None
