"""`sc.get`: host-only accessors of stored results (reference: src/scanpy/get/get.py) and `aggregate`, the grouping of cells on the
device (reference: src/scanpy/get/_aggregated.py; `_get_aggregate.py`, csrc/aggregate.hip)."""
from __future__ import annotations

import pandas as pd

from ._get_aggregate import aggregate

__all__ = ["aggregate", "rank_genes_groups_df"]


def rank_genes_groups_df(adata, group, *, key: str = "rank_genes_groups", pval_cutoff: float | None = None,
                         log2fc_min: float | None = None, log2fc_max: float | None = None, gene_symbols: str | None = None):
    """The tables `tl.rank_genes_groups` stored under `adata.uns[key]` as one long DataFrame (the reference's function of
    this name): columns group (left out for a single group), names, scores, logfoldchanges, pvals, pvals_adj, optionally
    `gene_symbols` (a column of `adata.var`), pct_nz_group / pct_nz_reference when `pts` was computed.  `group`: a name, a
    list of names, or None for every stored group.  `pval_cutoff` keeps pvals_adj < cutoff; `log2fc_min` / `log2fc_max` keep
    logfoldchanges strictly inside."""
    res = adata.uns[key]
    if isinstance(group, str):
        group = [group]
    if group is None:
        group = list(res["names"].dtype.names)
    group = list(group)
    slots = ["names", "scores"] if res["params"]["method"] == "logreg" else ["names", "scores", "logfoldchanges", "pvals", "pvals_adj"]
    parts = []
    for name in group:
        part = pd.DataFrame({slot: res[slot][name] for slot in slots})
        part.insert(0, "group", name)
        parts.append(part)
    d = pd.concat(parts)
    d["group"] = pd.Categorical(d["group"], categories=group)
    if "pvals_adj" in slots:
        if pval_cutoff is not None:
            d = d[d["pvals_adj"] < pval_cutoff]
        if log2fc_min is not None:
            d = d[d["logfoldchanges"] > log2fc_min]
        if log2fc_max is not None:
            d = d[d["logfoldchanges"] < log2fc_max]
    if gene_symbols is not None:
        d = d.join(adata.var[gene_symbols], on="names")
    for slot, column in (("pts", "pct_nz_group"), ("pts_rest", "pct_nz_reference")):
        if slot in res:
            long = res[slot][group].rename_axis(index="names").reset_index().melt(id_vars="names", var_name="group", value_name=column)
            d = d.merge(long)
    if len(group) == 1:
        del d["group"]
    return d
