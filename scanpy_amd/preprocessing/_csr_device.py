"""Host <-> device plumbing of the upstream normalisation chain: a host matrix (CSR / CSC / dense, float32 or integer)
becomes a CSR float32 on the device; the passes themselves are the HIP kernels of csrc/preprocess.hip
(`_kernels.pp_*`).  No arithmetic on the matrix happens on the host."""
from __future__ import annotations

import numpy as np
from scipy import sparse


class DeviceMatrix:
    """CSR float32 view of a host matrix on the device.

    kind 'csr' / 'csc': `indptr/indices` describe the compressed axis of the host format.  'csc' only occurs for the
    element-wise pass (log1p keeps the storage format); every row/column pass converts CSC -> CSR on upload, as the
    reference does (`x.tocsr()`, _normalization.py:266-267);
    kind 'dense': full pattern (indptr[i] = i * g, indices = column ids), `data` is the row-major matrix."""

    def __init__(self, kind, shape, indptr, indices, data, host):
        self.kind, self.shape, self.indptr, self.indices, self.data, self.host = kind, shape, indptr, indices, data, host

    @property
    def n_major(self) -> int:
        return int(self.indptr.numel() - 1)


def _check_dtype(dt) -> None:
    if np.issubdtype(dt, np.integer) or np.issubdtype(dt, np.bool_) or dt == np.float32:
        return
    msg = (f"the MI355X normalisation path computes in float32 (what scanpy's readers produce); got dtype {dt}. "
           "Cast with `.astype(np.float32)` first.")
    raise NotImplementedError(msg)


class GpuPPBackend:
    """The only product backend: everything runs through libscanpy_amd.so (raises without a GPU)."""

    def __init__(self):
        from .. import _kernels
        from .._device import require_gpu

        self.K = _kernels
        self.device = require_gpu()

    # ---- transfer ------------------------------------------------------------------------------------------
    def upload(self, x, *, want_csr_rows: bool = True) -> DeviceMatrix:
        import torch

        dev = self.device
        if sparse.issparse(x):
            _check_dtype(x.dtype)
            if x.format == "csc" and want_csr_rows:
                x = x.tocsr()
            elif x.format not in ("csr", "csc"):
                x = x.tocsr()
            if not x.has_canonical_format:
                x = x.copy()
                x.sum_duplicates()
            indptr = torch.from_numpy(x.indptr.astype(np.int64)).to(dev)
            indices = torch.from_numpy(x.indices.astype(np.int32)).to(dev)
            data = torch.from_numpy(np.ascontiguousarray(x.data, dtype=np.float32)).to(dev)
            return DeviceMatrix(x.format, x.shape, indptr, indices, data, x)
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError("expected a 2-D matrix")
        _check_dtype(x.dtype)
        n, g = x.shape
        data = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev).reshape(-1)
        indptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * g
        indices = torch.arange(g, dtype=torch.int32, device=dev).repeat(n)
        return DeviceMatrix("dense", x.shape, indptr, indices, data, x)

    def download(self, m: DeviceMatrix):
        """Host matrix of the input's kind with the device values (float32)."""
        data = m.data.cpu().numpy()
        if m.kind == "dense":
            return data.reshape(m.shape)
        cls = type(m.host)
        return cls((data, m.host.indices.copy(), m.host.indptr.copy()), shape=m.shape)

    # ---- passes (device in, small host vectors out) ---------------------------------------------------------
    def row_sums(self, m: DeviceMatrix, col_skip=None) -> np.ndarray:
        import torch

        skip = None if col_skip is None else torch.from_numpy(np.ascontiguousarray(col_skip, dtype=np.int32)).to(self.device)
        return self.K.pp_row_sums(m.indptr, m.indices, m.data, m.n_major, skip).cpu().numpy()

    def row_count_positive(self, m: DeviceMatrix) -> np.ndarray:
        return self.K.pp_row_count_positive(m.indptr, m.data, m.n_major).cpu().numpy().astype(np.int64)

    def count_high(self, m: DeviceMatrix, row_total: np.ndarray, max_fraction: float) -> np.ndarray:
        import torch

        rt = torch.from_numpy(np.ascontiguousarray(row_total, dtype=np.float32)).to(self.device)
        return self.K.pp_count_high(m.indptr, m.indices, m.data, m.n_major, m.shape[1], rt, max_fraction).cpu().numpy()

    def row_divide_(self, m: DeviceMatrix, factor: np.ndarray) -> None:
        import torch

        f = torch.from_numpy(np.ascontiguousarray(factor, dtype=np.float32)).to(self.device)
        self.K.pp_row_divide_(m.indptr, m.data, m.n_major, f)

    def log1p_(self, m: DeviceMatrix, base=None) -> None:
        self.K.pp_log1p_(m.data, base)

    def col_stats(self, m: DeviceMatrix, *, row_mask=None, expm1_scale=None, count_positive: bool = False):
        """-> (sum, sumsq, n_positive or None) per gene over the masked rows (numpy float64 / int64)."""
        import torch

        mask = None if row_mask is None else torch.from_numpy(np.ascontiguousarray(row_mask, dtype=np.uint8)).to(self.device)
        s, sq, npos = self.K.pp_col_stats(m.indptr, m.indices, m.data, m.n_major, m.shape[1], row_mask=mask,
                                          expm1_scale=expm1_scale, count_positive=count_positive)
        return s.cpu().numpy(), sq.cpu().numpy(), None if npos is None else npos.cpu().numpy()

    def qc_sweep(self, m: DeviceMatrix, *, gene_masks=None, positions=(), per_gene: bool = True) -> dict:
        """The device half of `pp.calculate_qc_metrics` (csrc/qc.hip): one sweep for the per-cell and per-gene primitives,
        one selection pass when `positions` (sorted, 1-based) are asked for.  gene_masks: bool [k, g], k <= 32.
        -> row_nnz int64 [n], row_total float64 [n], row_masked float64 [k, n], col_nnz int64 [g] / col_sum float64 [g]
        (None without per_gene), negative (a stored value below zero was seen), top float64 [n, len(positions)] or None."""
        import torch

        n, g = m.n_major, m.shape[1]
        masks = np.zeros((0, g), dtype=bool) if gene_masks is None else np.asarray(gene_masks, dtype=bool).reshape(-1, g)
        bits = None
        if masks.shape[0]:
            packed = (masks.astype(np.uint32) << np.arange(masks.shape[0], dtype=np.uint32)[:, None]).sum(axis=0, dtype=np.uint32)
            bits = torch.from_numpy(packed.view(np.int32)).to(self.device)
        nz, tot, mk, cn, cs, flags = self.K.pp_qc_sweep(m.indptr, m.indices, m.data, n, g, gene_mask=bits,
                                                        n_masks=masks.shape[0], per_gene=per_gene)
        top = self.K.pp_qc_top(m.indptr, m.data, n, positions).cpu().numpy() if len(positions) else None
        return {"row_nnz": nz.cpu().numpy().astype(np.int64), "row_total": tot.cpu().numpy(),
                "row_masked": np.zeros((0, n)) if mk is None else mk.cpu().numpy(),
                "col_nnz": None if cn is None else cn.cpu().numpy(), "col_sum": None if cs is None else cs.cpu().numpy(),
                "negative": bool(int(flags.cpu()[0]) & 1), "top": top}

    def nonnegative_integers(self, m: DeviceMatrix) -> bool:
        """`check_nonnegative_integers` (src/scanpy/_utils/__init__.py:761-773) on the stored values, on the device"""
        import torch

        d = m.data
        return not bool(torch.signbit(d).any()) and not bool((d != torch.floor(d)).any())

    def clip_col_sums(self, m: DeviceMatrix, clip_val: np.ndarray, *, row_mask=None):
        """`clip_square_sum` (_highly_variable_genes.py:75-115): per gene, sum and sum of squares of
        min(x, clip_val[gene]) over the stored values of the masked rows -> (sum of squares, sum), float64.
        One sweep of `scamd_pp_col_stats_clip_f32` (the column-statistics kernel with the clip applied before the sums)."""
        import torch

        dev = m.data.device
        clip = torch.from_numpy(np.ascontiguousarray(clip_val, dtype=np.float64)).to(dev)
        mask = None if row_mask is None else torch.from_numpy(np.ascontiguousarray(row_mask, dtype=np.uint8)).to(dev)
        s, sq = self.K.pp_col_stats_clip(m.indptr, m.indices, m.data, m.n_major, m.shape[1], clip, row_mask=mask)
        return sq.cpu().numpy(), s.cpu().numpy()

    def scale_csr_(self, m: DeviceMatrix, std: np.ndarray, *, max_value=None, row_mask=None) -> None:
        import torch

        mask = None if row_mask is None else torch.from_numpy(np.ascontiguousarray(row_mask, dtype=np.uint8)).to(self.device)
        sd = torch.from_numpy(np.ascontiguousarray(std, dtype=np.float64)).to(self.device)
        self.K.pp_scale_csr_(m.indptr, m.indices, m.data, m.n_major, sd, max_value=max_value, row_mask=mask)

    def scale_dense(self, m: DeviceMatrix, mean: np.ndarray, std: np.ndarray, *, max_value=None, row_mask=None,
                    out_f64: bool = True) -> np.ndarray:
        import torch

        mask = None if row_mask is None else torch.from_numpy(np.ascontiguousarray(row_mask, dtype=np.uint8)).to(self.device)
        mu = torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float64)).to(self.device)
        sd = torch.from_numpy(np.ascontiguousarray(std, dtype=np.float64)).to(self.device)
        out = self.K.pp_scale_dense(m.indptr, m.indices, m.data, m.n_major, m.shape[1], mu, sd, max_value=max_value,
                                    row_mask=mask, out_dtype=torch.float64 if out_f64 else torch.float32)
        return out.cpu().numpy()

    def _regress_model(self, w, codes):
        import torch

        wd = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(self.device)
        cd = None if codes is None else torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).to(self.device)
        return wd, cd

    def regress_sums(self, m: DeviceMatrix, *, w=None, codes=None, n_table: int, wbound: np.ndarray) -> dict:
        """The first device half of `pp.regress_out` (csrc/regress.hip): W^T X for W = `w` (float64 [n, n_table]) or the
        one-hot of `codes` (int32 [n], n_table categories); wbound[k] >= sum_i |W[i, k]|.
        -> sums float64 [n_table, g], col_min / col_max float32 [g] over all cells (implicit zeros included),
        nonfinite (a stored value was NaN or infinite), bad_code (a code outside [0, n_table))."""
        import torch

        wd, cd = self._regress_model(w, codes)
        wb = torch.from_numpy(np.ascontiguousarray(wbound, dtype=np.float64)).to(self.device)
        s, lo, hi, flags = self.K.pp_regress_sums(m.indptr, m.indices, m.data, m.n_major, m.shape[1], w=wd, codes=cd,
                                                  m=int(n_table), wbound=wb)
        f = int(flags.cpu()[0])
        return {"sums": s.cpu().numpy(), "col_min": lo.cpu().numpy(), "col_max": hi.cpu().numpy(),
                "nonfinite": bool(f & 1), "bad_code": bool(f & 2)}

    def regress_resid(self, m: DeviceMatrix, table: np.ndarray, keep: np.ndarray, *, w=None, codes=None,
                      out_f64: bool = True) -> np.ndarray:
        """The second half: the dense x - W @ table (float64 arithmetic, rounded once) for the genes with keep, x for the others"""
        import torch

        wd, cd = self._regress_model(w, codes)
        t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).to(self.device)
        kp = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8)).to(self.device)
        out = self.K.pp_regress_resid(m.indptr, m.indices, m.data, m.n_major, m.shape[1], kp, t, w=wd, codes=cd,
                                      out_dtype=torch.float64 if out_f64 else torch.float32)
        return out.cpu().numpy()

    # ---- analytic Pearson residuals (csrc/pearson.hip; `experimental.pp`) -------------------------------------
    def row_totals64(self, m: DeviceMatrix) -> np.ndarray:
        """the sum of every row in float64 (fixed order)"""
        return self.K.csr_row_stats(m.indptr, m.data, m.n_major)[0].cpu().numpy()

    def _csc_copy(self, m: DeviceMatrix):
        """the CSC copy of the resident CSR matrix, made once per matrix: on the device up to the 40 944 columns of
        `scamd_csr_transpose_f32`, beyond that by one pass on the host"""
        import torch

        if getattr(m, "csc", None) is None:
            n, g = m.n_major, m.shape[1]
            if g <= 40944:
                m.csc = self.K.csr_transpose(m.indptr, m.indices, m.data, n, g)
            else:
                t = sparse.csr_matrix((m.data.cpu().numpy(), m.indices.cpu().numpy(), m.indptr.cpu().numpy()), shape=(n, g)).tocsc()
                m.csc = (torch.from_numpy(t.indptr.astype(np.int64)).to(self.device), torch.from_numpy(t.indices.astype(np.int32)).to(self.device),
                         torch.from_numpy(t.data).to(self.device))
        return m.csc

    def pearson_gene_var(self, m: DeviceMatrix, gene_sum: np.ndarray, cell_total: np.ndarray, total: float, *, inv_theta: float,
                         clip: float, batch_codes=None, batch_id: int = 0, n_batch: int | None = None) -> np.ndarray:
        """-> float64 [g]: the population variance of every gene's clipped Pearson residuals over the cells with
        batch_codes == batch_id (all cells without codes); gene_sum and total are that batch's.  The distinct totals of the
        batch's cells and their multiplicities are found on the device (`torch.unique`, ascending)."""
        import torch

        n, g = m.n_major, m.shape[1]
        ct = torch.from_numpy(np.ascontiguousarray(cell_total, dtype=np.float64)).to(self.device)
        gs = torch.from_numpy(np.ascontiguousarray(gene_sum, dtype=np.float64)).to(self.device)
        codes = None if batch_codes is None else torch.from_numpy(np.ascontiguousarray(batch_codes, dtype=np.int32)).to(self.device)
        own = ct if codes is None else ct[codes == int(batch_id)]
        tot_u, mult_u = torch.unique(own, sorted=True, return_counts=True)
        t_indptr, t_rows, t_data = self._csc_copy(m)
        var = self.K.pp_pearson_gene_var(t_indptr, t_rows, t_data, n, g, gs, ct, float(total), float(inv_theta), float(clip),
                                         tot_u.contiguous(), mult_u.to(torch.float64).contiguous(),
                                         int(own.numel()) if n_batch is None else int(n_batch), batch_codes=codes, batch_id=int(batch_id))
        return var.cpu().numpy()

    def pearson_residuals(self, m: DeviceMatrix, gene_sum: np.ndarray, cell_total: np.ndarray, total: float, *, inv_theta: float,
                          clip: float, out_f64: bool = True) -> np.ndarray:
        """-> [n, g]: the dense matrix of clipped Pearson residuals, float64 arithmetic rounded once to the output type"""
        import torch

        ct = torch.from_numpy(np.ascontiguousarray(cell_total, dtype=np.float64)).to(self.device)
        gs = torch.from_numpy(np.ascontiguousarray(gene_sum, dtype=np.float64)).to(self.device)
        out = self.K.pp_pearson_residuals(m.indptr, m.indices, m.data, m.n_major, m.shape[1], gs, ct, float(total), float(inv_theta),
                                          float(clip), out_dtype=torch.float64 if out_f64 else torch.float32)
        return out.cpu().numpy()

    # ---- scrublet (csrc/scrublet.hip; the matrices stay on the device between these calls) --------------------
    def scrublet_simulate(self, m: DeviceMatrix, pairs: np.ndarray, row_total: np.ndarray):
        """Row-pair sums of the resident counts: -> (DeviceMatrix [n_sim, g] of the simulated doublets, total_sim numpy like
        row_total, inexact: a sum left the range in which float32 holds integers exactly)"""
        import torch

        pd_ = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)).to(self.device)
        rt = np.ascontiguousarray(row_total)
        rt = rt if rt.dtype in (np.float32, np.float64) else rt.astype(np.float64)
        rd = torch.from_numpy(rt).to(self.device)
        indptr, indices, data, total, flags = self.K.pp_scrublet_pairs(m.indptr, m.indices, m.data, m.n_major, m.shape[1], pd_, rd)
        if flags & 6:
            raise RuntimeError(f"scrublet row-pair kernel: flags {flags} (a parent index outside the matrix, or a bad row pointer)")
        sim = DeviceMatrix("csr", (int(pd_.shape[0]), m.shape[1]), indptr, indices, data, None)
        return sim, total.cpu().numpy().astype(np.asarray(row_total).dtype, copy=False), bool(flags & 1)

    def scrublet_download(self, m: DeviceMatrix) -> sparse.csr_matrix:
        return sparse.csr_matrix((m.data.cpu().numpy(), m.indices.cpu().numpy(), m.indptr.cpu().numpy()), shape=m.shape)

    def scrublet_call(self, m_obs: DeviceMatrix, m_sim: DeviceMatrix, *, log_transform: bool, renormalize: bool, mean_center: bool,
                      normalize_variance: bool, n_prin_comps: int, k_adj: int, metric: str, rho: float, r: float, se_rho: float,
                      want_neighbors: bool = False, want_manifold: bool = False) -> dict:
        """The resident stage of `pp.scrublet`; both matrices are rewritten in place.  (log1p) -> (normalize_total 1e6, each
        matrix by its own row sums) -> (1 / sigma scaling of both by the observed matrix's statistics) -> PCA / truncated SVD
        fitted on the observed matrix -> both projected by one spmm with the shift mean . V -> exact kNN on the concatenated
        manifold -> scores.  -> n_sim_neigh int32, score, score_err float64 [n_obs + n_sim] (+ neighbors int32, manifold float32)"""
        import torch

        K = self.K
        n_obs, g = m_obs.shape
        for m in (m_obs, m_sim):
            if log_transform:
                K.pp_log1p_(m.data)
            if renormalize:
                # the factor is numpy's float32 division, as `normalize_total` makes it (a device division by a scalar is a
                # multiplication by its reciprocal: other bits); the n row sums make the round trip, the matrix stays
                factor = K.pp_row_sums(m.indptr, m.indices, m.data, m.n_major).cpu().numpy() / 1e6
                K.pp_row_divide_(m.indptr, m.data, m.n_major, torch.from_numpy(factor).to(self.device))
        if normalize_variance:
            s, sq, _ = K.pp_col_stats(m_obs.indptr, m_obs.indices, m_obs.data, n_obs, g, count_positive=False)
            _, var = mean_var_from_sums(s, sq, n_obs, correction=1)
            std = torch.sqrt(var)
            flat = int((~(std > 0)).sum())
            if flat:
                raise ValueError(f"{flat} of {g} genes have zero variance over the observed cells: their z-score is undefined. "
                                 "Filter them out first (`filter_genes`) or pass `normalize_variance=False`.")
            for m in (m_obs, m_sim):
                K.pp_scale_csr_(m.indptr, m.indices, m.data, m.n_major, std)
        _, comps, _, _, mean, _ = K.pca_csr(m_obs.indptr, m_obs.indices, m_obs.data, n_obs, g, int(n_prin_comps),
                                            zero_center=bool(mean_center), seed=0)
        v = comps.t().contiguous()
        shift = (mean @ v) if mean_center else None
        manifold = torch.cat([K.spmm(m.indptr, m.indices, m.data, m.n_major, g, v, shift) for m in (m_obs, m_sim)], dim=0)
        rows = manifold
        if metric in ("cosine", "correlation"):  # as `neighbors` prepares its rows
            x64 = manifold.to(torch.float64)
            if metric == "correlation":
                x64 = x64 - x64.mean(dim=1, keepdim=True)
            norm = torch.linalg.norm(x64, dim=1, keepdim=True)
            if bool((norm == 0).any()):
                raise ValueError(f"metric={metric!r} is undefined for " + ("all-zero rows" if metric == "cosine" else "constant rows"))
            rows = (x64 / norm).to(torch.float32).contiguous()
        idx, _, _ = K.knn(rows, int(k_adj))
        cnt, score, err = K.scrublet_scores(idx, n_obs, rho=rho, r=r, se_rho=se_rho)
        out = {"n_sim_neigh": cnt.cpu().numpy(), "score": score.cpu().numpy(), "score_err": err.cpu().numpy()}
        if want_neighbors:
            out["neighbors"] = idx.cpu().numpy()
        if want_manifold:
            out["manifold"] = manifold.cpu().numpy()
        return out


def default_backend():
    return GpuPPBackend()


def in_memory(x):
    """The upstream chain works on a matrix in memory (most of its passes rewrite it); an on-disk matrix
    (`read_h5ad` / `read_zarr(..., backed='r')`) streams through `pp.pca`, `pp.highly_variable_genes` and
    `pp.calculate_qc_metrics`;
    `pp.normalize_total` / `pp.log1p` turn into pending transforms of it."""
    if getattr(x, "is_backed", False):
        raise NotImplementedError(
            "this function needs the matrix in memory: load it with `adata.X = adata.X.to_memory()` (or read without "
            "backed='r'); on a backed matrix only calculate_qc_metrics, normalize_total, log1p, highly_variable_genes and pca are offered")
    return x


def mean_var_from_sums(s: np.ndarray, sq: np.ndarray, n: int, *, correction: int = 1):
    """fast_array_utils.stats.mean_var semantics: mean, (E[x^2] - E[x]^2) * n / (n - correction)."""
    mean = s / n
    var = sq / n - mean * mean
    if correction and n > correction:
        var = var * (n / (n - correction))
    return mean, var
