"""`sc.pp.scrublet` / `sc.pp.scrublet_simulate_doublets` on MI355X (reference: src/scanpy/preprocessing/_scrublet/{__init__,core,
pipeline}.py, `sample_comb` in src/scanpy/preprocessing/_utils.py).

Scrublet is a PCA fit, a projection and an exact kNN search over (1 + sim_doublet_ratio) times the cells; the project owns all
three.  What is added on the device (csrc/scrublet.hip) is the building of the simulated doublets -- sparse row-pair sums -- and
the turning of neighbour lists into scores.  From the upload on, both matrices stay resident until the scores come down
(`GpuPPBackend.scrublet_call`):

* the z-score needs no dense matrix: both CSR matrices are scaled by 1 / sigma in place, the PCA of X D^-1 WITH centring is the
  PCA of the z-scored matrix, and both matrices are projected by one spmm with the shift mean . V;
* the parents are drawn on the host exactly as `sample_comb` draws them, so `doublet_parents` equals the reference's for the same
  `rng`; nothing else of the result depends on the generator (the eigensolver's start block has a fixed seed);
* the exact kNN engine serves k <= 256: k_adj = round(k (1 + n_sim / n_obs)) beyond that is refused (with the defaults above
  about 29 000 cells per run); Scrublet is meant per sample: `batch_key`.

Not offered: `synthetic_doublet_umi_subsampling < 1` (needs a device binomial sampler), approximate neighbours, metrics other
than those of `pp.neighbors`, a backed matrix, float64 input."""
from __future__ import annotations

import logging

import numpy as np
import pandas as pd

from .._anndata import AnnData
from .._utils import _UNSET
from ..neighbors._transformer import METRICS
from . import _csr_device
from ._filter import filter_cells, filter_genes
from ._highly_variable_genes import highly_variable_genes
from ._normalization import normalize_total
from ._pca import _get_arr
from ._simple import log1p

_log = logging.getLogger("scanpy_amd")

MAX_K = 256  # the exact kNN engine's limit (scamd_knn_workspace_bytes)
EXACT_F32 = 2.0 ** 24


class _LegacyRng:
    """the reference's `_LegacyRng` as far as scrublet uses it: the legacy `random_state` argument carried along"""

    def __init__(self, arg):
        self.arg = arg

    def spawn(self, n: int) -> list:
        return [self] * n


def _resolve_rng(rng, random_state):
    """`_accepts_legacy_random_state(0)`: -> (np.random.Generator | _LegacyRng, the `random_state` entry of uns, if any)"""
    if rng is not None and random_state is not _UNSET:
        raise TypeError("Specify at most one of `rng` and `random_state`.")
    if rng is not None:
        return (rng if isinstance(rng, _LegacyRng) else np.random.default_rng(rng)), {}
    arg = 0 if random_state is _UNSET else random_state
    return _LegacyRng(arg), {"random_state": arg}


def _sample_pairs(n_obs: int, n_sim: int, rng) -> np.ndarray:
    """`sample_comb((n_obs, n_obs), n_sim)`: distinct ordered pairs, int64 [n_sim, 2]"""
    if isinstance(rng, _LegacyRng):
        try:
            from sklearn.random_projection import sample_without_replacement
        except ImportError as e:  # pragma: no cover
            raise ImportError("the legacy `random_state` route of scrublet draws the parents with scikit-learn's "
                              "`sample_without_replacement`; install scikit-learn or pass `rng=`") from e
        idx = sample_without_replacement(n_obs * n_obs, n_sim, random_state=rng.arg)
    else:
        idx = rng.choice(n_obs * n_obs, size=n_sim, replace=False)
    return np.vstack(np.unravel_index(idx, (n_obs, n_obs))).T


def _threshold_minimum(scores: np.ndarray, *, nbins: int = 256, max_num_iter: int = 10000):
    """`skimage.filters.threshold_minimum` restated (scikit-image is not a dependency): -> (threshold, smoothing passes).
    A 256-bin histogram over [min, max] with its bin centres, the counts as float32, smoothed by
    `scipy.ndimage.uniform_filter1d(h, 3)` until fewer than three local maxima remain (a maximum is recorded where the histogram
    turns from non-decreasing to decreasing, so a plateau counts once), 10 000 passes at most; the result is the centre of the
    lowest smoothed bin between the two maxima, both included.  Raises RuntimeError unless exactly two maxima remain and the
    last pass did not hit the limit.

    Written from memory of scikit-image >= 0.19; the library is not available where this was written, so the restatement has
    not been cross-checked against it."""
    from scipy.ndimage import uniform_filter1d

    scores = np.asarray(scores, dtype=np.float64).ravel()
    if scores.size == 0 or not np.isfinite(scores).all():
        raise RuntimeError("Unable to find two maxima in histogram")
    counts, edges = np.histogram(scores, bins=nbins, range=(scores.min(), scores.max()))
    centres = (edges[:-1] + edges[1:]) / 2.0
    smooth = counts.astype(np.float32)

    def maxima(h):
        found, rising = [], True
        for i in range(h.shape[0] - 1):
            if rising:
                if h[i + 1] < h[i]:
                    rising = False
                    found.append(i)
            elif h[i + 1] > h[i]:
                rising = True
        return found

    peaks, counter = [], 0
    for counter in range(max_num_iter):
        smooth = uniform_filter1d(smooth, 3)
        peaks = maxima(smooth)
        if len(peaks) < 3:
            break
    if len(peaks) != 2:
        raise RuntimeError("Unable to find two maxima in histogram")
    if counter == max_num_iter - 1:
        raise RuntimeError("Maximum iteration reached for histogram shape")
    lowest = int(np.argmin(smooth[peaks[0]: peaks[1] + 1]))
    return float(centres[peaks[0] + lowest]), counter + 1


def _k_adjusted(n_obs: int, n_sim: int, n_neighbors) -> tuple:
    k = round(0.5 * np.sqrt(n_obs)) if n_neighbors is None else n_neighbors
    return k, round(k * (1 + n_sim / float(n_obs))) if n_obs else 0


def _check_k(n_obs: int, n_sim: int, n_neighbors, *, when: str = "") -> None:
    k, k_adj = _k_adjusted(n_obs, n_sim, n_neighbors)
    if k_adj > MAX_K:
        msg = (f"scrublet: k_adj = round(n_neighbors (1 + n_sim / n_obs)) = {k_adj} neighbours per cell for n_obs = {n_obs}{when}, "
               f"n_sim = {n_sim}, n_neighbors = {k}: the exact kNN engine serves at most {MAX_K}. With the defaults this is reached "
               "above about 29 000 cells per run. Scrublet is meant to be run per sample: pass `batch_key`, or lower `n_neighbors`.")
        raise NotImplementedError(msg)


def _check_options(*, knn_dist_metric, use_approx_neighbors, synthetic_doublet_umi_subsampling) -> None:
    if use_approx_neighbors:
        msg = ("use_approx_neighbors=True (annoy / pynndescent) is outside the MI355X hot path: the doublet scores come from "
               "the exact search.")
        raise NotImplementedError(msg)
    if callable(knn_dist_metric) or knn_dist_metric not in METRICS:
        msg = f"metric={knn_dist_metric!r}: the MI355X kNN kernel offers {METRICS}."
        raise NotImplementedError(msg)
    _check_subsampling(synthetic_doublet_umi_subsampling)


def _check_subsampling(rate) -> None:
    if rate < 1:
        msg = (f"synthetic_doublet_umi_subsampling={rate}: drawing binomial(count, rate) for every stored count needs a device "
               "binomial sampler, which is not built yet; only 1.0 (plain sums of the two parents) is offered.")
        raise NotImplementedError(msg)


def _set_obs_names(adata, names) -> None:
    try:
        adata.obs_names = names
    except AttributeError:  # the stand-in AnnData: obs_names is the index of obs
        adata.obs.index = names


def _simulate(be, m_raw, n_obs: int, sim_doublet_ratio: float, rng):
    """-> (DeviceMatrix of the doublets, parents int64 [n_sim, 2], total_sim float64 [n_sim])"""
    n_sim = int(n_obs * sim_doublet_ratio)
    pairs = _sample_pairs(n_obs, n_sim, rng)
    row_total = be.row_sums(m_raw).astype(np.float64)
    m_sim, total_sim, inexact = be.scrublet_simulate(m_raw, pairs, row_total)
    if inexact:
        raise ValueError(f"a simulated doublet holds a count above 2^24 = {int(EXACT_F32)}: float32 no longer holds such sums of "
                         "integer counts exactly. The input does not look like raw UMI counts.")
    return m_sim, pairs, total_sim


def scrublet_simulate_doublets(adata, *, layer: str | None = None, sim_doublet_ratio: float = 2.0,
                               synthetic_doublet_umi_subsampling: float = 1.0, rng=None, random_state=_UNSET):
    """Simulate doublets by adding the counts of random observed transcriptome pairs (drop-in for
    `scanpy.pp.scrublet_simulate_doublets`).  The sums are made on the device (`scamd_pp_scrublet_pair_*`).

    Returns an AnnData with the simulated doublets (CSR float32) in `.X`, `obs['n_counts']` (the sum of the parents' totals, in
    the dtype the reference gives: that of the matrix, int64 for integers), `obsm['doublet_parents']` and
    `uns['scrublet']['parameters']`.  Only `synthetic_doublet_umi_subsampling=1.0` is offered."""
    rng, _ = _resolve_rng(rng, random_state)
    _check_subsampling(synthetic_doublet_umi_subsampling)
    x = _csr_device.in_memory(_get_arr(adata, layer=layer))
    be = _csr_device.default_backend()
    m_sim, pairs, total_sim = _simulate(be, be.upload(x), x.shape[0], sim_doublet_ratio, rng)
    adata_sim = AnnData(be.scrublet_download(m_sim))
    dt = np.dtype(x.dtype)
    adata_sim.obs["n_counts"] = total_sim.astype(np.int64 if dt.kind in "iub" else dt)
    adata_sim.obsm["doublet_parents"] = pairs
    adata_sim.uns["scrublet"] = {"parameters": {"sim_doublet_ratio": sim_doublet_ratio}}
    return adata_sim


def _call_doublets(adata_obs, be, m_obs, m_sim, parents, *, sim_doublet_ratio, prepared: bool, log_transform: bool, n_neighbors,
                   expected_doublet_rate, stdev_doublet_rate, mean_center, normalize_variance, n_prin_comps, knn_dist_metric,
                   get_doublet_neighbor_parents, threshold, verbose, meta_random_state, hook=None):
    """`_scrublet_call_doublets`: prepared = the matrices are raw counts still to be (log-transformed and) normalised"""
    n_obs, n_sim = m_obs.shape[0], m_sim.shape[0]
    n_neighbors, k_adj = _k_adjusted(n_obs, n_sim, n_neighbors)
    _check_k(n_obs, n_sim, n_neighbors)
    _log.info("Embedding transcriptomes using PCA..." if mean_center else "Embedding transcriptomes using Truncated SVD...")
    r = n_sim / float(n_obs)
    res = be.scrublet_call(m_obs, m_sim, log_transform=bool(prepared and log_transform), renormalize=bool(prepared),
                           mean_center=bool(mean_center), normalize_variance=bool(normalize_variance), n_prin_comps=n_prin_comps,
                           k_adj=k_adj, metric=knn_dist_metric, rho=expected_doublet_rate, r=r, se_rho=stdev_doublet_rate,
                           want_neighbors=bool(get_doublet_neighbor_parents), want_manifold=hook is not None)
    if hook is not None:
        hook(dict(res, n_obs=n_obs, k_adj=k_adj))
    ld_obs, ld_sim = res["score"][:n_obs], res["score"][n_obs:]
    se_obs = res["score_err"][:n_obs]
    adata_obs.obs["doublet_score"] = ld_obs
    adata_obs.uns["scrublet"] = {
        "doublet_scores_sim": ld_sim,
        "doublet_parents": parents,
        "parameters": {"expected_doublet_rate": expected_doublet_rate, "sim_doublet_ratio": sim_doublet_ratio,
                       "n_neighbors": n_neighbors, **meta_random_state},
    }
    found = threshold is not None
    if threshold is None:
        try:
            threshold, _ = _threshold_minimum(ld_sim)
            found = True
            if verbose:
                _log.info("Automatically set threshold at doublet score = %.2f", threshold)
        except Exception:  # noqa: BLE001  (as the reference: any failure of the automatic threshold)
            if verbose:
                _log.warning("Failed to automatically identify doublet score threshold. "
                             "Run `call_doublets` with user-specified threshold.")
    if found:
        predicted = ld_obs > threshold
        detected = predicted.sum() / float(len(ld_obs))
        with np.errstate(divide="ignore", invalid="ignore"):
            detectable = (ld_sim > threshold).sum() / float(len(ld_sim))
            overall = detected / detectable
        if verbose:
            _log.info("Detected doublet rate = %.1f%%\nEstimated detectable doublet fraction = %.1f%%\nOverall doublet rate:\n"
                      "\tExpected   = %.1f%%\n\tEstimated  = %.1f%%", 100 * detected, 100 * detectable,
                      100 * expected_doublet_rate, 100 * overall)
        adata_obs.uns["scrublet"]["threshold"] = threshold
        adata_obs.obs["predicted_doublet"] = predicted
    else:
        adata_obs.obs["predicted_doublet"] = False
    del se_obs  # (the z-scores of the reference's Scrublet object are not part of what the front end returns)
    if get_doublet_neighbor_parents:
        neigh = res["neighbors"][:n_obs].astype(np.int64) - n_obs
        out = []
        for c in range(n_obs):
            mine = neigh[c][neigh[c] > -1]
            out.append(np.unique(parents[mine, :].flatten()) if len(mine) else np.array([], dtype=np.intp))
        adata_obs.uns["scrublet"]["doublet_neighbor_parents"] = out
    return adata_obs


def scrublet(adata, adata_sim=None, *, batch_key: str | None = None, sim_doublet_ratio: float = 2.0,  # noqa: PLR0913
             expected_doublet_rate: float = 0.05, stdev_doublet_rate: float = 0.02, synthetic_doublet_umi_subsampling: float = 1.0,
             knn_dist_metric="euclidean", normalize_variance: bool = True, log_transform: bool = False, mean_center: bool = True,
             n_prin_comps: int = 30, use_approx_neighbors: bool | None = None, get_doublet_neighbor_parents: bool = False,
             n_neighbors: int | None = None, threshold: float | None = None, verbose: bool = True, copy: bool = False,
             rng=None, random_state=_UNSET, _hook=None):
    """Predict doublets using Scrublet (drop-in for `scanpy.pp.scrublet`; parameters, slots and dtypes as there).

    Without `adata_sim`: raw counts in, `filter_genes(min_cells=3)`, `filter_cells(min_genes=3)`, `normalize_total`, `log1p`,
    `highly_variable_genes` on a copy, doublets simulated from the raw counts of the selected genes, both matrices normalised
    to 1e6 per cell.  With `adata_sim` (from `scrublet_simulate_doublets`): both objects are taken as prepared.
    Writes `obs['doublet_score']`, `obs['predicted_doublet']`, `uns['scrublet']` (`doublet_scores_sim`, `doublet_parents`,
    `parameters`, `threshold` when one was given or found; per batch under `batches` with `batched_by`).

    Limits: k_adj = round(n_neighbors (1 + n_sim / n_obs)) <= 256 (checked on the cell count before filtering, before anything
    runs, and again after); `knn_dist_metric` in ('euclidean', 'l2', 'sqeuclidean', 'cosine', 'correlation'), exact search only;
    `synthetic_doublet_umi_subsampling` must be 1.0; a gene with zero variance over the observed cells raises ValueError when
    `normalize_variance` (the reference produces NaN there and fails inside PCA).  `threshold=None` uses a restatement of
    scikit-image's `threshold_minimum` (`_threshold_minimum`)."""
    rng, meta_random_state = _resolve_rng(rng, random_state)
    _check_options(knn_dist_metric=knn_dist_metric, use_approx_neighbors=use_approx_neighbors,
                   synthetic_doublet_umi_subsampling=synthetic_doublet_umi_subsampling)
    if batch_key is not None and batch_key not in adata.obs.columns:
        msg = ("`batch_key` must be a column of .obs in the input AnnData object,"
               f"but {batch_key!r} is not in {adata.obs.keys()!r}.")
        raise ValueError(msg)
    if adata_sim is not None:
        if adata_sim.n_vars != adata.n_vars:
            raise ValueError(f"`adata_sim` has {adata_sim.n_vars} vars, `adata` has {adata.n_vars}: both must hold the same genes")
        if "doublet_parents" not in adata_sim.obsm:
            raise ValueError("`adata_sim.obsm['doublet_parents']` is missing: build `adata_sim` with `scrublet_simulate_doublets`")
    _csr_device._check_dtype(np.dtype(_csr_device.in_memory(adata.X).dtype))
    # the k limit, before any kernel starts: on the cell counts as they come in (filter_cells can only lower them)
    sizes = [adata.n_obs] if batch_key is None else [int(c) for c in adata.obs[batch_key].value_counts() if c]
    for n_b in sizes:
        _check_k(n_b, adata_sim.n_obs if adata_sim is not None else int(n_b * sim_doublet_ratio), n_neighbors, when=" (before filtering)")
    if copy:
        adata = adata.copy()
    _log.info("Running Scrublet")
    adata_obs = adata.copy()
    # `adata.obs_names` may contain duplicates and cells may get filtered out below: positional labels map the results back
    positions = pd.RangeIndex(adata.n_obs).astype(str)
    _set_obs_names(adata_obs, positions)
    be = _csr_device.default_backend()
    common = dict(n_neighbors=n_neighbors, expected_doublet_rate=expected_doublet_rate, stdev_doublet_rate=stdev_doublet_rate,
                  mean_center=mean_center, normalize_variance=normalize_variance, n_prin_comps=n_prin_comps,
                  knn_dist_metric=knn_dist_metric, get_doublet_neighbor_parents=get_doublet_neighbor_parents, threshold=threshold,
                  verbose=verbose, meta_random_state=meta_random_state, log_transform=log_transform, hook=_hook)

    def run(ad_obs, ad_sim, rng):
        if ad_sim is None:
            filter_genes(ad_obs, min_cells=3)
            filter_cells(ad_obs, min_genes=3)
            # doublets are simulated from the raw counts, but of the genes selected after normalisation
            ad_obs.layers["raw"] = ad_obs.X.copy()
            normalize_total(ad_obs)
            ad_obs.layers["log1p"] = ad_obs.X.copy()
            log1p(ad_obs, layer="log1p")
            highly_variable_genes(ad_obs, layer="log1p")
            del ad_obs.layers["log1p"]
            ad_obs = ad_obs[:, np.asarray(ad_obs.var["highly_variable"], dtype=bool)].copy()
            m_sim, parents, _ = _simulate(be, be.upload(ad_obs.layers["raw"]), ad_obs.n_obs, sim_doublet_ratio, rng)
            del ad_obs.layers["raw"]
            m_obs = be.upload(ad_obs.X)
            ad_obs = _call_doublets(ad_obs, be, m_obs, m_sim, parents, sim_doublet_ratio=sim_doublet_ratio, prepared=True, **common)
        else:
            m_obs, m_sim = be.upload(_csr_device.in_memory(ad_obs.X)), be.upload(_csr_device.in_memory(ad_sim.X))
            ratio = ad_sim.uns.get("scrublet", {}).get("parameters", {}).get("sim_doublet_ratio", None)
            ad_obs = _call_doublets(ad_obs, be, m_obs, m_sim, np.asarray(ad_sim.obsm["doublet_parents"]), sim_doublet_ratio=ratio,
                                    prepared=False, **common)
        return {"obs": ad_obs.obs, "uns": ad_obs.uns["scrublet"]}

    if batch_key is not None:
        batches = np.unique(adata.obs[batch_key])
        sub_rngs = rng.spawn(len(batches))
        scrubbed = [run(adata_obs[np.asarray(adata_obs.obs[batch_key] == batch)].copy(), adata_sim, sub)
                    for batch, sub in zip(batches, sub_rngs)]
        scrubbed_obs = pd.concat([s["obs"] for s in scrubbed]).astype(adata.obs.dtypes)
        adata.obs = scrubbed_obs.reindex(positions).set_axis(adata.obs_names)
        adata.uns["scrublet"] = {"batches": dict(zip(batches, [s["uns"] for s in scrubbed])), "batched_by": batch_key}
    else:
        scrubbed = run(adata_obs, adata_sim, rng)
        scrubbed_obs = scrubbed["obs"].reindex(positions)
        adata.obs["doublet_score"] = scrubbed_obs["doublet_score"].to_numpy()
        adata.obs["predicted_doublet"] = scrubbed_obs["predicted_doublet"].to_numpy()
        adata.uns["scrublet"] = scrubbed["uns"]
    _log.info("    Scrublet finished")
    return adata if copy else None
