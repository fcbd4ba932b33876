"""`sc.pp.harmony_integrate` on MI355X (src/scanpy/preprocessing/_harmony/): validation, batch codes, theta and the two
convergence loops (`HarmonyRun`) live here; every sum over cells runs in csrc/harmony.hip (scamd_harmony_*).  One small read-back (the
objective, 4 doubles) per clustering iteration."""
from __future__ import annotations

import warnings

import numpy as np

__all__ = ["harmony_integrate"]

MAX_D, MAX_K, MAX_LEVELS = 128, 256, 1024
KMEANS_SWEEPS = 25


def _fail(kind, text):
    raise kind(text)


def _encode_batches(obs, keys):
    """the batch columns as level numbers, the levels of column j counted on from those of the columns before it
    -> (codes int32 [cells, columns], level_counts int32 [columns])"""
    names = [keys] if isinstance(keys, str) else list(keys)
    if not names:
        _fail(ValueError, "batch_key must contain at least one column name")
    columns, counts = [], []
    for name in names:
        categorical = obs[name].astype("category").cat  # (a missing column is pandas' KeyError)
        column = np.asarray(categorical.codes, dtype=np.int32)
        if column.size and column.min() < 0:
            _fail(ValueError, f"Batch variable {name!r} contains missing values")
        columns.append(column + sum(counts))
        counts.append(len(categorical.categories))
    return np.stack(columns, axis=1).astype(np.int32), np.asarray(counts, dtype=np.int32)


def _theta_per_level(theta, level_counts):
    """theta for every level of every batch column, float64 [levels]: one number for all, one per column, or one per level"""
    level_counts = np.asarray(level_counts, dtype=np.int64)
    n_levels = int(level_counts.sum())
    try:
        values = np.atleast_1d(np.asarray(theta, dtype=np.float64)).ravel()
    except (TypeError, ValueError) as err:
        raise ValueError(f"theta must be a scalar or an array-like collection of numeric values, got {type(theta).__name__}") from err
    if np.ndim(theta) == 0:
        return np.repeat(values, n_levels)
    if values.size == level_counts.size:
        return np.repeat(values, level_counts)
    if values.size == n_levels:
        return values
    _fail(ValueError, f"theta array size ({values.size}) must match the number of batch variables ({level_counts.size}) or categorical "
                      f"levels ({n_levels})")


def _n_blocks(n_cells: int, block_proportion: float) -> int:
    # (floor division of floats: 1 // 0.05 is 19.0, hence 19 blocks at the default and not 20)
    return int(min(n_cells, 1 // block_proportion))


def _outer_converged(objectives, tol: float) -> bool:
    """the last recorded objective fell by less than tol of the one before"""
    if len(objectives) < 2:
        return False
    before, now = objectives[-2:]
    return before - now < tol * abs(before)


def _clustering_converged(objectives, tol: float, window: int = 3) -> bool:
    """the sum of the last `window` objectives fell by less than tol of the sum of the `window` before, one step back"""
    if len(objectives) <= window:
        return False
    before, now = sum(objectives[-window - 1:-1]), sum(objectives[-window:])
    return before - now < tol * abs(before)


def _check_arguments(flavor, correction_method, ridge_lambda, alpha, batch_prune_threshold):
    """the two choices, then a warning for every parameter that was set although the flavor does not read it"""
    if flavor not in ("harmony1", "harmony2"):
        _fail(ValueError, f"flavor must be 'harmony1' or 'harmony2', got {flavor!r}.")
    if correction_method != "fast":
        _fail(ValueError, f"correction_method must be 'fast', got {correction_method!r}.")
    unread = {
        "harmony2": [(ridge_lambda != 1.0, "ridge_lambda is ignored when flavor='harmony2'; use alpha to control regularization strength.")],
        "harmony1": [(alpha != 0.2, "alpha is ignored when flavor='harmony1'; use ridge_lambda instead."),
                     (batch_prune_threshold != 1e-5, "batch_prune_threshold is ignored when flavor='harmony1'.")],
    }
    for was_set, text in unread[flavor]:
        if was_set:
            warnings.warn(text, UserWarning, stacklevel=3)


def _check_ranges(flavor, ridge_lambda, alpha, batch_prune_threshold, max_iter_harmony):
    positive = lambda v: bool(np.isfinite(v)) and v > 0  # noqa: E731
    if max_iter_harmony < 1:
        _fail(ValueError, "max_iter_harmony must be >= 1")
    if flavor == "harmony2" and not positive(alpha):
        _fail(ValueError, f"alpha must be a finite positive number when dynamic_lambda=True, got {alpha}.")
    if flavor == "harmony2" and batch_prune_threshold is not None and not 0 <= batch_prune_threshold <= 1:
        _fail(ValueError, f"batch_prune_threshold must be in [0, 1] or None, got {batch_prune_threshold}.")
    if flavor == "harmony1" and not positive(ridge_lambda):
        _fail(ValueError, f"ridge_lambda must be a finite positive number when dynamic_lambda=False, got {ridge_lambda}.")


def _embedding(adata, basis, dtype):
    """`adata.obsm[basis]` as a C-contiguous array of `dtype`, free of NaN"""
    if basis not in adata.obsm:
        _fail(ValueError, f"The specified basis {basis!r} is not available in `adata.obsm`. Available bases: {list(adata.obsm.keys())}")
    stored = adata.obsm[basis]
    try:
        x = np.ascontiguousarray(stored, dtype=dtype)
    except Exception as err:  # whatever the container raises on conversion
        raise TypeError(f"Could not convert input of type {type(stored).__name__} to NumPy array.") from err
    if np.isnan(x).any():
        _fail(ValueError, "Input data contains NaN values. Please handle these before running harmony_integrate.")
    return x


def harmony_integrate(adata, key, *, basis: str = "X_pca", adjusted_basis: str = "X_pca_harmony", dtype=np.float64,
                      flavor: str = "harmony2", n_clusters: int | None = None, max_iter_harmony: int = 10, max_iter_clustering: int = 200,
                      tol_harmony: float = 1e-4, tol_clustering: float = 1e-5, sigma: float = 0.1, theta=2.0, tau: int = 0,
                      ridge_lambda: float = 1.0, alpha: float = 0.2, batch_prune_threshold: float | None = 1e-5,
                      correction_method: str = "fast", block_proportion: float = 0.05, rng=None) -> None:
    """Harmony batch correction of an embedding (drop-in for `scanpy.pp.harmony_integrate`): reads `adata.obsm[basis]` and the
    batch column `adata.obs[key]`, writes `adata.obsm[adjusted_basis]`.  Run it after `pp.pca` and before
    `pp.neighbors(use_rep='X_pca_harmony')`.  Signature, defaults, errors and warnings are the reference's; both flavors
    ('harmony2': stabilised penalty, lambda = alpha * E, pruning; 'harmony1': denominator O + 1, fixed `ridge_lambda`), `tau`
    and `theta` as a scalar, per key or per level are supported.

    Departures from the reference:

    1. The arithmetic is float64 on the device whatever `dtype` says: `dtype` rounds the input and is the type of the output.
    2. The k-means initialisation runs on the device, not in sklearn: k-means++ seeding by D^2 sampling with K uniforms drawn
       from `np.random.default_rng(rng)`, then at most 25 Lloyd sweeps (ties to the lowest cluster, an empty cluster keeps its
       centre, stop when no label changes).  The centres, hence the result, differ from the reference's for the same `rng`.
    3. The permutation of the cells of every clustering iteration is computed on the device, element by element, from a
       64-bit seed (drawn from the same generator) and the iteration counter: a keyed bijection (Feistel network with cycle
       walking), not `rng.permutation`.
    4. Several batch keys raise NotImplementedError: they need the general-design ridge solve, which is not built.
    5. Limits, refused with a message: at most 128 columns, 256 clusters, 1024 batch levels, fewer than 2^31 cells.

    Two runs with the same `rng` give the same bits."""
    _check_arguments(flavor, correction_method, ridge_lambda, alpha, batch_prune_threshold)
    x = _embedding(adata, basis, dtype)
    generator = np.random.default_rng(rng)
    _check_ranges(flavor, ridge_lambda, alpha, batch_prune_threshold, max_iter_harmony)
    codes, level_counts = _encode_batches(adata.obs, key)
    theta_levels = _theta_per_level(theta, level_counts)
    if level_counts.size > 1:
        _fail(NotImplementedError, "harmony_integrate: several batch keys need the exact general-design ridge solve of the correction step, "
                                   "which is separate work; pass one key (or one combined column).")
    run = HarmonyRun(flavor=flavor, n_clusters=n_clusters, max_iter_harmony=max_iter_harmony, max_iter_clustering=max_iter_clustering,
                     tol_harmony=tol_harmony, tol_clustering=tol_clustering, sigma=sigma, tau=tau, ridge_lambda=ridge_lambda, alpha=alpha,
                     batch_prune_threshold=batch_prune_threshold, block_proportion=block_proportion)
    adata.obsm[adjusted_basis] = run.fit(x.astype(np.float64, copy=False), codes[:, 0], int(level_counts[0]), theta_levels, generator).astype(
        x.dtype, copy=False)


class HarmonyRun:
    """One Harmony run on the device for one batch variable.  `fit` returns the corrected embedding and leaves behind what it drew and
    how far it went: `centroids_` (the k-means centres, [K, d]), `seed_` (of the block permutations; round r uses
    `scamd_harmony_permutation_i32(n, seed_, r)`), `n_clusters_`, `n_blocks_`, `kmeans_sweeps_`, `rounds_` (clustering iterations
    of every outer iteration) and `objectives_` (the initial objective and that of every clustering that converged)."""

    def __init__(self, *, flavor="harmony2", n_clusters=None, max_iter_harmony=10, max_iter_clustering=200, tol_harmony=1e-4,
                 tol_clustering=1e-5, sigma=0.1, tau=0, ridge_lambda=1.0, alpha=0.2, batch_prune_threshold=1e-5, block_proportion=0.05):
        self.flavor, self.n_clusters, self.sigma, self.tau = flavor, n_clusters, sigma, tau
        self.max_iter_harmony, self.max_iter_clustering = max_iter_harmony, max_iter_clustering
        self.tol_harmony, self.tol_clustering = tol_harmony, tol_clustering
        self.ridge_lambda, self.alpha, self.batch_prune_threshold = ridge_lambda, alpha, batch_prune_threshold
        self.block_proportion = block_proportion

    def fit(self, x, codes, n_levels, theta, generator):
        """x float64 [n, d] and codes int32 [n] on the host, theta float64 [n_levels] -> z_hat float64 [n, d] on the host"""
        import torch

        from .. import _kernels as K
        from .._device import require_gpu

        n, d = x.shape
        k = max(int(min(100, n / 30)), 2) if self.n_clusters is None else self.n_clusters
        if d > MAX_D or k > MAX_K or n_levels > MAX_LEVELS or n >= 2 ** 31 or d < 1 or k < 1:
            _fail(NotImplementedError, f"harmony_integrate: {n} cells x {d} columns, {k} clusters, {n_levels} batch levels is outside the "
                                       f"supported range (at most {MAX_D} columns, {MAX_K} clusters, {MAX_LEVELS} levels, fewer than 2^31 cells)")
        stabilized = self.flavor == "harmony2"
        n_b = np.bincount(codes, minlength=n_levels).astype(np.float64)
        if self.tau > 0:  # small batches are penalised less
            theta = theta * (1 - np.exp(-n_b / (k * self.tau)) ** 2)
        uniforms = generator.random(k)
        self.seed_ = int(generator.integers(0, 2 ** 64, dtype=np.uint64))
        self.n_clusters_, self.n_blocks_ = k, _n_blocks(n, self.block_proportion)

        dev = require_gpu()
        to_dev = lambda a, t: torch.from_numpy(np.array(a, dtype=t, order="C", copy=True)).to(dev)  # noqa: E731
        x_d, codes_d = to_dev(x, np.float64), to_dev(codes, np.int32)
        n_b_d, pr_b_d, theta_d = to_dev(n_b, np.float64), to_dev(n_b / n, np.float64), to_dev(theta, np.float64)
        z_norm = K.harmony_normalize(x_d)
        centroids, _, self.kmeans_sweeps_ = K.harmony_kmeans(z_norm, k, uniforms, max_iter=KMEANS_SWEEPS)
        self.centroids_ = centroids.cpu().numpy()
        r, e, o, obj = K.harmony_init(z_norm, codes_d, n_levels, centroids, pr_b_d, theta_d, self.sigma, stabilized)
        y_norm = torch.empty((k, d), dtype=torch.float64, device=dev)
        self.objectives_, self.rounds_ = [float(obj[0].item())], []
        rnd, z_hat = 0, None
        for _ in range(self.max_iter_harmony):
            inner = []
            while len(inner) < self.max_iter_clustering:
                perm = K.harmony_permutation(n, self.seed_, rnd)
                rnd += 1
                K.harmony_cluster_round_(z_norm, codes_d, n_levels, perm, self.n_blocks_, pr_b_d, theta_d, self.sigma, stabilized, r, e, o,
                                         y_norm, obj)
                inner.append(float(obj[0].item()))
                if _clustering_converged(inner, self.tol_clustering):
                    self.objectives_.append(inner[-1])  # (a clustering that ran into its cap records nothing)
                    break
            self.rounds_.append(len(inner))
            z_hat, z_norm, _ = K.harmony_correct(x_d, codes_d, n_levels, r, o, e, n_b_d, dynamic_lambda=stabilized, alpha=self.alpha,
                                                 batch_prune_threshold=self.batch_prune_threshold, ridge_lambda=self.ridge_lambda)
            if _outer_converged(self.objectives_, self.tol_harmony):
                break
        return z_hat.cpu().numpy()
