"""TEST INFRASTRUCTURE shared by tests/test_emu_harmony_cpu.py (host emulator, raw C ABI), tests/test_gpu_harmony.py (the
product library on the GPU) and the two front-end test files: the CPU truth of `sc.pp.harmony_integrate`, the case table and
ONE checker per stage.

The truth is a restatement of the Harmony algorithm (src/scanpy/preprocessing/_harmony/core.py, read, not run: it needs a newer
Python) in numpy, written for any float dtype so that it runs in float64 and in `np.longdouble`.  It takes the permutation of
every round and the initial centroids as INPUTS (`reference_way_draws` draws them as the reference does: `rng.permutation`,
sklearn `KMeans(max_iter=25)`), and it restates the two device-side generators: the keyed permutation and the k-means++ /
Lloyd initialisation driven by given uniforms.

Nothing here touches a device: a test hands in a `Runner` with

    permutation(n, seed, round)                                   -> int32 [n]
    kmeans(z_norm, K, uniforms, max_iter)                         -> (centroids [K, d], labels int32 [n], n_iter)
    init(z_norm, codes, B, centroids, pr_b, theta, sigma, stab)   -> (R, E, O, objective [4])
    cluster_round(z_norm, codes, B, perm, n_blocks, pr_b, theta, sigma, stab, R, E, O) -> (R, E, O, y_norm, objective [4])
    correct(x, codes, B, R, O, E, n_b, dynamic, alpha, threshold, ridge) -> (z_hat, z_norm, lambda_kb)
    Refused                                                       the exception of a refused call; `.outputs`: the NaN-filled outputs it was given

Tolerances are not constants: `bound(f64, ld)` is 16 x the difference between the float64 and the longdouble run of the truth on
that very case (its round-off sensitivity; 16 x covers another summation order over at most 2051 terms), with a floor of 1e-12
of the largest entry.  The measured figures are in profiles/harmony_tolerances.log
(written by tools/harmony_tolerance_log.py from the records of an emulator run and of a GPU run of these tests)."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

SENTINEL = 1e30
MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# the CPU truth
# ---------------------------------------------------------------------------------------------------------------------
def unit_rows(a):
    """rows divided by their Euclidean norm, the norm held at 1e-12 from below"""
    t = a.dtype.type
    nrm = np.sqrt((a * a).sum(axis=1, keepdims=True))
    return a / np.maximum(nrm, t(1e-12))


def n_blocks_of(n: int, block_proportion: float) -> int:
    return int(min(n, 1 // block_proportion))


def default_clusters(n: int) -> int:
    return max(2, int(min(100, n / 30)))


def batch_codes(columns):
    """columns: list of 1-d label arrays (pandas Categorical or anything `astype('category')` takes) -> (codes int32 [n, c] with
    the levels of variable j shifted behind those of the earlier ones, levels int32 [c])"""
    import pandas as pd

    if not columns:
        raise ValueError("batch_key must contain at least one column name")
    out, levels, offset = [], [], 0
    for name, col in columns:
        cat = pd.Series(col).astype("category").cat
        local = cat.codes.to_numpy(dtype=np.int32)
        if (local < 0).any():
            raise ValueError(f"Batch variable {name!r} contains missing values")
        out.append(local + offset)
        levels.append(cat.categories.size)
        offset += cat.categories.size
    return np.stack(out, axis=1).astype(np.int32), np.array(levels, np.int32)


def theta_row(theta, levels, dtype=np.float64):
    """scalar / one value per variable / one value per level -> [total levels]"""
    levels = np.asarray(levels, np.int64)
    try:
        t = np.asarray(theta, dtype=dtype)
    except (TypeError, ValueError) as e:
        raise ValueError(f"theta must be a scalar or an array-like collection of numeric values, got {type(theta).__name__}") from e
    total = int(levels.sum())
    if t.ndim == 0:
        return np.full(total, t.item(), dtype=dtype)
    t = t.ravel()
    if t.size == levels.size:
        return np.repeat(t, levels)
    if t.size != total:
        raise ValueError(f"theta array size ({t.size}) must match the number of batch variables ({levels.size}) or categorical "
                         f"levels ({total})")
    return t


def tau_discount(theta, n_b, n_clusters: int, tau):
    if tau <= 0:
        return theta
    return theta * (1 - np.exp(-n_b / (n_clusters * tau)) ** 2)


def objective_terms(y_norm, z_norm, r, theta, sigma, o, e, stabilized):
    t = z_norm.dtype.type
    sim = z_norm @ y_norm.T
    km = np.sum(r * t(2) * (t(1) - sim))
    rn = r / np.clip(r.sum(axis=1, keepdims=True), t(1e-12), None)
    ent = t(sigma) * np.sum(rn * np.log(rn + t(1e-12)))
    top = o + e + t(1) if stabilized else o + t(1)
    div = t(sigma) * np.sum(theta @ (o * np.log(top / (e + t(1)))))
    return np.array([km + ent + div, km, ent, div], dtype=z_norm.dtype)


def scatter_levels(r, codes, n_levels):
    o = np.zeros((n_levels, r.shape[1]), dtype=r.dtype)
    np.add.at(o, codes, r)
    return o


def init_state(z_norm, codes, n_levels, centroids, pr_b, theta, sigma, stabilized):
    t = z_norm.dtype.type
    y_norm = unit_rows(centroids)
    r = np.exp(t(-2) / t(sigma) * (t(1) - z_norm @ y_norm.T))
    r /= np.maximum(r.sum(axis=1, keepdims=True), t(1e-12))
    e = np.outer(pr_b, r.sum(axis=0))
    o = scatter_levels(r, codes, n_levels)
    return r, e, o, objective_terms(y_norm, z_norm, r, theta, sigma, o, e, stabilized)


def cluster_round(z_norm, codes, perm, n_blocks, pr_b, theta, sigma, stabilized, r, e, o):
    """one clustering iteration, in place on r, e, o -> (y_norm, objective [4])"""
    t = z_norm.dtype.type
    y_norm = unit_rows(r.T @ z_norm)
    n_levels = o.shape[0]
    for cells in np.array_split(perm, n_blocks):
        b = codes[cells]
        old = r[cells]
        o -= scatter_levels(old, b, n_levels)
        e -= np.outer(pr_b, old.sum(axis=0))
        pen = theta[:, None] * (np.log(e + t(1)) - np.log((o + e if stabilized else o) + t(1)))
        logit = t(-2) / t(sigma) * (t(1) - z_norm[cells] @ y_norm.T) + pen[b]
        logit -= logit.max(axis=1, keepdims=True)
        new = np.exp(logit)
        new /= np.maximum(new.sum(axis=1, keepdims=True), t(1e-12))
        r[cells] = new
        o += scatter_levels(new, b, n_levels)
        e += np.outer(pr_b, new.sum(axis=0))
    return y_norm, objective_terms(y_norm, z_norm, r, theta, sigma, o, e, stabilized)


def lambda_table(e, o, n_b, alpha, threshold, ridge_lambda, dynamic):
    t = e.dtype.type
    if not dynamic:
        lam = np.full_like(e, ridge_lambda)
    else:
        lam = t(alpha) * e
        if threshold is not None:
            share = o / np.where(n_b > 0, n_b, 1)[:, None]
            lam[(share < threshold) | (n_b[:, None] == 0)] = t(SENTINEL)
    lam[(o + lam) == 0] = t(SENTINEL)
    return lam


def correct_closed_form(x, codes, n_levels, r, o, lam):
    """the single-variable correction through the arrow-shaped normal equations of every cluster"""
    t = x.dtype.type
    z = x.copy()
    onehot = np.zeros((x.shape[0], n_levels), dtype=x.dtype)
    onehot[np.arange(x.shape[0]), codes] = 1
    for k in range(r.shape[1]):
        phi = (onehot * r[:, k:k + 1]).T @ x  # [levels, d]
        f = t(1) / (o[:, k] + lam[:, k])
        p = -f * o[:, k]
        c = np.sum(o[:, k]) + np.sum(-f * o[:, k] ** 2)
        head = (phi.sum(axis=0) + p @ phi) / c
        w = np.outer(p, head) + f[:, None] * phi
        z -= r[:, k:k + 1] * w[codes]
    return z


def correct_lstsq(x, codes, n_levels, r, lam):
    """the same correction as an explicit weighted ridge regression of every cluster on [1, one-hot level]; a level with the 1e30
    sentinel has no column (the limit of an infinite penalty)"""
    z = x.copy()
    n = x.shape[0]
    for k in range(r.shape[1]):
        active = np.flatnonzero(lam[:, k] < SENTINEL)
        col = {int(b): 1 + j for j, b in enumerate(active)}
        design = np.zeros((n + active.size, 1 + active.size))
        rhs = np.zeros((n + active.size, x.shape[1]))
        sq = np.sqrt(r[:, k])
        design[:n, 0] = sq
        for i in range(n):
            j = col.get(int(codes[i]))
            if j is not None:
                design[i, j] = sq[i]
        rhs[:n] = sq[:, None] * x
        for j, b in enumerate(active):
            design[n + j, 1 + j] = np.sqrt(lam[b, k])
        beta = np.linalg.lstsq(design, rhs, rcond=None)[0]
        w = np.zeros((n_levels, x.shape[1]))
        w[active] = beta[1:]
        z -= r[:, k:k + 1] * w[codes]
    return z


# ---- the device-side generators, restated ---------------------------------------------------------------------------
def _mix64(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def device_permutation(n: int, seed: int, rnd: int) -> np.ndarray:
    """six Feistel rounds on 2h bits (4^h >= n), walked along the cycle until the value is below n"""
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    mask = np.uint64((1 << h) - 1)
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(seed & MASK64) ^ _mix64(np.uint64((rnd + 0x9E3779B97F4A7C15) & MASK64)))
        x = np.arange(n, dtype=np.uint64)
        todo = np.ones(n, bool)
        while todo.any():
            v = x[todo]
            left, right = v >> np.uint64(h), v & mask
            for t in range(6):
                f = (_mix64(key + np.uint64(((t + 1) * 0xD1B54A32D192ED03) & MASK64) + right) >> np.uint64(32)) & mask
                left, right = right, left ^ f
            x[todo] = (left << np.uint64(h)) | right
            todo = x >= np.uint64(n)
    return x.astype(np.int32)


def kmeans_restated(z, n_clusters: int, uniforms, max_iter: int = 25):
    """k-means++ by D^2 sampling (centre 0 = cell floor(u n); centre c = the first cell whose running D^2 sum exceeds u * total),
    then Lloyd: ties to the lowest centre, an empty centre stays, stop after the sweep that changes nothing.
    -> (centroids, labels, sweeps, smallest best-vs-second gap, smallest distance of a draw from a prefix boundary / total)"""
    n = z.shape[0]
    picks = [min(n - 1, int(uniforms[0] * n))]
    margin = np.inf
    mind2 = None
    for c in range(1, n_clusters):
        d2 = ((z - z[picks[-1]]) ** 2).sum(axis=1)
        mind2 = d2 if mind2 is None else np.minimum(mind2, d2)
        run = np.cumsum(mind2)
        if run[-1] > 0:
            target = uniforms[c] * run[-1]
            pick = min(n - 1, int(np.searchsorted(run, target, side="right")))
            margin = min(margin, np.abs(run - target).min() / run[-1])
        else:
            pick = min(n - 1, int(uniforms[c] * n))
        picks.append(pick)
    centres = z[picks].copy()
    labels = np.full(n, -1, np.int32)
    gap, sweeps = np.inf, 0
    while sweeps < max_iter:
        d2 = ((z[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)
        new = d2.argmin(axis=1).astype(np.int32)
        if n_clusters > 1:
            part = np.partition(d2, 1, axis=1)
            gap = min(gap, (part[:, 1] - part[:, 0]).min())
        sweeps += 1
        changed = (new != labels).any()
        labels = new
        if not changed:
            break
        for k in range(n_clusters):
            if (labels == k).any():
                centres[k] = z[labels == k].sum(axis=0) / (labels == k).sum()
    return centres, labels, sweeps, gap, margin


def reference_way_draws(z_norm, n_clusters: int, rng):
    """the reference's own sources of randomness: sklearn KMeans(max_iter=25) centres and a `permutation(n)` per round"""
    from sklearn.cluster import KMeans

    rng = np.random.default_rng(rng)
    km = KMeans(n_clusters=n_clusters, random_state=int(rng.integers(2 ** 31 - 1)), max_iter=25, n_init=1).fit(z_norm)
    return km.cluster_centers_.copy(), (lambda rnd: rng.permutation(z_norm.shape[0]))


def harmony_truth(x, codes, n_levels, centroids, perm_of_round, *, flavor="harmony2", n_clusters=None, max_iter_harmony=10,
                  max_iter_clustering=200, tol_harmony=1e-4, tol_clustering=1e-5, sigma=0.1, theta=2.0, tau=0, ridge_lambda=1.0,
                  alpha=0.2, batch_prune_threshold=1e-5, block_proportion=0.05):
    """the whole algorithm for one batch variable -> (z_hat, dict(rounds=[clustering rounds per outer iteration], objectives,
    decision_margin = how far the closest convergence decision was from flipping, relative to the objective))"""
    n = x.shape[0]
    stab = flavor == "harmony2"
    n_b = np.bincount(codes, minlength=n_levels).astype(x.dtype)
    pr_b = n_b / n
    k = centroids.shape[0] if n_clusters is None else n_clusters
    th = tau_discount(theta_row(theta, [n_levels], x.dtype), n_b, k, tau)
    z_norm = unit_rows(x)
    r, e, o, obj = init_state(z_norm, codes, n_levels, centroids, pr_b, th, sigma, stab)
    objectives, rounds, rnd, margin = [obj[0]], [], 0, np.inf
    nb = n_blocks_of(n, block_proportion)

    def falls_short(before, now, tol):
        """the convergence rule; also keeps the smallest distance of a decision from flipping, relative to |before|"""
        nonlocal margin
        margin = min(margin, float(abs((before - now) - tol * abs(before)) / abs(before)))
        return (before - now) < tol * abs(before)

    for _ in range(max_iter_harmony):
        inner, done = [], None
        for _ in range(max_iter_clustering):
            _, ob = cluster_round(z_norm, codes, np.asarray(perm_of_round(rnd)), nb, pr_b, th, sigma, stab, r, e, o)
            rnd += 1
            inner.append(ob[0])
            if len(inner) >= 4 and falls_short(sum(inner[-4:-1]), sum(inner[-3:]), tol_clustering):
                done = inner[-1]
                break
        rounds.append(len(inner))
        if done is not None:
            objectives.append(done)
        lam = lambda_table(e, o, n_b, alpha, batch_prune_threshold, ridge_lambda, stab)
        z_hat = correct_closed_form(x, codes, n_levels, r, o, lam)
        z_norm = unit_rows(z_hat)
        if len(objectives) >= 2 and falls_short(objectives[-2], objectives[-1], tol_harmony):
            break
    return z_hat, {"rounds": rounds, "objectives": objectives, "decision_margin": margin}


# ---------------------------------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------------------------------
LOG: list = []  # (label, case, quantity, sensitivity, bound, deviation) of every comparison of this process


def record(label, case, quantity, sens, bnd, dev):
    """keeps the figures of one comparison; with SCAMD_HARMONY_RECORDS=FILE in the environment also appends them to FILE, tab-separated
    -- the input of tools/harmony_tolerance_log.py, which writes profiles/harmony_tolerances.log"""
    import os

    LOG.append((label, case, quantity, sens, bnd, dev))
    path = os.environ.get("SCAMD_HARMONY_RECORDS")
    if path:
        with open(path, "a") as f:
            f.write(f"{label}\t{case}\t{quantity}\t{sens:.3e}\t{bnd:.3e}\t{dev:.3e}\n")


def bound(f64, ld):
    """-> (sensitivity, bound): 16 x the float64-vs-longdouble difference of the truth, at least 1e-12 of the largest entry"""
    ld = np.asarray(ld, np.longdouble)
    sens = float(np.abs(np.asarray(f64, np.longdouble) - ld).max())
    return sens, max(16 * sens, 1e-12 * float(np.abs(ld).max()))


def check_close(label, case, quantity, got, f64, ld):
    sens, bnd = bound(f64, ld)
    got, f64 = np.asarray(got), np.asarray(f64)
    assert got.shape == f64.shape, (quantity, got.shape, f64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(f64)), f"{quantity}: NaN pattern differs"
    dev = float(np.nanmax(np.abs(got - f64))) if got.size else 0.0
    record(label, case, quantity, sens, bnd, dev)
    print(f"{label} {case} {quantity}: sensitivity {sens:.3e} bound {bnd:.3e} deviation {dev:.3e}")
    assert dev <= bnd, f"{label} {case} {quantity}: deviation {dev:.3e} exceeds the bound {bnd:.3e} (sensitivity {sens:.3e})"


# ---------------------------------------------------------------------------------------------------------------------
# permutation
# ---------------------------------------------------------------------------------------------------------------------
PERM_SIZES = [1, 2, 3, 63, 64, 65, 1000, 4097]


def run_permutation_case(run, n: int):
    seed = 0x1234ABCD5678EF01
    p = run.permutation(n, seed, 0)
    assert p.dtype == np.int32 and p.shape == (n,)
    assert np.array_equal(np.sort(p), np.arange(n)), "not a bijection"
    assert np.array_equal(p, device_permutation(n, seed, 0))
    assert np.array_equal(p, run.permutation(n, seed, 0)), "two runs differ"
    for rnd in (1, 7):
        assert np.array_equal(run.permutation(n, seed, rnd), device_permutation(n, seed, rnd))
    if n >= 63:
        assert not np.array_equal(p, run.permutation(n, seed, 1)), "rounds share a permutation"
        assert not np.array_equal(p, run.permutation(n, seed + 1, 0)), "seeds share a permutation"
    if n == 4097:
        # 19 blocks: a block of m cells drawn without order has a mean index of (n - 1) / 2 with sigma = n / sqrt(12 m)
        for rnd in range(3):
            for cells in np.array_split(run.permutation(n, seed, rnd), 19):
                s = n / np.sqrt(12 * cells.size)
                assert abs(cells.mean() - (n - 1) / 2) < 5 * s


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def planted(n: int, d: int, n_types: int, n_levels: int, seed: int, *, empty_level: int | None = None, shift: float = 1.0):
    """n cells in d dimensions: n_types blobs, every batch level shifted by about `shift` within-type standard deviations;
    -> (x float64, types, codes int32).  empty_level: a level that gets no cell."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_types, d)) * 4
    types = rng.integers(0, n_types, n)
    usable = [b for b in range(n_levels) if b != empty_level]
    codes = np.array(usable, np.int32)[rng.integers(0, len(usable), n)]
    codes[:len(usable)] = usable  # every usable level has a cell
    offsets = rng.standard_normal((n_levels, d)) * shift
    x = centres[types] + rng.standard_normal((n, d)) + offsets[codes]
    return x, types, codes.astype(np.int32)


# name: n, d, K, levels, block_proportion, flavor, theta, tau, sigma, extras
STATE_CASES = {
    "n12_k1_b1_oneCellBlocks": dict(n=12, d=2, K=1, B=1, bp=0.05, flavor="harmony2", theta=2.0, tau=0, sigma=0.1),
    "n12_k7_b2_h1_theta0": dict(n=12, d=2, K=7, B=2, bp=0.05, flavor="harmony1", theta=0.0, tau=0, sigma=0.1),
    "n157_d50_k7_b2_oneBlock_zeroRow_tau5": dict(n=157, d=50, K=7, B=2, bp=1.0, flavor="harmony2", theta=[0.5, 3.0], tau=5, sigma=0.1,
                                                  zero_row=3),
    "n157_d2_k100_b11_emptyLevel_sigma002": dict(n=157, d=2, K=100, B=11, bp=0.05, flavor="harmony2", theta=2.0, tau=0, sigma=0.02,
                                                  empty_level=4),
    "n157_d128_k256_b2_h1_tau5": dict(n=157, d=128, K=256, B=2, bp=0.05, flavor="harmony1", theta=2.0, tau=5, sigma=0.1),
    "n2051_d50_k100_b11": dict(n=2051, d=50, K=100, B=11, bp=0.05, flavor="harmony2", theta=2.0, tau=0, sigma=0.1),
    "n2051_d128_k256_b11_oneBlock_sigma002": dict(n=2051, d=128, K=256, B=11, bp=1.0, flavor="harmony2",
                                                   theta=list(np.linspace(0.0, 4.0, 11)), tau=0, sigma=0.02),
    "n2051_d2_k7_b1_h1": dict(n=2051, d=2, K=7, B=1, bp=0.05, flavor="harmony1", theta=2.0, tau=0, sigma=0.1),
}
ROUNDS = 3


@lru_cache(maxsize=None)
def state_case(name: str):
    """inputs and the truth of a case in float64 and longdouble, computed once: init, then ROUNDS rounds with the restated device
    permutations; read-only"""
    c = STATE_CASES[name]
    n, d, K, B = c["n"], c["d"], c["K"], c["B"]
    x, _, codes = planted(n, d, min(5, K), B, seed=n + d + K, empty_level=c.get("empty_level"))
    if "zero_row" in c:
        x[c["zero_row"]] = 0.0
    rng = np.random.default_rng(17)
    z64 = unit_rows(x)
    centroids = z64[rng.integers(0, n, K)] + 0.05 * rng.standard_normal((K, d))
    n_b = np.bincount(codes, minlength=B).astype(np.float64)
    theta = tau_discount(theta_row(c["theta"], [B]), n_b, K, c["tau"])
    perms = [device_permutation(n, 99, rnd) for rnd in range(ROUNDS)]
    stab = c["flavor"] == "harmony2"
    out = dict(c, x=x, codes=codes, centroids=centroids, n_b=n_b, pr_b=n_b / n, theta=theta, perms=perms, stab=stab,
               n_blocks=n_blocks_of(n, c["bp"]), z_norm=z64)
    for tag, t in (("f64", np.float64), ("ld", np.longdouble)):
        z = unit_rows(x.astype(t)) if t is np.longdouble else z64
        r, e, o, obj = init_state(z, codes, B, centroids.astype(t), (n_b / n).astype(t), theta.astype(t), c["sigma"], stab)
        steps = [dict(R=r.copy(), E=e.copy(), O=o.copy(), objective=obj)]
        for p in perms:
            y, obj = cluster_round(z, codes, p, out["n_blocks"], (n_b / n).astype(t), theta.astype(t), c["sigma"], stab, r, e, o)
            steps.append(dict(R=r.copy(), E=e.copy(), O=o.copy(), Y=y, objective=obj))
        out[tag] = steps
    return out


def _invariants(label, name, step, r, e, o, pr_b):
    """after init and after every round: O's column sums are R's and E is pr_b x the column sums of R, to 1e-12 of the largest
    column sum / entry (at least of 1)"""
    cols = r.sum(axis=0)
    dev_o = float(np.abs(o.sum(axis=0) - cols).max())
    dev_e = float(np.abs(e - np.outer(pr_b, cols)).max())
    b_o, b_e = 1e-12 * max(1.0, float(np.abs(cols).max())), 1e-12 * max(1.0, float(np.abs(e).max()))
    record(label, name, f"{step} sum O - sum R", float("nan"), b_o, dev_o)
    record(label, name, f"{step} E - pr_b sum R", float("nan"), b_e, dev_e)
    print(f"{label} {name} {step} sum O - sum R: sensitivity - bound {b_o:.3e} deviation {dev_o:.3e}")
    print(f"{label} {name} {step} E - pr_b sum R: sensitivity - bound {b_e:.3e} deviation {dev_e:.3e}")
    assert dev_o <= b_o, f"{name} {step}: column sums of O and R differ by {dev_o:.3e} (bound {b_o:.3e})"
    assert dev_e <= b_e, f"{name} {step}: E differs from pr_b x column sums of R by {dev_e:.3e} (bound {b_e:.3e})"


def run_state_case(run, name: str, label: str):
    c = state_case(name)
    B, sig, stab = c["B"], c["sigma"], c["stab"]
    r, e, o, obj = run.init(c["z_norm"], c["codes"], B, c["centroids"], c["pr_b"], c["theta"], sig, stab)
    r2, e2, o2, obj2 = run.init(c["z_norm"], c["codes"], B, c["centroids"], c["pr_b"], c["theta"], sig, stab)
    assert all(a.tobytes() == b.tobytes() for a, b in ((r, r2), (e, e2), (o, o2), (obj, obj2))), "two runs of init differ"
    for q, got in (("R", r), ("E", e), ("O", o), ("objective", obj)):
        check_close(label, name, f"init {q}", got, c["f64"][0][q], c["ld"][0][q])
    _invariants(label, name, "init", r, e, o, c["pr_b"])
    for rnd, perm in enumerate(c["perms"], start=1):
        before = (r.copy(), e.copy(), o.copy())
        r, e, o, y, obj = run.cluster_round(c["z_norm"], c["codes"], B, perm, c["n_blocks"], c["pr_b"], c["theta"], sig, stab, *before)
        if rnd == 1:
            again = run.cluster_round(c["z_norm"], c["codes"], B, perm, c["n_blocks"], c["pr_b"], c["theta"], sig, stab, *before)
            assert all(a.tobytes() == b.tobytes() for a, b in zip((r, e, o, y, obj), again)), "two runs of a round differ"
        if rnd in (1, ROUNDS):
            for q, got in (("R", r), ("E", e), ("O", o), ("Y", y), ("objective", obj)):
                check_close(label, name, f"round {rnd} {q}", got, c["f64"][rnd][q], c["ld"][rnd][q])
        _invariants(label, name, f"round {rnd}", r, e, o, c["pr_b"])
        assert np.abs(r.sum(axis=1) - 1).max() <= 1e-12, "rows of R do not sum to 1"


# ---------------------------------------------------------------------------------------------------------------------
# correction
# ---------------------------------------------------------------------------------------------------------------------
# name -> (state case, dynamic, alpha, threshold, ridge, doctor)
CORRECT_CASES = {
    "n12_k1_b1": ("n12_k1_b1_oneCellBlocks", True, 0.2, 1e-5, 1.0, None),
    "n12_k7_b2_h1_ridge05": ("n12_k7_b2_h1_theta0", False, 0.2, 1e-5, 0.5, None),
    "n157_k7_b2_pruned": ("n157_d50_k7_b2_oneBlock_zeroRow_tau5", True, 0.2, 0.05, 1.0, None),
    "n157_k100_b11_emptyLevel": ("n157_d2_k100_b11_emptyLevel_sigma002", True, 0.2, 1e-5, 1.0, None),
    "n157_k7_b2_zeroDenominator": ("n157_d50_k7_b2_oneBlock_zeroRow_tau5", True, 0.2, None, 1.0, "zero"),
    "n157_d128_k256_h1": ("n157_d128_k256_b2_h1_tau5", False, 0.2, 1e-5, 1.0, None),
    "n2051_d50_k100_b11": ("n2051_d50_k100_b11", True, 0.2, 1e-5, 1.0, None),
    "n2051_d128_k256_b11": ("n2051_d128_k256_b11_oneBlock_sigma002", True, 0.2, 1e-3, 1.0, None),
}


@lru_cache(maxsize=None)
def correct_case(name: str):
    sname, dynamic, alpha, threshold, ridge, doctor = CORRECT_CASES[name]
    c = state_case(sname)
    B, codes, x = c["B"], c["codes"], c["x"]
    st = c["f64"][1]
    r, o, e = st["R"].copy(), st["O"].copy(), st["E"].copy()
    if doctor == "zero":
        # level 1 has nothing in cluster 2 and expects nothing there: O + alpha E == 0 exactly
        r[codes == 1, 2] = 0.0
        o[1, 2] = 0.0
        e[1, 2] = 0.0
    out = dict(state=c, R=r, O=o, E=e, dynamic=dynamic, alpha=alpha, threshold=threshold, ridge=ridge)
    for tag, t in (("f64", np.float64), ("ld", np.longdouble)):
        lam = lambda_table(e.astype(t), o.astype(t), c["n_b"].astype(t), alpha, threshold, ridge, dynamic)
        out[tag] = dict(lam=lam, z_hat=correct_closed_form(x.astype(t), codes, B, r.astype(t), o.astype(t), lam))
    out["lstsq"] = correct_lstsq(x, codes, B, r, out["f64"]["lam"])
    return out


def run_correct_case(run, name: str, label: str):
    k = correct_case(name)
    c = k["state"]
    args = (c["x"], c["codes"], c["B"], k["R"], k["O"], k["E"], c["n_b"], k["dynamic"], k["alpha"], k["threshold"], k["ridge"])
    z_hat, z_norm, lam = run.correct(*args)
    again = run.correct(*args)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((z_hat, z_norm, lam), again)), "two runs differ"
    assert np.array_equal(lam, k["f64"]["lam"]), "lambda_kb differs from the truth"
    if name.endswith("zeroDenominator"):
        assert lam[1, 2] == SENTINEL and k["O"][1, 2] + k["alpha"] * k["E"][1, 2] == 0.0
    if name.endswith("pruned"):
        assert (lam == SENTINEL).any() and (lam < SENTINEL).any()
    if name.endswith("emptyLevel"):
        assert np.all(lam[4] == SENTINEL) and c["n_b"][4] == 0
    check_close(label, name, "z_hat", z_hat, k["f64"]["z_hat"], k["ld"]["z_hat"])
    check_close(label, name, "z_norm", z_norm, unit_rows(k["f64"]["z_hat"]), unit_rows(k["ld"]["z_hat"]))
    # against the explicit ridge regression, at the bound of the closed form itself (that the regression agrees with the truth
    # inside the same bound is asserted without a device in tests/test_harmony_front_cpu.py)
    sens, b_closed = bound(k["f64"]["z_hat"], k["ld"]["z_hat"])
    dev = float(np.abs(z_hat - k["lstsq"]).max())
    print(f"{label} {name} z_hat vs lstsq: sensitivity {sens:.3e} bound {b_closed:.3e} deviation {dev:.3e}")
    record(label, name, "z_hat vs lstsq", sens, b_closed, dev)
    assert dev <= b_closed, f"{label} {name}: z_hat differs from the ridge regression by {dev:.3e} (bound {b_closed:.3e})"


# ---------------------------------------------------------------------------------------------------------------------
# k-means
# ---------------------------------------------------------------------------------------------------------------------
KMEANS_CASES = [(157, 2, 1), (157, 2, 2), (157, 50, 7), (2051, 2, 7), (2051, 50, 2), (2051, 50, 7), ("empties", 2, 4)]
# twelve cells and draws (seeds on cells 2, 6, 8, 4) after which the second Lloyd sweep leaves a centre without a cell; every
# decision is at least 0.07 (distances) / 0.007 of the total (draws) from flipping
EMPTIES_Z = np.array([[7.2, 2.6], [15.0, 0.7], [0.8, 0.3], [1.0, 1.7], [15.1, 2.9], [14.9, 2.1], [4.5, 2.1], [8.0, 0.4], [16.4, 2.5], [1.4, 1.9],
                      [15.1, 1.2], [14.7, 2.5]])
EMPTIES_U = np.array([0.20833333333333334, 0.617503245348334, 0.9893499410377359, 0.9924857839155159])
KMEANS_SEED = {(157, 2, 1): 0, (157, 2, 2): 0, (157, 50, 7): 0, (2051, 2, 7): 0, (2051, 50, 2): 0, (2051, 50, 7): 0}


@lru_cache(maxsize=None)
def kmeans_case(n, d, K):
    if n == "empties":
        return EMPTIES_Z.copy(), EMPTIES_U.copy()
    x, _, _ = planted(n, d, max(K, 2), 1, seed=1000 + n + d + K, shift=0.0)
    z = unit_rows(x)
    for seed in range(KMEANS_SEED[(n, d, K)], 200):
        u = np.random.default_rng(seed).random(K)
        _, _, _, gap, margin = kmeans_restated(z, K, u)
        if gap > 1e-9 and margin > 1e-9:
            return z, u
    raise AssertionError("no seed meets the precondition")


def run_kmeans_case(run, n, d, K, label: str):
    z, u = kmeans_case(n, d, K)
    want_c, want_l, want_it, gap, margin = kmeans_restated(z, K, u)
    # the precondition, on the truth: no decision within 1e-9 of flipping
    assert gap > 1e-9 and margin > 1e-9, (gap, margin)
    cen, lab, it = run.kmeans(z, K, u, 25)
    cen2, lab2, it2 = run.kmeans(z, K, u, 25)
    assert cen.tobytes() == cen2.tobytes() and lab.tobytes() == lab2.tobytes() and it == it2, "two runs differ"
    print(f"{label} kmeans n={n} d={d} K={K}: {it} sweeps, gap {gap:.2e}, draw margin {margin:.2e}")
    assert np.array_equal(lab, want_l) and it == want_it
    np.testing.assert_allclose(cen, want_c, rtol=1e-9, atol=1e-15)
    if n == "empties":
        assert np.bincount(lab, minlength=K).min() == 0
    if K <= z.shape[0]:
        cen1, lab1, it1 = run.kmeans(z, K, u, 1)
        assert it1 == 1 and lab1.min() >= 0


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
REFUSALS = [("d", dict(d=129), "d=129"), ("K", dict(K=257), "K=257"), ("levels", dict(B=1025), "1025 batch levels"),
            ("covariates", dict(cov=2), "2 batch variables")]


def run_refusal(run, what: str):
    import pytest

    _, over, message = next(r for r in REFUSALS if r[0] == what)
    n, d, K, B, cov = 40, over.get("d", 3), over.get("K", 2), over.get("B", 2), over.get("cov", 1)
    rng = np.random.default_rng(0)
    z = unit_rows(rng.standard_normal((n, d)))
    codes = (np.arange(n) % B).astype(np.int32)
    n_b = np.bincount(codes, minlength=B).astype(np.float64)
    cen = z[:1].repeat(K, axis=0)
    with pytest.raises(run.Refused, match=message) as info:
        run.init(z, codes, B, cen, n_b / n, np.full(B, 2.0), 0.1, True, n_covariates=cov)
    r = info.value.outputs["R"]
    assert np.isnan(r).all(), "a refused call wrote its output"
    state = (np.full((n, K), 1.0 / K), np.zeros((B, K)), np.zeros((B, K)))
    with pytest.raises(run.Refused, match=message):
        run.cluster_round(z, codes, B, np.arange(n, dtype=np.int32), 2, n_b / n, np.full(B, 2.0), 0.1, True, *state, n_covariates=cov)
    with pytest.raises(run.Refused, match=message) as info:
        run.correct(z, codes, B, *state, n_b, True, 0.2, 1e-5, 1.0, n_covariates=cov)
    assert np.isnan(info.value.outputs["z_hat"]).all(), "a refused call wrote its output"
    if what in ("d", "K"):
        with pytest.raises(run.Refused, match=message):
            run.kmeans(z, K, np.full(K, 0.5), 25)


# ---------------------------------------------------------------------------------------------------------------------
# the planted pipeline input (tests/test_gpu_harmony_pipeline.py, precondition in tests/test_harmony_front_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def pipeline_input():
    """n = 3000, d = 20, 3 cell types x 2 batches, the batches about one within-type standard deviation apart"""
    x, types, codes = planted(3000, 20, 3, 2, seed=5, shift=1.0 / np.sqrt(2))
    for a in (x, types, codes):
        a.setflags(write=False)
    return x, types, codes


def acceptance(a, b):
    """the reference's own measure of agreement of two corrected embeddings -> (smallest per-column Pearson r, relative L2)"""
    rs = [np.corrcoef(a[:, j], b[:, j])[0, 1] for j in range(a.shape[1])]
    return float(min(rs)), float(np.linalg.norm(a - b) / np.linalg.norm(b))


def other_batch_share(x, codes, k: int = 15):
    from sklearn.neighbors import NearestNeighbors

    idx = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(x).kneighbors(x, return_distance=False)[:, 1:]
    return float((codes[idx] != codes[:, None]).mean())


def type_ari(x, types):
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score

    return float(adjusted_rand_score(types, KMeans(n_clusters=3, random_state=0, n_init=10).fit_predict(x)))
