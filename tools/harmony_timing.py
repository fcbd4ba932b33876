"""The probe behind profiles/harmony_timing.log: pp.harmony_integrate on bench-style planted data (50 PCs, 8 batch levels drawn at
random, every level shifted by half a standard deviation of each PC), defaults otherwise.
    python tools/harmony_timing.py N_OBS gpu [PCS.npz]   total (host to host), per clustering round, per correction, rounds run, and
                                                         the effective bytes/s of a round (device events, 2 warm-ups, median of
                                                         5); PCS.npz: where to keep the input for the host run
    python tools/harmony_timing.py PCS.npz host          the CPU truth of tests/harmony_cases.py drawn the reference's way (sklearn
                                                         KMeans, numpy permutations) on that input, once (no GPU needed)"""
import os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np

HBM_MEASURED = 6.29e12  # bytes/s, SURVEY.md 8(d)
def say(*a):
    print(*a, flush=True)

if sys.argv[2] == "host":
    import harmony_cases as H
    f = np.load(sys.argv[1])
    x, codes = f["x"].astype(np.float64), f["codes"]
    n = x.shape[0]
    t0 = time.perf_counter()
    cen, perms = H.reference_way_draws(H.unit_rows(x), H.default_clusters(n), 0)
    t1 = time.perf_counter()
    z, info = H.harmony_truth(x, codes, 8, cen, perms)
    t2 = time.perf_counter()
    say(f"host n={n}: numpy truth drawn the reference's way on {len(os.sched_getaffinity(0))} cores (numpy / BLAS threads as configured): "
        f"KMeans {t1 - t0:.1f} s, Harmony {t2 - t1:.1f} s, clustering rounds per outer iteration {info['rounds']}")
    raise SystemExit(0)

import torch
import bench
import scanpy_amd as sc
from scanpy_amd import _kernels as K
from scanpy_amd.preprocessing import _harmony

n_obs = int(sys.argv[1])
t0 = time.perf_counter()
out = bench.make_matrix(n_obs, 2000, 0, "planted")
adata = sc.AnnData(out[0] if isinstance(out, tuple) else out)
sc.pp.pca(adata, n_comps=50)
rng = np.random.default_rng(0)
codes = rng.integers(0, 8, n_obs).astype(np.int32)
pcs = adata.obsm["X_pca"].astype(np.float64)
x = pcs + 0.5 * pcs.std(axis=0) * rng.standard_normal((8, 50))[codes]
say(f"n={n_obs}: matrix + pca {time.perf_counter() - t0:.1f} s")
if len(sys.argv) > 3:
    np.savez(sys.argv[3], x=x.astype(np.float32), codes=codes)
    x = x.astype(np.float32).astype(np.float64)

def fit():
    run = _harmony.HarmonyRun()  # the defaults of pp.harmony_integrate
    torch.cuda.synchronize(); t0 = time.perf_counter()
    run.fit(x, codes, 8, np.full(8, 2.0), np.random.default_rng(0))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, run

fit()  # warm-up
wall, run = fit()
say(f"n={n_obs}: harmony_integrate host to host {wall:.3f} s; clustering rounds per outer iteration {run.rounds_} "
    f"({sum(run.rounds_)} rounds, {len(run.rounds_)} corrections), k-means sweeps {run.kmeans_sweeps_}")

# the stages on device-resident state, device events
dev = torch.device("cuda")
n, d, k = n_obs, 50, run.n_clusters_
x_d, codes_d = torch.from_numpy(x).to(dev), torch.from_numpy(codes).to(dev)
n_b = np.bincount(codes, minlength=8).astype(np.float64)
n_b_d, pr_b_d, theta_d = torch.from_numpy(n_b).to(dev), torch.from_numpy(n_b / n).to(dev), torch.full((8,), 2.0, dtype=torch.float64, device=dev)
z_norm = K.harmony_normalize(x_d)
def timed(fn, reps=5, warm=2):
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))
uniforms = np.random.default_rng(0).random(k)
say(f"n={n_obs}: k-means initialisation (K={k}) {timed(lambda: K.harmony_kmeans(z_norm, k, uniforms), reps=1, warm=1):.2f} ms")
cen, _, _ = K.harmony_kmeans(z_norm, k, uniforms)
r, e, o, obj = K.harmony_init(z_norm, codes_d, 8, cen, pr_b_d, theta_d, 0.1, True)
y = torch.empty((k, d), dtype=torch.float64, device=dev)
perm = K.harmony_permutation(n, 1, 0)
say(f"n={n_obs}: permutation {timed(lambda: K.harmony_permutation(n, 1, 0)):.3f} ms")
round_ms = timed(lambda: K.harmony_cluster_round_(z_norm, codes_d, 8, perm, run.n_blocks_, pr_b_d, theta_d, 0.1, True, r, e, o, y, obj))
# bytes a round has to move: the centroids read R and z once, every block reads its old rows of R, then reads z and writes R
round_bytes = n * (3 * k + 2 * d) * 8
say(f"n={n_obs}: one clustering round ({run.n_blocks_} blocks) {round_ms:.3f} ms device time; {round_bytes / 1e6:.0f} MB of compulsory traffic -> "
    f"{round_bytes / (round_ms * 1e-3) / 1e12:.3f} TB/s = {100 * round_bytes / (round_ms * 1e-3) / HBM_MEASURED:.1f}% of the measured 6.29 TB/s")
t0 = time.perf_counter()
K.harmony_cluster_round_(z_norm, codes_d, 8, perm, run.n_blocks_, pr_b_d, theta_d, 0.1, True, r, e, o, y, obj); float(obj[0].item())
host_ms = (time.perf_counter() - t0) * 1e3
say(f"n={n_obs}: the same round with its objective read-back, host clock {host_ms:.3f} ms"
    + (" -- the host-side loop costs more than the device time of the round: moving the inner loop into one C entry is the follow-up" if host_ms > 2 * round_ms else ""))
corr_ms = timed(lambda: K.harmony_correct(x_d, codes_d, 8, r, o, e, n_b_d, dynamic_lambda=True, alpha=0.2, batch_prune_threshold=1e-5, ridge_lambda=1.0))
say(f"n={n_obs}: one correction {corr_ms:.3f} ms device time")
