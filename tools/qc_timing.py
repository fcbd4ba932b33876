"""The probe behind profiles/qc_timing.log: pp.calculate_qc_metrics on two shapes.
    python tools/qc_timing.py bench [N_OBS]   the bench shape (bench.py's generator: N_OBS x 2000 at 5 %, default 1 000 000)
    python tools/qc_timing.py raw [N_OBS]     a raw-count shape generated here (seed 0): N_OBS x 30 000 genes (default 200 000),
                                              about 2000 Poisson-like integer entries per cell
Per shape (device events, 2 warm-ups, median of 5, the two sides of a comparison alternating in one process):
  1. the fused sweep without percent_top, beside scamd_pp_row_sums_f32 + scamd_pp_col_stats_f32 on the same matrix (the kernels
     calculate_qc_metrics would otherwise be assembled from; they read the matrix twice);
  2. the top-n pass with the default percent_top, and its achieved bytes/s over 8 * nnz against the measured HBM rate;
  3. sc.pp.calculate_qc_metrics host to host (upload included), and the numpy restatement of tests/qc_cases.py on the first rows of
     the same matrix, at the largest size it finishes in a minute."""
import os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "emu"))
import numpy as np
from scipy import sparse

HBM_MEASURED = 6.29e12  # bytes/s, SURVEY.md 8(d)
PERCENT_TOP = (50, 100, 200, 500)
def say(*a):
    print(*a, flush=True)


def raw_counts(n: int, g: int = 30_000, per_cell: int = 2000, seed: int = 0) -> sparse.csr_matrix:
    """row lengths Poisson(per_cell); the columns of a row are an arithmetic progression mod g with a stride coprime to g (distinct),
    sorted; values geometric: mostly 1 and 2, one in fifty with a tail into the hundreds"""
    rng = np.random.default_rng(seed)
    ln = np.clip(rng.poisson(per_cell, n), 0, g).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    indices = np.empty(indptr[-1], dtype=np.int32)
    data = np.empty(indptr[-1], dtype=np.float32)
    strides = np.array([s for s in range(1, 2000) if np.gcd(s, g) == 1], dtype=np.int64)
    for r0 in range(0, n, 20_000):
        r1 = min(r0 + 20_000, n)
        width = int(ln[r0:r1].max())
        start, stride = rng.integers(0, g, r1 - r0), rng.choice(strides, r1 - r0)
        c = (start[:, None] + np.arange(width)[None, :] * stride[:, None]) % g
        c[np.arange(width)[None, :] >= ln[r0:r1, None]] = g
        c.sort(axis=1)
        indices[indptr[r0]:indptr[r1]] = c[c < g]
        k = int(indptr[r1] - indptr[r0])
        data[indptr[r0]:indptr[r1]] = rng.geometric(0.45, k) + (rng.random(k) < 0.02) * rng.geometric(0.01, k)
    return sparse.csr_matrix((data, indices, indptr), shape=(n, g))


shape = sys.argv[1]
import torch
import scanpy_amd as sc
from scanpy_amd import _kernels as K
from scanpy_amd.preprocessing import _csr_device

t0 = time.perf_counter()
if shape == "bench":
    import bench
    n_obs = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    out = bench.make_matrix(n_obs, 2000, 0, "planted")
    x = sparse.csr_matrix(out[0] if isinstance(out, tuple) else out).astype(np.float32)
else:
    n_obs = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    x = raw_counts(n_obs)
n, g = x.shape
d = x.data
say(f"{shape}: {n} x {g}, nnz {x.nnz} ({x.nnz / n:.0f} per cell), values {d.min():.0f}..{d.max():.0f}, integer-valued "
    f"{bool((d == np.rint(d)).all())}; generated in {time.perf_counter() - t0:.1f} s")

be = _csr_device.GpuPPBackend()
m = be.upload(x)
rng = np.random.default_rng(1)
mt = rng.random(g) < 0.001


def timed(fn, reps=5, warm=2):
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


bits = torch.from_numpy(mt.astype(np.int32)).to(be.device)
sweep = lambda: K.pp_qc_sweep(m.indptr, m.indices, m.data, n, g)
sweep_mt = lambda: K.pp_qc_sweep(m.indptr, m.indices, m.data, n, g, gene_mask=bits, n_masks=1)
rows_only = lambda: K.pp_qc_sweep(m.indptr, m.indices, m.data, n, g, per_gene=False)
parent_rows = lambda: K.pp_row_sums(m.indptr, m.indices, m.data, n)
parent_cols = lambda: K.pp_col_stats(m.indptr, m.indices, m.data, n, g, count_positive=True)
res = {}
for rnd in range(2):  # the sides alternate
    for name, fn in (("sweep", sweep), ("row_sums", parent_rows), ("col_stats", parent_cols), ("sweep_mt", sweep_mt), ("rows_only", rows_only)):
        res.setdefault(name, []).append(timed(fn))
med = {k: float(np.median([v[0] for v in vs])) for k, vs in res.items()}
for k, vs in res.items():
    say(f"{shape}: {k}: " + "; ".join(f"median {a:.3f} ms (min {b:.3f}, max {c:.3f})" for a, b, c in vs))
bytes_sweep = 8 * x.nnz
say(f"{shape}: 1. fused sweep {med['sweep']:.3f} ms ({bytes_sweep / (med['sweep'] * 1e-3) / 1e12:.3f} TB/s over 8 B/entry) against "
    f"row_sums {med['row_sums']:.3f} + col_stats {med['col_stats']:.3f} = {med['row_sums'] + med['col_stats']:.3f} ms: "
    f"{'within' if med['sweep'] <= med['row_sums'] + med['col_stats'] else 'EXCEEDS'} their sum; with one qc_var mask "
    f"{med['sweep_mt']:.3f} ms; per-row outputs alone (4 B/entry) {med['rows_only']:.3f} ms")
top_ms = timed(lambda: K.pp_qc_top(m.indptr, m.data, n, PERCENT_TOP))
say(f"{shape}: 2. top-n pass, percent_top {PERCENT_TOP}: median {top_ms[0]:.3f} ms (min {top_ms[1]:.3f}, max {top_ms[2]:.3f}); "
    f"{bytes_sweep / (top_ms[0] * 1e-3) / 1e12:.3f} TB/s over 8 * nnz = {100 * bytes_sweep / (top_ms[0] * 1e-3) / HBM_MEASURED:.1f}% of the "
    f"measured 6.29 TB/s")

adata = sc.AnnData(x)
adata.var["mt"] = mt
walls = []
for i in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    obs, var = sc.pp.calculate_qc_metrics(adata, qc_vars=["mt"])
    walls.append(time.perf_counter() - t0)
say(f"{shape}: 3. sc.pp.calculate_qc_metrics(qc_vars=['mt']) host to host: first call {walls[0]:.3f} s, then {walls[1]:.3f} s and {walls[2]:.3f} s")

import qc_cases as Q
os.environ.setdefault("OMP_NUM_THREADS", "16")
last, spent = None, 0.0
for rows in (n // 1000, n // 100, n // 10, n):
    if rows < 1:
        continue
    if last is not None and last[1] * rows / last[0] > 60.0:
        break
    sub = x[:rows]
    t0 = time.perf_counter()
    prim = Q.ref_primitives(sub, mt[None, :], PERCENT_TOP)
    want_obs, want_var = Q.ref_columns(prim, sub.dtype, rows, qc_vars=["mt"], percent_top=PERCENT_TOP)
    last = (rows, time.perf_counter() - t0)
    same = all(np.array_equal(obs[c].to_numpy()[:rows], v, equal_nan=True) for c, v in want_obs.items())
    say(f"{shape}:    numpy restatement on the first {rows} cells: {last[1]:.2f} s ({len(os.sched_getaffinity(0))} cores available); "
        f"its obs columns equal the device's: {same}")
say(f"{shape}:    largest restatement within a minute: {last[0]} cells in {last[1]:.2f} s -> {last[1] * n / last[0]:.1f} s extrapolated to {n} cells "
    f"against {walls[-1]:.3f} s")
