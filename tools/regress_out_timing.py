"""The probe behind profiles/regress_out_timing.log: pp.regress_out on two shapes.
    python tools/regress_out_timing.py bench [N_OBS]   the bench shape (bench.py's generator: N_OBS x 2000 at 5 %, default 1 000 000)
    python tools/regress_out_timing.py raw [N_OBS]     the raw-count shape of tools/qc_timing.py: N_OBS x 30 000 genes (default
                                                       200 000), about 2000 counts per cell; kernels only (the dense result has
                                                       N_OBS * 30 000 elements)
Per shape, with two numeric keys (m = 3 table rows) and with one 64-level categorical key (device events, 2 warm-ups, median of 5,
the sides of a comparison alternating in one process, two rounds):
  1. the sums sweep (scamd_pp_regress_sums_f32: range sweep + fixed-point sweep + two small kernels);
  2. the residual kernel (scamd_pp_regress_resid_f32) for float32 and float64 output, its achieved share of the measured 6.29 TB/s for
     the bytes it WRITES, beside the yardstick: scamd_pp_scale_dense_f32 on the same matrix and output type, which writes the same
     bytes.  The margin of the ratio is the run-to-run spread of the yardstick's own repeats (max / min over both rounds);
  3. sc.pp.regress_out host to host (upload, both passes, download of the dense result), bench shape only."""
import sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
import pandas as pd
from scipy import sparse

HBM_MEASURED = 6.29e12  # bytes/s, SURVEY.md 8(d)
def say(*a):
    print(*a, flush=True)


shape = sys.argv[1]
import torch
import scanpy_amd as sc
from scanpy_amd import _kernels as K
from scanpy_amd.preprocessing import _csr_device, _regress_out

t0 = time.perf_counter()
if shape == "bench":
    import bench
    n_obs = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    out = bench.make_matrix(n_obs, 2000, 0, "planted")
    x = sparse.csr_matrix(out[0] if isinstance(out, tuple) else out).astype(np.float32)
else:
    n_obs = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    rng0 = np.random.default_rng(0)
    g0, per_cell = 30_000, 2000
    ln = np.clip(rng0.poisson(per_cell, n_obs), 0, g0).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    indices = np.empty(indptr[-1], dtype=np.int32)
    strides = np.array([s for s in range(1, 2000) if np.gcd(s, g0) == 1], dtype=np.int64)
    for r0 in range(0, n_obs, 20_000):   # the columns of a row: an arithmetic progression mod g with a stride coprime to g, sorted
        r1 = min(r0 + 20_000, n_obs)
        width = int(ln[r0:r1].max())
        start, stride = rng0.integers(0, g0, r1 - r0), rng0.choice(strides, r1 - r0)
        c = (start[:, None] + np.arange(width)[None, :] * stride[:, None]) % g0
        c[np.arange(width)[None, :] >= ln[r0:r1, None]] = g0
        c.sort(axis=1)
        indices[indptr[r0]:indptr[r1]] = c[c < g0]
    data = rng0.geometric(0.45, len(indices)).astype(np.float32)
    x = sparse.csr_matrix((data, indices, indptr), shape=(n_obs, g0))
n, g = x.shape
say(f"{shape}: {n} x {g}, nnz {x.nnz} ({x.nnz / n:.0f} per cell), values {x.data.min():.3g}..{x.data.max():.3g}; generated in "
    f"{time.perf_counter() - t0:.1f} s")

be = _csr_device.GpuPPBackend()
m = be.upload(x)
dev = be.device
rng = np.random.default_rng(1)
n_counts = np.asarray(x.sum(axis=1)).ravel().astype(np.float64)
percent = rng.random(n)
labels = rng.integers(0, 64, n).astype(np.int32)
w_host = np.ascontiguousarray(np.concatenate([np.ones((n, 1)), _regress_out._numeric_basis(np.c_[n_counts, percent])], axis=1))
w = torch.from_numpy(w_host).to(dev)
wb_num = torch.from_numpy(np.abs(w_host).sum(axis=0) * (1 + 1e-6)).to(dev)
codes = torch.from_numpy(labels).to(dev)
wb_cat = torch.from_numpy(np.bincount(labels, minlength=64).astype(np.float64)).to(dev)
keep = torch.ones(g, dtype=torch.uint8, device=dev)


def timed(fn, reps=5, warm=2):
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize()
        del r
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


s_num = K.pp_regress_sums(m.indptr, m.indices, m.data, n, g, w=w, m=w.shape[1], wbound=wb_num)[0]
t_num = s_num.clone(); t_num[0] /= n
s_cat = K.pp_regress_sums(m.indptr, m.indices, m.data, n, g, codes=codes, m=64, wbound=wb_cat)[0]
t_cat = s_cat / torch.clamp(wb_cat, min=1.0)[:, None]
mean = (s_num[0] / n).contiguous()
std = torch.ones(g, dtype=torch.float64, device=dev)
again = K.pp_regress_sums(m.indptr, m.indices, m.data, n, g, w=w, m=w.shape[1], wbound=wb_num)[0]
say(f"{shape}: the sums of two calls are bit-identical: {bool(torch.equal(s_num, again))}")
del again

sides = [("sums_num", lambda: K.pp_regress_sums(m.indptr, m.indices, m.data, n, g, w=w, m=w.shape[1], wbound=wb_num)),
         ("sums_cat", lambda: K.pp_regress_sums(m.indptr, m.indices, m.data, n, g, codes=codes, m=64, wbound=wb_cat))]
for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
    sides += [(f"resid_num_{tag}", lambda dt=dt: K.pp_regress_resid(m.indptr, m.indices, m.data, n, g, keep, t_num, w=w, out_dtype=dt)),
              (f"resid_cat_{tag}", lambda dt=dt: K.pp_regress_resid(m.indptr, m.indices, m.data, n, g, keep, t_cat, codes=codes, out_dtype=dt)),
              (f"scale_dense_{tag}", lambda dt=dt: K.pp_scale_dense(m.indptr, m.indices, m.data, n, g, mean, std, out_dtype=dt))]
res = {}
for rnd in range(2):  # the sides alternate
    for name, fn in sides:
        res.setdefault(name, []).append(timed(fn))
        torch.cuda.empty_cache()
med = {k: float(np.median([v[0] for v in vs])) for k, vs in res.items()}
for k, vs in res.items():
    say(f"{shape}: {k}: " + "; ".join(f"median {a:.3f} ms (min {b:.3f}, max {c:.3f})" for a, b, c in vs))
say(f"{shape}: 1. sums sweep: two numeric keys (3 table rows) {med['sums_num']:.3f} ms, one 64-level categorical key {med['sums_cat']:.3f} ms "
    f"({8 * x.nnz / 1e9:.2f} GB of matrix, read twice)")
for tag, size in (("f32", 4), ("f64", 8)):
    written = n * g * size
    base = res[f"scale_dense_{tag}"]
    spread = max(v[2] for v in base) / min(v[1] for v in base)
    for kind in ("num", "cat"):
        t = med[f"resid_{kind}_{tag}"]
        ratio = t / med[f"scale_dense_{tag}"]
        verdict = "faster than" if ratio < 1 / spread else ("SLOWER than" if ratio > spread else "within the spread of")
        say(f"{shape}: 2. residual {kind} {tag}: {t:.3f} ms, {written / 1e9:.2f} GB written = {written / (t * 1e-3) / 1e12:.3f} TB/s = "
            f"{100 * written / (t * 1e-3) / HBM_MEASURED:.1f}% of the measured 6.29 TB/s; scale_dense {tag} {med[f'scale_dense_{tag}']:.3f} ms; "
            f"ratio {ratio:.3f} (yardstick spread max/min {spread:.3f}): {verdict} the yardstick")

if shape == "bench":
    del s_num, s_cat, t_num, t_cat
    torch.cuda.empty_cache()
    for keys in (["n_counts", "percent_mito"], "label"):
        walls = []
        for i in range(2):
            adata = sc.AnnData(x)
            adata.obs["n_counts"], adata.obs["percent_mito"] = n_counts, percent
            adata.obs["label"] = pd.Categorical(labels)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sc.pp.regress_out(adata, keys)
            walls.append(time.perf_counter() - t0)
            dt, nb = adata.X.dtype, adata.X.nbytes
            del adata
        say(f"{shape}: 3. sc.pp.regress_out(keys={keys}) host to host ({dt}, {nb / 1e9:.1f} GB result): "
            + ", ".join(f"{v:.2f} s" for v in walls))
