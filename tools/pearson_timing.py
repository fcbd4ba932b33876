"""The probe behind profiles/pearson_residuals_timing.log: the two kernels of csrc/pearson.hip and the calls of experimental.pp.
    python tools/pearson_timing.py bench [N_OBS]   the bench shape (bench.py's generator: N_OBS x 2000 at 5 %, default 1 000 000)
    python tools/pearson_timing.py raw [N_OBS]     the raw-count shape of tools/qc_timing.py: N_OBS x 30 000 genes (default
                                                   200 000), about 2000 counts per cell
Per shape (device events, 2 warm-ups, median of 5, the sides of a comparison alternating in one process, two rounds):
  1. the residual matrix (scamd_pp_pearson_residuals_f32) for float32 and float64 output, its achieved share of the measured
     6.29 TB/s for the bytes it WRITES, beside the yardstick: scamd_pp_scale_dense_f32 on the same matrix and output type, which
     writes the same bytes.  The margin of a ratio is the run-to-run spread of the yardstick's own repeats (max / min);
  2. the gene variance (scamd_pp_pearson_gene_var_f32, the transpose not included) with the distinct totals of the matrix and
     with U = n and all multiplicities 1 (its own yardstick: what the collapse buys);
  3. host to host: experimental.pp.highly_variable_genes, and on the bench shape normalize_pearson_residuals, beside the numpy
     restatement on the host (timed on a slab of genes / rows and scaled: the whole thing does not fit the patience of a probe)."""
import sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
from scipy import sparse

HBM_MEASURED = 6.29e12  # bytes/s, SURVEY.md 8(d)
def say(*a):
    print(*a, flush=True)


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
integer = bool(np.all(x.data == np.floor(x.data)))
say(f"{shape}: {n} x {g}, nnz {x.nnz} ({x.nnz / n:.0f} per cell), values {x.data.min():.3g}..{x.data.max():.3g}, integers: {integer}; "
    f"generated in {time.perf_counter() - t0:.1f} s")

be = _csr_device.GpuPPBackend()
m = be.upload(x)
dev = be.device
theta, clip = 100.0, float(np.sqrt(n))


def timed(fn, reps=5, warm=2):
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize()
        del r
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


cell_total = K.csr_row_stats(m.indptr, m.data, n)[0]
gene_sum = K.pp_col_stats(m.indptr, m.indices, m.data, n, g, count_positive=False)[0]
total = float(gene_sum.sum())
tot_u, mult_u = torch.unique(cell_total, sorted=True, return_counts=True)
mult_u = mult_u.to(torch.float64)
ones = torch.ones(n, dtype=torch.float64, device=dev)
say(f"{shape}: {tot_u.numel()} distinct cell totals among {n} cells (U / n = {tot_u.numel() / n:.4f})")
mean = (gene_sum / n).contiguous()
std = torch.ones(g, dtype=torch.float64, device=dev)

# ---- 1. the residual matrix against scale_dense
sides = []
for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
    sides += [(f"pearson_{tag}", lambda dt=dt: K.pp_pearson_residuals(m.indptr, m.indices, m.data, n, g, gene_sum, cell_total, total,
                                                                     1.0 / theta, clip, out_dtype=dt)),
              (f"scale_dense_{tag}", lambda dt=dt: K.pp_scale_dense(m.indptr, m.indices, m.data, n, g, mean, std, out_dtype=dt))]
res = {}
for rnd in range(2):  # the sides alternate
    for name, fn in sides:
        res.setdefault(name, []).append(timed(fn))
        torch.cuda.empty_cache()
med = {k: float(np.median([v[0] for v in vs])) for k, vs in res.items()}
for k, vs in res.items():
    say(f"{shape}: {k}: " + "; ".join(f"median {a:.3f} ms (min {b:.3f}, max {c:.3f})" for a, b, c in vs))
for tag, size in (("f32", 4), ("f64", 8)):
    written = n * g * size
    base = res[f"scale_dense_{tag}"]
    spread = max(v[2] for v in base) / min(v[1] for v in base)
    own = res[f"pearson_{tag}"]
    t = med[f"pearson_{tag}"]
    ratio = t / med[f"scale_dense_{tag}"]
    verdict = "faster than" if ratio < 1 / spread else ("SLOWER than" if ratio > spread else "within the spread of")
    say(f"{shape}: 1. residual matrix {tag}: {t:.3f} ms (own spread max/min {max(v[2] for v in own) / min(v[1] for v in own):.3f}), "
        f"{written / 1e9:.2f} GB written = {written / (t * 1e-3) / 1e12:.3f} TB/s = {100 * written / (t * 1e-3) / HBM_MEASURED:.1f}% of the "
        f"measured 6.29 TB/s; scale_dense {tag} {med[f'scale_dense_{tag}']:.3f} ms; ratio {ratio:.3f} (yardstick spread max/min "
        f"{spread:.3f}): {verdict} the yardstick")
a = K.pp_pearson_residuals(m.indptr, m.indices, m.data, n, g, gene_sum, cell_total, total, 1.0 / theta, clip, out_dtype=torch.float32)
b = K.pp_pearson_residuals(m.indptr, m.indices, m.data, n, g, gene_sum, cell_total, total, 1.0 / theta, clip, out_dtype=torch.float32)
say(f"{shape}: the residual matrices of two calls are bit-identical: {bool(torch.equal(a, b))}")
del a, b
torch.cuda.empty_cache()

# ---- 2. the gene variance: collapsed totals against the plain sweep
def gene_var_section(label, mm):
    """mm: a resident matrix; its own sums, totals and transpose"""
    ct = K.csr_row_stats(mm.indptr, mm.data, n)[0]
    gs = K.pp_col_stats(mm.indptr, mm.indices, mm.data, n, g, count_positive=False)[0]
    tot = float(gs.sum())
    tu, mu_ = torch.unique(ct, sorted=True, return_counts=True)
    mu_ = mu_.to(torch.float64)
    ta = timed(lambda: K.csr_transpose(mm.indptr, mm.indices, mm.data, n, g))
    t_indptr, t_rows, t_data = K.csr_transpose(mm.indptr, mm.indices, mm.data, n, g)
    say(f"{shape}: {label}: csr_transpose (made once per matrix): median {ta[0]:.3f} ms")
    var_sides = [("collapsed", lambda: K.pp_pearson_gene_var(t_indptr, t_rows, t_data, n, g, gs, ct, tot, 1.0 / theta, clip, tu, mu_, n)),
                 ("plain", lambda: K.pp_pearson_gene_var(t_indptr, t_rows, t_data, n, g, gs, ct, tot, 1.0 / theta, clip, ct, ones, n))]
    vres = {}
    for rnd in range(2):
        for name, fn in var_sides:
            vres.setdefault(name, []).append(timed(fn, reps=5 if name == "collapsed" else 3, warm=1))
    for k, vs in vres.items():
        say(f"{shape}: {label}: gene_var {k}: " + "; ".join(f"median {a:.3f} ms (min {b:.3f}, max {c:.3f})" for a, b, c in vs))
    tc, tp = (float(np.median([v[0] for v in vres[k]])) for k in ("collapsed", "plain"))
    spread = max(v[2] for v in vres["plain"]) / min(v[1] for v in vres["plain"])
    say(f"{shape}: 2. gene variance, {label}: U = {tu.numel()}: {tc:.3f} ms; U = n = {n}, multiplicities 1: {tp:.3f} ms; the collapse buys a "
        f"factor {tp / tc:.2f} (spread of the plain sweep max/min {spread:.3f}); {n * g / (tc * 1e-3) / 1e12:.2f} T (cell, gene) pairs per second")
    v1 = var_sides[0][1](); v2 = var_sides[0][1](); v3 = var_sides[1][1]()
    say(f"{shape}: {label}: two calls bit-identical: {bool(torch.equal(v1, v2))}; collapsed against plain: max relative difference "
        f"{float(((v1 - v3).abs() / v3.abs().clamp(min=1e-300)).max()):.2e}")


gene_var_section("the values as they are", m)
torch.cuda.empty_cache()
if not integer:   # the bench generator makes normalised values: the same pattern with every value rounded up is count data
    xc = x.copy()
    xc.data = np.ceil(xc.data)
    mc = be.upload(xc)
    gene_var_section("every value rounded up to an integer (totals as count data gives them)", mc)
    del mc, xc
    torch.cuda.empty_cache()

# ---- 3. host to host
walls = []
for i in range(2):
    adata = sc.AnnData(x)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    df = sc.experimental.pp.highly_variable_genes(adata, n_top_genes=2000 if g > 2000 else 500, inplace=False, check_values=i == 0)
    walls.append(time.perf_counter() - t0)
say(f"{shape}: 3. experimental.pp.highly_variable_genes host to host (upload, sums, transpose, variance, ranking): "
    + ", ".join(f"{v:.2f} s" for v in walls) + " (the first with check_values)")
slab = 64
xs = x[:, :slab].toarray().astype(np.float64)
x64 = x.astype(np.float64)   # (scipy adds a float32 matrix in float32: the restatement takes its sums in float64)
tt = np.asarray(x64.sum(axis=1)).ravel()
ss = np.asarray(x64.sum(axis=0)).ravel()
del x64
t0 = time.perf_counter()
mu = np.outer(tt, ss[:slab]) / ss.sum()
r = np.clip((xs - mu) / np.sqrt(mu + mu ** 2 / theta), -clip, clip)
ref = r.var(axis=0)
dt_ref = time.perf_counter() - t0
live = ss[:slab] != 0
err = np.abs(df["residual_variances"].to_numpy()[:slab][live] - ref[live]) / ref[live]
say(f"{shape}: 3. the numpy restatement of the variance on {slab} genes: {dt_ref:.2f} s = {dt_ref * g / slab:.1f} s for {g} genes (one host "
    f"thread; numpy's element-wise passes do not use more); largest relative difference to the device on those genes {err.max():.2e}")
del xs, mu, r
if shape == "bench":
    walls = []
    for i in range(2):
        adata = sc.AnnData(x)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        sc.experimental.pp.normalize_pearson_residuals(adata)
        walls.append(time.perf_counter() - t0)
        dt, nb = adata.X.dtype, adata.X.nbytes
        del adata
    say(f"{shape}: 3. experimental.pp.normalize_pearson_residuals host to host ({dt}, {nb / 1e9:.1f} GB result): "
        + ", ".join(f"{v:.2f} s" for v in walls))
    rows = 50_000
    xs = x[:rows].toarray()
    t0 = time.perf_counter()
    s1, t1 = xs.sum(axis=0, keepdims=True), xs.sum(axis=1, keepdims=True)
    mu = t1 @ s1 / s1.sum()
    r = np.clip((xs - mu) / np.sqrt(mu + mu ** 2 / np.float32(theta)), -clip, clip)
    dt_ref = time.perf_counter() - t0
    say(f"{shape}: 3. the numpy restatement of the normalisation on {rows} cells (float32, as the reference): {dt_ref:.2f} s = "
        f"{dt_ref * n / rows:.1f} s for {n} cells")
