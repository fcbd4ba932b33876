"""The probe behind profiles/aggregate_timing.log: the two entry points of csrc/aggregate.hip beside their yardsticks, the whole
`sc.get.aggregate` call host to host, and a CPU baseline.
    python tools/aggregate_timing.py SHAPE      SHAPE: sparse64 (1M x 2000 at 5 %, 64 groups), sparse10k (the same, 10 000 groups),
                                               counts (200k x 30 000 raw counts at 3 %, 64 groups), dense (1M x 50, 64 groups: X_pca,
                                               the median's worst case).  A further argument scales the rows (0.1: a tenth).
The matrix is made on the device: every row stores the same number of entries, one in each stride of columns (a real matrix has
rows of varying length; the split is by entries, so the sweep does not see the difference).  Values: log1p of geometric counts
(sparse64 / sparse10k), the counts themselves (counts), normal (dense).  Group sizes are skewed (a Zipf-like draw).

Per entry point (device events, 2 warm-ups, median of 5, min and max given): the moments without and with m2, the median with
the share of pairs decided from the counts alone; the bytes each sweep of the matrix reads (12 B per stored entry, 12 B per row)
against the 6.29 TB/s copy rate the other logs use.  Yardsticks in the same run, sides alternating, two rounds, the margin being
the yardstick's own max / min: scamd_pp_regress_sums_f32 with codes (for 'sum'), scamd_csr_transpose_f32 +
scamd_rank_genes_group_stats_f32 (for sum + second moment + count, at most 2000 groups and 40 944 genes).  Then the front end host
to host (scipy CSR in, layers out; the host sort of the codes on its own) and the numpy / scipy restatement of sum, count and var
on the host CPUs."""
import sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import pandas as pd
from scipy import sparse

HBM_MEASURED = 6.29e12  # bytes/s, SURVEY.md 8(d)
SHAPES = {"sparse64": (1_000_000, 2000, 100, 64, "log"), "sparse10k": (1_000_000, 2000, 100, 10_000, "log"),
          "counts": (200_000, 30_000, 900, 64, "counts"), "dense": (1_000_000, 50, 50, 64, "normal")}


def say(*a):
    print(*a, flush=True)


shape = sys.argv[1]
scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
n, g, row, n_groups, kind = SHAPES[shape]
n = int(n * scale)
import torch
import scanpy_amd as sc
from scanpy_amd import _kernels as K
from scanpy_amd import _get_aggregate as G

be = G.GpuAggregateBackend()
dev = be.device


def timed(fn, reps=5, warm=2):
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize()
        del r
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


gen = torch.Generator(device=dev).manual_seed(0)
stride = g // row
indices = (torch.arange(row, device=dev, dtype=torch.int32) * stride)[None, :] + \
    torch.randint(0, stride, (n, row), generator=gen, device=dev, dtype=torch.int32)
indices = indices.reshape(-1).contiguous()
indptr = torch.arange(n + 1, device=dev, dtype=torch.int64) * row
if kind == "normal":
    data = torch.randn(n * row, generator=gen, device=dev, dtype=torch.float32)
else:
    u = torch.rand(n * row, generator=gen, device=dev, dtype=torch.float32)
    data = torch.floor(torch.log(1 - u) / np.log(0.6)) + 1          # geometric counts, 1, 2, 3, ...
    if kind == "log":
        data = torch.log1p(data)
nnz = n * row
rng = np.random.default_rng(0)
p = 1.0 / np.arange(1, n_groups + 1) ** 0.7
codes_h = rng.choice(n_groups, n, p=p / p.sum()).astype(np.int32)
codes_h[rng.random(n) < 0.02] = -1
t0 = time.perf_counter()
order_h, sizes_h = G._grouping(codes_h, n_groups)
t_sort = time.perf_counter() - t0
codes, order, sizes = (torch.from_numpy(a).to(dev) for a in (codes_h, order_h, sizes_h))
sweep_bytes = 12 * nnz + 12 * n
say(f"== {shape}: {n} x {g}, {row} entries per row, nnz {nnz}, {n_groups} groups of {sizes_h.min()}-{sizes_h.max()} rows "
    f"({int((codes_h < 0).sum())} rows without a group); parts of {K._lib.load().scamd_aggregate_part_entries(nnz)} entries, "
    f"{K._lib.load().scamd_aggregate_lanes_per_row(n, nnz)} lanes per row, {-(-g // 4096)} gene window(s); "
    f"one sweep reads {sweep_bytes / 1e9:.2f} GB = {sweep_bytes / HBM_MEASURED * 1e3:.3f} ms at the copy rate")
say(f"host: the group-order sort of the codes (numpy stable argsort + bincount) {t_sort * 1e3:.1f} ms")


def agg(**kw):
    return K.aggregate(indptr, indices, data, n, g, codes, order, sizes, **kw)


a1, a2 = agg(want_m2=True, want_median=(g <= 40944)), agg(want_m2=True, want_median=(g <= 40944))
same = all(bool(torch.equal(a1[k], a2[k]) if k != "median" else torch.equal(a1[k].nan_to_num(-1.0), a2[k].nan_to_num(-1.0)))
           for k in a1 if k not in ("flags", "info"))
say(f"two runs give the same bits: {same}; flags {a1['flags']}")
m_sum = timed(lambda: agg())
m_m2 = timed(lambda: agg(want_m2=True))
say(f"moments, sum + counts (range sweep + 1 sweep):  {m_sum[0]:8.3f} ms (min {m_sum[1]:.3f}, max {m_sum[2]:.3f}) = "
    f"{2 * sweep_bytes / m_sum[0] / 1e9:.2f} TB/s of matrix reads = {2 * sweep_bytes / m_sum[0] / 1e9 / 6.29 * 100:.1f} % of the copy rate")
say(f"moments with m2 (range sweep + 3 sweeps):       {m_m2[0]:8.3f} ms (min {m_m2[1]:.3f}, max {m_m2[2]:.3f}) = "
    f"{4 * sweep_bytes / m_m2[0] / 1e9:.2f} TB/s of matrix reads = {4 * sweep_bytes / m_m2[0] / 1e9 / 6.29 * 100:.1f} % of the copy rate")
if g <= 40944:
    m_med = timed(lambda: agg(want_median=True))
    info = a1["info"]
    say(f"moments + median:                               {m_med[0]:8.3f} ms (min {m_med[1]:.3f}, max {m_med[2]:.3f}); the median alone "
        f"{m_med[0] - m_sum[0]:.3f} ms; of {sum(info)} pairs {info[0]} ({info[0] / max(sum(info), 1) * 100:.2f} %) decided from the counts, "
        f"{info[1]} by a wave, {info[2]} by a workgroup")

# ---- yardsticks, sides alternating, two rounds
wbound = sizes.double().clamp(min=1.0)
sides = [("aggregate moments (sum)", lambda: agg())]
if n_groups <= 65536:
    sides.append(("pp_regress_sums with codes", lambda: K.pp_regress_sums(indptr, indices, data, n, g, codes=codes, m=n_groups, wbound=wbound)))
rounds = {name: [] for name, _ in sides}
for _ in range(2):
    for name, fn in sides:
        rounds[name].append(timed(fn))
for name in rounds:
    say(f"  {name:34s} " + "   ".join(f"{r[0]:8.3f} ms (min {r[1]:.3f}, max {r[2]:.3f})" for r in rounds[name]))
if len(sides) == 2:
    ours, yard = [r[0] for r in rounds[sides[0][0]]], [r[0] for r in rounds[sides[1][0]]]
    say(f"  ratio sum / regress_sums: {np.mean(ours) / np.mean(yard):.3f}; the yardstick's own max / min {max(yard) / min(yard):.3f}")
if n_groups <= 2000 and g <= 40944:
    def yard2():
        t = K.csr_transpose(indptr, indices, data, n, g)
        return K.rank_genes_group_stats(t[0], t[1], t[2], n, g, codes, n_groups)
    sides = [("aggregate moments with m2", lambda: agg(want_m2=True)), ("csr_transpose + group_stats", yard2)]
    rounds = {name: [] for name, _ in sides}
    for _ in range(2):
        for name, fn in sides:
            rounds[name].append(timed(fn))
    for name in rounds:
        say(f"  {name:34s} " + "   ".join(f"{r[0]:8.3f} ms (min {r[1]:.3f}, max {r[2]:.3f})" for r in rounds[name]))
    ours, yard = [r[0] for r in rounds[sides[0][0]]], [r[0] for r in rounds[sides[1][0]]]
    say(f"  ratio (sum, m2, count) / (transpose + group_stats): {np.mean(ours) / np.mean(yard):.3f}; the yardstick's own max / min "
        f"{max(yard) / min(yard):.3f}")

# ---- host to host, and the host restatement
x_host = sparse.csr_matrix((data.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()), shape=(n, g))
labels = pd.Categorical.from_codes(codes_h, [f"g{k}" for k in range(n_groups)])
adata = sc.AnnData(x_host if kind != "normal" else x_host.toarray(), obs=pd.DataFrame({"grp": labels}, index=pd.RangeIndex(n).astype(str)))
for funcs in [["sum"], ["sum", "mean", "var", "count_nonzero"]] + ([["median"]] if g <= 40944 else []):
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        sc.get.aggregate(adata, "grp", funcs)
        ts.append(time.perf_counter() - t0)
    say(f"sc.get.aggregate host to host, {'+'.join(funcs):32s} {min(ts) * 1e3:9.1f} ms (best of 3; the matrix is uploaded in every call)")
torch.set_num_threads(16)
t0 = time.perf_counter()
keep = codes_h >= 0
ind = sparse.csr_matrix((np.ones(keep.sum()), (codes_h[keep], np.flatnonzero(keep))), shape=(n_groups, n))
s = ind @ x_host
cnt = ind @ (x_host != 0).astype(np.float64)
t_sum = time.perf_counter() - t0
t0 = time.perf_counter()
sq = ind @ x_host.multiply(x_host)
t_var = time.perf_counter() - t0
say(f"host restatement (scipy indicator product, float64): sum + count {t_sum * 1e3:.0f} ms, the sum of squares for var a further "
    f"{t_var * 1e3:.0f} ms")
