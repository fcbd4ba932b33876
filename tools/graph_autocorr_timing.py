"""The probe behind profiles/graph_autocorr_timing.log: the edge sweep of metrics.morans_i / gearys_c beside a yardstick, the whole
call host to host, and a CPU baseline.
    python tools/graph_autocorr_timing.py sweep [n]   (a) on the bench's planted graph (pca -> neighbors at n cells, default 1M) and on
                                                  the same graph with hub rows and columns added: one slab of 64 float32 columns
                                                  through scamd_graph_autocorr_slab_f32 (column pass + sweep + reduction; the
                                                  column pass alone is timed on the empty graph and reported) beside
                                                  scamd_spmm_csr_f32 with l = 64 on the same graph, which gathers the same rows and
                                                  also writes n x 64 floats; then ncols = 50 at ld = 50 (X_pca in place), ncols = 1
                                                  (63 masked lanes), float64 values, float64 weights, and the two slab builders.
                                                  Device events, 2 warm-ups, median of 5, sides alternating, two rounds; the margin
                                                  is the yardstick's own max / min over both rounds.
    python tools/graph_autocorr_timing.py e2e [n]     (b) sc.metrics.morans_i host to host: n x 2000 sparse (the planted matrix after
                                                  normalize_total + log1p), n x 50 (obsm['X_pca'], read in place), n x 1.
    python tools/graph_autocorr_timing.py cpu [n]     (c) at n cells (default 100 000): the float64 numpy restatement of
                                                  tests/autocorr_cases.py on the host CPUs (on the first 128 genes, scaled to
                                                  2000) beside the device call."""
import sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
from scipy import sparse

HBM_MEASURED = 6.29e12  # bytes/s, SURVEY.md 8(d)
def say(*a):
    print(*a, flush=True)


mode = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else (100_000 if mode == "cpu" else 1_000_000)
import torch
import bench
import scanpy_amd as sc
from scanpy_amd import _kernels as K
from scanpy_amd.metrics import _autocorr

be = _autocorr.GpuAutocorrBackend()
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


def planted(n):
    t0 = time.perf_counter()
    x, truth = bench.make_matrix(n, 2000, 0, "planted")
    a = sc.AnnData(x)
    sc.pp.normalize_total(a)
    sc.pp.log1p(a)
    sc.pp.pca(a, n_comps=50)
    sc.pp.neighbors(a)
    g = a.obsp["connectivities"].tocsr()
    say(f"graph: {n} cells x 2000 genes (density {x.nnz / n / 2000:.3f}) -> pca 50 -> neighbors 15: {g.nnz} stored entries, "
        f"{g.dtype} weights, rows of {np.diff(g.indptr).min()}-{np.diff(g.indptr).max()}; built in {time.perf_counter() - t0:.1f} s")
    return a, g


def with_hubs(g, hubs=4, length=None, seed=1):
    """`hubs` rows of `length` entries each and the mirrored columns on top of g (asymmetric weights)"""
    n = g.shape[0]
    length = length or n // 10
    rng = np.random.default_rng(seed)
    rows = np.repeat(rng.choice(n, hubs, replace=False), length)
    cols = np.concatenate([rng.choice(n, length, replace=False) for _ in range(hubs)])
    add = sparse.coo_matrix((rng.uniform(0.05, 1, len(rows)).astype(g.dtype), (rows, cols)), shape=g.shape)
    add_t = sparse.coo_matrix((rng.uniform(0.05, 1, len(rows)).astype(g.dtype), (cols, rows)), shape=g.shape)
    return (g + add.tocsr() + add_t.tocsr()).tocsr()


def sweep_block(label, g):
    n = g.shape[0]
    h = be.open_graph(g.indptr, g.indices, g.data, n)
    nnz = g.nnz
    empty = be.open_graph(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, g.dtype), n)
    gen = torch.Generator(device=dev).manual_seed(0)
    s64 = torch.randn((n, 64), generator=gen, device=dev, dtype=torch.float32)
    s50 = s64[:, :50].contiguous()
    s1 = s64[:, :1].contiguous()
    s64d = s64.double()
    h64 = dict(h, weights=h["weights"].double())
    pe = K.graph_autocorr_part_entries(nnz)
    ln = np.diff(g.indptr)
    say(f"{label}: n {n}, nnz {nnz}, longest row {ln.max()} = {ln.max() / pe:.1f} parts of {pe} entries, {-(-nnz // pe)} parts")

    def slab(graph, s, ld, ncols):
        return K.graph_autocorr_slab(graph["indptr"], graph["indices"], graph["weights"], n, s.reshape(-1), ld, ncols)

    a1 = slab(h, s64, 64, 64)
    a2 = slab(h, s64, 64, 64)
    same = all(bool(torch.equal(p, q)) for p, q in zip(a1, a2))
    sides = [("slab call, 64 f32 columns", lambda: slab(h, s64, 64, 64)),
             ("spmm_csr_f32, l = 64", lambda: K.spmm(h["indptr"], h["indices"], h["weights"].float(), n, n, s64)),
             ("column pass alone (empty graph)", lambda: slab(empty, s64, 64, 64)),
             ("slab call, 50 f32 columns, ld 50", lambda: slab(h, s50, 50, 50)),
             ("slab call, 1 f32 column, ld 1", lambda: slab(h, s1, 1, 1)),
             ("slab call, 64 f64 columns", lambda: slab(h, s64d, 64, 64)),
             ("slab call, 64 f32 columns, f64 weights", lambda: slab(h64, s64, 64, 64)),
             ("weight sum", lambda: K.graph_weight_sum(h["weights"]))]
    res = {}
    for rnd in range(2):
        for name, fn in sides:
            res.setdefault(name, []).append(timed(fn))
    med = {k: float(np.median([v[0] for v in vs])) for k, vs in res.items()}
    say(f"{label}: two runs bit-identical: {same}")
    for k, vs in res.items():
        say(f"{label}: {k}: " + "; ".join(f"median {a:.3f} ms (min {b:.3f}, max {c:.3f})" for a, b, c in vs))
    base = res["spmm_csr_f32, l = 64"]
    spread = max(v[2] for v in base) / min(v[1] for v in base)
    t, col = med["slab call, 64 f32 columns"], med["column pass alone (empty graph)"]
    ratio = t / med["spmm_csr_f32, l = 64"]
    verdict = "faster than" if ratio < 1 / spread else ("SLOWER than" if ratio > spread else "within the spread of")
    gathered = nnz * 256
    say(f"{label}: slab call {t:.3f} ms, of which the column pass {col:.3f} ms; {gathered / 1e9:.2f} GB gathered (256-B rows) = "
        f"{gathered / (t * 1e-3) / 1e12:.3f} TB/s over the whole call, {gathered / (max(t - col, 1e-6) * 1e-3) / 1e12:.3f} TB/s over the sweep "
        f"alone; spmm {med['spmm_csr_f32, l = 64']:.3f} ms; ratio {ratio:.3f} (yardstick spread max/min {spread:.3f}): {verdict} the "
        f"yardstick; f64 values (512-B rows) {nnz * 512 / (med['slab call, 64 f64 columns'] * 1e-3) / 1e12:.3f} TB/s")
    del h, h64, s64, s64d, s50, s1
    torch.cuda.empty_cache()


if mode == "sweep":
    a, g = planted(n)
    sweep_block("planted", g)
    sweep_block("hubs", with_hubs(g))
    # the slab builders on the normalised matrix: 64 genes of a cell-major CSR, 64 feature-major rows
    x = a.X.tocsr()
    h = be.csr_cell_major(x.indptr, x.indices, x.data, n, x.shape[1])
    rows = torch.randn((64, n), device=dev, dtype=torch.float32)
    out = torch.empty((n, 64), device=dev, dtype=torch.float32)
    for name, fn in (("csr_dense_slab, genes 640..703", lambda: K.csr_dense_slab(h["indptr"], h["indices"], h["data"], n, x.shape[1], 640, 64, out)),
                     ("transpose_slab f32, 64 rows", lambda: K.transpose_slab(rows, out))):
        say(f"builders: {name}: " + "; ".join("median %.3f ms (min %.3f, max %.3f)" % timed(fn) for _ in range(2))
            + f"; writes {n * 256 / 1e9:.3f} GB")
elif mode == "e2e":
    a, g = planted(n)
    for label, kw in (("n x 2000 sparse X (32 slabs)", {}), ("n x 50 obsm['X_pca'] in place", dict(obsm="X_pca")),
                      ("n x 1 (one PC)", dict(vals=np.ascontiguousarray(a.obsm["X_pca"][:, 0])))):
        walls = []
        for i in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = sc.metrics.morans_i(a, **kw)
            walls.append(time.perf_counter() - t0)
        say(f"e2e: morans_i, {label}: " + ", ".join(f"{v * 1e3:.1f} ms" for v in walls) + f" host to host; first values "
            f"{np.atleast_1d(out)[:3]}")
    # the device part of the 2000-gene call with the matrix resident
    x = a.X.tocsr()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    h = be.csr_cell_major(x.indptr, x.indices, x.data, n, x.shape[1])
    gh = be.open_graph(g.indptr, g.indices, g.data, n)
    torch.cuda.synchronize(); t_up = time.perf_counter() - t0
    for i in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for c0 in range(0, 2000, 64):
            b = min(64, 2000 - c0)
            be.stats(gh, be.csr_slab(h, c0, b), 64, b)
        torch.cuda.synchronize()
        say(f"e2e: resident: 32 slabs (builder + column pass + sweep + reduction + read-back) {1e3 * (time.perf_counter() - t0):.1f} ms; "
            f"upload of matrix and graph {t_up * 1e3:.0f} ms")
else:
    import autocorr_cases as A
    a, g = planted(n)
    walls = []
    for i in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        dev_i = sc.metrics.morans_i(a)
        walls.append(time.perf_counter() - t0)
    sub = 128
    dense = a.X[:, :sub].toarray().astype(np.float64)
    t0 = time.perf_counter()
    ref_i, ref_c = A.restate(g.indptr, g.indices, g.data, dense)
    dt = time.perf_counter() - t0
    ok = ~np.isnan(ref_i)
    say(f"cpu: {n} cells: the float64 numpy restatement on {sub} genes {dt:.2f} s = {dt / sub * 1e3:.1f} ms per gene, {dt / sub * 2000:.0f} s "
        f"scaled to 2000 genes (both scores); sc.metrics.morans_i on all 2000 genes host to host " + ", ".join(f"{v:.3f} s" for v in walls)
        + f"; max |I_device - I_restatement| on the {sub} genes {np.abs(dev_i[:sub][ok] - ref_i[ok]).max():.2e}")
