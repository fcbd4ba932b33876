"""The probe behind profiles/scrublet_timing.log: the row-pair kernel beside a yardstick, and pp.scrublet host to host.
    python tools/scrublet_timing.py pairs     (a) scamd_pp_scrublet_pair_fill_f32 on 20 000 observed rows x 2 000 genes at 5 % with
                                              40 000 pairs, and the same at 30 000 genes: its share of the measured 6.29 TB/s for the
                                              bytes it reads and writes, beside scamd_csr_transpose_f32 on the OUTPUT matrix, which
                                              moves the same bytes (device events, 2 warm-ups, median of 5, sides alternating, two
                                              rounds; the margin is the yardstick's own max / min over both rounds)
    python tools/scrublet_timing.py e2e       (b) sc.pp.scrublet on 20 000 x 2 000 counts of the generator of tests/scrublet_cases.py,
                                              host to host, the device stages one by one (synchronised wall clock), and the
                                              numpy / scipy / sklearn restatement of tests/scrublet_cases.py on the host CPUs"""
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
import torch
import scanpy_amd as sc
from scanpy_amd import _kernels as K
from scanpy_amd.preprocessing import _csr_device

be = _csr_device.GpuPPBackend()
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


if mode == "pairs":
    lib = __import__("scanpy_amd._lib", fromlist=["load"]).load()
    from scanpy_amd._device import ptr, stream_ptr
    for g in (2000, 30000):
        n, n_sim = 20000, 40000
        x = sparse.random(n, g, density=0.05, format="csr", dtype=np.float32, random_state=g)
        x.data = np.ceil(x.data * 20).astype(np.float32)
        x.sort_indices()
        m = be.upload(x)
        pairs_h = np.ascontiguousarray(np.vstack(np.unravel_index(np.random.default_rng(0).choice(n * n, n_sim, replace=False), (n, n))).T, dtype=np.int32)
        pairs = torch.from_numpy(pairs_h).to(dev)
        tot = K.pp_row_sums(m.indptr, m.indices, m.data, n).double()
        oip, oix, odv, _, flags = K.pp_scrublet_pairs(m.indptr, m.indices, m.data, n, g, pairs, tot)
        again = K.pp_scrublet_pairs(m.indptr, m.indices, m.data, n, g, pairs, tot)
        same = all(bool(torch.equal(a, b)) for a, b in zip((oip, oix, odv), again[:3]))
        out_nnz = int(odv.numel())
        ln = np.diff(x.indptr)
        read = 8 * int(ln[pairs_h[:, 0]].sum() + ln[pairs_h[:, 1]].sum()) + 16 * n_sim
        moved = read + 8 * out_nnz
        fl = torch.zeros(1, dtype=torch.int32, device=dev)

        def fill():
            lib.scamd_pp_scrublet_pair_fill_f32(ptr(m.indptr), ptr(m.indices), ptr(m.data), n, g, m.data.numel(), ptr(pairs), n_sim,
                                                ptr(oip), out_nnz, ptr(oix), ptr(odv), ptr(fl), stream_ptr())

        sides = [("pair_both_phases", lambda: K.pp_scrublet_pairs(m.indptr, m.indices, m.data, n, g, pairs, tot)),
                 ("pair_fill", fill),
                 ("csr_transpose_of_output", lambda: K.csr_transpose(oip, oix, odv, n_sim, g))]
        res = {}
        for rnd in range(2):
            for name, fn in sides:
                res.setdefault(name, []).append(timed(fn))
        med = {k: float(np.median([v[0] for v in vs])) for k, vs in res.items()}
        say(f"pairs g={g}: {n} x {g}, nnz {x.nnz} ({x.nnz / n:.0f} per row), {n_sim} pairs -> {out_nnz} entries; flags {flags}; two runs "
            f"bit-identical: {same}")
        for k, vs in res.items():
            say(f"pairs g={g}: {k}: " + "; ".join(f"median {a:.3f} ms (min {b:.3f}, max {c:.3f})" for a, b, c in vs))
        base = res["csr_transpose_of_output"]
        spread = max(v[2] for v in base) / min(v[1] for v in base)
        t = med["pair_fill"]
        ratio = t / med["csr_transpose_of_output"]
        verdict = "faster than" if ratio < 1 / spread else ("SLOWER than" if ratio > spread else "within the spread of")
        say(f"pairs g={g}: fill {t:.3f} ms for {moved / 1e9:.3f} GB read + written = {moved / (t * 1e-3) / 1e12:.3f} TB/s = "
            f"{100 * moved / (t * 1e-3) / HBM_MEASURED:.1f}% of the measured 6.29 TB/s; csr_transpose of the output "
            f"{med['csr_transpose_of_output']:.3f} ms; ratio {ratio:.3f} (yardstick spread max/min {spread:.3f}): {verdict} the yardstick; "
            f"both phases with the scan, the read-back and the allocation {med['pair_both_phases']:.3f} ms")
        del m, oip, oix, odv, again
        torch.cuda.empty_cache()
else:
    import scrublet_cases as S
    n, g = 20000, 2000
    t0 = time.perf_counter()
    x, planted = S.make_counts(n, g, 8, 0)
    say(f"e2e: {n} x {g} counts, nnz {x.nnz} ({x.nnz / n:.0f} per cell), {planted.sum()} planted doublets; generated in "
        f"{time.perf_counter() - t0:.1f} s")
    walls = []
    for i in range(3):
        a = sc.AnnData(x.copy())
        torch.cuda.synchronize(); t0 = time.perf_counter()
        sc.pp.scrublet(a, rng=7, verbose=False)
        walls.append(time.perf_counter() - t0)
    called = a.obs["predicted_doublet"].to_numpy().astype(bool)
    say("e2e: sc.pp.scrublet(adata, rng=7) host to host (filters, normalisation, HVG, simulation, call): "
        + ", ".join(f"{v:.3f} s" for v in walls) + f"; threshold {a.uns['scrublet'].get('threshold')}, called {called.sum()}, of them "
        f"planted {(called & planted).sum()} of {planted.sum()}")

    # the device stages one by one, on all genes (the `adata_sim=` shape of the work: no gene selection)
    def stage(label, fn, acc):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        acc[label] = acc.get(label, 0.0) + (time.perf_counter() - t0) * 1e3
        return out

    pairs_h = np.ascontiguousarray(S.sample_pairs(n, 2 * n, 7), dtype=np.int32)
    for rep in range(2):
        acc = {}
        m = stage("upload", lambda: be.upload(x), acc)
        pairs = torch.from_numpy(pairs_h).to(dev)
        tot = K.pp_row_sums(m.indptr, m.indices, m.data, n).double()
        sip, six, sdv, _, _ = stage("simulate", lambda: K.pp_scrublet_pairs(m.indptr, m.indices, m.data, n, g, pairs, tot), acc)
        mats = ((m.indptr, m.indices, m.data, n), (sip, six, sdv, 2 * n))

        def normalise():
            for ip, ix, dv, rows in mats:
                factor = K.pp_row_sums(ip, ix, dv, rows).cpu().numpy() / 1e6
                K.pp_row_divide_(ip, dv, rows, torch.from_numpy(factor).to(dev))
            s, sq, _ = K.pp_col_stats(m.indptr, m.indices, m.data, n, g, count_positive=False)
            _, var = _csr_device.mean_var_from_sums(s, sq, n, correction=1)
            std = torch.sqrt(var)
            for ip, ix, dv, rows in mats:
                K.pp_scale_csr_(ip, ix, dv, rows, std)

        stage("normalise + scale", normalise, acc)

        def embed():
            _, comps, _, _, mean, _ = K.pca_csr(m.indptr, m.indices, m.data, n, g, 30, zero_center=True, seed=0)
            v = comps.t().contiguous()
            shift = mean @ v
            return torch.cat([K.spmm(ip, ix, dv, rows, g, v, shift) for ip, ix, dv, rows in mats], dim=0)

        man = stage("PCA + projection", embed, acc)
        k_adj = round(round(0.5 * np.sqrt(n)) * 3)
        idx = stage("kNN", lambda: K.knn(man, k_adj)[0], acc)
        out = stage("scores", lambda: K.scrublet_scores(idx, n, rho=0.05, r=2.0, se_rho=0.02), acc)
        stage("download", lambda: [t.cpu() for t in out], acc)
        say(f"e2e: device stages, all {g} genes, k_adj = {k_adj}, round {rep}: " + "; ".join(f"{k} {v:.2f} ms" for k, v in acc.items())
            + f"; sum {sum(acc.values()):.2f} ms")
        del m, sip, six, sdv, man, idx, out
    t0 = time.perf_counter()
    ref = S.ref_call(S.ref_normalize(x), S.ref_normalize(S.expected_pairs(x, pairs_h)))
    say(f"e2e: the float64 restatement of tests/scrublet_cases.py (scipy sums, dense z-score, sklearn PCA(arpack), brute-force "
        f"NearestNeighbors, formulas) on the host CPUs, all {g} genes: {time.perf_counter() - t0:.1f} s")
