"""The probe behind profiles/diffmap_timing.log: tl.diffmap(n_comps=15) on the planted graph bench.py generates -- device time
and operator applications of scamd_diffmap_f32 -- next to scipy eigsh on the same transition matrix on the host.
    python tools/diffmap_timing.py N_OBS host|nohost      (needs an MI355X; `host` also runs scipy, which may take very long)"""
import sys, time, warnings
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np, torch
import scanpy_amd as sc
import bench
from scanpy_amd import _kernels as K

warnings.filterwarnings("ignore", message="Transition matrix has many disconnected components")
n_obs, host = int(sys.argv[1]), sys.argv[2] == "host"
def say(*a):
    print(*a, flush=True)
t0 = time.perf_counter()
out = bench.make_matrix(n_obs, 2000, 0, "planted")
x = out[0] if isinstance(out, tuple) else out
say(f"n={n_obs}: matrix {time.perf_counter() - t0:.1f} s")
adata = sc.AnnData(x)
t0 = time.perf_counter()
sc.pp.pca(adata, n_comps=50)
sc.pp.neighbors(adata, n_neighbors=15)
torch.cuda.synchronize()
say(f"n={n_obs}: pca + neighbors {time.perf_counter() - t0:.1f} s; nnz {adata.obsp['connectivities'].nnz}, components {sc.Neighbors(adata)._number_connected_components}")
nb = sc.Neighbors(adata)
for rep in range(2):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    nb.compute_transitions()
    torch.cuda.synchronize(); t1 = time.perf_counter()
    say(f"n={n_obs} rep {rep}: compute_transitions (upload + kernel + download) {t1 - t0:.3f} s")
t = nb.transitions_sym
dev = torch.device("cuda")
ip, ix, tv = (torch.from_numpy(t.indptr.astype(np.int64)).to(dev), torch.from_numpy(t.indices.astype(np.int32)).to(dev), torch.from_numpy(t.data).to(dev))
for rep in range(2):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    try:
        evals, evecs, info = K.diffmap(ip, ix, tv, n_obs, 15)
    except NotImplementedError as e:
        say("REFUSED:", e); raise SystemExit(0)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    say(f"n={n_obs} rep {rep}: scamd_diffmap_f32 n_comps=15 device-resident {t1 - t0:.3f} s  {info}")
say("evals", evals.cpu().numpy())
for rep in range(1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    sc.tl.diffmap(adata)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    say(f"n={n_obs}: tl.diffmap host to host {t1 - t0:.3f} s")
if host:
    from scipy.sparse.linalg import eigsh
    t0 = time.perf_counter()
    lam, vec = eigsh(t.astype(np.float64), k=15, which="LM", v0=np.random.default_rng(0).standard_normal(n_obs))
    t1 = time.perf_counter()
    say(f"n={n_obs}: scipy eigsh(k=15, which='LM') on the host {t1 - t0:.2f} s")
    lam = np.sort(lam)[::-1]
    say("scipy evals", lam)
    say("max |evals - scipy|", np.abs(evals.cpu().numpy() - lam).max())
