"""TEST INFRASTRUCTURE shared by tests/test_gpu_diffmap.py (the product library on the GPU, through scanpy_amd/_kernels.py) and
tests/test_emu_diffmap_cpu.py (the same host code and kernels on the emulator): the smallest inputs at which the kernels of
`sc.tl.diffmap` / `sc.tl.dpt` can still go wrong -- scamd_transitions_sym_f32, scamd_diffmap_f32 (both instantiations of the
panel kernels and their upper edges), scamd_dpt_pseudotime_f32 -- ONE checker per property, and the CPU truth: a numpy / scipy
restatement of src/scanpy/neighbors/__init__.py:805-827 (transitions), :884-890 (`eigsh(which='LM')`, cast to float32) and
:920-953 (the dpt row and the pseudotime).  Nothing here touches a device: a test hands in a `Runner` with

    transitions(a, density_normalize) -> (t_sym [nnz] float32 on the pattern of `a`, z [n] float64)
    diffmap(t, n_comps)               -> (evals [k] float64, evecs [n, k] float64, info dict as scanpy_amd._lib.diffmap_info)
    dpt(evals, basis, iroot, labels, scale) -> DPT distances from iroot [n] float32, divided by their largest finite one if scale
    Refused                           the exception of a refused call

Tolerances.  Where rounding decides, the bound is derived and the derivation stands next to the constant.  For eigenvalues,
principal cosines and pseudotime the cases were run once on the emulator and once on the MI355X; the worst deviation from the
scipy truth per quantity is recorded in profiles/diffmap_tolerances.log and the tolerance is 4x the larger of the two (the
margin: the emulator does not share the accumulation order of the matrix cores)."""
from __future__ import annotations

from functools import lru_cache
from pathlib import Path

import numpy as np
from scipy import sparse

GOLDEN = Path(__file__).resolve().parent / "golden"
TOL_SOLVER = 2e-6  # the default of scanpy_amd/_kernels.py:diffmap, the project's TOL_SPECTRAL
U32 = 2.0 ** -24   # unit roundoff of float32

# profiles/diffmap_tolerances.log: worst deviation over all cases on the emulator / on the MI355X, tolerance = 4 x the larger
TOL_EVALS = 4 * 3.3e-8           # |lambda - scipy|: emulator 3.284e-8, MI355X 3.284e-8 (pbmc, n_comps = 10)
TOL_ONE_MINUS_COS = 4 * 1.62e-10  # 1 - smallest principal cosine of a group: emulator 1.613e-10, MI355X 1.612e-10 (pbmc, 15)
# pseudotime, the kernel against the float64 restatement on the same float32 eigenpairs: 0 on the emulator and on the MI355X
# (both round the same float64 value to float32 once), so 4 x the measurement says nothing.  The reference's own float32 cast
# of the eigenpairs moves the pseudotime by 1.8e-6 (scipy against scipy on the pbmc graph); a bound under that figure would
# test noise, so that figure is the bound.
TOL_PSEUDOTIME = 1.8e-6
# |column 0 - z / |z||, pbmc: emulator 6.29e-7 (n_comps = 26), MI355X 3.64e-7 (n_comps = 15)
TOL_STATIONARY = 4 * 6.3e-7
GROUP_GAP = 1e-3   # consecutive eigenvalues closer than this form one group (compared as an invariant subspace)

# ---------------------------------------------------------------------------------------------------------------------
# the CPU truth
# ---------------------------------------------------------------------------------------------------------------------
def transitions_truth(a: sparse.csr_matrix, density_normalize: bool = True):
    """neighbors/__init__.py:805-827 in float64 -> (T_sym CSR float64 on the pattern of a, z [n])"""
    a = a.astype(np.float64).tocsr()
    n = a.shape[0]
    if density_normalize:
        dens = np.asarray(a.sum(axis=0)).ravel()
        d = sparse.diags(1.0 / dens)
        k = (d @ a @ d).tocsr()
    else:
        k = a
    z = np.sqrt(np.asarray(k.sum(axis=0)).ravel())
    zi = sparse.diags(1.0 / z)
    t = (zi @ k @ zi).tocsr()
    t.sort_indices()
    assert t.shape == (n, n) and np.array_equal(t.indices, a.indices) and np.array_equal(t.indptr, a.indptr)
    return t, z


def eigen_truth(t32: sparse.csr_matrix, k: int):
    """`eigsh(T_sym.astype(float64), k, which='LM', tol=1e-12)`, descending (neighbors/__init__.py:879-890)"""
    from scipy.sparse.linalg import eigsh

    lam, vec = eigsh(t32.astype(np.float64), k=k, which="LM", tol=1e-12, v0=np.ones(t32.shape[0]))
    order = np.argsort(-lam)
    return lam[order], vec[:, order]


def dpt_truth(evals32, basis32, iroot: int, labels=None, scale: bool = True):
    """`_get_dpt_row(iroot)` (+ `_set_pseudotime` if scale) (neighbors/__init__.py:920-953) on float32 eigenpairs, float64
    arithmetic"""
    lam = evals32.astype(np.float64)
    basis = basis32.astype(np.float64)
    diff = basis[iroot][None, :] - basis
    with np.errstate(divide="ignore"):
        w = np.where(lam < 0.9994, lam / (1.0 - lam), 1.0)
    row = np.sqrt(((w[None, :] * diff) ** 2).sum(axis=1))
    if labels is not None:
        row[labels != labels[iroot]] = np.inf
    return (row / row[row < np.inf].max() if scale else row).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the graphs
# ---------------------------------------------------------------------------------------------------------------------
def _csr32(a):
    a = sparse.csr_matrix(a).astype(np.float32)
    a.sort_indices()
    return a


def _toy():
    f = np.load(GOLDEN / "neighbors_toy.npz")
    return _csr32(f["connectivities_umap"])


def _pbmc():
    """the reference's own connectivities of pbmc68k_reduced: 700 rows (no multiple of 64), 9992 entries, one component"""
    f = np.load(GOLDEN / "pbmc68k_reduced.npz")
    a = sparse.csr_matrix((f["connectivities_data"], f["connectivities_indices"], f["connectivities_indptr"]),
                          shape=tuple(f["connectivities_shape"]))
    return _csr32(a)


def _two_blobs():
    """n = 333 + 170 = 503 (odd, no multiple of 4): two Gaussian blobs in 5-d far apart, symmetric 10-NN graph with positive
    weights; vertex 0 gets edges to 150 more vertices of its own blob, so its row (> 64 entries) takes the lane-strided loop of
    the degree kernels more than once"""
    rng = np.random.default_rng(7)
    n1, n2, kn = 333, 170, 10
    pts = np.vstack([rng.standard_normal((n1, 5)), rng.standard_normal((n2, 5)) + 40.0])
    n = n1 + n2
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    nb = np.argsort(d, axis=1, kind="stable")[:, 1:kn + 1]
    dist = np.take_along_axis(d, nb, axis=1)
    g = sparse.csr_matrix((np.exp(-dist / dist.mean()).ravel(), nb.ravel(), np.arange(0, n * kn + 1, kn)), shape=(n, n))
    g = g.maximum(g.T).tolil()
    for v in rng.choice(np.arange(1, n1), size=150, replace=False):
        g[0, v] = g[v, 0] = 0.25
    return _csr32(g.tocsr())


def _even_ring():
    """cycle on 64 vertices, unit weights: T_sym = A / 2 has the eigenvalue -1"""
    n = 64
    i = np.arange(n)
    return _csr32(sparse.csr_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n)))


GRAPHS = {"toy": _toy, "pbmc": _pbmc, "two_blobs": _two_blobs, "even_ring": _even_ring}
K_TRUTH = 28  # eigenpairs of the truth: every requested width (<= 26) plus the first value not requested


@lru_cache(maxsize=None)
def graph_input(name: str):
    """-> dict(a, t32 (truth T_sym rounded to float32, CSR), z, lam [K_TRUTH], vec [n, K_TRUTH], labels); computed once, never
    written"""
    from scipy.sparse.csgraph import connected_components

    a = GRAPHS[name]()
    t, z = transitions_truth(a, True)
    t32 = t.astype(np.float32)
    out = {"a": a, "t32": t32, "z": z, "labels": connected_components(a)[1].astype(np.int32)}
    if name in ("pbmc", "two_blobs"):
        out["lam"], out["vec"] = eigen_truth(t32, K_TRUTH)
        # largest magnitude = largest algebraic value on these graphs: what the device solver relies on
        assert out["lam"].min() > 0.0
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# case 1 (and the transitions of every graph): compute_transitions
# ---------------------------------------------------------------------------------------------------------------------
TRANSITION_CASES = [("toy", True), ("toy", False), ("pbmc", True), ("two_blobs", True), ("two_blobs", False), ("even_ring", True)]


def run_transitions_case(run, name: str, density_normalize: bool, label: str = ""):
    a = graph_input(name)["a"]
    t_ref, z_ref = transitions_truth(a, density_normalize)
    t, z = run.transitions(a, density_normalize)
    t2, z2 = run.transitions(a, density_normalize)
    assert t.dtype == np.float32 and z.dtype == np.float64
    assert t.tobytes() == t2.tobytes() and z.tobytes() == z2.tobytes(), "two runs differ"
    # both sides round a float64 value (relative error ~1e-15) to float32 once: they agree up to one unit in the last place
    # where the two float64 values straddle a rounding boundary
    err_t = np.abs(t.astype(np.float64) / t_ref.data - 1).max()
    err_z = np.abs(z / z_ref - 1).max()
    print(f"{label} transitions {name} dn={density_normalize}: rel err T {err_t:.2e} z {err_z:.2e}")
    assert err_t <= 2 * U32 * (1 + 1e-6)
    assert err_z < 1e-13  # a float64 sum of <= 200 positive terms and one square root
    if name == "toy" and density_normalize:
        # the reference's own matrices, at its own rtol (tests/test_neighbors.py:225-226)
        f = np.load(GOLDEN / "neighbors_toy.npz")
        t_sym = sparse.csr_matrix((t, a.indices, a.indptr), shape=a.shape).astype(np.float64)
        np.testing.assert_allclose(t_sym.toarray(), f["transitions_sym_umap"], rtol=1e-5)
        trans = sparse.diags(1.0 / z) @ t_sym @ sparse.diags(z)  # Z T_sym Z^-1 with Z = diag(1 / z) (neighbors/__init__.py:537)
        np.testing.assert_allclose(trans.toarray(), f["transitions_umap"], rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# cases 2 and 3: compute_eigen
# ---------------------------------------------------------------------------------------------------------------------
EIGEN_CASES = [("pbmc", 3), ("pbmc", 10), ("pbmc", 15), ("pbmc", 26), ("two_blobs", 15)]  # blocks of 9, 16, 21, 32, 21 columns


def _groups(lam_all: np.ndarray, k: int):
    """the requested eigenvalues split where consecutive ones are >= GROUP_GAP apart -> [(lo, hi)]; the trailing group is
    dropped when the first value not requested is closer than GROUP_GAP (its subspace is then not determined by k values)"""
    cuts = [0] + [i for i in range(1, k) if lam_all[i - 1] - lam_all[i] >= GROUP_GAP] + [k]
    groups = list(zip(cuts[:-1], cuts[1:]))
    skipped = 0
    if lam_all[k - 1] - lam_all[k] < GROUP_GAP:
        groups.pop()
        skipped = 1
    return groups, skipped


def _max_row_entries(t):
    return int(np.diff(t.indptr).max())


def run_eigen_case(run, name: str, k: int, label: str = ""):
    g = graph_input(name)
    t32, lam_all, vec_all = g["t32"], g["lam"], g["vec"]
    n = t32.shape[0]
    lam, v, info = run.diffmap(t32, k)
    print(f"{label} diffmap {name} k={k}: {info}")
    lam2, v2, info2 = run.diffmap(t32, k)
    assert lam.tobytes() == lam2.tobytes() and v.tobytes() == v2.tobytes() and info == info2, "two runs differ"
    assert lam.dtype == np.float64 and v.dtype == np.float64 and v.shape == (n, k) and lam.shape == (k,)
    assert info["converged"] and info["residual"] < TOL_SOLVER and not info["guard_refused"]
    assert np.all(np.diff(lam) <= 0)
    # eigenvalues against scipy
    err = np.abs(lam - lam_all[:k]).max()
    print(f"{label} diffmap {name} k={k}: eigenvalue err {err:.2e}, lambda_min estimate {info['lambda_min_estimate']:.4f}")
    assert err < TOL_EVALS
    # residual, recomputed in float64 on the float32 matrix the solver was given.  The solver stops on the residual of the
    # pairs of M = (T + I) / 2, half that of T: 2 tol.  Its own M v carries the float32 rounding of the operand y and of the
    # SpMM: at most (r + 2) u |T| |y| per row with r the longest row and u = 2^-24, |T| = 1 in norm.
    resid = np.linalg.norm(t32.astype(np.float64) @ v - v * lam[None, :], axis=0).max()
    bound = 2 * TOL_SOLVER + (_max_row_entries(t32) + 2) * U32
    print(f"{label} diffmap {name} k={k}: residual {resid:.2e} (bound {bound:.2e})")
    assert resid < bound
    assert np.abs(v.T @ v - np.eye(k)).max() < 1e-10
    # the sign rule: the entry of largest magnitude of every column is positive, the lowest row on ties
    top = np.argmax(np.abs(v), axis=0)
    assert np.all(v[top, np.arange(k)] > 0)
    if name == "pbmc":
        # column 0 is the stationary vector z / |z| (positive, so the sign rule leaves it as it is)
        z = g["z"] / np.linalg.norm(g["z"])
        dev = np.linalg.norm(v[:, 0] - z)
        print(f"{label} diffmap {name} k={k}: |v0 - z/|z|| {dev:.2e}")
        assert dev < TOL_STATIONARY
    else:
        np.testing.assert_allclose(lam[:2], 1.0, atol=TOL_EVALS)  # one eigenvalue 1 per component
    # eigenvectors as invariant subspaces
    groups, skipped = _groups(lam_all, k)
    assert skipped <= 1
    worst = 0.0
    for lo, hi in groups:
        cosines = np.linalg.svd(vec_all[:, lo:hi].T @ v[:, lo:hi], compute_uv=False)
        worst = max(worst, 1.0 - cosines.min())
    print(f"{label} diffmap {name} k={k}: {len(groups)} groups ({skipped} skipped), 1 - cos {worst:.2e}")
    assert worst < TOL_ONE_MINUS_COS
    if name == "two_blobs":
        assert (0, 2) in groups  # the pair of eigenvalue 1: its projector matches scipy's
    return info


def run_eigen_refusals(run):
    import pytest

    g = graph_input("pbmc")
    with pytest.raises(run.Refused, match="diffmap"):
        run.diffmap(g["t32"], 27)  # a block of 33 columns
    small = graph_input("toy")["t32"]
    with pytest.raises(run.Refused, match="diffmap"):
        run.diffmap(small, 3)  # n = 4 <= b
    holed = g["t32"].tolil()
    holed[5, :] = 0
    holed = _csr32(holed.tocsr())
    holed.eliminate_zeros()
    assert holed.indptr[6] == holed.indptr[5]
    with pytest.raises(run.Refused, match="empty row"):
        run.diffmap(holed, 3)


def run_even_ring(run, label: str = ""):
    """case 4: T_sym of the even ring has the eigenvalue -1 -- refused by the largest-magnitude guard, no fault"""
    import pytest

    t32 = graph_input("even_ring")["t32"]
    np.testing.assert_array_equal(t32.data, np.float32(0.5))
    with pytest.raises(NotImplementedError, match="negative eigenvalue .* of larger magnitude than the last requested component"):
        run.diffmap(t32, 3)


# ---------------------------------------------------------------------------------------------------------------------
# case 5: pseudotime
# ---------------------------------------------------------------------------------------------------------------------
DPT_CASES = [(name, n_dcs, root) for name in ("pbmc", "two_blobs") for n_dcs in (10, 15) for root in ("first", "mid")]


def run_dpt_case(run, name: str, n_dcs: int, root: str, label: str = ""):
    g = graph_input(name)
    n = g["a"].shape[0]
    iroot = 0 if root == "first" else n // 2 - (0 if name == "pbmc" else 100)  # (two_blobs: a mid-graph root of the first blob)
    evals32, basis32 = g["lam"][:n_dcs].astype(np.float32), g["vec"][:, :n_dcs].astype(np.float32)
    # no eigenvalue near the branch point of the weights: the two sides could differ there for a reason that is no bug
    assert np.abs(evals32.astype(np.float64) - 0.9994).min() > 1e-4
    labels = g["labels"] if name == "two_blobs" else None
    want = dpt_truth(evals32, basis32, iroot, labels)
    got = run.dpt(evals32, basis32, iroot, labels, True)
    got2 = run.dpt(evals32, basis32, iroot, labels, True)
    assert got.dtype == np.float32 and got.shape == (n,) and got.tobytes() == got2.tobytes()
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    err = np.abs(got[fin].astype(np.float64) - want[fin]).max()
    print(f"{label} dpt {name} n_dcs={n_dcs} root={iroot}: err {err:.2e}")
    assert err < TOL_PSEUDOTIME
    assert got[iroot] == 0.0 and got[fin].max() == 1.0
    if name == "two_blobs":
        assert g["labels"][iroot] == g["labels"][0]
        assert np.array_equal(~fin, g["labels"] != g["labels"][0]) and (~fin).sum() == 170
        assert np.all(np.isposinf(got[~fin]))
    # a basis wider than n_dcs (the row stride the front end hands over after `n_dcs` cut a stored basis)
    wide = np.ascontiguousarray(g["vec"][:, :n_dcs + 3].astype(np.float32))
    assert run.dpt(evals32, wide, iroot, labels, True).tobytes() == got.tobytes()
    # the unscaled row (`distances_dpt[iroot]`): the same float64 value rounded without the division, so the same bound
    # relative to its largest entry
    raw, raw_want = run.dpt(evals32, basis32, iroot, labels, False), dpt_truth(evals32, basis32, iroot, labels, scale=False)
    assert np.array_equal(np.isfinite(raw), fin)
    err_raw = np.abs(raw[fin].astype(np.float64) - raw_want[fin]).max() / raw_want[fin].max()
    print(f"{label} dpt {name} n_dcs={n_dcs} root={iroot}: unscaled err / max {err_raw:.2e}")
    assert err_raw < TOL_PSEUDOTIME and raw[fin].max() != 1.0
