"""TEST INFRASTRUCTURE shared by tests/test_gpu_eigensolver.py (the product library on the GPU, through scanpy_amd/_kernels.py)
and tests/test_emu_eigensolver_cpu.py (the same host code and kernels on the emulator, through tests/emu/harness.py): the
smallest inputs at which each path of the Chebyshev-filtered subspace iteration of csrc/subspace.h exists -- the dense operator
of `sc.pp.pca` (scamd_eigh_topk_f64, scamd_pca_csr_f32) and the sparse, deflated one of `sc.tl.umap(init_pos='spectral')`
(scamd_spectral_embedding_f32) -- their inputs, ONE checker per entry point, and the counters by which a case proves which
path it took.  Nothing here touches a device: a test hands in a `Runner` whose methods take and return numpy arrays.

The bars are those of tests/test_gpu_dense.py (test_eigh_topk, test_pca_csr_entry_vs_sklearn, _many_components_against_arpack)
and tests/test_gpu_umap.py (test_spectral_init_on_the_device_equals_arpack).  The counters were read on both the emulator and the
MI355X (profiles/eigensolver_refactor_ab.log) and agree in every case, so each is asserted exactly; where a later change
moves one on one machine only, the inequality that names the path (`n_outer >= 2`, `chol_retries >= 1`) is what must stay.

Not pinned (no input inside the entry points' contract reaches them): the power step of `dense_topk` on a block whose smallest
Ritz value is not positive (such a block has rank below b, and then the first Rayleigh-Ritz is already exact), and the plain
step of the spectral driver on a block whose smallest Ritz value lies outside (0, 1)."""
from __future__ import annotations

import operator

import numpy as np
from scipy import sparse

TOL_DENSE, TOL_SPECTRAL = 2e-8, 2e-6  # the defaults of scanpy_amd/_kernels.py
_OPS = {"==": operator.eq, ">=": operator.ge, "<=": operator.le}


def _assert_path(info: dict, path: dict, label: str):
    for key, (op, want) in path.items():
        assert _OPS[op](info[key], want), f"{label}: {key} = {info[key]}, the path needs {op} {want} ({info})"


# ---------------------------------------------------------------------------------------------------------------------
# dense operator: A = Q diag(lam) Q^T, Q from the QR of a seeded Gaussian matrix
# ---------------------------------------------------------------------------------------------------------------------
def _workload_spectrum(i):  # the spectrum of tests/test_gpu_dense.py::test_eigh_topk
    return 100.0 * 0.93 ** np.minimum(i, 80) * np.where(i < 80, 1.0, 0.5)


def _bulk_spectrum(i):
    return np.where(i < 5, 100.0 * 0.8 ** i, 0.01 * (1.0 - 0.3 * i / len(i)))


# name -> (g, k, lam(i), single vectors comparable, counters)
DENSE_CASES = {
    # b == g: one CholeskyQR2 and one Rayleigh-Ritz
    "whole_space": (40, 5, lambda i: 10.0 * 0.8 ** i, True,
                    {"block_size": ("==", 40), "n_outer": ("==", 0), "n_gemm": ("==", 1), "chol_retries": ("==", 0)}),
    # b = 48, g >= 2 b: the first filter of degree 7 is enough
    "one_pass": (256, 8, _workload_spectrum, True,
                 {"block_size": ("==", 48), "n_outer": ("==", 1), "n_gemm": ("==", 10), "chol_retries": ("==", 0)}),
    # a second outer iteration with the full degree 16, CholeskyQR shifted at once (`filtered`)
    "slow_decay": (256, 8, lambda i: 1.0 / (1.0 + 0.02 * i), False,
                   {"block_size": ("==", 48), "n_outer": ("==", 2), "n_gemm": ("==", 26), "chol_retries": ("==", 0)}),
    "wider_block": (320, 40, lambda i: 1.0 / (1.0 + 0.02 * i), False,
                    {"block_size": ("==", 80), "n_outer": ("==", 2), "n_gemm": ("==", 26), "chol_retries": ("==", 0)}),
    # five eigenvalues above a flat bulk: the degree rule clamps to 4 (m < 8: unfiltered CholeskyQR), which meets a failed
    # pivot and answers with a shifted round; eight outer iterations
    "bulk": (256, 8, _bulk_spectrum, False,
             {"block_size": ("==", 48), "n_outer": ("==", 8), "n_gemm": ("==", 38), "chol_retries": ("==", 1)}),
    # rank 20 < b: the smallest Rayleigh quotient is not positive, so no first filter; the first residual is below tol
    "rank_deficient": (256, 8, lambda i: np.where(i < 20, 10.0 * 0.8 ** i, 0.0), False,
                       {"block_size": ("==", 48), "n_outer": ("==", 1), "n_gemm": ("==", 4), "chol_retries": ("==", 2)}),
}

_dense_inputs = {}


def dense_input(name: str):
    """-> (a [g, g] symmetric, k, eigenvalues descending [k], eigenvectors [g, k]); computed once, never written"""
    if name not in _dense_inputs:
        g, k, spectrum, _, _ = DENSE_CASES[name]
        rng = np.random.default_rng(1000 + sorted(DENSE_CASES).index(name))
        q, _ = np.linalg.qr(rng.standard_normal((g, g)))
        a = (q * spectrum(np.arange(g))[None, :]) @ q.T
        a = 0.5 * (a + a.T)
        ref_l, ref_v = np.linalg.eigh(a)
        for arr in (a, ref_l, ref_v):
            arr.setflags(write=False)
        _dense_inputs[name] = (a, k, ref_l[::-1][:k], ref_v[:, ::-1][:, :k])
    return _dense_inputs[name]


def run_dense_case(run, name: str, label: str = ""):
    a, k, ref_l, ref_v = dense_input(name)
    _, _, _, vectors, path = DENSE_CASES[name]
    lam, v, info = run.eigh_topk(a, k)
    print(f"{label} {name}: {info}")
    lam2, v2, info2 = run.eigh_topk(a, k)
    assert lam.tobytes() == lam2.tobytes() and v.tobytes() == v2.tobytes() and info == info2, f"{name}: two runs differ"
    top = ref_l[0]
    assert np.abs(lam - ref_l).max() < 1e-9 * top
    assert np.abs(a @ v - v * lam[None, :]).max() < 1e-6 * top
    assert np.abs(v.T @ v - np.eye(k)).max() < 1e-10
    assert info["residual"] < TOL_DENSE
    if vectors:
        assert np.abs(np.abs(np.sum(v * ref_v, axis=0)) - 1.0).max() < 1e-8  # same vectors up to sign
    _assert_path(info, path, name)
    return info


REFUSALS = [(150, 50),    # 128 < g < 2 * block (block = k + 32 rounded up to 16 = 96)
            (1000, 110)]  # k beyond the block


def run_refusals(run):
    import pytest

    for g, k in REFUSALS:
        with pytest.raises(run.Refused, match="eigh_topk"):
            run.eigh_topk(np.eye(g), k)


# ---- two batches: scamd_pca_csr_f32 with more components than one block holds ----------------------------------------
PCA_SHAPE = (600, 256, 100)  # n, g, n_comps: a batch of 96 on b = 128, deflation, a batch of 4 on b = 48
PCA_PATH = {"block_size": ("==", 48), "n_outer": ("==", 4), "n_gemm": ("==", 53), "chol_retries": ("==", 0)}


def pca_input():
    n, g, _ = PCA_SHAPE
    rng = np.random.default_rng(2024)
    x = sparse.random(n, g, density=0.2, format="csr", dtype=np.float32, random_state=rng, data_rvs=lambda m: rng.gamma(2.0, 1.0, m))
    x.sort_indices()
    return x


def run_two_batches(run, label: str = ""):
    x = pca_input()
    n, g, k = PCA_SHAPE
    got = run.pca_csr(x, k)
    print(f"{label} two_batches: {got['info']}")
    again = run.pca_csr(x, k)
    for key in ("scores", "components", "variance", "variance_ratio", "mean"):
        assert got[key].tobytes() == again[key].tobytes(), f"two_batches: two runs differ in {key}"
    assert got["info"] == again["info"]
    xd = x.toarray().astype(np.float64)
    ref_var = np.linalg.eigvalsh(np.cov(xd, rowvar=False))[::-1][:k]
    err = np.abs(got["variance"] / ref_var - 1).max()
    print(f"{label} two_batches: variance rel err {err:.2e}")
    assert err < 2e-5
    comps = got["components"]
    assert np.abs(comps @ comps.T - np.eye(k)).max() < 1e-5  # orthonormal ACROSS the batches too
    assert got["info"]["residual"] < TOL_DENSE
    _assert_path(got["info"], PCA_PATH, "two_batches")
    return got["info"]


# ---------------------------------------------------------------------------------------------------------------------
# spectral operator: M = (S + I) / 2, S = D^-1/2 A D^-1/2, the trivial eigenvector sqrt(deg) deflated
# ---------------------------------------------------------------------------------------------------------------------
def _sheet():
    """kNN graph (8 neighbours, exp(-d / mean) weights, symmetrised) of 600 uniform points in [0, 3] x [0, 1]"""
    rng = np.random.default_rng(0)
    n, kn = 600, 8
    pts = rng.uniform(size=(n, 2)) * [3.0, 1.0]
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    nb = np.argsort(d, axis=1, kind="stable")[:, 1:kn + 1]
    dist = np.take_along_axis(d, nb, axis=1)
    g = sparse.csr_matrix((np.exp(-dist / dist.mean()).ravel(), nb.ravel(), np.arange(0, n * kn + 1, kn)), shape=(n, n))
    return (g + g.T).tocsr().astype(np.float32)


def _ring():
    """cycle graph on 10 vertices: the smallest n the entry takes at dim = 2 (n > dim + 6); S = A / 2, eigenvalues cos(2 pi j / n)"""
    n = 10
    i = np.arange(n)
    return sparse.csr_matrix((np.ones(2 * n, np.float32), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n))


# name -> (graph, dim, counters)
SPECTRAL_CASES = {
    "sheet": (_sheet, 2, {"outer_iterations": ("==", 4), "operator_applications": ("==", 146)}),
    # the block (b = 8) nearly spans the space (n - 1 = 9 after the deflation)
    "ring": (_ring, 2, {"outer_iterations": ("==", 2), "operator_applications": ("==", 61)}),
}

_spectral_inputs = {}


def spectral_input(name: str):
    """-> (a CSR float32, dim, sqrt(deg), reference eigenvalues of S below the trivial one [dim], their eigenvectors [n, dim])"""
    if name not in _spectral_inputs:
        build, dim, _ = SPECTRAL_CASES[name]
        a = build()
        a.sort_indices()
        deg = np.asarray(a.sum(1)).ravel().astype(np.float64)
        dis = 1.0 / np.sqrt(deg)
        s_mat = (sparse.diags(dis) @ a.astype(np.float64) @ sparse.diags(dis)).tocsr()
        n = a.shape[0]
        if name == "ring":
            lam, vec = np.linalg.eigh(s_mat.toarray())  # (ARPACK takes k < n - 1 only; the values are checked in closed form)
            np.testing.assert_allclose(lam[::-1][1:dim + 1], np.cos(2 * np.pi / n), atol=1e-14)
        else:
            from scipy.sparse.linalg import eigsh

            lam, vec = eigsh(s_mat, k=dim + 1, which="LA", tol=1e-10, v0=np.ones(n))
        order = np.argsort(-lam)
        _spectral_inputs[name] = (a, dim, np.sqrt(deg), lam[order][1:dim + 1], vec[:, order][:, 1:dim + 1])
    return _spectral_inputs[name]


def run_spectral_case(run, name: str, label: str = ""):
    a, dim, t0, ref_l, ref_v = spectral_input(name)
    v, info = run.spectral_embedding(a, dim)
    print(f"{label} {name}: {info}")
    v2, info2 = run.spectral_embedding(a, dim)
    assert v.tobytes() == v2.tobytes() and info == info2, f"{name}: two runs differ"
    assert info["converged"] and info["residual"] < TOL_SPECTRAL
    assert np.abs(v.T @ v - np.eye(dim)).max() < 1e-10
    assert np.abs(v.T @ (t0 / np.linalg.norm(t0))).max() < 1e-6
    np.testing.assert_allclose(info["ritz_values"][:dim], ref_l, atol=2e-6)
    # the plane, never single vectors (the ring's two eigenvalues are a degenerate pair)
    cosines = np.linalg.svd(ref_v.T @ v, compute_uv=False)
    print(f"{label} {name}: principal cosines {cosines}")
    assert cosines.min() > 1 - 1e-4
    _assert_path(info, SPECTRAL_CASES[name][2], name)
    return info
