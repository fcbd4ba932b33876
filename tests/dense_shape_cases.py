"""TEST INFRASTRUCTURE shared by tests/test_gpu_dense_shapes.py (the product library on the GPU, through
scanpy_amd/_kernels.py:dense_debug) and tests/test_emu_dense_shapes_cpu.py (the same kernels on the host emulator): the smallest
shapes at which each code path of the four float64 kernels of the dense solve (csrc/dense.hip: dgemm_tn_kernel,
panel_small_kernel, chol_factor_kernel, jacobi_eigh_kernel) exists, their inputs and ONE checker per kernel.  Nothing here
touches a device: a test hands in a `run(op, in0, in1)` that takes and returns numpy arrays with the meaning of
`scamd_dense_debug_f64`.

Where the paths are:
  * GEMM: a wave fetches GEMM_KB = 8 k-steps of 4 per batch, K is split over eight waves in ranges that are multiples of 4:
    K below one step, one k short of / exactly / one past a batch (31, 32, 33), a full batch plus a tail in every wave (8 * 32 + 5),
    and K = 36, where three of the eight waves get an empty range; M and N on both sides of the 16- and 32-wide tiles.
  * panel product: 16 rows per workgroup at b = 82 / 128, 256 at b = 7, 512 at b = 1 (two rows per thread, a row group per
    4 << cq_shift columns): row counts around a workgroup and around half of one, and 2000 rows (many workgroups).
  * Cholesky: a lane adds four elements per wait, eight lanes per row: b below, at and above 8 and 32, and the full 128.
  * Jacobi: ceil(b / 8) elements per lane, compile-time: both sides of 8 and 16, odd b (a padding player), b = 1 (no pair).
"""
from __future__ import annotations

import numpy as np

GEMM_KB = 8  # csrc/dense.hip
_B4 = 4 * GEMM_KB
# (K, M, N): every K of the list with M, N in {1, 31, 33, 82, 96, 128, 129} taken pairwise
GEMM_CASES = [(1, 1, 1), (1, 129, 82), (3, 31, 33), (3, 128, 1), (_B4 - 1, 33, 31), (_B4 - 1, 82, 129), (_B4 - 1, 96, 1),
              (_B4, 96, 128), (_B4, 1, 33), (_B4 + 1, 128, 96), (_B4 + 1, 129, 129), (8 * _B4 + 5, 82, 82), (8 * _B4 + 5, 31, 128),
              (8 * _B4 + 5, 129, 1), (36, 33, 96), (36, 96, 31), (36, 1, 129), (36, 128, 82)]
PANEL_CASES = [(g, b) for b in (1, 7, 82, 128) for g in (1, 7, 8, 9, 2000)] + [(15, 82), (17, 82), (33, 128), (257, 7), (513, 1)]
CHOL_SIZES = [1, 2, 8, 9, 82, 127, 128]
JACOBI_SIZES = [1, 2, 3, 8, 9, 15, 16, 17, 82, 127, 128]
PANEL_PAIR_CASES = [(1, 1), (9, 7), (17, 82), (2000, 82), (33, 128)]  # both products of a Rayleigh-Ritz in one launch (op 5)
JACOBI_SYMMETRISED_SIZES = [1, 2, 9, 82, 128]  # T symmetrised by the kernel's load (op 6)
JACOBI_SPECIAL = [(kind, b) for kind in ("diagonal", "identity", "half_rank") for b in (2, 9, 82, 128)]


def check_gemm(run, kdim, m, n):
    rng = np.random.default_rng(1000 * kdim + 10 * m + n)
    p, q = rng.standard_normal((kdim, m)), rng.standard_normal((kdim, n))
    got = run(1, p, q)
    ref = p.T @ q
    err, bound = np.abs(got - ref).max(), 1e-12 * max(1.0, np.abs(ref).max()) * np.sqrt(kdim)
    print(f"gemm K={kdim} M={m} N={n}: err {err:.2e} bound {bound:.2e}")
    assert got.shape == ref.shape and err <= bound
    assert np.array_equal(got, run(1, p, q))  # fixed reduction order: bitwise reproducible


def check_panel(run, g, b):
    rng = np.random.default_rng(100 * g + b)
    z, s = rng.standard_normal((g, b)), rng.standard_normal((b, b))
    got = run(4, z, s)
    err, bound = np.abs(got - z @ s).max(), 1e-13 * b * np.abs(z).max() * np.abs(s).max()
    print(f"panel g={g} b={b}: err {err:.2e} bound {bound:.2e}")
    assert got.shape == (g, b) and err <= bound


def check_panel_pair(run, g, b):
    """two panels by one factor in ONE launch (gridDim.y = 2): each against numpy under the bound of check_panel, and equal to the
    bit to the same product launched alone"""
    rng = np.random.default_rng(100 * g + b + 7)
    z0, z1, s = rng.standard_normal((g, b)), rng.standard_normal((g, b)), rng.standard_normal((b, b))
    c0, c1 = run(5, np.concatenate([z0, z1]), s)
    for z, got in ((z0, c0), (z1, c1)):
        err, bound = np.abs(got - z @ s).max(), 1e-13 * b * np.abs(z).max() * np.abs(s).max()
        print(f"panel pair g={g} b={b}: err {err:.2e} bound {bound:.2e}")
        assert got.shape == (g, b) and err <= bound
        assert np.array_equal(got, run(4, z, s))


def check_chol(run, b):
    rng = np.random.default_rng(b)
    z = rng.standard_normal((900, b)) * np.exp(rng.uniform(-3, 3, size=b))[None, :]  # badly scaled columns (test_cholqr_factor)
    s, bad = run(2, z.T @ z, None)
    assert bad == 0
    q = z @ s
    err = np.abs(q.T @ q - np.eye(b)).max()
    print(f"chol b={b}: |Q^T Q - I| {err:.2e}")
    assert err < 1e-10
    assert np.array_equal(s, np.triu(s))  # upper triangular to the bit: nothing below the diagonal
    if b >= 2:  # a singular Gram matrix is reported, not factorised (one column has no other to duplicate)
        z[:, -1] = z[:, 0]
        s2, bad = run(2, z.T @ z, None)
        # (a pivot of +1e-17 instead of -1e-17 "succeeds" with a factor of ~1e8: either way the caller sees it)
        assert bad == 1 or not np.isfinite(s2).all() or np.abs(s2).max() > 1e5


def jacobi_input(kind, b):
    rng = np.random.default_rng(b + 5)
    if kind == "random":  # test_jacobi_eigh
        m = rng.standard_normal((3 * b, b)) * np.exp(rng.uniform(-2, 2, size=b))[None, :]
        return m.T @ m
    if kind == "diagonal":  # no rotation fires; the order is not the sorted one
        return np.diag(rng.uniform(0.5, 50.0, size=b))
    if kind == "identity":
        return 3.25 * np.eye(b)
    # PSD of rank b / 2: half of the rotated columns end with a norm of ~1e-16 of the largest, and rotations between two such
    # columns are decided on rounding noise.  (Columns that are EXACTLY zero -- a zero block in T -- never rotate and come back as
    # zero vectors, the kernel's contract for theta = 0; no orthonormality bound applies to those, so this input has none.)
    r = max(b // 2, 1)
    m = rng.standard_normal((r, b))
    return m.T @ m


def jacobi_bounds(t, theta, y):
    """the four figures of tests/test_gpu_dense.py::test_jacobi_eigh, each divided by its bound (<= 1 passes)"""
    b = t.shape[0]
    ref = np.linalg.eigvalsh(t)[::-1]
    top = ref[0]
    return {"eigenvalues": np.abs(theta - ref).max() / (1e-12 * top),
            "orthonormal": np.abs(y.T @ y - np.eye(b)).max() / 1e-11,
            "residual": np.abs(t @ y - y * theta[None, :]).max() / (1e-11 * top),
            "descending": 0.0 if (np.diff(theta) <= 0).all() else np.inf}


def check_jacobi(run, kind, b):
    t = jacobi_input(kind, b)
    theta, y, sweeps = run(3, t, None)
    fig = jacobi_bounds(t, theta, y)
    print(f"jacobi {kind} b={b}: {sweeps} sweeps, figures / bounds {fig}")
    assert all(v < 1.0 for v in fig.values()), fig


def check_jacobi_symmetrised(run, b):
    """a T that is far from symmetric (an antisymmetric part of the size of the matrix): the kernel's load forms (T + T^T) / 2, the
    four bounds hold against THAT matrix -- they cannot if the load skips it -- and the result equals, to the bit, the plain solve
    of the matrix symmetrised on the host (0.5 * (a + b) is one rounding either way)"""
    rng = np.random.default_rng(b + 11)
    sym = jacobi_input("random", b)
    anti = rng.standard_normal((b, b)) * np.abs(sym).max()
    t = sym + (anti - anti.T)
    want = 0.5 * (t + t.T)
    theta, y, sweeps = run(6, t, None)
    fig = jacobi_bounds(want, theta, y)
    print(f"jacobi symmetrised b={b}: {sweeps} sweeps, figures / bounds {fig}")
    assert all(v < 1.0 for v in fig.values()), fig
    theta2, y2, _ = run(3, want, None)
    assert np.array_equal(theta, theta2) and np.array_equal(y, y2)
