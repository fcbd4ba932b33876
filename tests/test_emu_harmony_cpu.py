"""The case table of tests/harmony_cases.py on the HOST emulator (tests/emu/README.md): the five Harmony entry points through the
raw C ABI -- the same cases and checkers as tests/test_gpu_harmony.py.  The emulator runs the host drivers and the kernels'
indexing as they are; the order of its integer sums differs from the device's, their result does not."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import harmony_cases as H  # noqa: E402


class Refused(RuntimeError):
    def __init__(self, msg, outputs):
        super().__init__(msg)
        self.outputs = outputs


class EmuRunner:
    Refused = Refused

    def __init__(self, harness, lib):
        self.H, self.lib = harness, lib

    def _check(self, rc, what, **outputs):
        if rc != 0:
            raise Refused(f"{what}: rc={rc}: {self.lib.scamd_last_error().decode()}", outputs)

    @staticmethod
    def _f64(a):
        return np.ascontiguousarray(a, dtype=np.float64)

    def permutation(self, n, seed, rnd):
        p = self.H._p
        perm = np.full(n, -1, np.int32)
        self._check(self.lib.scamd_harmony_permutation_i32(n, seed, rnd, p(perm), None, 0, None), "permutation")
        return perm

    def kmeans(self, z, K, uniforms, max_iter):
        p, lib = self.H._p, self.lib
        z = self._f64(z)
        n, d = z.shape
        u = self._f64(uniforms)
        cen, lab, it = np.full((K, d), np.nan), np.full(n, -7, np.int32), C.c_int(-1)
        ws = self.H._ws(lib.scamd_harmony_kmeans_workspace_bytes(n, d, K))
        rc = lib.scamd_harmony_kmeans_f64(p(z), n, d, K, u.ctypes.data_as(C.POINTER(C.c_double)), max_iter, p(cen), p(lab), C.byref(it), p(ws),
                                          ws.size, None)
        self._check(rc, "kmeans")
        return cen, lab, it.value

    def init(self, z, codes, B, centroids, pr_b, theta, sigma, stab, n_covariates=1):
        p, lib = self.H._p, self.lib
        z, cen, pr_b, theta = map(self._f64, (z, centroids, pr_b, theta))
        n, d = z.shape
        K = cen.shape[0]
        r, e, o, obj = np.full((n, K), np.nan), np.full((B, K), np.nan), np.full((B, K), np.nan), np.full(4, np.nan)
        ws = self.H._ws(lib.scamd_harmony_state_workspace_bytes(n, d, K, B))
        rc = lib.scamd_harmony_init_f64(p(z), p(codes), n, d, K, B, n_covariates, p(cen), p(pr_b), p(theta), sigma, int(stab), p(r), p(e), p(o),
                                        p(obj), p(ws), ws.size, None)
        self._check(rc, "init", R=r)
        return r, e, o, obj

    def cluster_round(self, z, codes, B, perm, n_blocks, pr_b, theta, sigma, stab, r, e, o, n_covariates=1):
        p, lib = self.H._p, self.lib
        z, pr_b, theta = map(self._f64, (z, pr_b, theta))
        r, e, o = (np.array(a, np.float64, order="C", copy=True) for a in (r, e, o))
        perm = np.ascontiguousarray(perm, np.int32)
        n, d = z.shape
        K = r.shape[1]
        y, obj = np.full((K, d), np.nan), np.full(4, np.nan)
        ws = self.H._ws(lib.scamd_harmony_state_workspace_bytes(n, d, K, B))
        rc = lib.scamd_harmony_cluster_round_f64(p(z), p(codes), n, d, K, B, n_covariates, p(perm), n_blocks, p(pr_b), p(theta), sigma, int(stab),
                                                 p(r), p(e), p(o), p(y), p(obj), p(ws), ws.size, None)
        self._check(rc, "cluster_round")
        return r, e, o, y, obj

    def correct(self, x, codes, B, r, o, e, n_b, dynamic, alpha, threshold, ridge, n_covariates=1):
        p, lib = self.H._p, self.lib
        x, r, o, e, n_b = map(self._f64, (x, r, o, e, n_b))
        n, d = x.shape
        K = r.shape[1]
        z_hat, z_norm, lam = np.full((n, d), np.nan), np.full((n, d), np.nan), np.full((B, K), np.nan)
        ws = self.H._ws(lib.scamd_harmony_correct_workspace_bytes(n, d, K, B))
        rc = lib.scamd_harmony_correct_f64(p(x), p(codes), n, d, K, B, n_covariates, p(r), p(o), p(e), p(n_b), int(dynamic), alpha,
                                           -1.0 if threshold is None else threshold, ridge, p(z_hat), p(z_norm), p(lam), p(ws), ws.size, None)
        self._check(rc, "correct", z_hat=z_hat)
        return z_hat, z_norm, lam


@pytest.fixture(scope="module")
def run():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    return EmuRunner(harness, harness.load())


@pytest.mark.parametrize("n", H.PERM_SIZES)
def test_permutation(run, n):
    H.run_permutation_case(run, n)


@pytest.mark.parametrize("n,d,K", H.KMEANS_CASES)
def test_kmeans(run, n, d, K):
    H.run_kmeans_case(run, n, d, K, label="emulator")


@pytest.mark.parametrize("name", list(H.STATE_CASES))
def test_init_and_rounds(run, name):
    H.run_state_case(run, name, label="emulator")


@pytest.mark.parametrize("name", list(H.CORRECT_CASES))
def test_correction(run, name):
    H.run_correct_case(run, name, label="emulator")


@pytest.mark.parametrize("what", [r[0] for r in H.REFUSALS])
def test_refusals(run, what):
    H.run_refusal(run, what)
