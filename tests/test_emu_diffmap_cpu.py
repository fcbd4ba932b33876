"""The case table of tests/diffmap_cases.py on the HOST emulator (tests/emu/README.md): scamd_transitions_sym_f32,
scamd_diffmap_f32 and scamd_dpt_pseudotime_f32 through the raw C ABI -- the same cases and checkers as tests/test_gpu_diffmap.py.
The emulator does not share the accumulation order of the matrix cores; it does run the host drivers as they are."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import diffmap_cases as D  # noqa: E402


class EmuRunner:
    Refused = RuntimeError

    def __init__(self, harness, lib):
        self.H, self.lib = harness, lib

    @staticmethod
    def _csr(a):
        return (np.ascontiguousarray(a.indptr, dtype=np.int64), np.ascontiguousarray(a.indices, dtype=np.int32),
                np.ascontiguousarray(a.data, dtype=np.float32))

    def transitions(self, a, density_normalize):
        H, lib = self.H, self.lib
        n = a.shape[0]
        ip, ix, w = self._csr(a)
        t, z = np.full(a.nnz, np.nan, np.float32), np.full(n, np.nan)
        ws = H._ws(lib.scamd_transitions_sym_workspace_bytes(n, a.nnz))
        rc = lib.scamd_transitions_sym_f32(H._p(ip), H._p(ix), H._p(w), n, a.nnz, int(density_normalize), H._p(t), H._p(z), H._p(ws),
                                           ws.size, None)
        H._check(lib, rc, "transitions")
        return t, z

    def diffmap(self, t, k):
        from scanpy_amd import _lib

        H, lib = self.H, self.lib
        n = t.shape[0]
        ip, ix, w = self._csr(t)
        lam, v = np.full(k, np.nan), np.full((n, k), np.nan)
        info = np.zeros(_lib.DIFFMAP_INFO_WORDS)
        ws = H._ws(lib.scamd_diffmap_workspace_bytes(n, t.nnz, k))
        rc = lib.scamd_diffmap_f32(H._p(ip), H._p(ix), H._p(w), n, t.nnz, k, 0, D.TOL_SOLVER, 60, 64, H._p(lam), H._p(v),
                                   info.ctypes.data_as(C.POINTER(C.c_double)), H._p(ws), ws.size, None)
        refused = _lib.diffmap_guard_error(rc, info, k)
        if refused is not None:
            raise refused
        H._check(lib, rc, "diffmap")
        return lam, v, _lib.diffmap_info(info)

    def dpt(self, evals, basis, iroot, labels, scale):
        H, lib = self.H, self.lib
        evals, basis = np.ascontiguousarray(evals, np.float32), np.ascontiguousarray(basis, np.float32)
        n, ld = basis.shape
        lab = None if labels is None else np.ascontiguousarray(labels, np.int32)
        out = np.full(n, np.nan, np.float32)
        ws = H._ws(lib.scamd_dpt_pseudotime_workspace_bytes(n))
        rc = lib.scamd_dpt_pseudotime_f32(H._p(evals), H._p(basis), n, evals.size, ld, iroot, H._p(lab), int(scale), H._p(out), H._p(ws), ws.size, None)
        H._check(lib, rc, "dpt")
        return out


@pytest.fixture(scope="module")
def run():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    return EmuRunner(harness, harness.load())


@pytest.mark.parametrize("name,density_normalize", D.TRANSITION_CASES)
def test_transitions(run, name, density_normalize):
    D.run_transitions_case(run, name, density_normalize, label="emulator")


@pytest.mark.parametrize("name,k", D.EIGEN_CASES)
def test_eigen(run, name, k):
    D.run_eigen_case(run, name, k, label="emulator")


def test_eigen_refusals(run):
    D.run_eigen_refusals(run)


def test_even_ring_is_refused_by_the_guard(run):
    D.run_even_ring(run, label="emulator")


@pytest.mark.parametrize("name,n_dcs,root", D.DPT_CASES)
def test_pseudotime(run, name, n_dcs, root):
    D.run_dpt_case(run, name, n_dcs, root, label="emulator")

