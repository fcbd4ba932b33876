"""The case table of tests/eigensolver_cases.py on the HOST emulator (tests/emu/README.md): every path of the Chebyshev-filtered
subspace iteration of csrc/subspace.h under both of its operators -- the same cases, checkers and counters as
tests/test_gpu_eigensolver.py.  The emulator does not share the accumulation order of the float64 matrix cores; it does run the
host drivers as they are, so it says whether the panels, the read-backs and the counters of every branch are right."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import eigensolver_cases as E  # noqa: E402


class EmuRunner:
    Refused = RuntimeError

    def __init__(self, harness, lib):
        self.H, self.lib = harness, lib

    def eigh_topk(self, a, k):
        return self.H.eigh_topk(self.lib, a, k, tol=E.TOL_DENSE)[:3]

    def pca_csr(self, x, k):
        out = self.H.pca_csr(self.lib, x, k, tol=E.TOL_DENSE)
        out["info"] = self.H.dense_info(out["info"])
        return out

    def spectral_embedding(self, a, dim):
        return self.H.spectral_embedding(self.lib, a, dim, tol=E.TOL_SPECTRAL)[:2]


@pytest.fixture(scope="module")
def run():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    return EmuRunner(harness, harness.load())


@pytest.mark.parametrize("name", list(E.DENSE_CASES))
def test_dense_case(run, name):
    E.run_dense_case(run, name, label="emulator")


def test_eigh_topk_unsupported_shapes(run):
    E.run_refusals(run)


def test_two_batches(run):
    E.run_two_batches(run, label="emulator")


@pytest.mark.parametrize("name", list(E.SPECTRAL_CASES))
def test_spectral_case(run, name):
    E.run_spectral_case(run, name, label="emulator")
