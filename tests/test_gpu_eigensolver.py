"""The case table of tests/eigensolver_cases.py on the GPU, through scanpy_amd/_kernels.py: every path of the Chebyshev-filtered
subspace iteration of csrc/subspace.h under both of its operators, at the smallest shapes at which the path exists.  The
workload-sized checks are tests/test_gpu_dense.py::test_eigh_topk and the 30k-vertex sheet of tests/test_gpu_umap.py."""
from __future__ import annotations

import numpy as np
import pytest

import eigensolver_cases as E

pytestmark = pytest.mark.gpu


class GpuRunner:
    def __init__(self):
        import torch

        from scanpy_amd import _kernels
        from scanpy_amd._lib import ScamdError

        self.torch, self.K, self.Refused = torch, _kernels, ScamdError

    def _dev(self, a, dtype):
        return self.torch.from_numpy(np.array(a, dtype=dtype, order="C", copy=True)).cuda()

    def eigh_topk(self, a, k):
        lam, v, info = self.K.eigh_topk(self._dev(a, np.float64), k, tol=E.TOL_DENSE)
        return lam.cpu().numpy(), v.cpu().numpy(), info

    def pca_csr(self, x, k):
        n, g = x.shape
        out = self.K.pca_csr(self._dev(x.indptr, np.int64), self._dev(x.indices, np.int32), self._dev(x.data, np.float32), n, g, k,
                             tol=E.TOL_DENSE)
        got = {key: t.cpu().numpy() for key, t in zip(("scores", "components", "variance", "variance_ratio", "mean"), out)}
        got["info"] = {key: out[5][key] for key in ("n_outer", "n_gemm", "block_size", "chol_retries", "residual")}
        return got

    def spectral_embedding(self, a, dim):
        v, info = self.K.spectral_embedding(self._dev(a.indptr, np.int64), self._dev(a.indices, np.int32), self._dev(a.data, np.float32),
                                            a.shape[0], dim, tol=E.TOL_SPECTRAL)
        return v.cpu().numpy(), info


@pytest.fixture(scope="module")
def run():
    return GpuRunner()


@pytest.mark.parametrize("name", list(E.DENSE_CASES))
def test_dense_case(run, name):
    E.run_dense_case(run, name, label="gpu")


def test_eigh_topk_unsupported_shapes(run):
    E.run_refusals(run)


def test_two_batches(run):
    E.run_two_batches(run, label="gpu")


@pytest.mark.parametrize("name", list(E.SPECTRAL_CASES))
def test_spectral_case(run, name):
    E.run_spectral_case(run, name, label="gpu")
