"""The case table of tests/harmony_cases.py on the GPU, through scanpy_amd/_kernels.py: the keyed permutation, the k-means
initialisation, the first responsibilities, clustering rounds and the correction of `pp.harmony_integrate`, at the smallest
shapes at which each kernel can still go wrong, and the refusals."""
from __future__ import annotations

import numpy as np
import pytest

import harmony_cases as H

pytestmark = pytest.mark.gpu


class Refused(RuntimeError):
    def __init__(self, msg, outputs):
        super().__init__(msg)
        self.outputs = outputs


class GpuRunner:
    Refused = Refused

    def __init__(self):
        import torch

        from scanpy_amd import _kernels, _lib
        from scanpy_amd._device import ptr, stream_ptr

        self.torch, self.K, self.lib, self.ptr, self.stream = torch, _kernels, _lib.load(), ptr, stream_ptr
        self.Error = _lib.ScamdError

    def _dev(self, a, dtype=np.float64):
        return self.torch.from_numpy(np.array(a, dtype=dtype, order="C", copy=True)).cuda()

    def _nan(self, *shape):
        return self._dev(np.full(shape, np.nan))

    def permutation(self, n, seed, rnd):
        return self.K.harmony_permutation(n, seed, rnd).cpu().numpy()

    def kmeans(self, z, K, uniforms, max_iter):
        try:
            cen, lab, it = self.K.harmony_kmeans(self._dev(z), K, uniforms, max_iter=max_iter)
        except self.Error as e:
            raise Refused(str(e), {}) from e
        return cen.cpu().numpy(), lab.cpu().numpy(), it

    def init(self, z, codes, B, centroids, pr_b, theta, sigma, stab, n_covariates=1):
        z, codes, cen, pr_b, theta = self._dev(z), self._dev(codes, np.int32), self._dev(centroids), self._dev(pr_b), self._dev(theta)
        try:
            out = self.K.harmony_init(z, codes, B, cen, pr_b, theta, sigma, stab, n_covariates=n_covariates)
        except self.Error as e:
            # the same call on outputs of our own, filled with NaN: a refused call writes nothing
            n, d, k = z.shape[0], z.shape[1], cen.shape[0]
            r, t1, t2, obj = self._nan(n, k), self._nan(B, k), self._nan(B, k), self._nan(4)
            p = self.ptr
            rc = self.lib.scamd_harmony_init_f64(p(z), p(codes), n, d, k, B, n_covariates, p(cen), p(pr_b), p(theta), sigma, int(stab), p(r), p(t1),
                                                 p(t2), p(obj), None, 0, self.stream())
            assert rc != 0
            self.torch.cuda.synchronize()
            raise Refused(str(e), {"R": r.cpu().numpy()}) from e
        return tuple(t.cpu().numpy() for t in out)

    def cluster_round(self, z, codes, B, perm, n_blocks, pr_b, theta, sigma, stab, r, e, o, n_covariates=1):
        r, e, o = self._dev(r), self._dev(e), self._dev(o)
        y, obj = self._nan(r.shape[1], z.shape[1]), self._nan(4)
        try:
            self.K.harmony_cluster_round_(self._dev(z), self._dev(codes, np.int32), B, self._dev(perm, np.int32), n_blocks, self._dev(pr_b),
                                          self._dev(theta), sigma, stab, r, e, o, y, obj, n_covariates=n_covariates)
        except self.Error as err:
            raise Refused(str(err), {}) from err
        return tuple(t.cpu().numpy() for t in (r, e, o, y, obj))

    def correct(self, x, codes, B, r, o, e, n_b, dynamic, alpha, threshold, ridge, n_covariates=1):
        x, codes, r, o, e, n_b = self._dev(x), self._dev(codes, np.int32), self._dev(r), self._dev(o), self._dev(e), self._dev(n_b)
        try:
            out = self.K.harmony_correct(x, codes, B, r, o, e, n_b, dynamic_lambda=dynamic, alpha=alpha, batch_prune_threshold=threshold,
                                         ridge_lambda=ridge, want_lambda=True, n_covariates=n_covariates)
        except self.Error as err:
            n, d, k = x.shape[0], x.shape[1], r.shape[1]
            z_hat, z_norm = self._nan(n, d), self._nan(n, d)
            p = self.ptr
            rc = self.lib.scamd_harmony_correct_f64(p(x), p(codes), n, d, k, B, n_covariates, p(r), p(o), p(e), p(n_b), int(dynamic), alpha,
                                                    -1.0 if threshold is None else threshold, ridge, p(z_hat), p(z_norm), None, None, 0,
                                                    self.stream())
            assert rc != 0
            self.torch.cuda.synchronize()
            raise Refused(str(err), {"z_hat": z_hat.cpu().numpy()}) from err
        return tuple(t.cpu().numpy() for t in out)


@pytest.fixture(scope="module")
def run():
    return GpuRunner()


@pytest.mark.parametrize("n", H.PERM_SIZES)
def test_permutation(run, n):
    H.run_permutation_case(run, n)


@pytest.mark.parametrize("n,d,K", H.KMEANS_CASES)
def test_kmeans(run, n, d, K):
    H.run_kmeans_case(run, n, d, K, label="gpu")


@pytest.mark.parametrize("name", list(H.STATE_CASES))
def test_init_and_rounds(run, name):
    H.run_state_case(run, name, label="gpu")


@pytest.mark.parametrize("name", list(H.CORRECT_CASES))
def test_correction(run, name):
    H.run_correct_case(run, name, label="gpu")


@pytest.mark.parametrize("what", [r[0] for r in H.REFUSALS])
def test_refusals(run, what):
    H.run_refusal(run, what)
