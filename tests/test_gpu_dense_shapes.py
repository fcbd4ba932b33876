"""Every shape of the four float64 kernels of the dense solve (csrc/dense.hip: the MFMA GEMM with batched operand loads, the
panel product with its factor staged in LDS, the Cholesky factor, the one-workgroup Jacobi) on the device, through
`scanpy_amd._kernels.dense_debug`: the tables and checkers of tests/dense_shape_cases.py, which the host emulator runs as well
(tests/test_emu_dense_shapes_cpu.py).  The shapes are the smallest at which each code path exists, not the workload's."""
from __future__ import annotations

import numpy as np
import pytest

import dense_shape_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import torch

    from scanpy_amd import _kernels as K

    def call(op, in0, in1):
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
        out = K.dense_debug(op, dev(in0), dev(in1))
        if op in (1, 4):
            return out.cpu().numpy()
        return tuple(o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out)

    return call


@pytest.mark.parametrize(("kdim", "m", "n"), D.GEMM_CASES)
def test_gemm(run, kdim, m, n):
    D.check_gemm(run, kdim, m, n)


@pytest.mark.parametrize(("g", "b"), D.PANEL_CASES)
def test_panel_product(run, g, b):
    D.check_panel(run, g, b)


@pytest.mark.parametrize("b", D.CHOL_SIZES)
def test_cholesky_factor(run, b):
    D.check_chol(run, b)


@pytest.mark.parametrize("b", D.JACOBI_SIZES)
def test_jacobi(run, b):
    D.check_jacobi(run, "random", b)


@pytest.mark.parametrize(("kind", "b"), D.JACOBI_SPECIAL)
def test_jacobi_special_input(run, kind, b):
    D.check_jacobi(run, kind, b)


@pytest.mark.parametrize(("g", "b"), D.PANEL_PAIR_CASES)
def test_panel_pair_in_one_launch(run, g, b):
    D.check_panel_pair(run, g, b)


@pytest.mark.parametrize("b", D.JACOBI_SYMMETRISED_SIZES)
def test_jacobi_symmetrises_on_load(run, b):
    D.check_jacobi_symmetrised(run, b)
