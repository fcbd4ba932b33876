"""The shape tables of tests/dense_shape_cases.py on the HOST emulator (tests/emu/README.md): the four float64 kernels of the
dense solve through `scamd_dense_debug_f64`, the same cases and checkers as tests/test_gpu_dense_shapes.py.  The emulator runs
the kernels lane by lane with every index checked by the host's memory, so it says whether the clamped loads, the batch tails
and the per-lane element counts are right at every shape; the accumulation order inside an MFMA is its own."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import dense_shape_cases as D  # noqa: E402


@pytest.fixture(scope="module")
def run():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    before = harness.stats(lib)

    def call(op, in0, in1):
        in0 = np.ascontiguousarray(in0, dtype=np.float64)
        in1 = None if in1 is None else np.ascontiguousarray(in1, dtype=np.float64)
        flag = C.c_int32(-1)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)  # noqa: E731
        if op == 1:
            (kdim, m), n = in0.shape, in1.shape[1]
            out0, out1 = np.full((m, n), np.nan), None
        elif op == 4:
            (m, kdim), n = in0.shape, in1.shape[1]
            out0, out1 = np.full((m, n), np.nan), None
        elif op == 5:
            m, kdim, n = in0.shape[0] // 2, in0.shape[1], in1.shape[1]
            out0, out1 = np.full((m, n), np.nan), np.full((m, n), np.nan)
        else:
            m = n = kdim = in0.shape[0]
            out0, out1 = np.full((m, m) if op == 2 else (m,), np.nan), np.full((m, m), np.nan)
        rc = lib.scamd_dense_debug_f64(op, ptr(in0), ptr(in1), m, n, kdim, ptr(out0), ptr(out1), C.byref(flag), None)
        assert rc == 0, lib.scamd_last_error().decode()
        return out0 if op in (1, 4) else (out0, out1) if op == 5 else (out0, int(flag.value)) if op == 2 else (out0, out1, int(flag.value))

    yield call
    after = harness.stats(lib)
    # (not `partial_collectives`: the groups of a Jacobi wave that have no pair in a step sit out its DPP sums by design)
    for key in ("mixed_collectives", "reads_of_inactive_lanes"):
        assert after[key] == before[key], f"{key}: {before[key]} -> {after[key]}"


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
