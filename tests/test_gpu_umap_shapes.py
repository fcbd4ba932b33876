"""Every shape of the UMAP layout kernel (csrc/umap.hip: scamd_umap_optimize_f32) on the GPU, at kernel level: the tables, input
builders and checker of tests/pp_umap_kernel_cases.py, which tests/test_emu_pp_umap_shapes_cpu.py runs on the host emulator.
Reference: oracle/umap.c `oracle_umap_synchronous_f64` -- the kernel's own firing schedule (float32) and hash, forces and
embedding in double.  Bound per coordinate: 4 M (alpha 2^-23 sum|term| + 2^-24 |y|), M = the distance of the float32 CPU
restatement from the float64 one in that unit, measured per case on the CPU (profiles/pp_umap_shape_tolerances.log)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import pp_umap_kernel_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    import harness

    from scanpy_amd import _lib

    return harness.Abi(_lib.load(), P.DeviceMem())


@pytest.mark.parametrize("case", P.UMAP_CASES, ids=lambda c: "n{}-deg{}-dim{}-rate{}-ep{}-alpha{:g}".format(*c))
def test_umap_case(abi, case):
    """every lanes-per-vertex G x DIM instantiation, one to three batches of negatives, odd and even n_epochs, empty rows, entries
    that never fire, a vertex of degree 3 G + 1: within the bound of the float64 oracle, moved, bit-identical twice, another
    seed differs"""
    P.run_umap_case(abi, case, label="gpu")


def test_umap_beyond_the_grid_cap(abi):
    """G = 32, 8192 * 8 + 50 vertices of degree ~100: the last 50 vertices are a second grid-stride trip"""
    P.run_umap_case(abi, P.UMAP_GRID_CAP_CASE, label="gpu grid cap", determinism=False)


def test_umap_return_codes_and_fixed_points(abi):
    """dim 0 and 9: SCAMD_EUNSUPPORTED and a workspace size of 0; a workspace one byte short: SCAMD_EWORKSPACE; n_epochs = 0,
    nnz = 0, one epoch and n = 1 give y back bit for bit"""
    P.run_umap_edges(abi, label="gpu")
