"""Every shape of the sparse half of PCA (csrc/pca.hip: scamd_spmm_csr_f32, scamd_spmm_csr_f32_f64acc, scamd_colsum_f32_f64,
scamd_csr_transpose_f32, scamd_csr_row_stats_f32) on the GPU, at kernel level: the tables, input builders and checkers of
tests/graph_kernel_cases.py, which tests/test_emu_graph_shapes_cpu.py runs on the host emulator.  Every output element is
compared with a float64 (or wider) reference under a derived per-element bound; outputs are prefilled with NaN, so an
element no lane wrote fails.  What only the hardware can say: the 160 KB of dynamic LDS of the transpose at g = 40944."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import graph_kernel_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    import harness

    from scanpy_amd import _lib

    return harness.Abi(_lib.load(), G.DeviceMem())


@pytest.mark.parametrize("l", G.SPMM_L)
def test_spmm_case(abi, l):
    """rows of 0 .. 200 entries around the chunk (64) and unroll (8, 16) boundaries, with and without `shift`: every column
    within (len + 2) 2^-24 (sum |a||b| + |shift|), two calls bit-identical"""
    G.run_spmm_case(abi, l, second_trip=False, label="gpu")


@pytest.mark.parametrize("l", G.SPMM_SECOND_TRIP_L)
def test_spmm_second_grid_stride_trip(abi, l):
    """n > 32768: the grid is capped and waves take a second row, whose extent they prefetched"""
    G.run_spmm_case(abi, l, second_trip=True, label="gpu")


@pytest.mark.parametrize("l", G.F64ACC_L)
def test_spmm_f64acc_case(abi, l):
    """rows at 2047 / 2048 / 2049 / 4096 / 4097 entries (segments of 2048), with and without scale x colsum"""
    G.run_f64acc_case(abi, l, label="gpu")


@pytest.mark.parametrize("l", G.COLSUM_L)
def test_colsum_cases(abi, l):
    worst = max(G.run_colsum_case(abi, n, l, label="gpu") for n in G.COLSUM_N)
    print(f"gpu colsum l={l}: worst error / bound = {worst:.3f}")


def test_row_stats_case(abi):
    G.run_row_stats_case(abi, label="gpu")


@pytest.mark.parametrize(("n", "g", "per_row"), G.TRANSPOSE_CASES)
def test_transpose_case(abi, n, g, per_row):
    """g = 40944 (160 KB of LDS), 64 / 65 chunks, rows_per_chunk = 512: equal to scipy's sorted CSC"""
    G.run_transpose_case(abi, n, g, per_row, label="gpu")


def test_sparse_pca_argument_checks(abi):
    """l = 0, l = 257, l = 129 (f64acc) -> SCAMD_EINVAL; g = 40945 -> SCAMD_EUNSUPPORTED"""
    G.run_spmm_argument_checks(abi)
