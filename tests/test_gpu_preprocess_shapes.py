"""Every shape of the normalisation-chain kernels (csrc/preprocess.hip: the eight scamd_pp_* row-wise entry points and
scamd_pp_log1p_f32) on the GPU, at kernel level: the tables, input builders and checkers of tests/pp_umap_kernel_cases.py, which
tests/test_emu_pp_umap_shapes_cpu.py runs on the host emulator.  What only the hardware can say: whether the column table of
more than 64 KB of dynamic LDS (3277 <= g <= 4096) is granted, the float64 LDS atomics under contention, the grid-stride trips
beyond the grid caps, and log1pf / expm1f of the device library."""
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


@pytest.mark.parametrize(("n", "avg"), P.PP_ROW_CASES)
def test_row_wise_kernels_at_every_lane_count(abi, n, avg):
    """one matrix per side of each threshold of lanes_per_row (rows of 0, 1, G - 1, G, G + 1, 4 G - 1, 4 G, 4 G + 1 entries, one of
    three times the mean, empty rows at both ends and in the middle, an all-zero row): row sums, highly-expressed counts and
    positive counts exact, row divide within one float32 rounding, column statistics (both tables, masked, expm1, clipped) and
    both scalings (CSR; dense float64 and float32) at the tolerances of tests/test_gpu_preprocess.py"""
    P.run_pp_row_case(abi, n, avg, label="gpu")


@pytest.mark.parametrize("g", P.PP_COL_TABLE_G)
def test_column_table_at_its_boundaries(abi, g):
    """g = 3276 is the last table within 64 KB of LDS, 3277 .. 4096 take up to 81 936 B, 4097 is the first in global memory; one
    column receives every row, some receive none and stay exactly 0"""
    P.run_pp_col_table_case(abi, g, label="gpu")


def test_row_wise_kernels_beyond_their_grid_caps(abi):
    """8192 * 32 + 40 mostly empty rows at G = 8: every row-wise kernel takes a second grid-stride trip, the LDS column
    statistics run past their 512 blocks"""
    P.run_pp_grid_cap_case(abi, label="gpu grid cap")


def test_dense_scale_beyond_the_fill_grid(abi):
    """1100 x 4000: the fill kernel strides; float64 and float32 output, masked rows keep their stored values, clipping at +-4"""
    P.run_pp_dense_cap_case(abi, label="gpu 1100x4000")


@pytest.mark.parametrize("offset", P.PP_LOG1P_OFFSETS)
def test_log1p_head_body_tail(abi, offset):
    """counts 0..9, 255..260, 1024..1027 at a pointer `offset` elements past a 16-byte boundary, natural log and bases 2 and 10;
    the elements before and after the range keep their bytes"""
    P.run_pp_log1p_cases(abi, offset, label="gpu")


def test_log1p_beyond_its_grid_cap(abi):
    P.check_log1p(abi, P.PP_LOG1P_GRID_CAP_COUNT, 1, 2.0, label="gpu grid cap")


def test_preprocess_argument_checks(abi):
    """NULL indptr, negative sizes, g = 2^31, transform = 2, base 1 and -2: SCAMD_EINVAL; n = 0 and g = 0: OK, nothing written"""
    P.run_pp_argument_checks(abi)
