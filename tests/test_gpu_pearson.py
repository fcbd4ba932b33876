"""`sc.experimental.pp` on the GPU.  Kernel level: the case table of tests/pearson_cases.py through the product library (the same
cases and the same checker tests/test_emu_pearson_cpu.py runs on the host emulator); what only the hardware can say: the
workgroups of one gene running at the same time, the device's float64 division and square root inside the stated bounds, the
16-byte stores of the residual matrix between their guard words, two runs and a permutation of the rows giving the same bits.
Front end: the bodies of tests/test_pearson_front_cpu.py end to end on the device."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import pearson_cases as P  # noqa: E402
import test_pearson_front_cpu as F  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from scanpy_amd import _lib

    return P.PearsonAbi(_lib.load(), P.DeviceMem())


def test_library_states_the_same_constants(abi):
    P.assert_library_agrees(abi.lib)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_every_case(abi, name):
    """the gene variance of every batch within the derived bound (collapsed totals and the plain sweep), NaN and 0 where the
    reference has them, the residual matrix within its tolerance in both output types between untouched guard words; the
    determinism cases bit-identical on a second run and, for the variance, with the rows permuted"""
    P.run_case(abi, name, label="gpu")


def test_argument_checks(abi):
    P.run_argument_checks(abi)


def test_worst_observed_ratios_stay_below_one(abi):
    """(runs after the table: prints what DESIGN.md 3.15 records)"""
    print("worst observed error / bound on the GPU:", P.worst)
    assert P.worst["var"] <= 1.0 and P.worst["resid64"] <= 1.0


@pytest.mark.parametrize("theta", [100, np.inf])
@pytest.mark.parametrize("clip", [None, np.inf, 30])
def test_front_general(theta, clip):
    F.check_general(theta, clip)


def test_front_batch_subset_layer():
    F.check_batch()
    F.check_batch(theta=np.inf, clip=30)
    F.check_subset_inplace_layer()


def test_front_formats_and_dtypes_give_the_same_bits():
    F.check_formats_give_the_same_bits()


@pytest.mark.parametrize(("theta", "clip", "dtype", "out_dtype"), [(100, None, np.float32, np.float32), (100, None, np.int64, np.float64),
                                                                   (np.inf, np.inf, np.float64, np.float64), (np.inf, 3.0, np.float32, np.float32)])
def test_front_normalize(theta, clip, dtype, out_dtype):
    F.check_normalize(theta, clip, dtype, out_dtype)


def test_front_pca_and_recipe():
    F.check_pca_and_recipe()


def test_front_pbmc68k_noninteger_warning(pbmc68k):
    F.check_pbmc68k_warns(pbmc68k)
