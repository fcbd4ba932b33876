"""`sc.pp.regress_out` on the GPU.  Kernel level: the case table of tests/regress_cases.py through the product library (the same
cases and the same checker tests/test_emu_regress_cpu.py runs on the host emulator); what only the hardware can say: the 64-bit
integer atomics in LDS and in global memory behind the order-independent sums, the 16-byte store path, two runs giving the
same bits on genes shared by many workgroups.  Front end: the reference's two golden outputs on pbmc68k_reduced through
`sc.pp.regress_out` on an AnnData."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import regress_cases as R  # noqa: E402

import scanpy_amd as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rabi():
    from scanpy_amd import _lib

    return R.RegressAbi(_lib.load(), R.DeviceMem())


@pytest.fixture(scope="module")
def pbmc_obs(tmp_path_factory):
    return R.pbmc68k_obs(tmp_path_factory.mktemp("pbmc68k"))


@pytest.mark.parametrize("name", [n for n in R.CASE_NAMES if n not in R.DETERMINISM_CASES])
def test_sums_and_residual_on_every_case(rabi, name):
    """the range with implicit zeros exactly, the fixed-point sums within their stated bound, the residual with and without the
    constant-gene rule within ulp_out / 2 + 1e-9 max|x_j| of the float64 restatement, every element written"""
    R.run_case(rabi, name, label="gpu")


@pytest.mark.parametrize("name", R.DETERMINISM_CASES)
def test_two_runs_are_bit_identical(rabi, name):
    """n = 5000, g = 40: every gene's sum is added to by many workgroups; one numeric, one categorical"""
    R.run_case(rabi, name, label="gpu", rerun=True)


def test_nonfinite_values_and_bad_codes_raise_their_flags(rabi):
    R.run_nonfinite_case(rabi, label="gpu")


def test_argument_checks(rabi):
    R.run_argument_checks(rabi)


def test_numeric_golden_pipeline(pbmc68k, pbmc_obs):
    a = R.golden_adata(pbmc68k["raw_X"], pbmc_obs)
    sc.pp.regress_out(a, ["n_counts", "percent_mito"])
    R.assert_matches_numeric_golden(a.X)
    b = R.golden_adata(pbmc68k["raw_X"], pbmc_obs)
    b.X = b.X.toarray()
    sc.pp.regress_out(b, ["n_counts", "percent_mito"])
    assert a.X.tobytes() == b.X.tobytes()   # sparse and dense input: the same bits


def test_categorical_golden_pipeline(pbmc68k, pbmc_obs):
    a = R.golden_adata(pbmc68k["raw_X"], pbmc_obs)
    sc.pp.regress_out(a, "bulk_labels")
    R.assert_matches_categorical_golden(a.X)
    dense = pbmc68k["raw_X"][:200, :200].toarray().astype(np.float64)
    want = R.ref_categorical(dense, a.obs["bulk_labels"].cat.codes.to_numpy(), len(a.obs["bulk_labels"].cat.categories))
    R.assert_residual_close(a.X, want, np.abs(dense).max(axis=0), "bulk_labels")
