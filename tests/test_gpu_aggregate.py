"""`sc.get.aggregate` on the GPU.  Kernel level: the case table of tests/aggregate_cases.py through the product library (the same
cases and the same checker tests/test_emu_aggregate_cpu.py runs on the host emulator); what only the hardware can say: the
64-bit LDS and global integer adds of parts that run at the same time, the shuffles of the in-wave median, two runs and a
permutation of the rows giving the same bits.  Front end: the pbmc68k comparison with pandas of
tests/test_aggregate_front_cpu.py end to end on the device."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import aggregate_cases as A  # noqa: E402

import scanpy_amd as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from scanpy_amd import _lib

    return A.AggregateAbi(_lib.load(), A.DeviceMem())


def test_library_states_the_same_rules(abi):
    A.assert_library_agrees(abi.lib)


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_every_case(abi, name):
    """the two counts and the median (mid_in_f32 on and off) exactly, sum and m2 within the bounds the header states, nothing
    written beyond [n_groups x g]; the determinism cases bit-identical on a second run and with the rows permuted"""
    cs, got, out = A.run_case(abi, name, label="gpu")
    A.check_case_specifics(name, cs, got, out)


def test_nonfinite_values_are_flagged_and_stay_in_their_pair(abi):
    A.run_nan_case(abi, label="gpu")


def test_argument_checks(abi):
    A.run_argument_checks(abi)


@pytest.mark.parametrize("source", ["raw_csr", "raw_csc", "dense_X"])
@pytest.mark.parametrize("use_mask", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("with_na", [True, False], ids=["na", "no_na"])
def test_front_pbmc68k_against_pandas(pbmc68k, source, use_mask, with_na):
    A.front_vs_pandas(pbmc68k, source, use_mask, with_na)


def test_front_routes_agree_bit_for_bit_and_refuse_nonfinite(pbmc68k):
    """CSR, CSC (the device transpose) and the dense full pattern of one matrix give the same bits on either axis"""
    raw = pbmc68k["raw_X"]
    obs = pd.DataFrame({"louvain": pd.Categorical(pbmc68k["louvain_codes"])}, index=[f"cell{i}" for i in range(raw.shape[0])])
    funcs = ["sum", "var", "count_nonzero", "median"]
    runs = {name: sc.get.aggregate(sc.AnnData(m, obs=obs), "louvain", funcs).layers
            for name, m in (("csr", raw), ("csc", raw.tocsc()), ("dense", raw.toarray()))}
    for f in funcs:
        for name in ("csc", "dense"):
            assert np.array_equal(np.asarray(runs[name][f], dtype=np.float64), np.asarray(runs["csr"][f], dtype=np.float64)), (name, f)
    t = sc.AnnData(raw.T.tocsr(), var=obs)
    by_var = sc.get.aggregate(t, "louvain", funcs, axis="var").layers
    for f in funcs:
        assert np.array_equal(by_var[f].T, runs["csr"][f]), f
    bad = raw.copy()
    bad.data[17] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        sc.get.aggregate(sc.AnnData(bad, obs=obs), "louvain", "sum")
