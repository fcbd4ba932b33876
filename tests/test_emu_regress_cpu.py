"""The case table of tests/regress_cases.py on the HOST emulator (tests/emu/README.md): the kernels of csrc/regress.hip
(`scamd_pp_regress_sums_f32`, `scamd_pp_regress_resid_f32`), the same cases and the same checker as tests/test_gpu_regress_out.py.
The emulator says nothing about the hardware's 64-bit integer atomics or its store path; it does say whether every instantiation
indexes, stages, scales and rounds correctly.  Also here, needing neither GPU nor emulator: every (lanes per row, range table,
sums table) of the sweeps and every (threads per row, model, output type) of the residual kernel has a case, and the rules'
constants still stand in the source.

The kernels use no cross-lane operation and their loops are uniform over the workgroup: `partial_collectives`,
`mixed_collectives` and `reads_of_inactive_lanes` all stay 0."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import regress_cases as R  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, R.RegressAbi(lib, harness.HostMem())


def _only_full_waves(H, lib, what):
    st = H.stats(lib)
    assert st["partial_collectives"] == st["mixed_collectives"] == st["reads_of_inactive_lanes"] == 0, (what, st)


def test_table_covers_every_instantiation_and_branch():
    """no GPU, no emulator"""
    sweeps, resids = R.assert_every_regress_path_has_a_case()
    assert {G for G, _, _ in sweeps} == {8, 16, 32, 64} and {t for t, _, _ in resids} == {256, 128, 64}
    assert [R.sweep_lanes(a * 100, 100) for a in (0, 32, 33, 160, 161, 512, 513)] == [8, 8, 16, 16, 32, 32, 64]
    assert (R.range_table(2048), R.range_table(2049)) == ("lds", "global")
    assert (R.sums_table(3, 2048), R.sums_table(3, 2049), R.sums_table(17, 361), R.sums_table(17, 362)) == ("lds", "global", "lds", "global")
    assert [R.resid_threads(m, False) for m in (1, 4, 5, 8, 9, 17)] == [256, 256, 128, 128, 64, 64] and R.resid_threads(1000, True) == 256


def test_sources_still_say_what_the_table_assumes():
    R.assert_sources_still_say_so()


def test_restatement_on_a_matrix_worked_by_hand():
    """two cells per category: the residual is +- half the difference; one numeric key that IS the gene: residual 0"""
    x = np.array([[1.0, 5.0, 2.0], [3.0, 5.0, 2.0], [10.0, 5.0, 2.0], [20.0, 5.0, 4.0]])
    codes = np.array([0, 0, 1, 1])
    out = R.ref_categorical(x, codes, 2)
    assert out.tolist() == [[-1.0, 5.0, 0.0], [1.0, 5.0, 0.0], [-5.0, 5.0, -1.0], [5.0, 5.0, 1.0]]   # (gene 1 is constant: kept)
    out = R.ref_numeric(x, x[:, :1] * 3.0 + 7.0, keep_constant=False)
    assert np.abs(out[:, 0]).max() < 1e-14 and np.abs(out[:, 1]).max() == 0
    assert np.allclose(out[:, 2], x[:, 2] - np.polyval(np.polyfit(x[:, 0], x[:, 2], 1), x[:, 0]), atol=1e-13)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_sums_and_residual_on_every_case(emu, name):
    """per case: the range with implicit zeros exactly, the fixed-point sums within their stated bound, the residual with and
    without the constant-gene rule within ulp_out / 2 + 1e-9 max|x_j| of the float64 restatement, every element written, constant
    genes returned bit for bit; the two n = 5000 cases bit-identical on a second run"""
    H, lib, rabi = emu
    lib.emu_reset_stats()
    R.run_case(rabi, name, label="emulator")
    _only_full_waves(H, lib, name)


def test_staged_table_slice_is_what_the_rule_says(emu):
    """the dynamic LDS of the residual kernel: m rows of CS = 4 * threads-per-row float64"""
    H, lib, rabi = emu
    for name in ("n63-r2", "r5", "n64-r16"):
        mdl = R.case_model(name)
        x = R.case_csr(name)
        lib.emu_reset_stats()
        rc, _ = rabi.resid(x, np.zeros((mdl["m"], x.shape[1])), np.ones(x.shape[1], np.uint8), w=mdl["w"], out_f64=False)
        assert rc == 0 and lib.emu_max_dyn_lds() == mdl["m"] * 4 * R.resid_threads(mdl["m"], False) * 8, name


def test_nonfinite_values_and_bad_codes_raise_their_flags(emu):
    H, lib, rabi = emu
    R.run_nonfinite_case(rabi, label="emulator")


def test_argument_checks_start_no_kernel(emu):
    H, lib, rabi = emu
    R.run_argument_checks(rabi, launches=lib.emu_launches)
