"""The list builders, the apply step and the community totals of csrc/leiden.hip on the device -- the kernels whose workgroups
share a few counter words, bounded by SCAMD_LEIDEN_COUNT_GRID: the case table and checkers of
tests/leiden_counter_cases.py through the test entry scamd_leiden_debug_counters_f32 (the emulator runs the same table:
tests/test_emu_leiden_counters_cpu.py), and whole clusterings of three 20k-vertex graphs against the labels, modularity and
community count recorded from the build before the change (tests/golden/leiden_counters/, tools/leiden_counters_fixtures.py)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import leiden_counter_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import torch

    from scanpy_amd import _kernels as K

    def graph(m):
        return [torch.from_numpy(np.array(a, dtype=t)).cuda()  # (a copy: the case graphs are read-only)
                for a, t in ((m.indptr, np.int64), (m.indices, np.int32), (m.data, np.float32))]

    class Device:
        bounds = staticmethod(K.leiden_tier_bounds)

        @staticmethod
        def counters(m, memb, decision, flags, n_cls, salt):
            dev = lambda a: None if a is None else torch.from_numpy(np.array(a, dtype=np.int32)).cuda()  # noqa: E731
            out = K.leiden_debug_counters(*graph(m), m.shape[0], dev(memb), dev(decision), flags=dev(flags), n_cls=n_cls, salt=salt)
            return {key: (val.cpu().numpy() if isinstance(val, torch.Tensor) else val) for key, val in out.items()}

        @staticmethod
        def leiden(m, **kw):
            memb, q, nc = K.leiden(*graph(m), m.shape[0], **kw)
            return memb.cpu().numpy(), q, nc

    return Device


@pytest.mark.parametrize("knob", cases.KNOBS, ids=lambda k: f"grid{k or 'default'}")
@pytest.mark.parametrize("name", sorted(cases.UNIT_CASES))
def test_counter_case(run, monkeypatch, name, knob):
    """every flagged vertex once and in the list of its class, the tier lists by row length, totals, moved / blocked and the
    state after the apply step equal to a recomputation; the classes the same in two calls"""
    cases.run_unit_case(run, name, knob, monkeypatch)


@pytest.mark.parametrize("count_grid", (2, None), ids=lambda g: f"grid{g or 'default'}")
@pytest.mark.parametrize("name", cases.WHOLE_RUNS)
def test_whole_run_equals_the_build_before(run, monkeypatch, name, count_grid):
    """labels, modularity (to the bit) and community count of a whole n_iterations=-1 run"""
    cases.check_whole_run(run, name, monkeypatch, count_grid)
