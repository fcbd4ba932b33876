"""An iteration's quality from its last level, the starting quality from the level-0 set-up pass (csrc/leiden.hip
`iteration_quality`, `ld_level0_setup_kernel`) on the device: the case table of tests/leiden_quality_cases.py, whose
recorded figures the emulator reproduces bit for bit (tests/test_emu_leiden_quality_cpu.py).  Here: labels and counters as
recorded, Q within 1e-12 of the recorded one, and no walk of the level-0 graph for an iteration's quality."""
from __future__ import annotations

import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import leiden_quality_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import torch

    from scanpy_amd import _kernels as K
    from scanpy_amd import _lib

    class Device:
        @staticmethod
        def leiden(adj, **kw):
            dev = [torch.from_numpy(np.array(a, dtype=t)).cuda()  # (a copy: the case graphs are read-only)
                   for a, t in ((adj.indptr, np.int64), (adj.indices, np.int32), (adj.data, np.float32))]
            if "objective" in kw:
                kw["objective"] = "CPM" if kw["objective"] == 1 else "modularity"
            for key, dtype in (("node_weights", np.float32), ("initial_membership", np.int32)):
                if kw.get(key) is not None:
                    kw[key] = torch.from_numpy(np.ascontiguousarray(kw[key], dtype=dtype)).cuda()
            memb, q, nc = K.leiden(*dev, adj.shape[0], **kw)
            return memb.cpu().numpy(), q, nc

        stats = staticmethod(K.leiden_last_stats)

        @staticmethod
        def raw_stats():
            out = (C.c_int32 * 20)()
            _lib.load().scamd_leiden_last_stats(out, 20)
            return list(out)

    return Device


@pytest.mark.parametrize("case", cases.CASES)
def test_quality_case(run, monkeypatch, case):
    cases.run_case(run, case, monkeypatch, "gpu")
