"""The tiers of a Leiden decide step on the device (csrc/leiden.hip `decide_tiers`: main, wave-per-row and block tier in ONE
launch, the giant tier in a launch of its own; tier lists written by the list builders): the case table of
tests/leiden_tier_cases.py, whose recorded figures the emulator reproduces too (tests/test_emu_leiden_tiers_cpu.py)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import leiden_tier_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import torch

    from scanpy_amd import _kernels as K

    class Device:
        @staticmethod
        def leiden(adj, **kw):
            dev = [torch.from_numpy(np.array(a, dtype=t)).cuda()  # (a copy: the case graphs are read-only)
                   for a, t in ((adj.indptr, np.int64), (adj.indices, np.int32), (adj.data, np.float32))]
            if "objective" in kw:
                kw["objective"] = "CPM" if kw["objective"] == 1 else "modularity"
            if kw.get("node_weights") is not None:
                kw["node_weights"] = torch.from_numpy(np.ascontiguousarray(kw["node_weights"], dtype=np.float32)).cuda()
            memb, q, nc = K.leiden(*dev, adj.shape[0], **kw)
            return memb.cpu().numpy(), q, nc

        stats = staticmethod(K.leiden_last_stats)
        bounds = staticmethod(K.leiden_tier_bounds)

    return Device


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_tier_case(run, monkeypatch, name):
    """same partition with 64, 16 and 32 lanes per vertex, Q is the labels' modularity, every tier the case is for was
    reached, and labels, Q, sweeps, iterations and the tier statistics are the recorded ones"""
    cases.run_case(run, name, monkeypatch, "gpu")


def test_tier_bounds_accessor(run):
    from scanpy_amd import _lib

    for lanes, want in cases.RECORDED_BOUNDS.items():
        assert run.bounds(lanes) == want
    with pytest.raises(_lib.ScamdError):
        run.bounds(48)
