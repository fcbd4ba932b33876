"""One level of a Leiden iteration on the device -- the refinement and the coarse graph (csrc/leiden.hip `refinement`,
`aggregate`) -- through the test entry scamd_leiden_debug_level_f32: the cases and checkers of tests/leiden_level_cases.py, exact
against int64 sums (the coarse graph is P^T Wq P entry for entry; Kref, Eref and refsize equal a recomputation).  The emulator
runs the same table in tests/test_emu_leiden_level_cpu.py."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import leiden_level_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import torch

    from scanpy_amd import _kernels as K

    def graph(adj):  # (copies: the case graphs are read-only; the entries go in as they are stored)
        return [torch.from_numpy(np.array(a, dtype=t)).cuda() for a, t in ((adj.indptr, np.int64), (adj.indices, np.int32), (adj.data, np.float32))]

    class Device:
        @staticmethod
        def level(adj, membership, refined_in=None, **kw):
            given = None if refined_in is None else torch.from_numpy(np.array(refined_in, dtype=np.int32)).cuda()
            out = K.leiden_debug_level(*graph(adj), adj.shape[0], torch.from_numpy(np.array(membership, dtype=np.int32)).cuda(),
                                       refined_in=given, **kw)
            return {key: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for key, v in out.items()}

        @staticmethod
        def leiden(adj, **kw):
            adj = adj.tocsr()
            adj.sort_indices()
            memb, q, nc = K.leiden(*graph(adj), adj.shape[0], **kw)
            return memb.cpu().numpy(), q, nc

        stats = staticmethod(K.leiden_last_stats)
        bounds = staticmethod(K.leiden_tier_bounds)

    return Device


@pytest.mark.parametrize("name", cases.agg_case_names("gpu"))
def test_coarse_graph_case(run, monkeypatch, name):
    """the coarse graph under a given refined partition is P^T Wq P entry for entry, built by the builders the case names"""
    cases.run_agg_case(run, name, monkeypatch)


@pytest.mark.parametrize("name", sorted(cases.FORCED))
def test_coarse_graph_forced_builder(run, monkeypatch, name):
    """every forced builder gives P^T Wq P itself (not merely what another builder gives)"""
    cases.run_forced_case(run, name, monkeypatch)


@pytest.mark.parametrize("seed", cases.SEEDS)
@pytest.mark.parametrize("beta", cases.BETAS)
@pytest.mark.parametrize("name", sorted(cases.REFINE_CASES))
def test_refinement_case(run, monkeypatch, name, beta, seed):
    """nested, connected groups of well-connected vertices whose Kref / Eref / refsize equal a recomputation; the same with 64, 16
    and 32 lanes per vertex and when repeated"""
    cases.run_refine_case(run, name, beta, seed, monkeypatch)


def test_level_entry_refuses_bad_partitions(run):
    """ids outside [0, n), a group not named by a member, a group across two communities"""
    from scanpy_amd import _lib

    m, membership, refined = cases._once("one_group", cases.AGG_CASES["one_group"][0])
    for memb, ref in ((np.full(200, 200), refined), (membership, np.full(200, -1)), (membership, np.where(np.arange(200) < 5, 17, 3)),
                      (np.arange(200) % 2, refined)):
        with pytest.raises(_lib.ScamdError, match="leiden level"):
            run.level(m, memb, refined_in=ref)


def test_renumbering_orders_equal_sizes_by_smallest_member(run):
    cases.check_renumbering(run)


@pytest.mark.parametrize("name", sorted(cases.SMALL_ENTRY_CASES))
def test_one_workgroup_path_at_its_entry_bounds(run, name):
    """n = 17, n = 1024 with 65536 entries (the one-workgroup kernel), with 65538 and n = 1025 (separate kernels)"""
    cases.check_small_entry_case(run, name)
