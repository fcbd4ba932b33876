"""The quality of an outer Leiden iteration taken from the level the iteration ended on, and the starting quality of a run
from singletons taken from the level-0 set-up pass (csrc/leiden.hip `iteration_quality`, `quality_from_sums`,
`ld_level0_setup_kernel`) -- instead of walks over the level-0 graph.  Nothing a run returns may change
by that: the table below was recorded from the emulator build of the commit BEFORE the change (which walked level 0 for every
quality) and both suites compare against it: tests/test_emu_leiden_quality_cpu.py bit for bit, tests/test_gpu_leiden_quality.py
the labels and counters bit for bit and Q to 1e-12.

Of the one-workgroup kernel's counters only the moves reach the statistics, through `quiet_reuse_iterations`; the table holds
that, the iteration and level counts, the round trips, the sweeps, the reuse counters and every polish_* figure.  `launches`
and `device_fills` are lower by the removed kernels and are not compared.

    python tests/leiden_quality_cases.py <emulator library>     prints the EXPECTED table of that build"""
from __future__ import annotations

import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np
from scipy import sparse

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

L0_WALKS_SLOT = 14  # scamd_leiden_last_stats: walks of the level-0 graph for a quality (the slot has no key)
STAT_KEYS = ("iterations", "host_round_trips", "levels_first_iteration", "lm_sweeps", "levels_reused", "quiet_reuse_iterations",
             "polish_full_sweeps", "polish_rounds", "polish_moves", "polish_skipped_proven", "polish_splits",
             "polish_ended_by_round_cap", "ended_by_iteration_cap")


def _sym(m):
    m = sparse.csr_matrix(m, dtype=np.float32)
    m = m.maximum(m.T).tocsr()
    m.sort_indices()
    return m


def _two():
    return _sym(np.array([[0.0, 1.0], [1.0, 0.0]]))


def _dense40():
    """four loose groups of ten, every pair adjacent: the coarse levels reach n <= 16 (one vertex at a time)"""
    rng = np.random.default_rng(40)
    w = rng.random((40, 40)) * 0.2 + 0.05
    grp = np.arange(40) // 10
    w[grp[:, None] == grp[None, :]] += 0.6
    np.fill_diagonal(w, 0.0)
    return _sym(np.triu(w))


def _pbmc():
    f = np.load(ROOT / "tests" / "golden" / "pbmc68k_reduced.npz")
    m = sparse.csr_matrix((f["connectivities_data"], f["connectivities_indices"], f["connectivities_indptr"]),
                          shape=tuple(f["connectivities_shape"])).astype(np.float32)
    m.sort_indices()
    return m


def _blobs(n, seed, spread):
    from oracle import connectivities as oconn
    from oracle import knn as oknn

    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((12, 10)) * spread
    x = (cent[rng.integers(0, 12, n)] + rng.standard_normal((n, 10))).astype(np.float32)
    idx, dist = oknn.knn_exact_f64(x, np.arange(n), 15)
    conn, _, _ = oconn.fuzzy_simplicial_set(idx, dist, n, 15)
    conn = conn.tocsr().astype(np.float32)
    conn.sort_indices()
    return conn


def _with_diagonal():
    """900 vertices in blobs, every third vertex with a stored diagonal entry (self loops count towards the internal weight
    and the strengths; the decide kernels skip them)"""
    m = _blobs(900, 3, 2.0).tolil()
    rng = np.random.default_rng(9)
    for v in range(0, 900, 3):
        m[v, v] = np.float32(0.25 + 0.5 * rng.random())
    m = m.tocsr().astype(np.float32)
    m.sort_indices()
    return m


GRAPHS = {
    "two": _two,
    "dense40": _dense40,
    "pbmc700": _pbmc,
    "separated6000": lambda: _blobs(6000, 0, 4.0),   # the planted-like one: the second iteration only verifies the first
    "overlapping6000": lambda: _blobs(6000, 0, 0.8),
    "diagonal900": _with_diagonal,
}

# variant -> (environment, leiden arguments).  "init": a start partition (blocks of 7 consecutive vertices); "cpm_weights":
# CPM with the caller's node weights; "polish": SCAMD_LEIDEN_MAX_ITERS=1 cuts the run short so that the polish meets an
# unfinished partition -- it then moves something on the graphs whose communities overlap (asserted for pbmc700 and
# overlapping6000) and a verifying iteration follows
VARIANTS = {
    "default": ({}, {}),
    "small_off": ({"SCAMD_LEIDEN_SMALL": "0"}, {}),
    "reuse_off": ({"SCAMD_LEIDEN_REUSE": "0"}, {}),
    "resolution_0.3": ({}, dict(resolution=0.3)),
    "resolution_2.0": ({}, dict(resolution=2.0)),
    "two_iterations": ({}, dict(n_iterations=2)),
    "until_stable_seed3": ({}, dict(n_iterations=-1, seed=3)),
    "cpm_weights": ({}, dict(objective=1, resolution=0.02, node_weights="weights")),
    "init": ({}, dict(initial_membership="blocks")),
    "polish": ({"SCAMD_LEIDEN_MAX_ITERS": "1"}, dict(seed=1)),
}
ENV_KEYS = ("SCAMD_LEIDEN_SMALL", "SCAMD_LEIDEN_REUSE", "SCAMD_LEIDEN_MAX_ITERS")
POLISH_MUST_MOVE = ("pbmc700", "overlapping6000")
CASES = [f"{g}/{v}" for g in GRAPHS for v in VARIANTS]

_graphs = {}


def graph(name: str):
    """computed once, never written"""
    if name not in _graphs:
        m = GRAPHS[name]()
        for arr in (m.data, m.indices, m.indptr):
            arr.setflags(write=False)
        _graphs[name] = m
    return _graphs[name]


def _arguments(m, kw):
    n = m.shape[0]
    kw = dict(kw)
    if isinstance(kw.get("node_weights"), str):
        kw["node_weights"] = (0.5 + np.random.default_rng(5).random(n)).astype(np.float32)
    if isinstance(kw.get("initial_membership"), str):
        kw["initial_membership"] = (np.arange(n) // 7 * 7).astype(np.int32)
    return kw


def run_case(run, case: str, monkeypatch, where: str, expected="table"):
    """run: .leiden(adj, **kw) -> (labels [n] numpy, Q, communities), .stats() -> dict of the last call, .raw_stats() -> the 20
    slots of scamd_leiden_last_stats.  where: 'emu' (Q bit for bit) or 'gpu' (Q to 1e-12).  Returns the case's table entry."""
    from oracle import leiden as ol

    gname, vname = case.split("/")
    m = graph(gname)
    env, kw = VARIANTS[vname]
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    kw = _arguments(m, kw)
    memb, q, nc = run.leiden(m, **kw)
    st = run.stats()
    walks = int(run.raw_stats()[L0_WALKS_SLOT])
    got = (hashlib.sha256(np.ascontiguousarray(memb, dtype=np.int32).tobytes()).hexdigest(), float(q).hex(), nc,
           tuple(int(st[k]) for k in STAT_KEYS))
    print(f"{where} {case}: Q={q!r} nc={nc} level-0 quality walks={walks} launches={st['launches']} {dict(zip(STAT_KEYS, got[3]))}")
    # the reported number is the labels' modularity (CPM runs report the resolution-1 modularity of their partition)
    q_oracle = ol.modularity(m, memb, resolution=1.0 if kw.get("objective") == 1 else kw.get("resolution", 1.0))
    print(f"   Q - oracle.modularity(labels) = {q - q_oracle:.3e}")
    assert abs(q - q_oracle) < 1e-9 and nc == int(memb.max()) + 1
    if vname == "polish" and gname in POLISH_MUST_MOVE:
        assert st["polish_moves"] > 0 and st["iterations"] >= 2, st
    # Walks of the level-0 graph: a run from singletons needs one per polish pass that moved something at the most (a pass
    # runs at least one full sweep), plus the modularity report of a CPM run; a given start partition is walked once more.
    allowed = st["polish_full_sweeps"] + (1 if kw.get("objective") == 1 else 0) + (1 if "initial_membership" in kw else 0)
    if expected != "parent":
        assert walks <= allowed, f"{case}: {walks} walks of the level-0 graph, {allowed} allowed"
        if gname == "separated6000" and vname in ("default", "small_off", "reuse_off", "two_iterations"):
            assert walks == 0
    if expected == "table":
        want = EXPECTED[case]
        if where == "gpu":
            # After a polish pass that moved something the components inside the communities are searched by in-place label
            # propagation (ld_cc_prop_kernel): how far a launch carries a label is the schedule's, and every four launches are
            # a round trip -- in such a run the device's round trips are not the emulator's (616 recorded, 623 on an MI355X for
            # overlapping6000/polish, with every other figure equal).  They are compared wherever no polish pass moved anything.
            if st["polish_moves"] > 0:
                trips = STAT_KEYS.index("host_round_trips")
                got, want = ((x[0], x[1], x[2], x[3][:trips] + x[3][trips + 1:]) for x in (got, want))
            assert got[0] == want[0] and got[2:] == want[2:], f"{case}: {got} != recorded {want}"
            assert abs(q - float.fromhex(want[1])) <= 1e-12, f"{case}: Q {q!r} != recorded {float.fromhex(want[1])!r}"
        else:
            assert got == want, f"{case}: {got} != recorded {want}"
    return got


# case -> labels sha256, Q (float.hex), communities, the statistics of STAT_KEYS: the emulator build of the parent commit
EXPECTED = {
    "two/default": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x0.0p+0', 1, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "two/small_off": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x0.0p+0', 1, (2, 22, 2, 5, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "two/reuse_off": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x0.0p+0', 1, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "two/resolution_0.3": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x1.6666666666666p-1', 1, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "two/resolution_2.0": ('01acecb507abfe1a354aa8064f4af5d3f1acd019e37db3c11c97523b71c76e9d', '-0x1.0000000000000p+0', 2, (1, 7, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "two/two_iterations": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x0.0p+0', 1, (2, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    "two/until_stable_seed3": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x0.0p+0', 1, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "two/cpm_weights": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x0.0p+0', 1, (2, 24, 2, 5, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "two/init": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x0.0p+0', 1, (1, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "two/polish": ('af5570f5a1810b7af78caf4bc70a660f0df51e42baf91d4de5b2328de0e83dfc', '0x0.0p+0', 1, (1, 7, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "dense40/default": ('e2e9910ee477c01e9fb86f84362abc4df29391d77bd088f1f2dc67e4f90475ae', '0x1.6de0167859a00p-2', 4, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "dense40/small_off": ('e2e9910ee477c01e9fb86f84362abc4df29391d77bd088f1f2dc67e4f90475ae', '0x1.6de0167859a00p-2', 4, (2, 23, 2, 6, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "dense40/reuse_off": ('e2e9910ee477c01e9fb86f84362abc4df29391d77bd088f1f2dc67e4f90475ae', '0x1.6de0167859a00p-2', 4, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "dense40/resolution_0.3": ('b393978842a0fa3d3e1470196f098f473f9678e72463cb65ec4ab5581856c2e4', '0x1.6666666666666p-1', 1, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "dense40/resolution_2.0": ('e2e9910ee477c01e9fb86f84362abc4df29391d77bd088f1f2dc67e4f90475ae', '0x1.b7798ebbac900p-4', 4, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "dense40/two_iterations": ('e2e9910ee477c01e9fb86f84362abc4df29391d77bd088f1f2dc67e4f90475ae', '0x1.6de0167859a00p-2', 4, (2, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    "dense40/until_stable_seed3": ('e2e9910ee477c01e9fb86f84362abc4df29391d77bd088f1f2dc67e4f90475ae', '0x1.6de0167859a00p-2', 4, (2, 8, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "dense40/cpm_weights": ('b393978842a0fa3d3e1470196f098f473f9678e72463cb65ec4ab5581856c2e4', '0x0.0p+0', 1, (2, 35, 3, 9, 3, 1, 0, 0, 0, 1, 0, 0, 0)),
    "dense40/init": ('e2e9910ee477c01e9fb86f84362abc4df29391d77bd088f1f2dc67e4f90475ae', '0x1.6de0167859a00p-2', 4, (2, 9, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "dense40/polish": ('e2e9910ee477c01e9fb86f84362abc4df29391d77bd088f1f2dc67e4f90475ae', '0x1.6de0167859a00p-2', 4, (1, 7, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "pbmc700/default": ('655b8069579d1034a6b441a2ac4e548cd74fdaef765706e9e1157d0dd0399ad3', '0x1.9fc4f04c6ef11p-1', 12, (4, 10, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "pbmc700/small_off": ('655b8069579d1034a6b441a2ac4e548cd74fdaef765706e9e1157d0dd0399ad3', '0x1.9fc4f04c6ef11p-1', 12, (3, 96, 5, 32, 5, 1, 0, 0, 0, 1, 0, 0, 0)),
    "pbmc700/reuse_off": ('655b8069579d1034a6b441a2ac4e548cd74fdaef765706e9e1157d0dd0399ad3', '0x1.9fc4f04c6ef11p-1', 12, (4, 10, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "pbmc700/resolution_0.3": ('016f8ac88d542967181977ab3ef1284b49906d34d14460107ab02d2e6e453d20', '0x1.d85a2ae29ddf1p-1', 7, (3, 9, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "pbmc700/resolution_2.0": ('b4e78453106bc0bb95707076d4e750bd7db8f1edd312aa8b44eb942fe94ac0ab', '0x1.697758b9ae026p-1', 15, (4, 10, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "pbmc700/two_iterations": ('1d55f92eb94eeb862e19168eb320ceb54cead2c8c80688eae2b66f70e75097e6', '0x1.9fa88001a8c1bp-1', 12, (2, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    "pbmc700/until_stable_seed3": ('655b8069579d1034a6b441a2ac4e548cd74fdaef765706e9e1157d0dd0399ad3', '0x1.9fc4f04c6ef11p-1', 12, (4, 10, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "pbmc700/cpm_weights": ('52b42689e78dacc11b9564e2dde0aed0f346a8b1369b7608bde9bdaf22027b45', '0x1.8aa4e5173fd9cp-1', 21, (5, 176, 6, 49, 5, 1, 0, 0, 0, 1, 0, 0, 0)),
    "pbmc700/init": ('d2a449ea03fc1348e8af05bd981d812253e5feaf0c8187d63577f5e289a38da4', '0x1.9fc5812a5173bp-1', 12, (3, 10, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "pbmc700/polish": ('00fa4a671afb8e20ec4b65abfdc243fd41e8083b8e6c5fd2e06f685f393d2040', '0x1.9ecb4e4373882p-1', 12, (2, 21, 0, 0, 0, 0, 3, 8, 10, 0, 0, 0, 0)),
    "separated6000/default": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.d5477441ccd4bp-1', 12, (2, 39, 2, 21, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "separated6000/small_off": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.d5477441ccd4cp-1', 12, (2, 74, 6, 32, 6, 1, 0, 0, 0, 1, 0, 0, 0)),
    "separated6000/reuse_off": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.d5477441ccd4bp-1', 12, (2, 49, 2, 21, 0, 0, 0, 0, 0, 1, 0, 0, 0)),
    "separated6000/resolution_0.3": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.f32cde9c4d9a0p-1', 12, (2, 39, 2, 21, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "separated6000/resolution_2.0": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.aa9200e514df8p-1', 12, (2, 35, 2, 17, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "separated6000/two_iterations": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.d5477441ccd4bp-1', 12, (2, 39, 2, 21, 2, 1, 0, 0, 0, 0, 0, 0, 0)),
    "separated6000/until_stable_seed3": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.d5477441ccd4bp-1', 12, (2, 39, 2, 21, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "separated6000/cpm_weights": ('c45fd9cfd07e36d6688686f2e6123f107f3938f11db8f67bb4cbd40dfa94d6c7', '0x1.172d8fd0846a1p-1', 215, (14, 562, 5, 153, 5, 1, 0, 0, 0, 1, 0, 0, 0)),
    "separated6000/init": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.d5477441ccd4bp-1', 12, (2, 40, 2, 21, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "separated6000/polish": ('ea38e5917be8f7a362171e8fe201cf3fa83884b3035fb42da00eaea69a328b5d', '0x1.d5477441ccd4bp-1', 12, (1, 34, 2, 17, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "overlapping6000/default": ('7ece1af2a7e8f1413a462de23fa685c03c3dfceec0271ce5111032506ec70f15', '0x1.550394ff957f6p-1', 10, (12, 231, 2, 83, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "overlapping6000/small_off": ('558d596eb52c181ccc9392f8eb1baa2a1e2df23e5bf92b4a0089185bbcf77dc9', '0x1.53a28536881c3p-1', 9, (13, 593, 7, 155, 6, 1, 0, 0, 0, 1, 0, 0, 0)),
    "overlapping6000/reuse_off": ('45e44741d1343351c23e1ca8b328c4458f5094d3f4ace323f0cd77fcb3147b51', '0x1.5504dfae17c96p-1', 10, (13, 257, 2, 86, 0, 0, 0, 0, 0, 1, 0, 0, 0)),
    "overlapping6000/resolution_0.3": ('08497471d64ca1bb723b10043a7b48bcb159d84cf6bf8a58ad36c83b64a0cf98', '0x1.8db4add3389dap-1', 3, (9, 169, 2, 60, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "overlapping6000/resolution_2.0": ('bbe403cbcd363acd06c8d53c82f22285796b118becf37460391b3914d0a47de8', '0x1.2782767cd6718p-1', 25, (13, 245, 2, 84, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "overlapping6000/two_iterations": ('acdaddf5dc1b79726c87a147755d031f73b915c2d506798f860cc77789d6c695', '0x1.5275601b17442p-1', 10, (2, 53, 2, 25, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    "overlapping6000/until_stable_seed3": ('73b14f1353a50b84f0ab490545f6a91e9b52c30fb158dcd1476bac7c7906a3f6', '0x1.54fd3c9ee61b5p-1', 10, (16, 300, 2, 100, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "overlapping6000/cpm_weights": ('3e6b757ff870f8236e12790ef09bc437a530fb5513a5f036830f8ada709e56b4', '0x1.dcb2a92520f82p-2', 292, (11, 436, 6, 129, 5, 1, 0, 0, 0, 1, 0, 0, 0)),
    "overlapping6000/init": ('12ac8bb7319145ee2111e48f3d4ae8471b02fb2ff6d5cde5cbda9882cba6a409', '0x1.537f0ec65e993p-1', 10, (18, 353, 2, 126, 2, 1, 0, 0, 0, 1, 0, 0, 0)),
    "overlapping6000/polish": ('1bddbc36e0ca4ee7010ec0ab9ed82c0514378bf6f5c385e98bab911f5b5c1914', '0x1.5482897593e55p-1', 10, (7, 616, 2, 37, 0, 0, 20, 438, 803, 0, 0, 0, 0)),
    "diagonal900/default": ('4e3b901c5b863d00f4f19019617da9b51af2fd5457aac7c16084ca6a03285df0', '0x1.caf904075c72ep-1', 12, (3, 9, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "diagonal900/small_off": ('4e3b901c5b863d00f4f19019617da9b51af2fd5457aac7c16084ca6a03285df0', '0x1.caf904075c72ep-1', 12, (3, 89, 4, 31, 5, 1, 0, 0, 0, 1, 0, 0, 0)),
    "diagonal900/reuse_off": ('4e3b901c5b863d00f4f19019617da9b51af2fd5457aac7c16084ca6a03285df0', '0x1.caf904075c72ep-1', 12, (3, 9, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "diagonal900/resolution_0.3": ('268d530253df51454f6327ca9fdfa7a93b1bf8bc698de14ce8322e60b0e7d9d7', '0x1.ebddaf9531465p-1', 11, (3, 9, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "diagonal900/resolution_2.0": ('4e3b901c5b863d00f4f19019617da9b51af2fd5457aac7c16084ca6a03285df0', '0x1.9ff176630489ap-1', 12, (3, 9, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "diagonal900/two_iterations": ('4e3b901c5b863d00f4f19019617da9b51af2fd5457aac7c16084ca6a03285df0', '0x1.caf904075c72ep-1', 12, (2, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    "diagonal900/until_stable_seed3": ('4e3b901c5b863d00f4f19019617da9b51af2fd5457aac7c16084ca6a03285df0', '0x1.caf904075c72ep-1', 12, (3, 9, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "diagonal900/cpm_weights": ('94aa37b408751a50800abe5c594ca8ee049061166b79edc352591f32beae919c', '0x1.ca1ff28428f15p-1', 13, (3, 99, 5, 33, 5, 1, 0, 0, 0, 1, 0, 0, 0)),
    "diagonal900/init": ('4e3b901c5b863d00f4f19019617da9b51af2fd5457aac7c16084ca6a03285df0', '0x1.caf904075c72ep-1', 12, (3, 10, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0)),
    "diagonal900/polish": ('4e3b901c5b863d00f4f19019617da9b51af2fd5457aac7c16084ca6a03285df0', '0x1.caf904075c72ep-1', 12, (2, 18, 0, 0, 0, 0, 2, 6, 4, 0, 0, 0, 0)),
}


if __name__ == "__main__":
    import time

    import pytest

    sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "tests" / "emu")]
    import harness

    lib = C.CDLL(sys.argv[1])
    for fn_name in ("scamd_leiden_workspace_bytes", "scamd_leiden_csr_nw_f32", "scamd_leiden_last_stats", "scamd_leiden_stat_name",
                    "scamd_last_error"):
        fn = getattr(lib, fn_name)
        fn.restype, fn.argtypes = harness.SIGNATURES[fn_name]

    class Recorded:
        leiden = staticmethod(lambda adj, **kw: harness.leiden(lib, adj, **kw))
        stats = staticmethod(lambda: harness.leiden_stats(lib))
        raw_stats = staticmethod(lambda: [0] * 20)

    mp = pytest.MonkeyPatch()
    for case_name in sys.argv[2:] or CASES:
        t0 = time.time()
        entry = run_case(Recorded, case_name, mp, "emu", expected="parent")
        print(f'TABLE    "{case_name}": {entry!r},  # {time.time() - t0:.1f} s', flush=True)
    mp.undo()
