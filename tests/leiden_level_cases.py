"""TEST INFRASTRUCTURE shared by tests/test_gpu_leiden_level.py (the product library on the GPU) and
tests/test_emu_leiden_level_cpu.py (the same host code and kernels on the emulator, through tests/emu/harness.py): ONE level of
a Leiden iteration -- the refinement and the coarse graph (csrc/leiden.hip `refinement`, `aggregate`) -- through the test entry
`scamd_leiden_debug_level_f32`, against sums recomputed here in int64.  Everything in these two stages is integer arithmetic
on weights quantised by 2^32, so every comparison is exact: no tolerance anywhere but the one the merge rule itself has (a
float64 threshold, see `well_connected`).  Nothing here touches a device: a test hands in a `Runner`:

    run.level(adj, membership, refined_in=None, resolution=, beta=, seed=) -> dict of numpy arrays and integers (the keys of
        tests/emu/harness.py:leiden_level);  run.stats() -> the statistics of the last call;  run.bounds(lanes)

Aggregation cases hand the entry a refined partition (`refined_in`): group shapes are chosen, not drawn, and sit at the bounds of
the coarse-row builders.  A coarse row c with members of `dsum` entries in all on a level of `nn` coarse vertices
(need = min(dsum, nn): the bound on its distinct neighbours) is built by

    the wave builder       need <= AGG_WAVE_MAX (384) and dsum <= AGG_WAVE_WORK (2048); tables of 128 / 256 / 512 slots for
                           need <= 96 / <= 192 / more
    the split path         else, dsum > AGG_SPLIT_WORK (262144) and nn <= 5600: parts of AGG_SPLIT_CHUNK (131072) member entries
    the 512-thread builder else, need <= AGG_MID_MAX (2048) and dsum <= AGG_MID_WORK (65536)
    the 1024-thread one    else; more than AGG_PASS_KEYS (4096) keys: several passes, after ONE optimistic pass (HUB_TRY_PROBES)

(`expected_tiers` restates that rule; the entry returns how many rows went where, and every case states what it expects.)
The order of a group's members in the scatter is whatever the atomics give on the device and the vertex order on the emulator,
so where a case aims at a cut between PARTS of a split row it reaches exactly that cut on the emulator only.
"""
from __future__ import annotations

import os

import numpy as np
from scipy import sparse
from scipy.sparse.csgraph import connected_components

import leiden_tier_cases as tier_cases

QUADS = ("0", "1", "2")
AGG_ENV_KEYS = ("SCAMD_LEIDEN_AGG_WAVE_MAX", "SCAMD_LEIDEN_AGG_MID_MAX", "SCAMD_LEIDEN_AGG_PASS_KEYS", "SCAMD_LEIDEN_AGG_WAVE_WORK",
                "SCAMD_LEIDEN_AGG_MID_WORK", "SCAMD_LEIDEN_AGG_SPLIT_CHUNK", "SCAMD_LEIDEN_AGG_SPLIT_WORK", "SCAMD_LEIDEN_HUB_TRY_PROBES")
SPLIT_NN_MAX = 5600


# ---- the reference -----------------------------------------------------------------------------------------------------------
def quantise(w):
    """ld_quantize_kernel: llrint(w * 2^32) (ties to even, as np.rint), 0 for w <= 0"""
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.where(w > 0.0, np.rint(w * 4294967296.0), 0.0).astype(np.int64)


def _rows(m):
    return np.repeat(np.arange(m.shape[0], dtype=np.int64), np.diff(m.indptr))


def _segment_sums(values, indptr):
    cs = np.concatenate(([0], np.cumsum(values, dtype=np.int64)))
    return cs[indptr[1:]] - cs[indptr[:-1]]


def _sum_by(keys, values, size):
    out = np.zeros(size, dtype=np.int64)
    np.add.at(out, keys, values)
    return out


def _canonical(n_rows, rows, cols, wq):
    """(row * n_rows + col) sorted, the int64 sums per distinct key"""
    key = rows.astype(np.int64) * n_rows + cols.astype(np.int64)
    order = np.argsort(key, kind="stable")
    key, wq = key[order], wq[order]
    if key.size == 0:
        return key, wq
    first = np.concatenate(([True], key[1:] != key[:-1]))
    return key[first], np.add.reduceat(wq, np.flatnonzero(first))


def agg_knobs():
    """the bounds of the coarse-row builders as read_knobs() resolves the environment"""
    env = lambda k, d: int(os.environ.get("SCAMD_LEIDEN_AGG_" + k, d))  # noqa: E731
    chunk = max(64, env("SPLIT_CHUNK", 131072))
    return dict(wave_max=min(env("WAVE_MAX", 384), 384), mid_max=min(env("MID_MAX", 2048), 2048), wave_work=max(1, env("WAVE_WORK", 2048)),
                mid_work=max(1, env("MID_WORK", 65536)), split_work=max(chunk, env("SPLIT_WORK", 262144)))


def expected_tiers(m, cid, nn):
    """rows the 512-thread builder, the 1024-thread builder and the split path take -> (n_mid, n_big, n_split)"""
    kn = agg_knobs()
    dsum = _sum_by(cid, np.diff(m.indptr).astype(np.int64), nn)
    need = np.minimum(dsum, nn)
    leaves = (need > kn["wave_max"]) | (dsum > kn["wave_work"])
    split = leaves & (dsum > kn["split_work"]) & (nn <= SPLIT_NN_MAX)
    mid = leaves & ~split & (need <= kn["mid_max"]) & (dsum <= kn["mid_work"])
    return int(mid.sum()), int((leaves & ~split & ~mid).sum()), int(split.sum())


def check_aggregation(m, membership, refined, out, tiers=None):
    """the coarse graph of `out` is P^T Wq P for P = onehot(cid), entry for entry; `refined` is the partition it was built under.
    tiers: the (n_mid, n_big, n_split) the case states, None: whatever the rule gives"""
    n = m.shape[0]
    membership, refined = np.asarray(membership), np.asarray(refined)
    wq = quantise(m.data)
    reps, inv = np.unique(refined, return_inverse=True)
    nn = reps.size
    assert out["n_coarse"] == nn, (out["n_coarse"], nn)
    if nn == n:
        assert out["skipped"] == 1 and out["merges"] == 0 and "cid" not in out, "nothing merged: no graph is built"
        return
    assert out["skipped"] == 0
    cid = out["cid"].astype(np.int64)
    # the map: onto [0, nn), one id per refined group, increasing with the group's representative
    assert cid.shape == (n,) and cid.min() == 0 and cid.max() == nn - 1 and np.unique(cid).size == nn
    assert (cid[refined] == cid).all(), "a vertex and the representative of its group have different coarse ids"
    assert (np.diff(cid[reps]) > 0).all(), "coarse ids do not increase with the representative"
    assert np.array_equal(cid, inv)
    # the graph
    indptr, indices, cw = out["indptr"], out["indices"], out["wq"]
    assert indptr.shape == (nn + 1,) and indptr[0] == 0 and (np.diff(indptr) >= 0).all()
    want_key, want_w = _canonical(nn, cid[_rows(m)], cid[m.indices], wq)
    assert indptr[-1] == want_key.size == out["coarse_nnz"] == indices.size == cw.size, (int(indptr[-1]), want_key.size, out["coarse_nnz"])
    assert indices.size == 0 or (indices.min() >= 0 and indices.max() < nn)
    got_rows = np.repeat(np.arange(nn, dtype=np.int64), np.diff(indptr))
    got_key = got_rows * nn + indices
    order = np.argsort(got_key, kind="stable")
    assert (np.diff(got_key[order]) > 0).all(), "a column appears twice in a coarse row"
    assert np.array_equal(got_key[order], want_key), "entries are not exactly where a member edge leads"
    bad = np.flatnonzero(cw[order] != want_w)
    assert bad.size == 0, f"{bad.size} coarse weights differ, first: row {want_key[bad[0]] // nn} col {want_key[bad[0]] % nn} " \
                          f"got {cw[order][bad[0]]} want {want_w[bad[0]]}"
    assert int(cw.sum()) == int(wq.sum()), "total weight is not conserved"
    # strengths: the row sums (= the sums of the members' strengths)
    k = _segment_sums(wq, m.indptr)
    assert np.array_equal(out["k"], _segment_sums(cw, indptr)) and np.array_equal(out["k"], _sum_by(cid, k, nn))
    # the partition of the coarse vertices: that of their members, named by the smallest coarse vertex of the community
    assert (membership[refined] == membership).all(), "the case's refined partition is not nested in its communities"
    _, comm_ix = np.unique(membership, return_inverse=True)
    label = np.full(comm_ix.max() + 1, nn, dtype=np.int64)
    np.minimum.at(label, comm_ix, cid)
    want_comm = np.empty(nn, dtype=np.int64)
    want_comm[cid] = label[comm_ix]
    assert np.array_equal(out["comm"], want_comm)
    got_tiers = (out["n_mid"], out["n_big"], out["n_split"])
    assert got_tiers == expected_tiers(m, cid, nn), (got_tiers, expected_tiers(m, cid, nn))
    if tiers is not None:
        assert got_tiers == tuple(tiers), f"the case was built for {tiers} rows beyond the wave builder, {got_tiers} ran"


def check_group_sums(m, refined, out):
    """refsize and Kref at the representatives (size, total strength), zero elsewhere"""
    n = m.shape[0]
    refined = np.asarray(refined)
    assert np.array_equal(out["refined"], refined)
    k = _segment_sums(quantise(m.data), m.indptr)
    assert np.array_equal(out["refsize"], np.bincount(refined, minlength=n))
    assert np.array_equal(out["Kref"], _sum_by(refined, k, n))
    assert out["merges"] == n - np.unique(refined).size


def well_connected(m, membership, resolution):
    """-> (a_in, threshold, near): a_in[v] = w(v, C - v) in int64, threshold = (gamma / 2m) k_v (K_C - k_v) in float64 as
    ld_refine_candidates_kernel computes it, near = within relative 1e-9 of it (where float64 rounding may decide)"""
    membership = np.asarray(membership)
    wq = quantise(m.data)
    rows = _rows(m)
    k = _segment_sums(wq, m.indptr)
    inside = (membership[rows] == membership[m.indices]) & (rows != m.indices)
    a_in = _segment_sums(np.where(inside, wq, 0), m.indptr)
    _, comm_ix = np.unique(membership, return_inverse=True)
    k_c = _sum_by(comm_ix, k, comm_ix.max() + 1)[comm_ix]
    thr = (resolution / float(k.sum())) * k.astype(np.float64) * (k_c - k).astype(np.float64)
    near = np.abs(a_in.astype(np.float64) - thr) <= 1e-9 * np.maximum(thr, 1.0)
    return a_in, thr, near


def check_refinement(m, membership, resolution, out):
    """what the refinement guarantees of ANY draw: nested, connected groups; only well-connected vertices leave their
    singleton; and the sums it keeps per group equal a from-scratch recomputation"""
    n = m.shape[0]
    membership = np.asarray(membership)
    ref = out["refined"].astype(np.int64)
    wq = quantise(m.data)
    rows, cols = _rows(m), m.indices.astype(np.int64)
    k = _segment_sums(wq, m.indptr)
    assert ref.min() >= 0 and ref.max() < n and (ref[ref] == ref).all(), "a group is not named by one of its members"
    assert (membership[ref] == membership).all(), "a refined group crosses communities"
    reps = np.unique(ref)
    # connected through positive-weight edges inside itself
    keep = (ref[rows] == ref[cols]) & (wq > 0)
    sub = sparse.csr_matrix((np.ones(int(keep.sum()), dtype=np.int8), (rows[keep], cols[keep])), shape=(n, n))
    n_comp, _ = connected_components(sub, directed=False)
    assert n_comp == reps.size, f"{n_comp} connected pieces in {reps.size} refined groups"
    # a vertex that is not well connected stays a singleton; nobody joins it either
    a_in, thr, near = well_connected(m, membership, resolution)
    assert near.mean() <= 0.01
    poor = (a_in.astype(np.float64) < thr) & ~near
    size = np.bincount(ref, minlength=n)
    assert (ref[poor] == np.flatnonzero(poor)).all() and (size[poor] == 1).all(), "a vertex that is not well connected was merged"
    lone = np.diff(m.indptr) == 0
    assert (ref[lone] == np.flatnonzero(lone)).all() and (size[lone] == 1).all(), "an isolated vertex was merged"
    # the sums at the representatives, zero elsewhere
    assert np.array_equal(out["refsize"], size)
    assert np.array_equal(out["Kref"], _sum_by(ref, k, n))
    cut = (membership[rows] == membership[cols]) & (ref[rows] != ref[cols])
    want_e = _sum_by(ref[rows[cut]], wq[cut], n)
    bad = np.flatnonzero(out["Eref"] != want_e)
    assert bad.size == 0, f"Eref differs at {bad.size} representatives, first {bad[0]}: got {out['Eref'][bad[0]]} want {want_e[bad[0]]}"
    assert out["merges"] == n - reps.size
    return a_in, thr, near


def same_outputs(a, b):
    """two calls gave the same refinement and the same coarse graph (the order of a row's entries is free)"""
    for key in ("merges", "n_coarse", "coarse_nnz", "skipped"):
        assert a[key] == b[key], key
    for key in ("refined", "Kref", "Eref", "refsize") + (() if a["skipped"] else ("cid", "indptr", "k", "comm")):
        assert np.array_equal(a[key], b[key]), key
    if not a["skipped"]:
        nn = a["n_coarse"]
        ca, cb = (_canonical(nn, np.repeat(np.arange(nn), np.diff(o["indptr"])), o["indices"], o["wq"]) for o in (a, b))
        assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1])


# ---- graphs ------------------------------------------------------------------------------------------------------------------
def _csr(n, rows, cols, w):
    m = sparse.csr_matrix((np.asarray(w, dtype=np.float32), (rows, cols)), shape=(n, n))
    m.sort_indices()
    assert m.nnz == len(rows), "duplicate entries"
    return m


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def random_graph(n, deg, seed):
    """every vertex draws `deg` neighbours, symmetrised; float32 weights in [0.1, 1)"""
    rng = np.random.default_rng(seed)
    a = sparse.coo_matrix((np.ones(n * deg), (np.repeat(np.arange(n), deg), rng.integers(0, n, n * deg))), shape=(n, n)).tocsr()
    a.setdiag(0)
    a.eliminate_zeros()
    return tier_cases._symmetric_weights((a + a.T).astype(bool), rng)


def planted_graph(n, n_blocks, k_in, k_out, seed):
    """a kNN-like graph: every vertex draws k_in neighbours inside its block and k_out anywhere, symmetrised -> (graph, block)"""
    rng = np.random.default_rng(seed)
    blk = np.arange(n) % n_blocks
    per = n // n_blocks
    src = np.repeat(np.arange(n), k_in)
    inside = (rng.integers(0, per, n * k_in) * n_blocks + blk[src]) % n
    a = sparse.coo_matrix((np.ones(n * (k_in + k_out)), (np.concatenate((src, np.repeat(np.arange(n), k_out))),
                                                         np.concatenate((inside, rng.integers(0, n, n * k_out))))), shape=(n, n)).tocsr()
    a.setdiag(0)
    a.eliminate_zeros()
    return tier_cases._symmetric_weights((a + a.T).astype(bool), rng), blk


def groups_within(membership, sizes, seed):
    """a refined partition nested in `membership`: groups of the given sizes cut from shuffled members of one community after
    the other (what is left over stays single); every group is named by a member that is NOT its smallest"""
    rng = np.random.default_rng(seed)
    membership = np.asarray(membership)
    ref = np.arange(membership.size)
    pools = [rng.permutation(np.flatnonzero(membership == c)) for c in np.unique(membership)]
    used = [0] * len(pools)
    for i, s in enumerate(sizes):
        for j in range(len(pools)):
            p = (i + j) % len(pools)
            if used[p] + s <= pools[p].size:
                members = pools[p][used[p]:used[p] + s]
                used[p] += s
                ref[members] = np.sort(members)[-1]
                break
        else:
            raise AssertionError(f"no community has {s} members left")
    return ref


def hub_graph(groups, n_fill, seed, *, disjoint=False, intra=True, symmetric=False, fill_pairs=1):
    """one refined group per list of `groups`, one member per element: a vertex whose row has EXACTLY that many entries, all to
    `n_fill` filler vertices (no edges among themselves) -- but for one entry from the first member of a group to its second
    (`intra`: the coarse row then has a self entry).  disjoint: the members of a group share no neighbour (the row's distinct
    neighbours are its entries).  The fillers are single but for `fill_pairs` groups of two; symmetric: they get the entries
    back (otherwise their rows are empty).  Ids are shuffled; communities: every hub group with a third of the fillers.  -> (graph, membership, refined)"""
    rng = np.random.default_rng(seed)
    n_hub = sum(len(g) for g in groups)
    n = n_hub + n_fill
    ids = rng.permutation(n)
    hub_ids, fill_ids = ids[:n_hub], ids[n_hub:]
    refined = np.arange(n)
    comm_of = np.empty(n, dtype=np.int64)
    comm_of[fill_ids] = np.arange(n_fill) // 2 % 3  # (pairs of consecutive fillers share a community)
    for p in range(fill_pairs):
        refined[fill_ids[2 * p:2 * p + 2]] = fill_ids[2 * p:2 * p + 2].max()
    rows, cols = [], []
    at = 0
    for gi, lengths in enumerate(groups):
        members = hub_ids[at:at + len(lengths)]
        at += len(lengths)
        refined[members] = members[len(members) // 2]
        comm_of[members] = gi % 3
        link = intra and len(lengths) >= 2 and lengths[0] >= 1
        n_ext = sum(lengths) - int(link)
        pool = rng.choice(n_fill, n_ext, replace=False) if disjoint else None
        used = 0
        for mi, length in enumerate(lengths):
            ext = length - int(link and mi == 0)
            if disjoint:
                t = pool[used:used + ext]
                used += ext
            else:
                t = rng.choice(n_fill, ext, replace=False)
            rows.append(np.full(ext, members[mi]))
            cols.append(fill_ids[t])
            if link and mi == 0:
                rows.append(members[:1])
                cols.append(members[1:2])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    w = rng.random(rows.size) * 0.9 + 0.1
    if symmetric:  # (the fillers get their entries back; the entry inside a group stays one-way: the rows keep their lengths)
        back = np.isin(cols, fill_ids)
        rows, cols, w = np.concatenate((rows, cols[back])), np.concatenate((cols, rows[back])), np.concatenate((w, w[back]))
    m = _csr(n, rows, cols, w)
    assert np.array_equal(np.diff(m.indptr)[hub_ids], [x for g in groups for x in g])
    # a community is named by its LARGEST member: the coarse label (smallest coarse vertex) is not a copy of it
    membership = np.empty(n, dtype=np.int64)
    for c in np.unique(comm_of):
        membership[comm_of == c] = np.flatnonzero(comm_of == c).max()
    return m, membership, refined


def _random_case(n, seed, sizes):
    m = random_graph(n, 3, seed)
    membership = np.arange(n) % 4 + n - 4  # (labels are vertex ids, not 0 .. 3)
    return m, membership, groups_within(membership, sizes, seed)


def _special_weights():
    """a weight of 0, a negative one, a subnormal, ties of the rounding (1.5 and 2.5 units of 2^-32: both round to 2) and 1.0 in
    one row; stored entries that differ between (u, v) and (v, u), or exist in one direction only"""
    unit = 2.0 ** -32
    rows = [0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 3, 4, 6, 6, 7, 7]
    cols = [1, 2, 3, 4, 5, 6, 7, 0, 0, 4, 7, 3, 0, 7, 6, 2]
    w = [0.0, 1e-40, 1.0, 1.5 * unit, 2.5 * unit, -1.0, 0.75, 0.5, 0.0, 0.25, 1e-40, 0.125, 1.0, 0.0, 3.5 * unit, 1.0]
    m = _csr(9, rows, cols, w)  # (vertex 8: isolated)
    assert (m.data == 0).sum() == 3 and (m != m.T).nnz > 0
    membership = np.array([8, 8, 8, 5, 5, 8, 8, 8, 8])
    refined = np.array([1, 1, 2, 4, 4, 5, 7, 7, 8])
    return m, membership, refined


# name -> (builder -> (graph, membership, refined_in), environment, rows (512-thread, 1024-thread, split) or None, platforms)
BOTH, GPU = ("gpu", "emu"), ("gpu",)
SPLIT64 = {"SCAMD_LEIDEN_AGG_WAVE_WORK": "32", "SCAMD_LEIDEN_AGG_SPLIT_CHUNK": "64", "SCAMD_LEIDEN_AGG_SPLIT_WORK": "64"}
_BIG = lambda: hub_graph([[1500, 1501], [2100, 2101]], 4300, 7, disjoint=True, symmetric=True)  # noqa: E731
_SPLIT_GROUPS = [[130], [64, 1], [64, 64], [30] * 5, [65, 65, 1], [1] * 66, [200, 0, 3]]
AGG_CASES = {
    # the member fetch loop of the wave builder: the odd last pair, the second block of 64 members
    "member_counts": (lambda: _random_case(640, 1, [1, 2, 63, 64, 65, 129]), {}, (0, 0, 0), BOTH),
    # member rows of 0 / 64 / 65 / 130 entries (the tails beyond the first 64 of a row), a group of isolated members only; pairs
    # and triples of long rows: both rows of a pair have a tail whatever the order of the members
    "member_rows": (lambda: hub_graph([[0, 64, 65, 130], [130, 65, 64], [0, 0, 0], [64, 64], [65], [130, 130], [65, 65, 65]], 200, 2,
                                      symmetric=True), {}, (0, 0, 0), BOTH),
    # the wave builder's tables: 96 | 97, 192 | 193, 384 | 385 distinct neighbours (385: the 512-thread builder)
    "wave_tables": (lambda: hub_graph([[48, 48], [48, 49], [96, 96], [96, 97], [192, 192], [192, 193]], 450, 3, disjoint=True), {},
                    (1, 0, 0), BOTH),
    # member entries 2048 | 2049: the wave builder | the 512-thread builder, on a level of <= 384 coarse vertices
    "wave_work_bound": (lambda: hub_graph([[64] * 32, [64] * 31 + [65]], 300, 4), {}, (1, 0, 0), BOTH),
    # ... 65536 | 65537: the 512-thread | the 1024-thread builder, on a level of <= 2048 coarse vertices
    "mid_work_bound": (lambda: hub_graph([[1024] * 64, [1024] * 63 + [1025]], 1500, 5), {}, (1, 1, 0), BOTH),
    # a row that touches every one of 2048 | 2049 coarse vertices, itself included
    "mid_table_2048": (lambda: hub_graph([[1024, 1024]], 2047, 6, disjoint=True, fill_pairs=0), {}, (1, 0, 0), BOTH),
    "mid_table_2049": (lambda: hub_graph([[1025, 1024]], 2048, 6, disjoint=True, fill_pairs=0), {}, (0, 1, 0), BOTH),
    # the 8192-slot table: 3001 keys in one pass; 4201 (> AGG_PASS_KEYS) after the optimistic pass, by class passes alone, and
    # after a trial that gives up at its first long probe
    "big_table": (_BIG, {}, (0, 2, 0), BOTH),
    "big_table_class_passes": (_BIG, {"SCAMD_LEIDEN_HUB_TRY_PROBES": "0"}, (0, 2, 0), BOTH),
    "big_table_failed_trial": (_BIG, {"SCAMD_LEIDEN_HUB_TRY_PROBES": "1"}, (0, 2, 0), BOTH),
    # split rows at the default bounds: 262400 member entries on a level of 5600 coarse vertices (three parts, the last without
    # a member), and on one of 5601, which one table cannot merge: the 1024-thread builder
    "split_default_nn5600": (lambda: hub_graph([[1025] * 256], 5599, 8, fill_pairs=0), {}, (0, 0, 1), GPU),
    "split_default_nn5601": (lambda: hub_graph([[1025] * 256], 5600, 8, fill_pairs=0), {}, (0, 1, 0), GPU),
    # parts of 64 entries: one member row across every cut (one part with members), a last part of one entry, full parts, parts
    # of several members, single-entry members
    "split_parts": (lambda: hub_graph(_SPLIT_GROUPS, 300, 9), SPLIT64, (0, 0, 7), BOTH),
    "split_nn5600": (lambda: hub_graph([[40, 41]], 5599, 10, fill_pairs=0), SPLIT64, (0, 0, 1), BOTH),
    "split_nn5601": (lambda: hub_graph([[40, 41]], 5600, 10, fill_pairs=0), SPLIT64, (1, 0, 0), BOTH),
    "one_group": (lambda: (random_graph(200, 3, 11), np.full(200, 44), np.full(200, 17)), {}, (0, 0, 0), BOTH),
    "identity": (lambda: (random_graph(200, 3, 11), np.arange(200) % 4, np.arange(200)), {}, None, BOTH),
    "special_weights": (_special_weights, {}, (0, 0, 0), BOTH),
}

# every forced builder of test_gpu_leiden.py:test_leiden_coarse_row_tiers_agree, on one random case; the tier each must reach
_W0 = {"SCAMD_LEIDEN_AGG_WAVE_MAX": "0"}
_B0 = dict(_W0, SCAMD_LEIDEN_AGG_MID_MAX="0")
_P16 = dict(_B0, SCAMD_LEIDEN_AGG_PASS_KEYS="16")
FORCED = {
    "default": ({}, None),
    "mid": (_W0, "n_mid"),
    "big": (_B0, "n_big"),
    "big-multipass": (_P16, "n_big"),
    "big-classpasses": (dict(_P16, SCAMD_LEIDEN_HUB_TRY_PROBES="0"), "n_big"),
    "big-failed-trial": (dict(_P16, SCAMD_LEIDEN_HUB_TRY_PROBES="1"), "n_big"),
    "work-tiers": ({"SCAMD_LEIDEN_AGG_WAVE_WORK": "64", "SCAMD_LEIDEN_AGG_MID_WORK": "512"}, "n_big"),
    "split-64": (SPLIT64, "n_split"),
    "split-1024": ({"SCAMD_LEIDEN_AGG_SPLIT_CHUNK": "1024", "SCAMD_LEIDEN_AGG_SPLIT_WORK": "4096"}, "n_split"),
}


def _forced_case():
    m, blk = planted_graph(3000, 4, 6, 2, 12)
    membership = blk + 2990  # (labels are vertex ids, not 0 .. 3)
    sizes = [700, 300, 150, 90, 40] + [17] * 20 + [5] * 60 + [2] * 100
    return m, membership, groups_within(membership, sizes, 12)


_built = {}


def _once(key, builder):
    """computed once, never written"""
    if key not in _built:
        m, membership, refined = builder()
        membership, refined = np.asarray(membership, dtype=np.int32), np.asarray(refined, dtype=np.int32)
        _freeze(m.data, m.indices, m.indptr, membership, refined)
        _built[key] = (m, membership, refined)
    return _built[key]


def agg_case_names(platform):
    return sorted(name for name, c in AGG_CASES.items() if platform in c[3])


def _set_env(monkeypatch, env):
    for key in AGG_ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)


def run_agg_case(run, name, monkeypatch):
    builder, env, tiers, _ = AGG_CASES[name]
    m, membership, refined = _once(builder if name.startswith("big_table") else name, builder)
    _set_env(monkeypatch, env)
    out = run.level(m, membership, refined_in=refined)
    print(f"{name}: n={m.shape[0]} nnz={m.nnz} -> {out['n_coarse']} coarse vertices, {out['coarse_nnz']} entries; rows beyond the wave "
          f"builder {(out['n_mid'], out['n_big'], out['n_split'])}")
    check_group_sums(m, refined, out)
    assert not out["Eref"].any()
    check_aggregation(m, membership, refined, out, tiers)
    return out


def run_forced_case(run, name, monkeypatch):
    env, tier = FORCED[name]
    m, membership, refined = _once("forced", _forced_case)
    _set_env(monkeypatch, env)
    out = run.level(m, membership, refined_in=refined)
    print(f"forced {name}: {out['n_coarse']} coarse vertices; rows beyond the wave builder {(out['n_mid'], out['n_big'], out['n_split'])}")
    check_group_sums(m, refined, out)
    check_aggregation(m, membership, refined, out)
    if tier is not None:
        assert out[tier] > 0, f"no row went through the builder {name} is to force"
    else:
        assert out["n_mid"] > 0 and out["n_big"] == 0 and out["n_split"] == 0  # (the groups of 700 .. 90: beyond the wave's work bound)
    return out


# ---- refinement inputs -------------------------------------------------------------------------------------------------------
def _odd_labelling():
    """two blocks without an edge between them under ONE label, a vertex that is a community by itself, isolated vertices
    inside a community and as communities of their own"""
    m, blk = planted_graph(900, 3, 6, 2, 13)
    a = m.toarray()
    cut = (blk[:, None] == 0) & (blk[None, :] == 1)
    a[cut | cut.T] = 0
    for v in (7, 8, 9, 301, 302):
        a[v, :] = 0
        a[:, v] = 0
    a = sparse.csr_matrix(a)
    assert a[blk == 0][:, blk == 1].nnz == 0
    membership = np.where(blk == 2, 899, 898)  # blocks 0 and 1: one community, disconnected
    membership[10] = 10    # a community of one vertex (with edges)
    membership[8] = 8      # an isolated vertex as a community
    membership[301] = 301
    return a, membership


def _boundary():
    bounds = sorted({x for t in tier_cases.RECORDED_BOUNDS.values() for x in t})
    m = tier_cases.boundary_graph(bounds).tocsr()
    m.sort_indices()
    return m, np.arange(m.shape[0]) % 4


# name -> (builder -> (graph, membership), resolution)
REFINE_CASES = {
    "planted": (lambda: tuple(planted_graph(3000, 10, 6, 2, 14)), 1.0),
    "one_community": (lambda: (planted_graph(3000, 10, 6, 2, 14)[0], np.full(3000, 5)), 1.0),
    "odd_labelling": (_odd_labelling, 1.0),
    # rows of 96 | 97 .. 1536 | 1537 entries among the candidates: the wave, block and giant tiers of the propose step
    "boundary_rows": (_boundary, 0.5),
}
BETAS = (0.01, 0.0)
SEEDS = (0, 1)


def refine_input(name):
    if ("refine", name) not in _built:
        m, membership = REFINE_CASES[name][0]()
        m = m.tocsr()
        membership = np.asarray(membership, dtype=np.int32)
        assert (m != m.T).nnz == 0 and m.diagonal().sum() == 0 and (m.data > 0).all()
        # (the generator's own check: float64 rounding may decide the well-connectedness of at most 1 % of the vertices)
        assert well_connected(m, membership, REFINE_CASES[name][1])[2].mean() <= 0.01
        _freeze(m.data, m.indices, m.indptr, membership)
        _built[("refine", name)] = (m, membership)
    return _built[("refine", name)]


def run_refine_case(run, name, beta, seed, monkeypatch):
    """QUAD 0 / 1 / 2 and a repeated call give the same outputs; they hold what check_refinement asks, and the coarse graph
    built under the refinement's own result is P^T Wq P"""
    m, membership = refine_input(name)
    resolution = REFINE_CASES[name][1]
    _set_env(monkeypatch, {})
    deg = np.diff(m.indptr)
    if name == "boundary_rows":  # (the input's own property: at least two candidates in every tier of a 16-lane propose step)
        a_in, thr, near = well_connected(m, membership, resolution)
        for lo, hi in zip(run.bounds(16), run.bounds(16)[1:] + (1 << 30,)):
            assert ((a_in.astype(np.float64) >= thr) & ~near & (deg > lo) & (deg <= hi)).sum() >= 2, f"no candidate row in ({lo}, {hi}]"
    outs = {}
    for quad in QUADS + ("0",):
        monkeypatch.setenv("SCAMD_LEIDEN_QUAD", quad)
        out = run.level(m, membership, resolution=resolution, beta=beta, seed=seed)
        st = run.stats()
        if quad not in outs:
            print(f"{name} beta={beta} seed={seed} QUAD={quad}: {out['merges']} merges -> {out['n_coarse']} groups; hub pass "
                  f"{st['hub_pass_vertices']} overflow pass {st['overflow_pass_vertices']}")
            a_in, thr, near = check_refinement(m, membership, resolution, out)
            check_aggregation(m, membership, out["refined"], out)
            # every candidate proposes exactly once, in the tier of its row
            cand = a_in.astype(np.float64) >= thr
            main_max, wave_max, block_max = run.bounds(tier_cases.LANES[quad])
            lanes16 = tier_cases.LANES[quad] == 16  # (32 lanes: the refinement runs its 64-lane kernels)
            if not near[deg > main_max].any():
                assert st["hub_pass_vertices"] == int((cand & (deg > wave_max)).sum())
                assert st["overflow_pass_vertices"] == (int((cand & (deg > main_max)).sum()) if lanes16 else 0)
            outs[quad] = out
        else:
            same_outputs(outs["0"], out)  # the repeated call
    for quad in QUADS[1:]:
        same_outputs(outs["0"], outs[quad])
    assert outs["0"]["merges"] > 0 or name == "odd_labelling"
    return outs["0"]


# ---- two gaps of the run itself: the renumbering's tie rule, the one-workgroup path at its entry bounds ------------------------
def renumber_case():
    """disjoint cliques -- two of 7, six of 5, three of 3 -- on shuffled ids, and four isolated vertices: the run must return
    exactly the cliques, numbered by decreasing size and, among equals, by their smallest member -> (graph, the labels)"""
    rng = np.random.default_rng(21)
    sizes = [5, 3, 7, 5, 5, 1, 3, 5, 1, 7, 5, 3, 1, 5, 1]
    n = sum(sizes)
    ids = rng.permutation(n)
    a = np.zeros((n, n), dtype=np.float32)
    groups, at = [], 0
    for s in sizes:
        g = ids[at:at + s]
        at += s
        a[np.ix_(g, g)] = 1.0
        groups.append(g)
    np.fill_diagonal(a, 0.0)
    groups.sort(key=lambda g: (-g.size, g.min()))
    want = np.empty(n, dtype=np.int64)
    for label, g in enumerate(groups):
        want[g] = label
    assert len({(g.size, g.min()) for g in groups}) == len(groups) and [g.size for g in groups[:3]] == [7, 7, 5]
    return sparse.csr_matrix(a), want


def check_renumbering(run):
    m, want = renumber_case()
    for seed in SEEDS:
        memb, q, nc = run.leiden(m, seed=seed)
        assert nc == want.max() + 1
        assert np.array_equal(memb, want), "communities of equal size are not numbered by their smallest member"


def _planted_edges(n, n_blocks, n_in, n_out, seed):
    """exactly n_in + n_out undirected edges, n_in of them inside the blocks; weights k / 64 (exact in the fixed point)"""
    rng = np.random.default_rng(seed)
    blk = np.arange(n) % n_blocks
    iu, ju = np.triu_indices(n, k=1)
    same = blk[iu] == blk[ju]
    pick = np.concatenate((rng.choice(np.flatnonzero(same), n_in, replace=False), rng.choice(np.flatnonzero(~same), n_out, replace=False)))
    w = rng.integers(8, 64, pick.size) / 64.0
    m = sparse.coo_matrix((w, (iu[pick], ju[pick])), shape=(n, n)).tocsr()
    return (m + m.T).tocsr().astype(np.float32)


def _plus_vertex(m, targets):
    n = m.shape[0]
    a = sparse.lil_matrix((n + 1, n + 1), dtype=np.float32)
    a[:n, :n] = m
    for t in targets:
        a[n, t] = a[t, n] = 0.5
    return a.tocsr()


# name -> (graph, its n, its nnz, does the run start in the one-workgroup kernel: n <= SMALL_N = 1024 and nnz <= SMALL_NNZ = 65536)
SMALL_ENTRY_CASES = {
    "n17": (lambda: _planted_edges(17, 2, 40, 12, 31), 17, 104, True),  # the first size above SMALL_SEQ_N = 16
    "n1024_nnz65536": (lambda: _planted_edges(1024, 16, 24000, 8768, 32), 1024, 65536, True),
    "n1024_nnz65538": (lambda: _planted_edges(1024, 16, 24000, 8769, 32), 1024, 65538, False),
    "n1025": (lambda: _plus_vertex(_planted_edges(1024, 16, 12000, 3000, 33), (3, 19, 500)), 1025, 30006, False),
}


def check_small_entry_case(run, name):
    """the stable partition: connected communities, no improving move, no mergeable pair, Q that of the labels"""
    from oracle import leiden as ol
    from oracle import leiden_guarantees as lg

    builder, n, nnz, small = SMALL_ENTRY_CASES[name]
    m = _once(("small", name), lambda: (builder(), np.zeros(1), np.zeros(1)))[0]
    assert m.shape == (n, n) and m.nnz == nnz and (m != m.T).nnz == 0
    memb, q, nc = run.leiden(m, n_iterations=-1, seed=0)
    st = run.stats()
    print(f"{name}: n={n} nnz={m.nnz} Q={q!r} communities={nc} levels by separate kernels in the first iteration {st['levels_first_iteration']}")
    assert (st["levels_first_iteration"] == 0) == small, "the run did not start on the path the case is for"
    assert abs(q - ol.modularity(m, memb)) < 1e-9 and nc == int(memb.max()) + 1
    same = memb[_rows(m)] == memb[m.indices]
    inner = sparse.csr_matrix((same.astype(np.int8), m.indices.copy(), m.indptr.copy()), shape=m.shape)
    inner.eliminate_zeros()
    assert connected_components(inner, directed=False)[0] == nc
    im, mp = lg.improving_moves(m, memb), lg.mergeable_pairs(m, memb)
    assert im["count"] == 0, im
    assert mp["count"] == 0, mp
