"""TEST INFRASTRUCTURE shared by tests/test_gpu_scrublet.py (the product library on the GPU), tests/test_emu_scrublet_cpu.py (the
same kernels on the host emulator) and tests/test_scrublet_front_cpu.py (the front end on a CPU stand-in): the case tables of
csrc/scrublet.hip (`scamd_pp_scrublet_pair_count`, `scamd_pp_scrublet_pair_fill_f32`, `scamd_scrublet_scores_f64`), the lane-group
rules restated, callers through the raw C ABI over host memory (tests/emu/harness.py:HostMem) or device memory
(graph_kernel_cases.DeviceMem), a count generator with planted doublets, a float64 restatement of the whole pipeline (scipy row
sums, numpy z-score, sklearn PCA(arpack) / TruncatedSVD, brute-force NearestNeighbors, the score formulas) and a CPU stand-in
for the three `GpuPPBackend.scrublet_*` methods.  Nothing here touches a device.

Tolerances: none.  Row-pair sums of float32 values are one IEEE addition each and are compared bitwise; the neighbour counts
are integers; the scores are float64 formulas of IEEE operations in a fixed order and are compared bitwise with numpy."""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
from scipy import sparse

from graph_kernel_cases import EINVAL, EUNSUPPORTED, DeviceMem  # noqa: F401  (DeviceMem: for the GPU tests)
from stub_backend import CpuStubPPBackend

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "scanpy_amd" / "csrc"

# ---------------------------------------------------------------------------------------------------------------------
# The dispatch rules restated; `assert_sources_still_say_so` ties them to the text of csrc/scrublet.hip.
# ---------------------------------------------------------------------------------------------------------------------
SB_BLOCK = 256
SB_GRID_CAP = 256 * 32
SB_G = (8, 16, 32, 64)
FLAG_INEXACT, FLAG_BAD_PAIR, FLAG_CAPACITY = 1, 2, 4


def pair_lanes(nnz: int, n: int) -> int:
    avg = nnz // n if n > 0 else 0
    return 8 if avg <= 32 else (16 if avg <= 160 else (32 if avg <= 512 else 64))


def score_lanes(k: int) -> int:
    return 8 if k <= 8 else (16 if k <= 16 else (32 if k <= 32 else 64))


def assert_sources_still_say_so():
    src = (CSRC / "scrublet.hip").read_text()

    def has(pattern, what):
        assert re.search(pattern, src), f"{what}: /{pattern}/ no longer in csrc/scrublet.hip -- restate the rule and its cases"

    has(rf"constexpr int SB_BLOCK = {SB_BLOCK};", "SB_BLOCK")
    has(r"constexpr int SB_GRID_CAP = 256 \* 32;", "SB_GRID_CAP")
    has(r"constexpr float SB_EXACT_MAX = 16777216\.0f;", "2^24")
    has(r"return avg <= 32 \? 8 : \(avg <= 160 \? 16 : \(avg <= 512 \? 32 : 64\)\);", "sb_lanes_per_row")
    has(r"return k <= 8 \? 8 : \(k <= 16 \? 16 : \(k <= 32 \? 32 : 64\)\);", "sb_score_lanes")
    has(r"SB_FLAG_INEXACT = 1u, SB_FLAG_BAD_PAIR = 2u, SB_FLAG_CAPACITY = 4u;", "flag bits")
    for G in SB_G[:-1]:
        for what in ("count", "fill", "scores"):
            has(rf"case {G}: sb_launch_{what}<{G}>\(", f"{what} G = {G}")
    for what in ("count", "fill", "scores"):
        has(rf"default: sb_launch_{what}<64>\(", f"{what} G = 64")
    has(r"const int64_t at = o0 \+ p \+ pos_a - \(carry_a \+ __popcll\(ma & below\)\);", "the rank formula, row A")
    has(r"const int64_t at = o0 \+ p \+ pos_b - \(carry_b \+ __popcll\(mb & below\)\);", "the rank formula, row B")


# ---------------------------------------------------------------------------------------------------------------------
# Pair-kernel cases: name -> (x CSR float32 canonical, pairs int32 [n_sim, 2], row_total dtype, flags expected)
# ---------------------------------------------------------------------------------------------------------------------
def _rows_matrix(rows, g, values=None, seed=0):
    """rows: list of sorted column lists -> CSR float32 with integer values 1 .. 9 (or `values`: list of value lists)"""
    rng = np.random.default_rng(seed)
    ln = np.array([len(r) for r in rows], dtype=np.int64)
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if ln.sum() else np.zeros(0, np.int32)
    if values is None:
        data = rng.integers(1, 10, int(ln.sum())).astype(np.float32)
    else:
        data = np.concatenate([np.asarray(v, dtype=np.float32) for v in values]) if ln.sum() else np.zeros(0, np.float32)
    x = sparse.csr_matrix((data, indices.astype(np.int32), np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)), shape=(len(rows), g))
    assert x.has_sorted_indices and all(len(set(r)) == len(r) for r in rows)
    return x


def _random_rows(lengths, g, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(g, size=int(ln), replace=False)) for ln in lengths]


def _all_pairs(m):
    return np.array([(i, j) for i in range(m) for j in range(m)], dtype=np.int32).reshape(-1, 2)


def _lengths_case(lead, filler, n_filler, g, seed):
    lengths = list(lead) + [filler] * n_filler
    x = _rows_matrix(_random_rows(lengths, g, seed), g, seed=seed)
    return x, _all_pairs(len(lead))


@lru_cache(maxsize=None)
def pair_case(name: str):
    big = float(2 ** 23)
    if name == "n1-self":
        return _rows_matrix([[0, 2, 4]], 5), np.array([[0, 0]], np.int32), np.float32, 0
    if name == "nsim0":
        return _rows_matrix([[0, 1], [2]], 5), np.zeros((0, 2), np.int32), np.float64, 0
    if name == "g1":
        return _rows_matrix([[0], [], [0], [0]], 1), _all_pairs(4), np.float64, 0
    if name == "both-empty":
        return _rows_matrix([[], [], [1, 2]], 4), np.array([[0, 1], [1, 1], [0, 0]], np.int32), np.float32, 0
    if name == "one-empty":
        return _rows_matrix([[], [0, 3, 7, 8]], 9), np.array([[0, 1], [1, 0]], np.int32), np.float32, 0
    if name == "disjoint":
        return _rows_matrix([[0, 2, 4, 6], [1, 3, 5, 7, 9], [10, 11], [8]], 12), _all_pairs(4), np.float64, 0
    if name == "identical":
        return _rows_matrix([[1, 4, 5, 9], [1, 4, 5, 9]], 10), np.array([[0, 1], [1, 0], [0, 0]], np.int32), np.float32, 0
    if name == "ij-ji":
        x = _rows_matrix(_random_rows([20, 31, 7], 40, 5), 40, seed=5)
        return x, np.array([[0, 1], [1, 0], [2, 1], [1, 2]], np.int32), np.float64, 0
    if name == "match-first-last":
        rows = [[0, 5, 9], [0, 3, 8], [1, 4, 9], [0, 9], [0], [9]]
        return _rows_matrix(rows, 10), _all_pairs(6), np.float32, 0
    if name == "stored-zero":
        rows = [[1, 3, 5], [1, 4, 5], [3]]
        return _rows_matrix(rows, 6, values=[[0.0, 2.0, 0.0], [0.0, 1.0, 7.0], [0.0]]), _all_pairs(3), np.float32, 0
    if name == "values-2^23":
        rows = [[0, 1, 2], [1, 2, 3]]
        return _rows_matrix(rows, 4, values=[[big, big, 1.0], [big, big - 1, big]]), _all_pairs(2), np.float64, 0
    if name == "sum-beyond-2^24":
        rows = [[0, 1, 2], [1, 2, 3]]
        return _rows_matrix(rows, 4, values=[[1.0, big + 1, 1.0], [big + 1, 2.0, 3.0]]), np.array([[0, 1]], np.int32), np.float32, FLAG_INEXACT
    # row lengths 63 / 64 / 65 and 2049 against 3 under every lane-group size (the filler rows steer the mean row length)
    if name == "len-G8":
        return _lengths_case([63, 64, 65, 7, 8, 9, 0], 1, 40, 300, 11) + (np.float32, 0)
    if name == "len-2049v3-G8":
        return _lengths_case([2049, 3, 0, 2048], 0, 200, 4096, 12) + (np.float64, 0)
    if name == "len-G16":
        return _lengths_case([63, 64, 65, 15, 16, 17, 33], 60, 10, 300, 13) + (np.float32, 0)
    if name == "len-G32":
        return _lengths_case([63, 64, 65, 31, 32, 33, 300], 290, 10, 300, 14) + (np.float64, 0)
    if name == "len-G64":
        return _lengths_case([63, 64, 65, 2049, 3, 129], 1500, 6, 4096, 15) + (np.float32, 0)
    if name == "big":
        rng = np.random.default_rng(16)
        x = sparse.random(3000, 2049, density=0.05, format="csr", dtype=np.float32, random_state=16)
        x.data = np.ceil(x.data * 40).astype(np.float32)
        x.sort_indices()
        x = sparse.csr_matrix((x.data, x.indices.astype(np.int32), x.indptr.astype(np.int64)), shape=x.shape)
        return x, rng.integers(0, 3000, (6000, 2)).astype(np.int32), np.float32, 0
    raise KeyError(name)


PAIR_CASES = ("n1-self", "nsim0", "g1", "both-empty", "one-empty", "disjoint", "identical", "ij-ji", "match-first-last", "stored-zero",
              "values-2^23", "sum-beyond-2^24", "len-G8", "len-2049v3-G8", "len-G16", "len-G32", "len-G64", "big")
RERUN_CASES = ("big",)


def assert_every_pair_path_has_a_case():
    lanes = set()
    for name in PAIR_CASES:
        x, pairs, _, _ = pair_case(name)
        lanes.add(pair_lanes(x.nnz, x.shape[0]))
    assert lanes == set(SB_G), lanes
    for name, G in (("len-G8", 8), ("len-2049v3-G8", 8), ("len-G16", 16), ("len-G32", 32), ("len-G64", 64)):
        x, _, _, _ = pair_case(name)
        assert pair_lanes(x.nnz, x.shape[0]) == G, (name, x.nnz // x.shape[0])
        ln = np.diff(x.indptr)
        assert {G - 1, G, G + 1} <= set(ln.tolist()) or name == "len-2049v3-G8", name   # a length either side of the group size
    x, pairs, _, _ = pair_case("big")
    assert x.shape == (3000, 2049) and len(pairs) == 6000 and -(-6000 // (SB_BLOCK // pair_lanes(x.nnz, 3000))) > 1   # several blocks
    return lanes


def expected_pairs(x, pairs):
    """scipy's X[a] + X[b] made canonical WITHOUT dropping anything: the entries of both rows as COO duplicates, summed"""
    n_sim = len(pairs)
    ln = np.diff(x.indptr)
    parts_r, parts_c, parts_v = [], [], []
    for side in (0, 1):
        src = pairs[:, side].astype(np.int64)
        cnt = ln[src]
        out_row = np.repeat(np.arange(n_sim), cnt)
        start = np.repeat(x.indptr[src], cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        at = start + within
        parts_r.append(out_row), parts_c.append(x.indices[at]), parts_v.append(x.data[at])
    coo = sparse.coo_matrix((np.concatenate(parts_v).astype(np.float32), (np.concatenate(parts_r), np.concatenate(parts_c))),
                            shape=(n_sim, x.shape[1]))
    out = coo.tocsr()
    out.sum_duplicates()
    out.sort_indices()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Callers of the entry points through the raw C ABI; outputs prefilled so that an element nobody wrote shows.
# ---------------------------------------------------------------------------------------------------------------------
class ScrubletAbi:
    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def pair_count(self, x, pairs, row_total, *, n=None, g=None, nnz=None, n_sim=None, null=(), ws_short=0):
        """-> (rc, dict(out_indptr, total_sim, flags, nnz))"""
        m, z = self.mem, C.c_void_p(0)
        self._keep = bufs = (m.put(x.indptr, np.int64), m.put(x.indices, np.int32), m.put(pairs, np.int32), m.put(row_total, row_total.dtype))
        ns = len(pairs)
        out = {"out_indptr": m.full(ns + 1, np.int64, -1), "total_sim": m.full(max(ns, 1), row_total.dtype, np.nan),
               "flags": m.full(1, np.int32, -1)}
        nbytes = int(self.lib.scamd_pp_scrublet_workspace_bytes(ns))
        ws = m.full(max(nbytes - ws_short, 1), np.uint8, 0xAB)
        total = C.c_int64(-1)

        def p(name, buf):
            return z if name in null else m.ptr(buf)

        rc = self.lib.scamd_pp_scrublet_pair_count(
            p("indptr", bufs[0]), p("indices", bufs[1]), x.shape[0] if n is None else n, x.shape[1] if g is None else g,
            x.nnz if nnz is None else nnz, p("pairs", bufs[2]), ns if n_sim is None else n_sim, p("row_total", bufs[3]),
            int(row_total.dtype == np.float64), p("out_indptr", out["out_indptr"]), p("total_sim", out["total_sim"]),
            p("flags", out["flags"]), None if "out_nnz" in null else C.byref(total), p("workspace", ws), max(nbytes - ws_short, 0), m.stream)
        m.sync()
        res = {k: m.get(v) for k, v in out.items()}
        res["total_sim"] = res["total_sim"][:ns]
        res["nnz"] = int(total.value)
        return rc, res

    def pair_fill(self, x, pairs, out_indptr, out_nnz, *, n=None, g=None, nnz=None, n_sim=None, null=(), cap=None):
        """-> (rc, dict(indices, data, flags)); cap: the size passed as out_nnz where it is to differ from the buffers'"""
        m, z = self.mem, C.c_void_p(0)
        self._keep = bufs = (m.put(x.indptr, np.int64), m.put(x.indices, np.int32), m.put(x.data, np.float32), m.put(pairs, np.int32),
                             m.put(out_indptr, np.int64))
        out = {"indices": m.full(max(out_nnz, 1), np.int32, -1), "data": m.full(max(out_nnz, 1), np.float32, np.nan),
               "flags": m.full(1, np.int32, -1)}

        def p(name, buf):
            return z if name in null else m.ptr(buf)

        rc = self.lib.scamd_pp_scrublet_pair_fill_f32(
            p("indptr", bufs[0]), p("indices", bufs[1]), p("data", bufs[2]), x.shape[0] if n is None else n,
            x.shape[1] if g is None else g, x.nnz if nnz is None else nnz, p("pairs", bufs[3]), len(pairs) if n_sim is None else n_sim,
            p("out_indptr", bufs[4]), out_nnz if cap is None else cap, p("out_indices", out["indices"]), p("out_data", out["data"]),
            p("flags", out["flags"]), m.stream)
        m.sync()
        return rc, {k: m.get(v) for k, v in out.items()}

    def pairs(self, x, pairs, row_total):
        """both phases -> (CSR result, total_sim, flags of the two phases or-ed, raw outputs)"""
        rc, cnt = self.pair_count(x, pairs, row_total)
        assert rc == 0, rc
        rc, fill = self.pair_fill(x, pairs, cnt["out_indptr"], cnt["nnz"])
        assert rc == 0, rc
        z = cnt["nnz"]
        out = sparse.csr_matrix((fill["data"][:z], fill["indices"][:z], cnt["out_indptr"]), shape=(len(pairs), x.shape[1]))
        return out, cnt["total_sim"], int(cnt["flags"][0]) | int(fill["flags"][0]), (cnt, fill)

    def scores(self, idx, n_obs, rho, r, se_rho, *, n_all=None, k=None, null=()):
        """-> (rc, n_sim_neigh int32, score, score_err), prefilled with -1 / NaN"""
        m, z = self.mem, C.c_void_p(0)
        na, kk = idx.shape
        d_idx = m.put(idx, np.int32)
        out = {"cnt": m.full(max(na, 1), np.int32, -1), "score": m.full(max(na, 1), np.float64, np.nan),
               "err": m.full(max(na, 1), np.float64, np.nan)}

        def p(name, buf):
            return z if name in null else m.ptr(buf)

        rc = self.lib.scamd_scrublet_scores_f64(p("idx", d_idx), na if n_all is None else n_all, kk if k is None else k, int(n_obs),
                                                float(rho), float(r), float(se_rho), p("cnt", out["cnt"]), p("score", out["score"]),
                                                p("err", out["err"]), m.stream)
        m.sync()
        return rc, m.get(out["cnt"])[:na], m.get(out["score"])[:na], m.get(out["err"])[:na]


def run_pair_case(abi: ScrubletAbi, name: str, label=""):
    x, pairs, tot_dtype, want_flags = pair_case(name)
    what = f"{label} {name}"
    rng = np.random.default_rng(99)
    row_total = (np.asarray(x.sum(axis=1)).ravel() + rng.integers(0, 5, x.shape[0])).astype(tot_dtype)
    got, total_sim, flags, raw = abi.pairs(x, pairs, row_total)
    want = expected_pairs(x, pairs)
    assert flags == want_flags, (what, flags)
    assert np.array_equal(got.indptr, want.indptr), (what, "row lengths")
    assert raw[0]["nnz"] == want.nnz
    assert got.indices.tobytes() == want.indices.astype(np.int32).tobytes(), (what, "columns")
    assert got.data.tobytes() == want.data.astype(np.float32).tobytes(), (what, "values")
    assert got.has_sorted_indices
    assert total_sim.dtype == tot_dtype
    assert total_sim.tobytes() == (row_total[pairs[:, 0]] + row_total[pairs[:, 1]]).tobytes(), (what, "totals")
    if len(pairs):
        # and scipy's own addition, which drops the zeros it meets: equal once both are rid of them
        sc = (x[pairs[:, 0]] + x[pairs[:, 1]]).tocsr()
        sc.sort_indices()
        mine = got.copy()
        mine.eliminate_zeros()
        sc.eliminate_zeros()
        assert np.array_equal(mine.indptr, sc.indptr) and np.array_equal(mine.indices, sc.indices), (what, "scipy pattern")
        assert mine.data.tobytes() == sc.data.astype(np.float32).tobytes(), (what, "scipy values")
    # a pair (i, i) is row i doubled
    for r in np.flatnonzero(pairs[:, 0] == pairs[:, 1])[:8]:
        i = pairs[r, 0]
        assert np.array_equal(got[r].indices, x[i].indices) and np.array_equal(got[r].data, 2 * x[i].data), (what, "(i, i)")
    if name in RERUN_CASES:
        got2, total2, flags2, _ = abi.pairs(x, pairs, row_total)
        assert got2.indptr.tobytes() == got.indptr.tobytes() and got2.indices.tobytes() == got.indices.tobytes()
        assert got2.data.tobytes() == got.data.tobytes() and total2.tobytes() == total_sim.tobytes() and flags2 == flags
    return got


def run_pair_flag_cases(abi: ScrubletAbi):
    """a pair outside [0, n): bit 1 and an empty output row; an out_indptr that is not this input's: bit 2 and no write outside"""
    x, _, _, _ = pair_case("disjoint")
    tot = np.ones(4, np.float32)
    pairs = np.array([[0, 1], [4, 0], [-1, 2], [2, 3]], np.int32)
    got, total, flags, _ = abi.pairs(x, pairs, tot)
    assert flags == FLAG_BAD_PAIR
    assert np.diff(got.indptr).tolist() == [9, 0, 0, 3] and total.tolist() == [2.0, 0.0, 0.0, 2.0]
    good = np.array([[0, 1], [2, 3]], np.int32)
    rc, cnt = abi.pair_count(x, good, tot)
    assert rc == 0 and cnt["nnz"] == 12
    rc, fill = abi.pair_fill(x, good, cnt["out_indptr"] + 7, 12)       # positions 7 .. 18 of 12
    assert rc == 0 and int(fill["flags"][0]) == FLAG_CAPACITY
    assert (fill["indices"][:7] == -1).all() and np.isnan(fill["data"][:7]).all()


def run_pair_argument_checks(abi: ScrubletAbi, launches=None):
    """the documented codes; a rejected call starts no kernel and writes no output"""
    x, pairs, _, _ = pair_case("disjoint")
    tot = np.ones(4, np.float64)
    before = launches() if launches else 0
    for kw, code in ((dict(null=("indptr",)), EINVAL), (dict(null=("indices",)), EINVAL), (dict(null=("pairs",)), EINVAL),
                     (dict(null=("row_total",)), EINVAL), (dict(null=("out_indptr",)), EINVAL), (dict(null=("total_sim",)), EINVAL),
                     (dict(null=("flags",)), EINVAL), (dict(null=("out_nnz",)), EINVAL), (dict(null=("workspace",)), EINVAL),
                     (dict(ws_short=256), EINVAL), (dict(n=-1), EINVAL), (dict(g=-1), EINVAL), (dict(nnz=-1), EINVAL),
                     (dict(n_sim=-1), EINVAL), (dict(n=0), EINVAL), (dict(n=1 << 31), EUNSUPPORTED), (dict(g=1 << 31), EUNSUPPORTED),
                     (dict(n_sim=1 << 31), EUNSUPPORTED)):
        rc, out = abi.pair_count(x, pairs, tot, **kw)
        assert rc == code, (kw, rc)
        assert (out["out_indptr"] == -1).all() and np.isnan(out["total_sim"]).all() and out["flags"][0] == -1 and out["nnz"] == -1, kw
    indptr = np.arange(len(pairs) + 1, dtype=np.int64)
    for kw, code in ((dict(null=("indptr",)), EINVAL), (dict(null=("indices",)), EINVAL), (dict(null=("data",)), EINVAL),
                     (dict(null=("pairs",)), EINVAL), (dict(null=("out_indptr",)), EINVAL), (dict(null=("out_indices",)), EINVAL),
                     (dict(null=("out_data",)), EINVAL), (dict(null=("flags",)), EINVAL), (dict(cap=-1), EINVAL), (dict(n=-1), EINVAL),
                     (dict(g=-1), EINVAL), (dict(nnz=-1), EINVAL), (dict(n_sim=-1), EINVAL), (dict(n=0), EINVAL),
                     (dict(n=1 << 31), EUNSUPPORTED), (dict(g=1 << 31), EUNSUPPORTED), (dict(n_sim=1 << 31), EUNSUPPORTED)):
        rc, out = abi.pair_fill(x, pairs, indptr, len(pairs), **kw)
        assert rc == code, (kw, rc)
        assert (out["indices"] == -1).all() and np.isnan(out["data"]).all() and out["flags"][0] == -1, kw
    idx = np.zeros((5, 3), np.int32)
    for kw, code in ((dict(null=("idx",)), EINVAL), (dict(null=("cnt",)), EINVAL), (dict(null=("score",)), EINVAL),
                     (dict(null=("err",)), EINVAL), (dict(n_all=-1), EINVAL), (dict(k=0), EINVAL), (dict(n_all=1 << 31), EUNSUPPORTED)):
        rc, cnt, sc, er = abi.scores(idx, 2, 0.05, 2.0, 0.02, **kw)
        assert rc == code, (kw, rc)
        assert (cnt == -1).all() and np.isnan(sc).all() and np.isnan(er).all(), kw
    rc, cnt, sc, er = abi.scores(idx, 6, 0.05, 2.0, 0.02)       # n_obs > n_all
    assert rc == EINVAL and (cnt == -1).all()
    if launches:
        assert launches() == before, "an argument check let a kernel start"


# ---------------------------------------------------------------------------------------------------------------------
# Score-kernel cases
# ---------------------------------------------------------------------------------------------------------------------
def ref_scores(n_sim_neigh, k_adj, rho, r, se_rho):
    """the reference's formulas (`_nearest_neighbor_classifier`), numpy float64"""
    nd = np.asarray(n_sim_neigh).astype(np.float64)
    n = float(k_adj)
    with np.errstate(all="ignore"):
        q = (nd + 1) / (n + 2)
        ld = q * rho / r / (1 - rho - q * (1 - rho - rho / r))
        se_q = np.sqrt(q * (1 - q) / (n + 3))
        se_ld = q * rho / r / (1 - rho - q * (1 - rho - rho / r)) ** 2 * np.sqrt((se_q / q * (1 - rho)) ** 2 + (se_rho / rho * (1 - q)) ** 2)
    return ld, se_ld


#              name            n_all  k    n_obs  rho   r    se_rho
SCORE_CASES = (("k1",           70,    1,   30,  0.05, 2.0, 0.02),
               ("k8",           65,    8,   20,  0.05, 2.0, 0.02),
               ("k9",           65,    9,   20,  0.10, 1.5, 0.03),
               ("k16",          64,   16,   21,  0.05, 2.0, 0.02),
               ("k17",          63,   17,   21,  0.05, 2.0, 0.02),
               ("k32",         130,   32,   40,  0.06, 2.25, 0.02),
               ("k33",         130,   33,   40,  0.06, 2.25, 0.02),
               ("k66",        1000,   66,  333,  0.05, 2.0, 0.02),
               ("k256",        300,  256,  100,  0.05, 2.0, 0.02),
               ("no-sim",      100,   20,  100,  0.05, 2.0, 0.02),
               ("no-obs",      100,   20,    0,  0.05, 2.0, 0.02),
               ("all-sim-rows", 90,   66,   30,  0.05, 2.0, 0.02),
               ("many-blocks", 20000,  5, 7000,  0.05, 1.857, 0.02))
SCORE_CASE_NAMES = tuple(c[0] for c in SCORE_CASES)


def run_score_case(abi: ScrubletAbi, name: str, label=""):
    _, n_all, k, n_obs, rho, r, se_rho = next(c for c in SCORE_CASES if c[0] == name)
    rng = np.random.default_rng(sum(map(ord, name)))
    idx = rng.integers(0, n_all, (n_all, k)).astype(np.int32)
    if name == "all-sim-rows":
        idx[::3] = rng.integers(n_obs, n_all, (len(idx[::3]), k))   # every neighbour simulated
        idx[1::3] = rng.integers(0, n_obs, (len(idx[1::3]), k))     # none
    rc, cnt, score, err = abi.scores(idx, n_obs, rho, r, se_rho)
    assert rc == 0, (label, name, rc)
    want = (idx >= n_obs).sum(axis=1).astype(np.int32)
    assert np.array_equal(cnt, want), (label, name, "counts")
    ld, se = ref_scores(want, k, rho, r, se_rho)
    assert score.tobytes() == ld.tobytes(), (label, name, "scores", float(np.abs(score - ld).max()))
    assert err.tobytes() == se.tobytes(), (label, name, "errors", float(np.abs(err - se).max()))
    if name == "no-sim":
        assert (cnt == 0).all()
    if name == "no-obs":
        assert (cnt == k).all()
    if name == "all-sim-rows":
        assert (cnt[::3] == k).all() and (cnt[1::3] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# Count generator with planted doublets, for the end-to-end cases
# ---------------------------------------------------------------------------------------------------------------------
PLANTED_SHARE = 0.08


@lru_cache(maxsize=None)
def make_counts(n: int, g: int, t: int, seed: int):
    """-> (CSR float32 counts [n, g], planted bool [n]).  t expression programmes drawn gamma(0.3) and normalised per type, a
    type per cell, depth lognormal(log 1500, 0.3), Poisson counts; the first 8 % of the cells get the rates of a second random
    cell added: the planted doublets."""
    rng = np.random.default_rng(seed)
    prog = rng.gamma(0.3, size=(t, g))
    prog /= prog.sum(axis=1, keepdims=True)
    types = rng.integers(0, t, n)
    depth = rng.lognormal(np.log(1500.0), 0.3, n)
    rates = prog[types] * depth[:, None]
    n_d = int(PLANTED_SHARE * n)
    partner = rng.integers(0, n, n_d)
    rates[:n_d] = rates[:n_d] + rates[partner]
    x = sparse.csr_matrix(rng.poisson(rates).astype(np.float32))
    x.sort_indices()
    x = sparse.csr_matrix((x.data, x.indices.astype(np.int32), x.indptr.astype(np.int64)), shape=x.shape)
    planted = np.zeros(n, dtype=bool)
    planted[:n_d] = True
    for a in (x.data, x.indices, x.indptr, planted):
        a.setflags(write=False)
    return x, planted


def sample_pairs(n: int, n_sim: int, rng) -> np.ndarray:
    """`sample_comb((n, n), n_sim)` for a new-style generator"""
    idx = np.random.default_rng(rng).choice(n * n, size=n_sim, replace=False)
    return np.vstack(np.unravel_index(idx, (n, n))).T


# ---------------------------------------------------------------------------------------------------------------------
# The restatement, float64
# ---------------------------------------------------------------------------------------------------------------------
def ref_normalize(x, target=1e6):
    x = sparse.csr_matrix(x, dtype=np.float64)
    s = np.asarray(x.sum(axis=1)).ravel()
    f = s / target
    f[f == 0] = 1.0
    return sparse.diags(1.0 / f) @ x


def prepare_rows(m: np.ndarray, metric: str) -> np.ndarray:
    m = np.asarray(m, dtype=np.float64)
    if metric in ("cosine", "correlation"):
        if metric == "correlation":
            m = m - m.mean(axis=1, keepdims=True)
        m = m / np.linalg.norm(m, axis=1, keepdims=True)
    return m


def ref_call(x_obs, x_sim, *, mean_center=True, normalize_variance=True, n_prin_comps=30, n_neighbors=None, rho=0.05, se_rho=0.02,
             metric="euclidean", seed=0):
    """`_scrublet_call_doublets` up to the scores, on normalised matrices -> dict(manifold [n_obs + n_sim, d], k_adj, neighbors,
    n_sim_neigh, score, score_err, r)"""
    from sklearn.decomposition import PCA, TruncatedSVD
    from sklearn.neighbors import NearestNeighbors

    o = np.asarray(sparse.csr_matrix(x_obs, dtype=np.float64).todense())
    s = np.asarray(sparse.csr_matrix(x_sim, dtype=np.float64).todense())
    n_obs, n_sim = o.shape[0], s.shape[0]
    mean, std = o.mean(axis=0), np.sqrt(o.var(axis=0, ddof=1))
    if mean_center and normalize_variance:
        o, s = (o - mean) / std, (s - mean) / std
    elif mean_center:
        o, s = o - mean, s - mean
    elif normalize_variance:
        o, s = o / std, s / std
    if mean_center:
        fit = PCA(n_components=n_prin_comps, svd_solver="arpack", random_state=seed).fit(o)
    else:
        fit = TruncatedSVD(n_components=n_prin_comps, algorithm="arpack", random_state=seed).fit(o)
    manifold = np.concatenate([fit.transform(o), fit.transform(s)], axis=0)
    k = round(0.5 * np.sqrt(n_obs)) if n_neighbors is None else n_neighbors
    r = n_sim / float(n_obs)
    k_adj = round(k * (1 + r))
    rows = prepare_rows(manifold, metric)
    nn = NearestNeighbors(n_neighbors=k_adj + 1, algorithm="brute").fit(rows)
    dist, neigh = nn.kneighbors(rows)
    cnt = (neigh[:, :k_adj] >= n_obs).sum(axis=1)
    ld, se = ref_scores(cnt, k_adj, rho, r, se_rho)
    return {"manifold": manifold, "k_adj": k_adj, "neighbors": neigh[:, :k_adj], "neighbors_next": neigh[:, k_adj], "dist": dist,
            "n_sim_neigh": cnt, "score": ld,
            "score_err": se, "r": r, "n_obs": n_obs}


@lru_cache(maxsize=None)
def ref_generator_run(n: int, g: int, t: int, seed: int, rng_seed: int):
    """the restatement on the generator's counts, all genes, defaults -> dict as ref_call plus pairs, x_obs, x_sim (normalised),
    planted"""
    x, planted = make_counts(n, g, t, seed)
    pairs = sample_pairs(n, int(n * 2.0), rng_seed)
    sim = expected_pairs(x, pairs.astype(np.int32))
    out = ref_call(ref_normalize(x), ref_normalize(sim))
    out.update(pairs=pairs, counts=x, sim_counts=sim, planted=planted)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU stand-in for GpuPPBackend.scrublet_simulate / scrublet_download / scrublet_call (the front-end tests)
# ---------------------------------------------------------------------------------------------------------------------
class CpuStubScrubletBackend(CpuStubPPBackend):
    calls = 0

    def scrublet_simulate(self, m, pairs, row_total):
        x = sparse.csr_matrix((m.data, m.indices, m.indptr), shape=m.shape)
        out = expected_pairs(x, np.asarray(pairs, dtype=np.int32))
        tot = np.asarray(row_total)
        inexact = bool(out.nnz and np.abs(out.data).max() > 2.0 ** 24)
        return self.upload(out), tot[pairs[:, 0]] + tot[pairs[:, 1]], inexact

    def scrublet_download(self, m):
        return sparse.csr_matrix((m.data.copy(), m.indices.copy(), m.indptr.copy()), shape=m.shape)

    def scrublet_call(self, m_obs, m_sim, *, log_transform, renormalize, mean_center, normalize_variance, n_prin_comps, k_adj, metric,
                      rho, r, se_rho, want_neighbors=False, want_manifold=False):
        from sklearn.decomposition import PCA, TruncatedSVD
        from sklearn.neighbors import NearestNeighbors

        type(self).calls += 1
        mats = []
        for m in (m_obs, m_sim):
            x = sparse.csr_matrix((m.data.astype(np.float64), m.indices, m.indptr), shape=m.shape)
            if log_transform:
                x.data = np.log1p(x.data)
            mats.append(np.asarray((ref_normalize(x) if renormalize else x).todense()))
        o, s = mats
        n_obs = o.shape[0]
        mean, std = o.mean(axis=0), np.sqrt(o.var(axis=0, ddof=1))
        if normalize_variance and (std == 0).any():
            raise ValueError(f"{int((std == 0).sum())} genes have zero variance")
        if normalize_variance:
            o, s = o / std, s / std
        if mean_center:
            fit = PCA(n_components=n_prin_comps, svd_solver="arpack", random_state=0).fit(o)
        else:
            fit = TruncatedSVD(n_components=n_prin_comps, algorithm="arpack", random_state=0).fit(o)
        manifold = np.concatenate([fit.transform(o), fit.transform(s)], axis=0)
        rows = prepare_rows(manifold, metric)
        neigh = NearestNeighbors(n_neighbors=k_adj, algorithm="brute").fit(rows).kneighbors(rows, return_distance=False)
        cnt = (neigh >= n_obs).sum(axis=1)
        ld, se = ref_scores(cnt, k_adj, rho, r, se_rho)
        out = {"n_sim_neigh": cnt.astype(np.int32), "score": ld, "score_err": se}
        if want_neighbors:
            out["neighbors"] = neigh.astype(np.int32)
        if want_manifold:
            out["manifold"] = manifold.astype(np.float32)
        return out
