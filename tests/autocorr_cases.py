"""TEST INFRASTRUCTURE shared by tests/test_gpu_autocorr.py (the product library on the GPU), tests/test_emu_autocorr_cpu.py (the
same kernels on the host emulator) and tests/test_autocorr_front_cpu.py (the front end on a CPU stand-in): the case table of the
graph-autocorrelation kernels (csrc/graph_autocorr.hip), restatements of the rules by which the host code sizes its work, a
float64 numpy restatement of Moran's I and Geary's C on raw COO triplets, ONE checker, and a CPU stand-in for
`scanpy_amd.metrics._autocorr.GpuAutocorrBackend`.  Nothing here touches a device; the callers hand in `AutocorrAbi` over host
memory (tests/emu/harness.py:HostMem) or device memory (graph_kernel_cases.DeviceMem).

The restatement is written from the two formulas, not from the reference's loops:
    W = sum w;  z = x - mean(x);  I = n / W * sum_e w_e z_i(e) z_j(e) / sum z^2;  C = (n - 1) / (2 W) * sum_e w_e (x_i(e) - x_j(e))^2 / sum z^2
over the stored entries e = (i, j, w) as they are stored (duplicates, explicit zeros, self-loops and negative weights included).

Tolerance against it: atol = 1e-11, rtol = 1e-9 -- the reference's own bounds between its variants (tests/test_metrics.py:45,71
of the reference).  The two sides differ by summation order only (float64 sums of at most 6e4 terms here: 1e-12 relative even
for a worst-case recursive sum), so a miss means an arithmetic difference, not noise."""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
from scipy import sparse

from graph_kernel_cases import EINVAL, EUNSUPPORTED, DeviceMem  # noqa: F401  (DeviceMem: for the GPU tests)

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "scanpy_amd" / "csrc"
ATOL, RTOL = 1e-11, 1e-9
SLAB = 64

# ---------------------------------------------------------------------------------------------------------------------
# The sizing rules restated; `assert_sources_still_say_so` ties them to the text of csrc/graph_autocorr.hip.
# ---------------------------------------------------------------------------------------------------------------------
GA_PART_MIN, GA_PART_MAX, GA_PART_TARGET = 256, 4096, 8192
GA_COL_CHUNKS, GA_COL_CHUNK_ROWS = 1024, 256
GA_WSUM_CHUNKS, GA_WSUM_CHUNK_MIN = 1024, 4096
GA_UNROLL = 4


def part_entries(nnz: int) -> int:
    return min(max(-(-nnz // GA_PART_TARGET), GA_PART_MIN), GA_PART_MAX)


def parts(nnz: int) -> int:
    return -(-nnz // part_entries(nnz))


def col_chunk_rows(n: int) -> int:
    return max(-(-n // GA_COL_CHUNKS), GA_COL_CHUNK_ROWS)


def col_chunks(n: int) -> int:
    return max(-(-n // col_chunk_rows(n)), 1)


def wsum_chunks(nnz: int) -> int:
    return -(-nnz // max(-(-nnz // GA_WSUM_CHUNKS), GA_WSUM_CHUNK_MIN))


def assert_sources_still_say_so():
    src = (CSRC / "graph_autocorr.hip").read_text()

    def has(pattern, what):
        assert re.search(pattern, src), f"{what}: /{pattern}/ no longer in csrc/graph_autocorr.hip -- restate the rule and its cases"

    has(r"constexpr int GA_BLOCK = 256;", "GA_BLOCK")
    has(rf"constexpr int GA_SLAB = {SLAB};", "GA_SLAB")
    has(rf"constexpr int GA_UNROLL = {GA_UNROLL}; ", "GA_UNROLL")
    has(rf"constexpr int GA_PART_MIN = {GA_PART_MIN};", "GA_PART_MIN")
    has(rf"constexpr int GA_PART_MAX = {GA_PART_MAX};", "GA_PART_MAX")
    has(rf"constexpr int GA_PART_TARGET = {GA_PART_TARGET};", "GA_PART_TARGET")
    has(rf"constexpr int GA_COL_CHUNKS = {GA_COL_CHUNKS};", "GA_COL_CHUNKS")
    has(rf"constexpr int GA_COL_CHUNK_ROWS = {GA_COL_CHUNK_ROWS};", "GA_COL_CHUNK_ROWS")
    has(rf"constexpr int GA_WSUM_CHUNKS = {GA_WSUM_CHUNKS};", "GA_WSUM_CHUNKS")
    has(rf"constexpr int GA_WSUM_CHUNK_MIN = {GA_WSUM_CHUNK_MIN};", "GA_WSUM_CHUNK_MIN")
    has(r"constexpr int GA_REDUCE_GROUP = 64;", "GA_REDUCE_GROUP")
    has(r"const int64_t per = \(nnz \+ GA_PART_TARGET - 1\) / GA_PART_TARGET;", "part rule")
    has(r"std::min<int64_t>\(std::max<int64_t>\(per, GA_PART_MIN\), GA_PART_MAX\)", "part clamp")
    has(r"std::max<int64_t>\(\(n \+ GA_COL_CHUNKS - 1\) / GA_COL_CHUNKS, GA_COL_CHUNK_ROWS\)", "column chunk rule")
    has(r"std::max<int64_t>\(\(nnz \+ GA_WSUM_CHUNKS - 1\) / GA_WSUM_CHUNKS, GA_WSUM_CHUNK_MIN\)", "weight-sum chunk rule")
    has(r"if \(weights_is_f64\) ga_launch_sweep<VT, double>\(", "float64 weights")
    has(r"else ga_launch_sweep<VT, float>\(", "float32 weights")
    has(r"return ga_slab<float>\(", "float32 values")
    has(r"return ga_slab<double>\(", "float64 values")
    has(r"return ga_transpose<float>\(", "float32 transpose")
    has(r"return ga_transpose<double>\(", "float64 transpose")
    # no atomics, no printf / assert in the kernels
    assert not re.search(r"\batomic\w*\(|\bprintf\(|\bassert\(|\basm\b", src)


# ---------------------------------------------------------------------------------------------------------------------
# Case table.  graph: "random" (rows of Poisson(avg) sorted unique columns, a fifth of the rows empty), "hub" (one row and one
# other column of 4 000 entries, the others 5-15, some empty, asymmetric), "messy" (unsorted, duplicates, explicit zeros,
# self-loops, negative weights).  source: how the slab is made -- "inplace" (a dense cell-major array of leading dimension m +
# pad, the pad filled with NaN, read through pointer / ld / ncols), "csr" (scamd_csr_dense_slab_f32 from a cell-major CSR, a
# third of the entries stored), "rows" (scamd_transpose_slab_* from feature-major rows).  values: "normal", "offset" (1000 + N(0, 1):
# centring in float32 would fail), "const" (columns 1, 3 and the last are constant: implicit zeros where the source is sparse
# else 0, stored zeros / 42, 42).
# ---------------------------------------------------------------------------------------------------------------------
#     name            n     m   graph     avg  wdtype      vdtype      source     pad  values
CASES = (
    ("n2-m1",          2,    1, "random",   1, np.float32, np.float64, "inplace", 0, "normal"),
    ("n63-m63",       63,   63, "random",   6, np.float64, np.float32, "inplace", 3, "normal"),
    ("n64-m64",       64,   64, "random",   6, np.float32, np.float32, "csr",     0, "normal"),
    ("n65-m65",       65,   65, "random",   6, np.float64, np.float64, "rows",    0, "normal"),
    ("n1000-m129",  1000,  129, "random",  12, np.float32, np.float64, "inplace", 5, "normal"),
    ("n1000-m1",    1000,    1, "random",  12, np.float64, np.float32, "rows",    0, "normal"),
    ("n65-m129-csr",  65,  129, "random",   6, np.float64, np.float32, "csr",     0, "const"),
    ("hub",         5000,    3, "hub",     10, np.float32, np.float32, "inplace", 0, "normal"),
    ("hub-f64",     5000,   65, "hub",     10, np.float64, np.float64, "rows",    0, "normal"),
    ("messy",        200,    5, "messy",    8, np.float64, np.float64, "inplace", 1, "normal"),
    ("offset",      1000,    2, "random",  12, np.float32, np.float64, "inplace", 0, "offset"),
    ("const",        300,    7, "random",   8, np.float32, np.float32, "inplace", 0, "const"),
    ("n1",             1,    2, "random",   1, np.float32, np.float32, "inplace", 0, "normal"),
)
CASE_NAMES = tuple(c[0] for c in CASES)
DETERMINISM_CASES = ("hub", "hub-f64")
HUB_ROW, HUB_COL, HUB_LEN = 7, 11, 4000


def _case(name):
    return next(c for c in CASES if c[0] == name)


def _seed(name: str) -> int:
    return 4000 + sum(map(ord, name))


@lru_cache(maxsize=None)
def case_graph(name: str):
    """-> (indptr int64 [n + 1], indices int32, weights of the case's dtype), read-only, as the kernels get them"""
    _, n, _, kind, avg, wdtype, *_ = _case(name)
    rng = np.random.default_rng(_seed(name))
    rows = []
    if kind == "hub":
        senders = set(rng.choice(np.setdiff1d(np.arange(n), [HUB_ROW]), HUB_LEN, replace=False).tolist())
        for i in range(n):
            if i == HUB_ROW:
                cols = np.sort(rng.choice(n, HUB_LEN, replace=False))
            elif i % 17 == 3 and i not in senders:
                cols = np.zeros(0, dtype=np.int64)
            else:
                cols = rng.choice(np.setdiff1d(np.arange(n), [HUB_COL]), int(rng.integers(5, 16)), replace=False)
                if i in senders:
                    cols[0] = HUB_COL
                cols = np.sort(cols)
            rows.append(cols)
    else:
        for i in range(n):
            ln = 0 if (i % 5 == 2 and n > 2) else int(min(rng.poisson(avg), n))
            cols = np.sort(rng.choice(n, ln, replace=False))
            if kind == "messy" and ln:
                cols = rng.permutation(np.concatenate([cols, cols[: max(ln // 3, 1)], [i]]))   # duplicates, a self-loop, unsorted
            rows.append(cols)
    ln = np.array([len(r) for r in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    indices = (np.concatenate(rows) if ln.sum() else np.zeros(0)).astype(np.int32)
    w = rng.uniform(0.05, 1.0, len(indices))
    if kind == "messy":
        w[::4] = 0.0          # explicit zeros
        w[1::5] *= -1.0       # negative weights
    w = w.astype(wdtype)
    for a in (indptr, indices, w):
        a.setflags(write=False)
    return indptr, indices, w


@lru_cache(maxsize=None)
def case_values(name: str) -> np.ndarray:
    """-> X [n, m] of the case's value dtype (cell-major), read-only; for a "csr" source two thirds of it are zero"""
    _, n, m, _, _, _, vdtype, source, _, kind = _case(name)
    rng = np.random.default_rng(_seed(name) + 1)
    x = rng.normal(size=(n, m)) * 10.0 ** rng.uniform(-2, 2, m)
    if kind == "offset":
        x = 1000.0 + rng.normal(size=(n, m))
    if source == "csr":
        x[rng.random((n, m)) < 2 / 3] = 0.0
    if kind == "const":
        x[:, 1] = 0.0
        x[:, 3] = 0.0 if source == "csr" else 42.0
        x[:, m - 1] = 42.0
    x = np.ascontiguousarray(x.astype(vdtype))
    x.setflags(write=False)
    return x


def constant_columns(name: str):
    _, _, m, _, _, _, _, _, _, kind = _case(name)
    return (1, 3, m - 1) if kind == "const" else ()


def assert_table_covers_every_path():
    """-> the sets the table reaches: (value dtype, weight dtype) of the sweep, (source, value dtype) of the builders"""
    sweeps, builders = set(), set()
    ns, ms = set(), set()
    for name, n, m, kind, _, wdtype, vdtype, source, pad, _ in CASES:
        indptr, indices, w = case_graph(name)
        x = case_values(name)
        assert x.shape == (n, m) and x.dtype == vdtype and w.dtype == wdtype and len(indptr) == n + 1
        sweeps.add((np.dtype(vdtype).name, np.dtype(wdtype).name))
        builders.add((source, np.dtype(vdtype).name))
        ns.add(n), ms.add(m)
        if kind == "random" and n >= 63:
            assert (np.diff(indptr) == 0).any(), name   # empty rows
        assert source != "csr" or vdtype == np.float32
    assert sweeps == {(v, w) for v in ("float32", "float64") for w in ("float32", "float64")}
    assert builders >= {("inplace", "float32"), ("inplace", "float64"), ("csr", "float32"), ("rows", "float32"), ("rows", "float64")}
    assert ns >= {1, 2, 63, 64, 65, 1000, 5000} and ms >= {1, 63, 64, 65, 129}
    assert any(c[8] > 0 for c in CASES), "ld > ncols"
    # a partial last slab, exactly one slab, more than one
    assert {-(-m // SLAB) for m in ms} >= {1, 2, 3} and any(m % SLAB == 0 for m in ms) and any(m % SLAB for m in ms)
    # the hub row is shared by at least three parts, its part count is no multiple of the four waves of a workgroup somewhere,
    # and an entry count that is no multiple of the unroll occurs
    for name in DETERMINISM_CASES:
        indptr, indices, _ = case_graph(name)
        nnz = int(indptr[-1])
        assert indptr[HUB_ROW + 1] - indptr[HUB_ROW] == HUB_LEN and (indices == HUB_COL).sum() >= HUB_LEN
        assert HUB_LEN >= 3 * part_entries(nnz)
        assert (np.diff(indptr) == 0).any() and not np.array_equal(np.diff(indptr), np.bincount(indices, minlength=5000))
    assert any(int(case_graph(c[0])[0][-1]) % GA_UNROLL for c in CASES)
    assert any(parts(int(case_graph(c[0])[0][-1])) % 4 for c in CASES)
    # both sides of the sizing rules that n <= 5000 can reach: one column chunk and several, one weight-sum chunk and several,
    # one part and several.  (The upper branches -- more than 256 * 8192 entries, more than 256 * 1024 cells -- are beyond the size
    # limit of a test; the rules themselves are restated above and checked against the library's own answer.)
    assert {col_chunks(n) for n in ns} >= {1, 4, 20}
    nnzs = [int(case_graph(c[0])[0][-1]) for c in CASES]
    assert min(wsum_chunks(z) for z in nnzs if z) == 1 and max(wsum_chunks(z) for z in nnzs) > 1
    assert min(parts(z) for z in nnzs if z) == 1 and max(parts(z) for z in nnzs) > 3 * 64   # (more than one group of the reduction, the last one partial)
    assert max(parts(z) for z in nnzs) % 64
    assert [part_entries(z) for z in (0, 1, 256 * 8192, 256 * 8192 + 1, 4096 * 8192, 10 ** 10)] == [256, 256, 256, 257, 4096, 4096]
    return sweeps, builders


# ---------------------------------------------------------------------------------------------------------------------
# The restatement, float64 numpy on the raw arrays.
# ---------------------------------------------------------------------------------------------------------------------
def coo_rows(indptr) -> np.ndarray:
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def restate(indptr, indices, weights, x):
    """x [n] or [n, m] (cell-major) -> (I, C) float64, NaN where sum z^2 is 0"""
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = x.reshape(len(x), -1)
    n = x.shape[0]
    w = np.asarray(weights, dtype=np.float64)
    i, j = coo_rows(indptr), np.asarray(indices, dtype=np.int64)
    w_sum = w.sum()
    z = x - x.mean(axis=0)
    z2 = (z * z).sum(axis=0)
    mor, gea = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for c0 in range(0, x.shape[1], 32):
        sl = slice(c0, c0 + 32)
        mor[sl] = (w[:, None] * z[i, sl] * z[j, sl]).sum(axis=0)
        d = x[i, sl] - x[j, sl]
        gea[sl] = (w[:, None] * d * d).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        big_i = n / w_sum * mor / z2
        big_c = (n - 1) / (2 * w_sum) * gea / z2
    return (big_i[0], big_c[0]) if one else (big_i, big_c)


def assert_close(got, want, what=""):
    np.testing.assert_allclose(got, want, atol=ATOL, rtol=RTOL, err_msg=str(what))


# ---------------------------------------------------------------------------------------------------------------------
# Callers of the entry points through the raw C ABI: numpy in, numpy out, the return code handed back, outputs prefilled with
# NaN so that an element nobody wrote shows.  `mem`: tests/emu/harness.py:HostMem or graph_kernel_cases.DeviceMem.
# ---------------------------------------------------------------------------------------------------------------------
OUT_KEYS = ("mean", "z2", "moran", "geary", "min", "max")


class AutocorrAbi:
    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def _ws(self, n, nnz, short=0):
        nbytes = int(self.lib.scamd_graph_autocorr_workspace_bytes(max(int(n), 0), max(int(nnz), 0)))
        return self.mem.full(max(nbytes - short, 1), np.uint8, 0xAB), max(nbytes - short, 0)

    def slab(self, graph, n, buf, ld, ncols, *, offset=0, n_arg=None, nnz_arg=None, null=(), ws_short=0):
        """buf: a numpy array of float32 / float64 holding the slab at element `offset`, leading dimension ld.
        -> (rc, dict of OUT_KEYS -> float64 [ncols] prefilled with NaN)"""
        m, z = self.mem, C.c_void_p(0)
        indptr, indices, w = graph
        d_ip, d_ix, d_w = m.put(indptr, np.int64), m.put(indices, np.int32), m.put(w, w.dtype)
        d_s = m.put(np.ravel(buf), buf.dtype)
        width = max(min(int(ncols), SLAB), 1)
        outs = {k: m.full(width, np.float64, np.nan) for k in OUT_KEYS}
        ws, wsz = self._ws(n, len(indices), ws_short)
        base = m.ptr(d_s).value or 0
        sp = z if "slab" in null else C.c_void_p(base + offset * buf.dtype.itemsize)
        entry = self.lib.scamd_graph_autocorr_slab_f64 if buf.dtype == np.float64 else self.lib.scamd_graph_autocorr_slab_f32

        def p(name, b):
            return z if name in null else m.ptr(b)

        rc = entry(p("indptr", d_ip), p("indices", d_ix), p("weights", d_w), int(w.dtype == np.float64), n if n_arg is None else n_arg,
                   len(indices) if nnz_arg is None else nnz_arg, sp, int(ld), int(ncols), *(p(k, outs[k]) for k in OUT_KEYS),
                   z if "workspace" in null else m.ptr(ws), wsz, m.stream)
        m.sync()
        return rc, {k: m.get(v) for k, v in outs.items()}

    def weight_sum(self, w, *, nnz_arg=None, null=(), ws_bytes=None):
        m, z = self.mem, C.c_void_p(0)
        d_w = m.put(w, w.dtype)
        out = m.full(1, np.float64, np.nan)
        ws, wsz = self._ws(1, len(w))
        rc = self.lib.scamd_graph_weight_sum_f64(z if "weights" in null else m.ptr(d_w), int(w.dtype == np.float64),
                                                 len(w) if nnz_arg is None else nnz_arg, z if "out" in null else m.ptr(out),
                                                 z if "workspace" in null else m.ptr(ws), wsz if ws_bytes is None else ws_bytes, m.stream)
        m.sync()
        return rc, float(m.get(out)[0])

    def csr_slab(self, x, c0, ncols, *, ld=SLAB, g_arg=None, null=()):
        """x: canonical scipy CSR float32 cells x features -> (rc, slab float32 [n, ld] prefilled with NaN)"""
        m, z = self.mem, C.c_void_p(0)
        n, g = x.shape
        d_ip, d_ix, d_dv = m.put(x.indptr, np.int64), m.put(x.indices, np.int32), m.put(x.data, np.float32)
        slab = m.full((max(n, 1), ld), np.float32, np.nan)
        rc = self.lib.scamd_csr_dense_slab_f32(z if "indptr" in null else m.ptr(d_ip), m.ptr(d_ix), m.ptr(d_dv), n, g if g_arg is None else g_arg,
                                               x.nnz, int(c0), int(ncols), z if "slab" in null else m.ptr(slab), ld, m.stream)
        m.sync()
        return rc, m.get(slab)[:n]

    def transpose(self, rows, *, ld=SLAB, ncols_arg=None, null=()):
        """rows: numpy [b, n] float32 / float64 -> (rc, slab [n, ld] of the same dtype prefilled with NaN)"""
        m, z = self.mem, C.c_void_p(0)
        b, n = rows.shape
        d_r = m.put(rows, rows.dtype)
        slab = m.full((max(n, 1), ld), rows.dtype, np.nan)
        entry = self.lib.scamd_transpose_slab_f64 if rows.dtype == np.float64 else self.lib.scamd_transpose_slab_f32
        rc = entry(z if "vals" in null else m.ptr(d_r), n, n, b if ncols_arg is None else ncols_arg, z if "slab" in null else m.ptr(slab), ld,
                   m.stream)
        m.sync()
        return rc, m.get(slab)[:n]


# ---------------------------------------------------------------------------------------------------------------------
# The checker: one case, slab by slab, through the builder its source names and the sweep.
# ---------------------------------------------------------------------------------------------------------------------
def case_stats(abi: AutocorrAbi, name: str, x=None, what=""):
    """-> dict of OUT_KEYS -> float64 [m], and W_sum"""
    _, n, m, _, _, _, vdtype, source, pad, _ = _case(name)
    graph = case_graph(name)
    x = case_values(name) if x is None else x
    m = x.shape[1]
    res = {k: np.full(m, np.nan) for k in OUT_KEYS}
    if source == "inplace":
        whole = np.full((n, m + pad), np.nan, dtype=vdtype)
        whole[:, :m] = x
    elif source == "csr":
        xs = sparse.csr_matrix(x)
        xs.sort_indices()
    for c0 in range(0, m, SLAB):
        b = min(SLAB, m - c0)
        if source == "inplace":
            rc, out = abi.slab(graph, n, whole, m + pad, b, offset=c0)
        elif source == "csr":
            rc, slab = abi.csr_slab(xs, c0, b)
            assert rc == 0, (what, name, rc)
            assert np.array_equal(slab[:, :b], x[:, c0:c0 + b]) and np.isnan(slab[:, b:]).all(), (what, name, "csr slab", c0)
            rc, out = abi.slab(graph, n, slab, SLAB, b)
        else:
            rc, slab = abi.transpose(np.ascontiguousarray(x[:, c0:c0 + b].T))
            assert rc == 0, (what, name, rc)
            assert np.array_equal(slab[:, :b], x[:, c0:c0 + b]) and np.isnan(slab[:, b:]).all(), (what, name, "transposed slab", c0)
            rc, out = abi.slab(graph, n, slab, SLAB, b)
        assert rc == 0, (what, name, rc)
        for k in OUT_KEYS:
            res[k][c0:c0 + b] = out[k][:b]
            assert np.isnan(out[k][b:]).all(), (what, name, k, "written beyond ncols")
    rc, w_sum = abi.weight_sum(graph[2])
    assert rc == 0
    return res, w_sum


def scores(res, w_sum, n):
    with np.errstate(divide="ignore", invalid="ignore"):
        return n / np.float64(w_sum) * res["moran"] / res["z2"], (n - 1) / (2 * np.float64(w_sum)) * res["geary"] / res["z2"]


def run_case(abi: AutocorrAbi, name: str, label="", rerun=None):
    _, n, m, *_ = _case(name)
    what = f"{label} {name}"
    indptr, indices, w = case_graph(name)
    x = case_values(name)
    res, w_sum = case_stats(abi, name, what=what)
    x64 = x.astype(np.float64)
    assert np.array_equal(res["min"], x64.min(axis=0)) and np.array_equal(res["max"], x64.max(axis=0)), (what, "min / max")
    np.testing.assert_allclose(res["mean"], x64.mean(axis=0), rtol=1e-12, atol=1e-300, err_msg=what)
    np.testing.assert_allclose(w_sum, w.astype(np.float64).sum(), rtol=1e-12, err_msg=what)
    const = np.zeros(m, dtype=bool)
    const[list(constant_columns(name))] = True
    if n == 1:
        const[:] = True
    assert np.array_equal(res["min"] == res["max"], const), (what, "constant columns are those with min == max")
    got_i, got_c = scores(res, w_sum, n)
    want_i, want_c = restate(indptr, indices, w, x64)
    assert_close(got_i[~const], want_i[~const], (what, "I"))
    assert_close(got_c[~const], want_c[~const], (what, "C"))
    if rerun if rerun is not None else name in DETERMINISM_CASES:
        res2, w_sum2 = case_stats(abi, name, what=what)
        assert w_sum2 == w_sum
        for k in OUT_KEYS:
            assert res[k].tobytes() == res2[k].tobytes(), (what, k, "two runs differ")
        # a feature's result does not depend on its lane: the columns in reverse order
        res3, _ = case_stats(abi, name, x=np.ascontiguousarray(x[:, ::-1]), what=what)
        for k in OUT_KEYS:
            assert res[k].tobytes() == res3[k][::-1].tobytes(), (what, k, "a result depends on the lane it sat in")
    return res, w_sum


def two_cells():
    """weights 1 both ways, x = [0, 1]: z = [-1/2, 1/2], sum w z_i z_j = -1/2, sum z^2 = 1/2, I = 2 / 2 * -1 = -1;
    sum w (x_i - x_j)^2 = 2, C = 1 / 4 * 2 / (1 / 2) = 1"""
    return (np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32), np.ones(2, np.float32)), np.array([0.0, 1.0])


def block_graph(size: int, seed: int = 0):
    """the reference's block graph (tests/test_metrics.py:87-96 of the reference): 100 cells in two fully connected groups"""
    rng = np.random.default_rng(seed)
    connected = np.zeros(100)
    connected[rng.choice(100, size=size, replace=False)] = 1
    on = connected.astype(bool)
    graph = np.zeros((100, 100))
    graph[np.ix_(on, on)] = 1
    graph[np.ix_(~on, ~on)] = 1
    return sparse.csr_matrix(graph), connected


def run_hand_cases(abi: AutocorrAbi, label=""):
    graph, x = two_cells()
    assert restate(*graph, x) == (-1.0, 1.0)   # (validates the restatement)
    for dt in (np.float32, np.float64):
        rc, out = abi.slab(graph, 2, x.astype(dt).reshape(2, 1), 1, 1)
        rc2, w_sum = abi.weight_sum(graph[2])
        assert rc == 0 and rc2 == 0 and w_sum == 2.0
        i, c = scores(out, w_sum, 2)
        assert i[0] == -1.0 and c[0] == 1.0, (label, dt, i, c)
    for size, key, want, tol in ((30, 1, 0.0, 0.0), (50, 0, 1.0, 1e-14)):
        g, x = block_graph(size)
        graph = (g.indptr.astype(np.int64), g.indices.astype(np.int32), g.data)
        rc, out = abi.slab(graph, 100, x.reshape(100, 1), 1, 1)
        rc2, w_sum = abi.weight_sum(g.data)
        assert rc == 0 and rc2 == 0
        got = scores(out, w_sum, 100)[key][0]
        assert abs(got - want) <= tol, (label, size, got)
        assert restate(*graph, x)[key] == want


def run_nan_case(abi: AutocorrAbi, label=""):
    """a column with one NaN, one with an infinity: their means are not finite; their slab neighbours keep their bits"""
    name = "n63-m63"
    clean, w_sum = case_stats(abi, name)
    x = case_values(name).copy()
    x[5, 10], x[6, 20] = np.nan, np.inf
    dirty, _ = case_stats(abi, name, x=x)
    assert not np.isfinite(dirty["mean"][10]) and not np.isfinite(dirty["mean"][20]), label
    keep = np.ones(63, dtype=bool)
    keep[[10, 20]] = False
    for k in OUT_KEYS:
        assert clean[k][keep].tobytes() == dirty[k][keep].tobytes(), (label, k)


def run_argument_checks(abi: AutocorrAbi, launches=None):
    """the documented codes; a rejected call starts no kernel and writes no output"""
    graph = case_graph("n63-m63")
    x = case_values("n63-m63")
    before = launches() if launches else 0
    for kw, code in ((dict(null=("indptr",)), EINVAL), (dict(null=("indices",)), EINVAL), (dict(null=("weights",)), EINVAL),
                     (dict(null=("slab",)), EINVAL), (dict(n_arg=0), EINVAL), (dict(n_arg=-1), EINVAL), (dict(nnz_arg=-1), EINVAL),
                     (dict(n_arg=1 << 31), EUNSUPPORTED), (dict(ncols=0), EINVAL), (dict(ncols=65), EINVAL), (dict(ld=62), EINVAL),
                     (dict(null=("mean",)), EINVAL), (dict(null=("z2",)), EINVAL), (dict(null=("moran",)), EINVAL),
                     (dict(null=("geary",)), EINVAL), (dict(null=("min",)), EINVAL), (dict(null=("max",)), EINVAL),
                     (dict(null=("workspace",)), EINVAL), (dict(ws_short=256), EINVAL)):
        args = dict(ld=63, ncols=63)
        args.update(kw)
        rc, out = abi.slab(graph, 63, x, args.pop("ld"), args.pop("ncols"), **args)
        assert rc == code, (kw, rc)
        for k, a in out.items():
            assert np.isnan(a).all(), (kw, k)
    w = graph[2]
    for kw in (dict(null=("weights",)), dict(null=("out",)), dict(null=("workspace",)), dict(nnz_arg=-1), dict(ws_bytes=100)):
        rc, v = abi.weight_sum(w, **kw)
        assert rc == EINVAL and np.isnan(v), kw
    xs = sparse.csr_matrix(case_values("n64-m64"))
    for c0, b, kw in ((0, 0, {}), (0, 65, {}), (-1, 4, {}), (61, 4, {}), (0, 4, dict(ld=3)), (0, 4, dict(null=("indptr",))),
                      (0, 4, dict(null=("slab",))), (0, 4, dict(g_arg=-1)), (0, 4, dict(g_arg=1 << 31))):
        rc, slab = abi.csr_slab(xs, c0, b, **kw)
        assert rc == EINVAL and np.isnan(slab).all(), (c0, b, kw)
    rows = np.ascontiguousarray(x[:, :5].T)
    for kw in (dict(ncols_arg=65), dict(ncols_arg=-1), dict(ld=4), dict(null=("vals",)), dict(null=("slab",))):
        rc, slab = abi.transpose(rows, **kw)
        assert rc == EINVAL and np.isnan(slab).all(), kw
    if launches:
        assert launches() == before, "an argument check let a kernel start"
    # an empty graph is legal: both numerators are 0, W_sum is 0
    empty = (np.zeros(64, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    rc, out = abi.slab(empty, 63, x, 63, 63)
    rc2, w_sum = abi.weight_sum(empty[2])
    assert rc == 0 and rc2 == 0 and w_sum == 0.0 and (out["moran"] == 0).all() and (out["geary"] == 0).all()
    assert abi.lib.scamd_graph_autocorr_part_entries(-1) == 0 and abi.lib.scamd_graph_autocorr_workspace_bytes(-1, 0) == 0
    for z in (0, 1, 58000, 256 * 8192 + 1, 10 ** 10):
        assert abi.lib.scamd_graph_autocorr_part_entries(z) == part_entries(z), z


# ---------------------------------------------------------------------------------------------------------------------
# CPU stand-in for scanpy_amd.metrics._autocorr.GpuAutocorrBackend (the front-end tests): plain float64 numpy.  Every sum is
# strictly sequential down the rows (`cumsum`; `add.reduce` switches to pairwise summation when the array has one column): a
# feature's result depends neither on its neighbours nor on the width of its slab, as on the device.
# ---------------------------------------------------------------------------------------------------------------------
def _seq_sum(a: np.ndarray) -> np.ndarray:
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1])


class CpuStubAutocorrBackend:
    def __init__(self):
        self.calls = []

    def open_graph(self, indptr, indices, weights, n):
        assert weights.dtype in (np.float32, np.float64)
        return {"i": coo_rows(indptr), "j": np.asarray(indices, dtype=np.int64), "w": np.asarray(weights, dtype=np.float64), "n": n,
                "wdtype": weights.dtype}

    def weight_sum(self, g):
        return float(g["w"].sum())

    def stats(self, g, slab, ld, ncols, offset=0):
        n = g["n"]
        assert slab.dtype in (np.float32, np.float64) and slab.ndim == 1 and 1 <= ncols <= SLAB and ncols <= ld
        idx = offset + np.arange(n)[:, None] * ld + np.arange(ncols)[None, :]
        x = slab[idx].astype(np.float64)
        self.calls.append(("stats", slab.dtype.name, g["wdtype"].name, ld, ncols, offset))
        with np.errstate(invalid="ignore", over="ignore"):
            mean = _seq_sum(x) / n
            z = x - mean
            d = x[g["i"]] - x[g["j"]]
            return {"mean": mean, "z2": _seq_sum(z * z), "moran": _seq_sum(g["w"][:, None] * (z[g["i"]] * z[g["j"]])),
                    "geary": _seq_sum(g["w"][:, None] * (d * d)),
                    "min": np.fmin.reduce(x, axis=0), "max": np.fmax.reduce(x, axis=0)}

    def dense_cell_major(self, block):
        assert block.flags.c_contiguous and block.dtype in (np.float32, np.float64)
        self.calls.append(("dense_cell_major", block.dtype.name, block.shape))
        return block.reshape(-1).copy()

    def rows_slab(self, rows):
        assert rows.flags.c_contiguous and rows.shape[0] <= SLAB and rows.dtype in (np.float32, np.float64)
        self.calls.append(("rows_slab", rows.dtype.name, rows.shape))
        slab = np.full((rows.shape[1], SLAB), np.nan, dtype=rows.dtype)
        slab[:, : rows.shape[0]] = rows.T
        return slab.reshape(-1)

    def csr_cell_major(self, indptr, indices, data, n, m):
        x = sparse.csr_matrix((np.asarray(data, dtype=np.float32), indices, indptr), shape=(n, m))
        assert x.has_canonical_format
        self.calls.append(("csr_cell_major", np.dtype(data.dtype).name))
        return x

    def csr_feature_major(self, indptr, indices, data, n, m):
        x = sparse.csr_matrix((np.asarray(data, dtype=np.float32), indices, indptr), shape=(m, n))
        assert x.has_canonical_format
        self.calls.append(("csr_feature_major", np.dtype(data.dtype).name))
        return x.T.tocsr()

    def csr_slab(self, h, c0, ncols):
        slab = np.full((h.shape[0], SLAB), np.nan, dtype=np.float32)
        slab[:, :ncols] = h[:, c0:c0 + ncols].toarray()
        return slab.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# Front-end checks shared by tests/test_autocorr_front_cpu.py (on the stand-in above) and tests/test_gpu_autocorr.py (on the
# device): the reference's test_consistency (tests/test_metrics.py:41-77 of the reference) restated on the committed pbmc68k
# fixture, and the raw-matrix inputs.  `metric`: sc.metrics.morans_i or sc.metrics.gearys_c.
# ---------------------------------------------------------------------------------------------------------------------
PC1 = {"morans_i": 0.95462308, "gearys_c": 0.02310419}   # the restatement on the fixture graph x PC1


def pbmc_adata(pbmc68k):
    import scanpy_amd as sc

    a = sc.AnnData(pbmc68k["X"].copy(), obsm={"X_pca": pbmc68k["X_pca"].copy()}, obsp={"connectivities": pbmc68k["connectivities"].copy()},
                   uns={"neighbors": {"connectivities_key": "connectivities", "distances_key": "distances", "params": {}}})
    a.obs["n_counts"] = pbmc68k["obs_n_counts"].astype(np.float64)
    a.layers["raw"] = pbmc68k["raw_X"].copy()
    a.raw = sc.AnnData(pbmc68k["raw_X"].copy(), a.obs)
    return a


def restate_metric(metric, graph, x):
    g = graph.tocsr()
    return restate(g.indptr, g.indices, g.data, x)[0 if metric.__name__ == "morans_i" else 1]


def front_consistency(metric, pbmc68k):
    a = pbmc_adata(pbmc68k)
    g = a.obsp["connectivities"]
    assert g.shape == (700, 700) and g.nnz == 9992 and g.dtype == np.float64
    col = a.obs["n_counts"]
    one = metric(g, col)
    assert isinstance(one, np.float64) and one == metric(g, col)
    assert one == metric(a, vals=col) == metric(g, col.values)            # Series = ndarray = AnnData path
    assert_close(one, restate_metric(metric, g, col.to_numpy()), "n_counts")
    pcs = metric(a, obsm="X_pca")                                         # read in place: float32, cell-major, ld = 50
    assert pcs.dtype == np.float64 and pcs.shape == (50,)
    assert pcs.tobytes() == metric(g, a.obsm["X_pca"].T).tobytes()
    assert_close(pcs, restate_metric(metric, g, a.obsm["X_pca"].astype(np.float64)), "X_pca")
    assert abs(pcs[0] - PC1[metric.__name__]) < 5e-9
    return a, g


def front_raw_matrix(metric, pbmc68k):
    """700 x 765 = 11 * 64 + 61, density 0.33, no constant column: CSR cells x genes (layer / use_raw), CSC vals, CSR vals and
    dense vals give the same bits; result[0] is the 1-D call on gene 0"""
    a, g = pbmc_adata(pbmc68k), pbmc68k["connectivities"]
    raw = pbmc68k["raw_X"]
    assert raw.shape == (700, 765) and raw.dtype == np.float32 and raw.format == "csr"
    import warnings as _w

    with _w.catch_warnings():
        _w.simplefilter("error")   # no constant column: no warning
        by_layer = metric(a, layer="raw")
        runs = {"use_raw": metric(a, use_raw=True), "csc vals": metric(g, raw.T.tocsc()), "csr vals": metric(g, raw.T.tocsr()),
                "coo vals": metric(g, raw.T.tocoo()), "dense vals": metric(g, raw.T.toarray()),
                "dense C-ordered vals": metric(g, np.ascontiguousarray(raw.T.toarray()))}
    assert by_layer.shape == (765,) and not np.isnan(by_layer).any()
    for k, v in runs.items():
        assert v.tobytes() == by_layer.tobytes(), k
    assert_close(by_layer, restate_metric(metric, g, raw.toarray().astype(np.float64)), "raw_X")
    first = metric(g, raw[:, 0].toarray().ravel())
    assert isinstance(first, np.float64) and first.tobytes() == by_layer[:1].tobytes()
    return by_layer
