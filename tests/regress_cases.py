"""TEST INFRASTRUCTURE shared by tests/test_gpu_regress_out.py (the product library on the GPU), tests/test_emu_regress_cpu.py
(the same kernels on the host emulator) and tests/test_regress_out_front_cpu.py (the front end on a CPU stand-in): the case
table of the regress_out kernels (csrc/regress.hip: `scamd_pp_regress_sums_f32`, `scamd_pp_regress_resid_f32`), restatements of
the rules by which the host code picks an instantiation, a float64 numpy restatement of the two models (centred-QR projection
on the numeric keys; group means for a categorical key; both with the constant-gene rule), ONE checker and a CPU stand-in for
`GpuPPBackend.regress_sums / regress_resid`.  Nothing here touches a device; the callers hand in `RegressAbi` over host memory
(tests/emu/harness.py:HostMem) or device memory (graph_kernel_cases.DeviceMem).

Tolerances (derived, not tuned):
  residual vs restatement   |out - want| <= ulp_out(|want|) / 2 + 1e-9 * (max |x| of the gene); the first term is the single
                            final rounding (0 for float64 output), the second covers the fixed-point and float64 error for
                            regressors whose centred, unit-scaled matrix has a condition number below 1e3 (asserted per case);
  sums vs exact             the bound stated in csrc/regress.hip, (n 2^-61 + 2^-52) wbound[k] max|x_j|, plus numpy's own
                            recursive-summation error n 2^-52 wbound[k] max|x_j| of the float64 product it is compared with."""
from __future__ import annotations

import ctypes as C
import re
import zipfile
from functools import lru_cache
from pathlib import Path

import numpy as np
import pandas as pd
from scipy import sparse

from graph_kernel_cases import EINVAL, EUNSUPPORTED, DeviceMem  # noqa: F401  (DeviceMem: for the GPU tests)
from stub_backend import CpuStubPPBackend

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "scanpy_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden"

# ---------------------------------------------------------------------------------------------------------------------
# The dispatch rules restated; `assert_sources_still_say_so` ties them to the text of csrc/regress.hip.
# ---------------------------------------------------------------------------------------------------------------------
RG_BLOCK = 256
RG_MAX_W = 17
RG_MAX_CATEGORIES = 65536
RG_RANGE_LDS_GENES = 2048
RG_LDS_TABLE_BYTES = 48 * 1024
RG_RESID_GRID = 2048
RG_BATCH_PASSES = 4
RG_G = (8, 16, 32, 64)
RG_TPR = (256, 128, 64)


def sweep_lanes(nnz: int, n: int) -> int:
    avg = nnz // n if n > 0 else 0
    return 8 if avg <= 32 else (16 if avg <= 160 else (32 if avg <= 512 else 64))


def range_table(g: int) -> str:
    return "lds" if g <= RG_RANGE_LDS_GENES else "global"


def sums_table(m: int, g: int) -> str:
    return "lds" if m * g * 8 <= RG_LDS_TABLE_BYTES else "global"


def resid_threads(m: int, cat: bool) -> int:
    return 256 if cat or m <= 4 else (128 if m <= 8 else 64)


def resid_slices(g: int, tpr: int) -> int:
    return -(-g // (4 * tpr))


def resid_row_blocks(n: int, g: int, tpr: int) -> int:
    return min(max(-(-n // (RG_BATCH_PASSES * (RG_BLOCK // tpr))), 1), max(RG_RESID_GRID // resid_slices(g, tpr), 1))


def assert_sources_still_say_so():
    src = (CSRC / "regress.hip").read_text()

    def has(pattern, what):
        assert re.search(pattern, src), f"{what}: /{pattern}/ no longer in csrc/regress.hip -- restate the rule and its cases"

    has(rf"constexpr int RG_BLOCK = {RG_BLOCK};", "RG_BLOCK")
    has(rf"constexpr int RG_MAX_W = {RG_MAX_W};", "RG_MAX_W")
    has(rf"constexpr int RG_MAX_CATEGORIES = {RG_MAX_CATEGORIES};", "RG_MAX_CATEGORIES")
    has(rf"constexpr int RG_RANGE_LDS_GENES = {RG_RANGE_LDS_GENES};", "RG_RANGE_LDS_GENES")
    has(r"constexpr int RG_LDS_TABLE_BYTES = 48 \* 1024;", "RG_LDS_TABLE_BYTES")
    has(rf"constexpr int RG_RESID_GRID = {RG_RESID_GRID};", "RG_RESID_GRID")
    has(r"return avg <= 32 \? 8 : \(avg <= 160 \? 16 : \(avg <= 512 \? 32 : 64\)\);", "rg_lanes_per_row")
    has(r"return \(cat \|\| m <= 4\) \? 256 : \(m <= 8 \? 128 : 64\);", "rg_resid_threads")
    has(r"const bool range_lds = g <= RG_RANGE_LDS_GENES;", "range table split")
    has(r"const bool sums_lds = cells \* 8 <= RG_LDS_TABLE_BYTES;", "sums table split")
    has(rf"constexpr int RG_BATCH_PASSES = {RG_BATCH_PASSES};", "RG_BATCH_PASSES")
    has(r"constexpr int CS = TPR \* 4, RPB = RG_BLOCK / TPR, R = RG_BATCH_PASSES \* RPB;", "columns per slice, rows per batch")
    has(r"std::max<int64_t>\(RG_RESID_GRID / slices, 1\)", "residual grid")
    for G in RG_G[:-1]:
        has(rf"case {G}: rg_launch_range<{G}>\(", f"range G = {G}")
        has(rf"case {G}: rg_launch_sums<{G}>\(", f"sums G = {G}")
    has(r"default: rg_launch_range<64>\(", "range G = 64")
    has(r"default: rg_launch_sums<64>\(", "sums G = 64")
    has(r"case 256: rg_launch_resid<OutT, 256>\(", "TPR 256")
    has(r"case 128: rg_launch_resid<OutT, 128>\(", "TPR 128")
    has(r"default: rg_launch_resid<OutT, 64>\(", "TPR 64")


# ---------------------------------------------------------------------------------------------------------------------
# Case table.  model: ("num", r) = r numeric keys (W = [1, Q], m = r + 1) or ("cat", K).  avg: the mean row length nnz // n the
# matrix is built to (it selects the lanes per row).  Every sparse matrix with g >= 5 and n >= 3 carries three special genes:
# gene 0 is never stored (constant as implicit zeros), gene 1 holds 2.5 in every row (constant as stored values), gene 2 holds
# 2.5 in every row but the last (constant except one cell); row 0 is empty but for them, row 1 is full, row 2 holds one more entry.
# ---------------------------------------------------------------------------------------------------------------------
#     name            n     g    avg  model         fmt      out_f64  values
CASES = (
    ("n1",            1,    5,    2, ("num", 1),   "csr",   True,  "lognormal"),
    ("n2-cat2",       2,    3,    1, ("cat", 2),   "csr",   True,  "counts"),
    ("n63-r2",       63,  255,   20, ("num", 2),   "csr",   False, "lognormal"),
    ("n64-r16",      64,  257,  100, ("num", 16),  "csc",   True,  "lognormal"),
    ("n65-wide",     65, 2049,  300, ("num", 2),   "csr",   False, "wide"),
    ("n1000-r0",   1000,    5,    5, ("num", 0),   "dense", False, "counts"),
    ("g1-k1",        64,    1,    0, ("cat", 1),   "csr",   True,  "counts"),
    ("g3-k3",        65,    3,    1, ("cat", 3),   "csc",   False, "lognormal"),
    ("k64",        1000,  257,   40, ("cat", 64),  "csr",   True,  "lognormal"),
    ("k1000",      1000,  255,   10, ("cat", 1000), "csr",  False, "wide"),
    ("full-rows",    63,  600,  600, ("num", 1),   "dense", True,  "lognormal"),
    ("r5",           65,  260,   50, ("num", 5),   "csr",   False, "counts"),
    ("r16-slices",   64, 2049,   60, ("num", 16),  "csr",   True,  "lognormal"),
    ("k2-slices",    63, 2049,  170, ("cat", 2),   "csr",   False, "counts"),
    ("all-zero",     65,  257,    0, ("num", 2),   "csr",   False, "zero"),
    ("all-zero-cat", 65,  257,    0, ("cat", 3),   "csr",   True,  "zero"),
    ("row-stride", 3000, 2049,    8, ("num", 2),   "csr",   False, "lognormal"),
    ("long",       5000,   40,    8, ("num", 2),   "csr",   False, "lognormal"),
    ("long-cat",   5000,   40,    8, ("cat", 64),  "csr",   True,  "lognormal"),
)
CASE_NAMES = tuple(c[0] for c in CASES)
DETERMINISM_CASES = ("long", "long-cat")   # n = 5000, g = 40: every gene is shared by many workgroups
COND_LIMIT = 1e3


def _case(name):
    return next(c for c in CASES if c[0] == name)


def _seed(name: str) -> int:
    return 1000 + sum(map(ord, name))


@lru_cache(maxsize=None)
def case_matrix(name: str):
    """-> the host matrix in the case's format (float32), read-only"""
    _, n, g, avg, _, fmt, _, kind = _case(name)
    rng = np.random.default_rng(_seed(name))
    special = g >= 5 and n >= 3 and fmt != "dense" and kind != "zero"
    if fmt == "dense":
        assert avg == g
        dense = _values(kind, (n, g), rng)
        dense.setflags(write=False)
        return dense
    lengths = np.zeros(n, dtype=np.int64)
    if kind != "zero":
        lo, hi = (3, g - 1) if special else (0, g)
        lengths[:] = np.clip(rng.poisson(max(avg, 1), n), lo, hi)
        if special:
            lengths[0], lengths[1], lengths[2] = 2, g - 1, 3
        free = np.arange(3 if special else 0, n)
        diff = avg * n + n // 2 - int(lengths.sum())   # nnz // n == avg
        i = 0
        while diff != 0:
            j = free[i % len(free)]
            step = 1 if diff > 0 else -1
            if lo <= lengths[j] + step <= hi:
                lengths[j] += step
                diff -= step
            i += 1
            assert i < 64 * n * max(g, 1), name
    rows = []
    for i, ln in enumerate(lengths):
        if special:
            must = [1] if i == n - 1 else [1, 2]
            pool = np.setdiff1d(np.arange(g), [0, 1, 2])
            extra = rng.choice(pool, size=min(max(int(ln) - len(must), 0), len(pool)), replace=False)
            rows.append(np.sort(np.concatenate([must, extra])))
        else:
            rows.append(np.sort(rng.choice(g, size=int(ln), replace=False)))
    ln = np.array([len(r) for r in rows], dtype=np.int64)
    indices = np.concatenate(rows).astype(np.int32) if len(rows) and ln.sum() else np.zeros(0, np.int32)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    cols_scale = 10.0 ** rng.uniform(-6, 6, g) if kind == "wide" else None
    data = _values(kind, (len(indices),), rng)
    if cols_scale is not None:
        data = (data * cols_scale[indices]).astype(np.float32)
    if special:
        data[(indices == 1) | (indices == 2)] = 2.5
    x = sparse.csr_matrix((data, indices, indptr), shape=(n, g))
    assert x.has_canonical_format
    if fmt == "csc":
        x = x.tocsc()
    for a in (x.data, x.indices, x.indptr):
        a.setflags(write=False)
    return x


def _values(kind, shape, rng):
    if kind == "counts":
        return np.floor(2.0 ** rng.uniform(0, 12, shape)).astype(np.float32)
    if kind == "lognormal":
        return rng.lognormal(0.5, 1.0, shape).astype(np.float32)
    if kind == "wide":   # signs; the spread over 1e-6 .. 1e6 comes from the per-gene scale
        return (rng.lognormal(0.0, 0.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    if kind == "zero":
        return np.zeros(shape, dtype=np.float32)
    raise ValueError(kind)


def case_csr(name: str) -> sparse.csr_matrix:
    """the matrix as the device sees it: canonical CSR float32 (a dense matrix as the full pattern)"""
    x = case_matrix(name)
    if sparse.issparse(x):
        return x.tocsr()
    n, g = x.shape
    return sparse.csr_matrix((x.ravel().copy(), np.tile(np.arange(g, dtype=np.int32), n), np.arange(n + 1, dtype=np.int64) * g),
                             shape=(n, g))


def basis(regressors: np.ndarray) -> np.ndarray:
    """orthonormal basis (SVD) of the centred, unit-scaled columns; constant columns dropped"""
    n, p = regressors.shape
    if p == 0 or n == 0:
        return np.zeros((n, 0))
    c = regressors - regressors.mean(axis=0)
    c[:, regressors.max(axis=0) == regressors.min(axis=0)] = 0.0
    nrm = np.sqrt((c * c).sum(axis=0))
    live = nrm > 0
    if not live.any():
        return np.zeros((n, 0))
    u, s, _ = np.linalg.svd(c[:, live] / nrm[live], full_matrices=False)
    return np.ascontiguousarray(u[:, s > max(n, p) * np.finfo(float).eps * s[0]])


@lru_cache(maxsize=None)
def case_model(name: str) -> dict:
    """-> dict(regressors float64 [n, r] | None, w float64 [n, m] | None, codes int32 [n] | None, m, wbound float64 [m])"""
    _, n, g, _, (kind, k), _, _, _ = _case(name)
    rng = np.random.default_rng(_seed(name) + 7)
    if kind == "cat":
        if k >= n:                      # more categories than cells: singletons and empty categories
            codes = rng.permutation(k)[:n].astype(np.int32)
        else:
            codes = rng.integers(0, k, n).astype(np.int32)
            if k >= 3 and n > 3:
                codes[codes == 1] = 0   # category 1 is empty ...
                codes[n // 2] = 2       # ... and category 2 a singleton
                codes[(codes == 2) & (np.arange(n) != n // 2)] = 0
        size = np.bincount(codes, minlength=k).astype(np.float64)
        return {"regressors": None, "w": None, "codes": codes, "m": k, "wbound": size}
    # numeric: columns of different offsets and scales (counts next to fractions), conditioned after centring and scaling
    reg = rng.normal(size=(n, k)) * 10.0 ** rng.uniform(-2, 3, k) + 10.0 ** rng.uniform(0, 4, k)
    if k and n > k + 1:
        c = reg - reg.mean(axis=0)
        cond = np.linalg.cond(c / np.sqrt((c * c).sum(axis=0)))
        assert cond < COND_LIMIT, (name, cond)
    w = np.ascontiguousarray(np.concatenate([np.ones((n, 1)), basis(reg)], axis=1))
    return {"regressors": reg, "w": w, "codes": None, "m": w.shape[1], "wbound": np.abs(w).sum(axis=0) * (1 + 1e-6)}


def assert_every_regress_path_has_a_case():
    """-> the sets of (G, range table, sums table) and (TPR, categorical, out_f64) the table reaches"""
    sweeps, resids = set(), set()
    ns, gs, rs, ks, fmts = set(), set(), set(), set(), set()
    for name, n, g, avg, (kind, k), fmt, f64, _ in CASES:
        x = case_csr(name)
        mdl = case_model(name)
        assert x.shape == (n, g) and (avg == 0 or x.nnz // n == avg), (name, x.nnz // n, avg)
        G = sweep_lanes(x.nnz, n)
        sweeps.add((G, range_table(g), sums_table(mdl["m"] if kind == "num" else k, g)))
        tpr = resid_threads(mdl["m"], kind == "cat")
        resids.add((tpr, kind == "cat", f64))
        ns.add(n), gs.add(g), fmts.add(fmt)
        (rs if kind == "num" else ks).add(k)
        ln = np.diff(x.indptr)
        if g >= 5 and n >= 3 and fmt != "dense" and x.nnz:
            assert ln[0] == 2 and ln[1] == g - 1 and ln.min() >= 1, name   # (near-)empty, full, short rows
    assert {G for G, _, _ in sweeps} == set(RG_G)
    assert {t for _, t, _ in sweeps} == {"lds", "global"} and {t for _, _, t in sweeps} == {"lds", "global"}
    assert {(t, c) for t, c, _ in resids} == {(256, False), (128, False), (64, False), (256, True)}
    assert {(c, f) for _, c, f in resids} == {(False, False), (False, True), (True, False), (True, True)}
    assert ns >= {1, 2, 63, 64, 65, 1000} and gs >= {1, 3, 5, 255, 257, 2049} and fmts == {"csr", "csc", "dense"}
    assert rs >= {0, 1, 2, 16} and ks >= {1, 2, 3, 64, 1000}
    # a slice boundary inside the matrix for every thread count, the vector and the scalar store, and the row-block stride
    assert resid_slices(2049, 256) == 3 and resid_slices(2049, 64) == 9 and resid_slices(260, 128) == 1
    assert resid_row_blocks(5000, 40, 256) == 1250 and resid_row_blocks(3000, 2049, 256) == 2048 // 3 < 3000 // 4   # (a row-block stride)
    assert any(c[1] == 3000 and c[2] == 2049 and resid_threads(case_model(c[0])['m'], False) == 256 for c in CASES)
    assert any(c[2] % 4 == 0 for c in CASES) and any(c[2] % 4 for c in CASES)
    for name in DETERMINISM_CASES:
        assert _case(name)[1] == 5000 and _case(name)[2] == 40
    kinds = {c[7] for c in CASES}
    assert {"wide", "zero"} <= kinds
    return sweeps, resids


# ---------------------------------------------------------------------------------------------------------------------
# The restatement, float64 numpy on the dense matrix.
# ---------------------------------------------------------------------------------------------------------------------
def constant_genes(dense: np.ndarray) -> np.ndarray:
    return (dense == dense[:1]).all(axis=0) if dense.shape[0] else np.ones(dense.shape[1], bool)


def ref_numeric(dense: np.ndarray, regressors: np.ndarray, *, keep_constant: bool) -> np.ndarray:
    """the residual of projecting every gene on span[1, regressors]: centred-QR projection, orthogonalised twice"""
    x = np.asarray(dense, dtype=np.float64)
    n = x.shape[0]
    out = x - x.mean(axis=0)
    if regressors is not None and regressors.shape[1] and n:
        c = regressors - regressors.mean(axis=0)
        c[:, regressors.max(axis=0) == regressors.min(axis=0)] = 0.0
        nrm = np.sqrt((c * c).sum(axis=0))
        c = c[:, nrm > 0] / nrm[nrm > 0]
        if c.shape[1]:
            q, r = np.linalg.qr(c)
            q = q[:, np.abs(np.diag(r)) > max(c.shape) * np.finfo(float).eps * np.abs(np.diag(r)).max()]
            out = out - q @ (q.T @ out)
            out = out - q @ (q.T @ out)
    if keep_constant:
        const = constant_genes(x)
        out[:, const] = x[:, const]
    return out


def ref_categorical(dense: np.ndarray, codes: np.ndarray, k: int, *, keep_constant: bool = True) -> np.ndarray:
    x = np.asarray(dense, dtype=np.float64)
    out = x.copy()
    for c in range(k):
        sel = codes == c
        if sel.any():
            out[sel] = x[sel] - x[sel].mean(axis=0)
    if keep_constant:
        const = constant_genes(x)
        out[:, const] = x[:, const]
    return out


def half_ulp(want: np.ndarray, out_dtype) -> np.ndarray:
    if np.dtype(out_dtype) == np.float64:
        return np.zeros_like(want)
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) / 2


def assert_residual_close(got: np.ndarray, want: np.ndarray, gene_absmax: np.ndarray, what=""):
    """|out - want| <= ulp_out(|want|) / 2 + 1e-9 * max|x| of the gene"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), (what, "elements not written", np.argwhere(np.isnan(got))[:4])
    err = np.abs(got.astype(np.float64) - want)
    tol = half_ulp(want, got.dtype) + 1e-9 * gene_absmax[None, :]
    worst = (err - tol).max() if err.size else 0.0
    assert worst <= 0, (what, "error beyond the tolerance by", float(worst), np.unravel_index(np.argmax(err - tol), err.shape))


def table_from_sums(sums: np.ndarray, n: int, mdl: dict) -> np.ndarray:
    """T as the front end makes it: category means, or [mean; Q^T X]"""
    if mdl["codes"] is not None:
        return sums / np.maximum(mdl["wbound"], 1.0)[:, None]
    t = sums.copy()
    t[0] /= max(n, 1)
    return t


# ---------------------------------------------------------------------------------------------------------------------
# Callers of the entry points through the raw C ABI: numpy in, numpy out, the return code handed back, outputs prefilled with
# NaN / -1 so that an element nobody wrote shows.  `mem`: tests/emu/harness.py:HostMem or graph_kernel_cases.DeviceMem.
# ---------------------------------------------------------------------------------------------------------------------
class RegressAbi:
    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def _in(self, x, null):
        m = self.mem
        bufs = (m.put(x.indptr, np.int64), m.put(x.indices, np.int32), m.put(x.data, np.float32))
        z = C.c_void_p(0)
        return bufs, [z if name in null else m.ptr(b) for name, b in zip(("indptr", "indices", "data"), bufs)]

    def _model(self, w, codes, null):
        m, z = self.mem, C.c_void_p(0)
        dw = None if w is None else m.put(w, np.float64)
        dc = None if codes is None else m.put(codes, np.int32)
        return (dw, dc), (z if dw is None or "w" in null else m.ptr(dw)), (z if dc is None or "codes" in null else m.ptr(dc))

    def sums(self, x, *, w=None, codes=None, m_rows, wbound, n=None, g=None, nnz=None, null=(), ws_short=0):
        """-> (rc, dict(sums [m_rows, g of x], col_min, col_max, flags))"""
        m = self.mem
        keep, (ip, ix, dv) = self._in(x, null)
        alive, pw, pc = self._model(w, codes, null)
        nr, gx = x.shape
        mr = max(min(int(m_rows), 1 << 17), 1)
        d_wb = m.put(np.resize(np.asarray(wbound, dtype=np.float64), mr) if len(np.atleast_1d(wbound)) else np.ones(mr), np.float64)
        out = {"sums": m.full((mr, max(gx, 1)), np.float64, np.nan), "col_min": m.full(max(gx, 1), np.float32, np.nan),
               "col_max": m.full(max(gx, 1), np.float32, np.nan), "flags": m.full(1, np.int32, -1)}
        nbytes = int(self.lib.scamd_pp_regress_workspace_bytes(gx, mr))
        ws = m.full(max(nbytes - ws_short, 1), np.uint8, 0xAB)
        z = C.c_void_p(0)

        def p(name):
            return z if name in null else m.ptr(out[name])

        rc = self.lib.scamd_pp_regress_sums_f32(ip, ix, dv, nr if n is None else n, gx if g is None else g,
                                                x.nnz if nnz is None else nnz, pw, pc, int(m_rows),
                                                z if "wbound" in null else m.ptr(d_wb), p("sums"), p("col_min"), p("col_max"),
                                                p("flags"), z if "workspace" in null else m.ptr(ws), max(nbytes - ws_short, 0), m.stream)
        m.sync()
        res = {name: m.get(a) for name, a in out.items()}
        res["sums"] = res["sums"][:, :gx] if gx else res["sums"][:, :0]
        res["col_min"], res["col_max"] = res["col_min"][:gx], res["col_max"][:gx]
        return rc, res

    def resid(self, x, table, keep_mask, *, w=None, codes=None, out_f64=True, m_rows=None, n=None, g=None, nnz=None, null=()):
        """-> (rc, out [rows of x, columns of x], prefilled with NaN)"""
        m = self.mem
        keep, (ip, ix, dv) = self._in(x, null)
        alive, pw, pc = self._model(w, codes, null)
        nr, gx = x.shape
        d_t = m.put(table, np.float64)
        d_k = m.put(keep_mask, np.uint8)
        out = m.full((max(nr, 1), max(gx, 1)), np.float64 if out_f64 else np.float32, np.nan)
        z = C.c_void_p(0)
        rc = self.lib.scamd_pp_regress_resid_f32(ip, ix, dv, nr if n is None else n, gx if g is None else g,
                                                 x.nnz if nnz is None else nnz, z if "keep" in null else m.ptr(d_k),
                                                 z if "table" in null else m.ptr(d_t), pw, pc,
                                                 int(np.shape(table)[0] if m_rows is None else m_rows),
                                                 z if "out" in null else m.ptr(out), int(out_f64), m.stream)
        m.sync()
        return rc, m.get(out)[:nr, :gx]


# ---------------------------------------------------------------------------------------------------------------------
# The checker: one case through both entry points.
# ---------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -52


def run_case(rabi: RegressAbi, name: str, label="", rerun=None):
    _, n, g, _, (kind, k), _, out_f64, _ = _case(name)
    x = case_csr(name)
    mdl = case_model(name)
    dense = x.toarray().astype(np.float64)
    what = f"{label} {name}"
    kw = {"w": mdl["w"], "codes": mdl["codes"]}
    rc, s = rabi.sums(x, m_rows=mdl["m"], wbound=mdl["wbound"], **kw)
    assert rc == 0, (what, rc)
    assert int(s["flags"][0]) == 0, (what, s["flags"])
    # the range, implicit zeros included: exact
    assert np.array_equal(s["col_min"], dense.min(axis=0).astype(np.float32)), what
    assert np.array_equal(s["col_max"], dense.max(axis=0).astype(np.float32)), what
    amax = np.abs(dense).max(axis=0)
    # the sums against the float64 product, within the stated bound (plus numpy's own summation error)
    wmat = mdl["w"] if kind == "num" else (mdl["codes"][:, None] == np.arange(k)[None, :]).astype(np.float64)
    exact = wmat.T @ dense
    tol = (n * 2.0 ** -61 + (n + 2) * U) * mdl["wbound"][:, None] * amax[None, :]
    assert np.all(np.abs(s["sums"] - exact) <= tol), (what, "sums", float((np.abs(s["sums"] - exact) - tol).max()))
    assert np.all(s["sums"][:, amax == 0] == 0), what
    table = table_from_sums(s["sums"], n, mdl)
    const = constant_genes(dense)
    assert np.array_equal(s["col_min"] == s["col_max"], const), what
    if g >= 5 and n >= 3 and _case(name)[5] != "dense" and x.nnz:
        assert const[0] and const[1] and not const[2], what   # the three special genes
    # the residual: with the constant-gene rule (the float64 routes of the front end) and without it
    for keep_constant in (True, False):
        keep = (~const).astype(np.uint8) if keep_constant else np.ones(g, dtype=np.uint8)
        rc, out = rabi.resid(x, table, keep, out_f64=out_f64, **kw)
        assert rc == 0, (what, rc)
        want = (ref_numeric(dense, mdl["regressors"], keep_constant=keep_constant) if kind == "num"
                else ref_categorical(dense, mdl["codes"], k, keep_constant=keep_constant))
        assert_residual_close(out, want, amax, f"{what} keep_constant={keep_constant}")
        if keep_constant:
            assert np.array_equal(out[:, const].astype(np.float64), dense[:, const]), (what, "a constant gene was changed")
    if rerun if rerun is not None else name in DETERMINISM_CASES:
        rc2, s2 = rabi.sums(x, m_rows=mdl["m"], wbound=mdl["wbound"], **kw)
        rc3, out2 = rabi.resid(x, table, np.ones(g, dtype=np.uint8), out_f64=out_f64, **kw)
        assert rc2 == 0 and rc3 == 0
        for key in s:
            assert s[key].tobytes() == s2[key].tobytes(), (what, key, "two runs differ")
        assert out.tobytes() == out2.tobytes(), (what, "two runs of the residual differ")
    return s, out


def run_nonfinite_case(rabi: RegressAbi, label=""):
    """a stored NaN and a stored infinity raise bit 0 and take part in nothing; a code outside [0, m) raises bit 1"""
    rng = np.random.default_rng(5)
    x = sparse.random(70, 33, density=0.3, format="csr", dtype=np.float32, random_state=5)
    x.data = np.ceil(x.data * 9).astype(np.float32)
    clean = x.copy()
    x.data[3], x.data[40] = np.nan, np.inf
    clean.data[3], clean.data[40] = 0.0, 0.0
    w = np.concatenate([np.ones((70, 1)), basis(rng.normal(size=(70, 2)))], axis=1)
    wb = np.abs(w).sum(axis=0) * (1 + 1e-6)
    rc, s = rabi.sums(x, w=w, m_rows=3, wbound=wb)
    assert rc == 0 and int(s["flags"][0]) == 1, (label, rc, s["flags"])
    exact = w.T @ clean.toarray().astype(np.float64)
    amax = np.abs(clean.toarray()).max(axis=0)
    assert np.all(np.abs(s["sums"] - exact) <= (70 * 2.0 ** -61 + 72 * U) * wb[:, None] * amax[None, :]), label
    rc, s = rabi.sums(clean, w=w, m_rows=3, wbound=wb)
    assert rc == 0 and int(s["flags"][0]) == 0, label
    codes = rng.integers(0, 4, 70).astype(np.int32)
    codes[11] = 4
    rc, s = rabi.sums(clean, codes=codes, m_rows=4, wbound=np.bincount(codes, minlength=5)[:4].astype(float))
    assert rc == 0 and int(s["flags"][0]) == 2, (label, s["flags"])


def run_argument_checks(rabi: RegressAbi, launches=None):
    """the documented codes; a rejected call starts no kernel and writes no output"""
    x = sparse.random(20, 64, density=0.2, format="csr", dtype=np.float32, random_state=3)
    rng = np.random.default_rng(3)
    w = np.concatenate([np.ones((20, 1)), basis(rng.normal(size=(20, 2)))], axis=1)
    wb = np.abs(w).sum(axis=0) * 1.001
    codes = rng.integers(0, 3, 20).astype(np.int32)
    before = launches() if launches else 0
    for kw, code in ((dict(null=("indptr",)), EINVAL), (dict(n=-1), EINVAL), (dict(g=-1), EINVAL), (dict(nnz=-1), EINVAL),
                     (dict(g=1 << 31), EINVAL), (dict(null=("data",)), EINVAL), (dict(null=("indices",)), EINVAL),
                     (dict(null=("wbound",)), EINVAL), (dict(null=("sums",)), EINVAL), (dict(null=("col_min",)), EINVAL),
                     (dict(null=("col_max",)), EINVAL), (dict(null=("flags",)), EINVAL), (dict(null=("workspace",)), EINVAL),
                     (dict(ws_short=256), EINVAL), (dict(null=("w",)), EINVAL), (dict(codes=codes), EINVAL),
                     (dict(m_rows=0), EINVAL), (dict(m_rows=RG_MAX_W + 1), EUNSUPPORTED)):
        args = dict(w=w, m_rows=3, wbound=wb)
        args.update(kw)
        rc, out = rabi.sums(x, **args)
        assert rc == code, (kw, rc)
        for name, a in out.items():
            assert np.isnan(a).all() if a.dtype.kind == "f" else (a == -1).all(), (kw, name)
    rc, _ = rabi.sums(x, codes=codes, m_rows=RG_MAX_CATEGORIES + 1, wbound=np.ones(3))
    assert rc == EUNSUPPORTED
    table, keep = np.zeros((3, 64)), np.ones(64, dtype=np.uint8)
    for kw, code in ((dict(null=("indptr",)), EINVAL), (dict(n=-1), EINVAL), (dict(g=-1), EINVAL), (dict(nnz=-1), EINVAL),
                     (dict(g=1 << 31), EINVAL), (dict(null=("data",)), EINVAL), (dict(null=("indices",)), EINVAL),
                     (dict(null=("keep",)), EINVAL), (dict(null=("table",)), EINVAL), (dict(null=("out",)), EINVAL),
                     (dict(null=("w",)), EINVAL), (dict(codes=codes), EINVAL), (dict(m_rows=0), EINVAL),
                     (dict(m_rows=RG_MAX_W + 1), EUNSUPPORTED)):
        args = dict(w=w)
        args.update(kw)
        rc, out = rabi.resid(x, table, keep, **args)
        assert rc == code, (kw, rc)
        assert np.isnan(out).all(), kw
    if launches:
        assert launches() == before, "an argument check let a kernel start"
    # n = 0: the sums are zero, the range is [0, 0], nothing else is written; g = 0: only the flag word is zeroed
    rc, s = rabi.sums(x, w=w, m_rows=3, wbound=wb, n=0)
    assert rc == 0 and (s["sums"] == 0).all() and (s["col_min"] == 0).all() and (s["col_max"] == 0).all() and s["flags"][0] == 0
    rc, out = rabi.resid(x, table, keep, w=w, n=0)
    assert rc == 0 and np.isnan(out).all()
    empty = sparse.csr_matrix((7, 0), dtype=np.float32)
    rc, s = rabi.sums(empty, w=w[:7], m_rows=3, wbound=wb)
    assert rc == 0 and s["flags"][0] == 0
    rc, out = rabi.resid(empty, np.zeros((3, 0)), np.zeros(0, np.uint8), w=w[:7])
    assert rc == 0


# ---------------------------------------------------------------------------------------------------------------------
# The pbmc68k fixture of the reference's golden outputs (tests/_data/regress_test_small*.npy were computed on
# pbmc68k_reduced().raw.to_adata()[:200, :200]): the obs columns come from the committed zarr store.
# ---------------------------------------------------------------------------------------------------------------------
ZIP_PARTS = sorted(GOLDEN.glob("10x_pbmc68k_reduced.zarr.zip.part*"), key=lambda f: int(f.name.rsplit("part", 1)[1]))


def pbmc68k_obs(tmp_dir) -> pd.DataFrame:
    import scanpy_amd as sc

    f = Path(tmp_dir) / "10x_pbmc68k_reduced.zarr.zip"
    f.write_bytes(b"".join(part.read_bytes() for part in ZIP_PARTS))
    assert zipfile.is_zipfile(f)
    return sc.read_zarr(f).obs


def golden_adata(raw_x, obs: pd.DataFrame):
    import scanpy_amd as sc

    a = sc.AnnData(raw_x[:200, :200].copy())
    for key in ("n_counts", "percent_mito", "bulk_labels"):
        a.obs[key] = obs[key].iloc[:200].to_numpy() if key != "bulk_labels" else pd.Categorical(obs[key].iloc[:200].astype(str))
    return a


def assert_matches_numeric_golden(got: np.ndarray):
    golden = np.load(GOLDEN / "regress_test_small.npy")
    atol = 2.0 ** -23 * np.abs(golden).max()   # one float32 ulp at the largest entry
    assert got.dtype == np.float32 and got.shape == golden.shape
    err = np.abs(got.astype(np.float64) - golden.astype(np.float64)).max()
    assert err <= atol, (err, atol)


def assert_matches_categorical_golden(got: np.ndarray):
    golden = np.load(GOLDEN / "regress_test_small_cat.npy")
    assert got.dtype == np.float64 and got.shape == golden.shape
    np.testing.assert_allclose(got, golden, rtol=0, atol=1e-6)   # the reference's own atol


# ---------------------------------------------------------------------------------------------------------------------
# CPU stand-in for GpuPPBackend.regress_sums / regress_resid (the front-end tests): plain float64 numpy
# ---------------------------------------------------------------------------------------------------------------------
class CpuStubRegressBackend(CpuStubPPBackend):
    @staticmethod
    def _dense(m):
        d = np.zeros(m.shape, dtype=np.float64)
        d[m.rows, m.indices] = m.data
        return d

    @staticmethod
    def _w(n, w, codes, k):
        return np.asarray(w, dtype=np.float64) if w is not None else (np.asarray(codes)[:, None] == np.arange(k)[None, :]).astype(np.float64)

    def regress_sums(self, m, *, w=None, codes=None, n_table, wbound):
        d = self._dense(m)
        bad = ~np.isfinite(d)
        wm = self._w(m.shape[0], w, codes, n_table)
        assert wm.shape == (m.shape[0], n_table) and np.all(np.abs(wm).sum(axis=0) <= np.asarray(wbound) + 1e-300)
        clean = np.where(bad, 0.0, d)
        return {"sums": wm.T @ clean, "col_min": clean.min(axis=0, initial=0.0 if not len(d) else np.inf).astype(np.float32),
                "col_max": clean.max(axis=0, initial=0.0 if not len(d) else -np.inf).astype(np.float32),
                "nonfinite": bool(bad.any()), "bad_code": bool(codes is not None and ((codes < 0) | (codes >= n_table)).any())}

    def regress_resid(self, m, table, keep, *, w=None, codes=None, out_f64=True):
        d = self._dense(m)
        fit = self._w(m.shape[0], w, codes, np.shape(table)[0]) @ np.asarray(table, dtype=np.float64)
        out = np.where(np.asarray(keep, dtype=bool)[None, :], d - fit, d)
        return out.astype(np.float64 if out_f64 else np.float32)
