"""TEST INFRASTRUCTURE shared by tests/test_gpu_pearson.py (the product library on the GPU), tests/test_emu_pearson_cpu.py (the
same kernels on the host emulator) and tests/test_pearson_front_cpu.py (the front end on a CPU stand-in): the case table of the
kernels of csrc/pearson.hip (`scamd_pp_pearson_gene_var_f32`, `scamd_pp_pearson_residuals_f32`), the float64 numpy restatement
(the clipped residual matrix, and per batch the direct `np.var` of it), ONE checker and a CPU stand-in for
`GpuPPBackend.row_totals64 / pearson_gene_var / pearson_residuals`.  Nothing here touches a device; the callers hand in
`PearsonAbi` over host memory (tests/emu/harness.py:HostMem) or device memory (graph_kernel_cases.DeviceMem).

Tolerances (derived from the operation counts stated in csrc/pearson.hip, not tuned; u = 2^-53):
  residual, float64 out   |out - want| <= 20 u (|x| + mu) / sigma: 10 u for each side (mu: 2 roundings, x - mu: 1, sigma^2: 3,
                          the square root, the division, and 2 u of slack for the two ways mu is parenthesised); (|x| + mu) / sigma
                          >= |r|, so this is 20 u relative where nothing cancels and the matching absolute term where x is
                          close to mu.  The clip is 1-Lipschitz: entries at the clip edge need no exemption.
  residual, float32 out   the float64 value rounded once: within 1 ulp of float32 of the restatement.
  gene variance           `var_bound`: the forward bound of the header -- N u on the sweep over the totals (N = U + 16 + 8 for the
                          roundings inside a term), nnz_j gmax 2^-62 + 2 u |sum| on each fixed-point sum, the 20 u (|x| + mu) /
                          sigma of every residual carried through the mean and the squares to first order plus the square, and
                          numpy's own (n + 4) u on the `np.var` it is compared with."""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
from scipy import sparse

from graph_kernel_cases import EINVAL, DeviceMem  # noqa: F401  (DeviceMem: for the GPU tests)
from stub_backend import CpuStubPPBackend

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "scanpy_amd" / "csrc"
EWORKSPACE = -2
U53 = 2.0 ** -53

# the constants of csrc/pearson.hip the table is built around (`assert_sources_still_say_so`, `assert_library_agrees`)
PR_BLOCK = 256
PR_CHUNK = 4096
PR_CS = 1024
PR_ROWS = 8


def assert_sources_still_say_so():
    src = (CSRC / "pearson.hip").read_text()
    for pattern in (rf"constexpr int PR_BLOCK = {PR_BLOCK};", rf"constexpr int PR_CHUNK = {PR_CHUNK};",
                    r"constexpr int PR_CS = 4 \* PR_BLOCK;", rf"constexpr int PR_ROWS = {PR_ROWS};",
                    r"return j \+ t_indptr\[j\] / PR_CHUNK;", r"r\.slots = g \+ nnz / PR_CHUNK \+ 1;"):
        assert re.search(pattern, src), f"/{pattern}/ no longer in csrc/pearson.hip -- restate the rule and its cases"
    assert "atomic" not in src.split("#include", 1)[1], "csrc/pearson.hip is stated to use no atomics"


def assert_library_agrees(lib):
    v = [C.c_int32(-1) for _ in range(4)]
    assert lib.scamd_pp_pearson_limits(*[C.byref(a) for a in v]) == 0
    assert [a.value for a in v] == [PR_CHUNK, PR_BLOCK, PR_CS, PR_ROWS]
    assert lib.scamd_pp_pearson_limits(None, None, None, None) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# The restatement: float64 numpy.
# ---------------------------------------------------------------------------------------------------------------------
def restate_residuals(dense: np.ndarray, theta: float, clip: float) -> np.ndarray:
    """the clipped Pearson residuals of a dense float64 matrix, as `_pearson_residuals` of the reference forms them"""
    x = np.asarray(dense, dtype=np.float64)
    s, t = x.sum(axis=0, keepdims=True), x.sum(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        mu = t @ s / s.sum()
        r = (x - mu) / np.sqrt(mu + mu ** 2 / theta)
    return np.clip(r, -clip, clip)


def restate_gene_var(dense: np.ndarray, theta: float, clip: float, codes=None, batch=0) -> np.ndarray:
    """per gene `np.var` of the clipped residual matrix of one batch's cells; genes whose sum is 0 are left out and get 0"""
    x = np.asarray(dense, dtype=np.float64)
    if codes is not None:
        x = x[np.asarray(codes) == batch]
    live = x.sum(axis=0) != 0
    out = np.zeros(x.shape[1])
    if live.any():
        with np.errstate(all="ignore"):
            out[live] = np.var(restate_residuals(x[:, live], theta, clip), axis=0)
    return out


def residual_tolerance(dense: np.ndarray, theta: float) -> np.ndarray:
    x = np.asarray(dense, dtype=np.float64)
    s, t = x.sum(axis=0, keepdims=True), x.sum(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        mu = t @ s / s.sum()
        return 20 * U53 * (np.abs(x) + mu) / np.sqrt(mu + mu ** 2 / theta)


def var_bound(dense: np.ndarray, stored: np.ndarray, theta: float, clip: float, n_u: int) -> np.ndarray:
    """the per-gene tolerance of the module docstring for one batch's cells (dense, stored: [n, g] of that batch)"""
    x = np.asarray(dense, dtype=np.float64)
    n = x.shape[0]
    with np.errstate(all="ignore"):
        rho = restate_residuals(x, theta, clip)
        s, t = x.sum(axis=0, keepdims=True), x.sum(axis=1, keepdims=True)
        mu = t @ s / s.sum()
        sigma = np.sqrt(mu + mu ** 2 / theta)
        z = np.clip(-mu / sigma, -clip, clip)
        e_res = 20 * U53 * (np.abs(x) + mu) / sigma
        m = rho.mean(axis=0, keepdims=True)
        nnz = stored.sum(axis=0)
        d = np.where(stored, rho - z, 0.0)
        big_n = n_u + 24
        err_mean = (big_n * U53 * np.abs(z).sum(axis=0) + nnz * np.abs(d).max(axis=0, initial=0.0) * 2.0 ** -62
                    + 2 * U53 * np.abs(d.sum(axis=0)) + e_res.sum(axis=0)) / n + 2 * U53 * np.abs(m[0])
        e = np.where(stored, (rho - m) ** 2 - (z - m) ** 2, 0.0)
        carried = e_res + err_mean[None, :]
        err = (big_n * U53 * ((z - m) ** 2).sum(axis=0) + nnz * np.abs(e).max(axis=0, initial=0.0) * 2.0 ** -62
               + 2 * U53 * np.abs(e).sum(axis=0) + 8 * U53 * np.where(stored, (rho - m) ** 2 + (z - m) ** 2, 0.0).sum(axis=0)
               + (2 * np.abs(rho - m) * carried + carried ** 2).sum(axis=0)) / n
        err = err + (n + 8) * U53 * ((rho - m) ** 2).sum(axis=0) / n
    return err


# ---------------------------------------------------------------------------------------------------------------------
# Case table.  Every matrix holds small integers (the sums s, t and T are exact in float64 whatever their order).
# ---------------------------------------------------------------------------------------------------------------------
def _counts(rng, n, g, density=0.3, mean=3.0):
    x = rng.poisson(mean, (n, g)) * (rng.random((n, g)) < density)
    if n > 1 or g > 1:
        x[rng.integers(n), rng.integers(g)] += 40   # one entry far beyond the clip of small n
    x[:, 0] = np.maximum(x[:, 0], 1) if g > 0 else x[:, 0]   # no cell with total 0
    return sparse.csr_matrix(x.astype(np.float32))


def _ladder(n, g, n_u):
    """n cells with exactly n_u distinct totals: 10 (i mod n_u + 1) in gene 0 and three ones elsewhere"""
    rng = np.random.default_rng(n * 31 + n_u)
    x = np.zeros((n, g), dtype=np.float32)
    x[:, 0] = 10.0 * (np.arange(n) % n_u + 1)
    for i in range(n):
        x[i, rng.choice(np.arange(1, g), size=3, replace=False)] = 1.0
    return sparse.csr_matrix(x)


def _case_sizes(n, g):
    return lambda: dict(x=_counts(np.random.default_rng(100 * n + g), n, g))


def _case_special():
    rng = np.random.default_rng(7)
    x = _counts(rng, 65, 7).toarray()
    x[:, 1] = rng.integers(1, 9, 65)      # stored in every cell: no implicit zero
    x[:, 2] = 0
    x[17, 2] = 5                          # one entry
    x[:, 3] = 0                           # sum 0 between two live genes
    x[:, 4] = np.maximum(x[:, 4], rng.integers(0, 3, 65))
    return dict(x=sparse.csr_matrix(x.astype(np.float32)), zero_genes=(3,))


def _case_entry_split():
    """gene 0 stored in 2 * PR_CHUNK + 37 cells (three chunks, the last one short) beside 200 genes of at most 3 entries"""
    n, g = 2 * PR_CHUNK + 37, 201
    rng = np.random.default_rng(11)
    rows, cols, vals = [np.arange(n)], [np.zeros(n, dtype=np.int64)], [rng.integers(1, 30, n)]
    for j in range(1, g):
        k = int(rng.integers(0, 4))
        rows.append(rng.choice(n, size=k, replace=False)), cols.append(np.full(k, j)), vals.append(rng.integers(1, 6, k))
    x = sparse.csr_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(cols))), shape=(n, g))
    return dict(x=x)


def _case_stored_zero_negative():
    """two STORED zeros in gene 2 and a negative value in gene 4 (whose sum stays positive), clipped at 1.5"""
    dense = _counts(np.random.default_rng(13), 65, 9).toarray()
    dense[3, 2], dense[4, 2], dense[5, 4] = 0.0, 0.0, -2.0
    pattern = dense != 0
    pattern[3, 2] = pattern[4, 2] = True
    rows, cols = np.nonzero(pattern)
    indptr = np.concatenate([[0], np.cumsum(pattern.sum(axis=1))]).astype(np.int64)
    out = sparse.csr_matrix((dense[rows, cols].astype(np.float32), cols.astype(np.int32), indptr), shape=dense.shape)
    assert (out.data == 0).sum() == 2 and (out.data < 0).sum() == 1 and dense[:, 4].sum() > 0 and dense[5].sum() > 0
    return dict(x=out, clip=1.5)


def _case_zero_total():
    x = _counts(np.random.default_rng(17), 20, 6).tolil()
    x[7, :] = 0
    return dict(x=sparse.csr_matrix(x.tocsr()), nan_rows=(7,))


def _case_batches(k):
    def make():
        rng = np.random.default_rng(19 + k)
        n, g = 67, 12
        x = _counts(rng, n, g).toarray()
        codes = (np.arange(n) % k).astype(np.int32)      # interleaved rows
        if k == 3:
            codes[codes == 2] = 0
            codes[40] = 2                                # a batch of a single cell
        x[codes == 1, 5] = 0                             # gene 5 is absent from batch 1
        x[codes == 1, 0] = np.maximum(x[codes == 1, 0], 1)
        return dict(x=sparse.csr_matrix(x.astype(np.float32)), codes=codes, n_batches=k)
    return make


def _case_wide(g):
    """(b) only: rows of 0, 1 and g entries and ordinary rows, more rows than one batch of the residual kernel"""
    def make():
        rng = np.random.default_rng(g)
        n = PR_ROWS + 3
        x = (rng.poisson(2.0, (n, g)) * (rng.random((n, g)) < 0.05)).astype(np.float32)
        x[0, :] = 0                                      # no entry: total 0, a NaN row
        x[1, :] = 0
        x[1, g - 1] = 4                                  # one entry, in the last column
        x[2, :] = rng.integers(1, 5, g)                  # every column stored
        x[n - 1, :] = 0
        x[n - 1, min(PR_CS, g - 1)] = 2                  # one entry, the first column of the second slice (if there is one)
        return dict(x=sparse.csr_matrix(x), nan_rows=(0,), resid_only=True)
    return make


CASES = {}
for _n in (1, 2, 63, 64, 65):
    for _g in (1, 63, 65):
        CASES[f"n{_n}-g{_g}"] = _case_sizes(_n, _g)
CASES["special-genes"] = _case_special
CASES["entry-split"] = _case_entry_split
CASES["u1"] = lambda: dict(x=_ladder(70, 9, 1))
CASES["u-all-distinct"] = lambda: dict(x=_ladder(70, 9, 70))
CASES[f"u{PR_BLOCK - 1}"] = lambda: dict(x=_ladder(300, 9, PR_BLOCK - 1))
CASES[f"u{PR_BLOCK + 1}"] = lambda: dict(x=_ladder(300, 9, PR_BLOCK + 1))
for _t in (100.0, np.inf, 1e-3):
    for _c in ("sqrt", np.inf, 3.0, 0.0):
        CASES[f"theta{_t:g}-clip{_c if isinstance(_c, str) else format(_c, 'g')}"] = (
            lambda _t=_t, _c=_c: dict(x=_counts(np.random.default_rng(23), 65, 63), theta=_t, clip=_c))
CASES["stored-zero-negative"] = _case_stored_zero_negative
CASES["zero-total-cell"] = _case_zero_total
CASES["batch2"] = _case_batches(2)
CASES["batch3"] = _case_batches(3)
for _g in (PR_CS - 1, PR_CS, PR_CS + 1, 2 * PR_CS + 1):
    CASES[f"wide-g{_g}"] = _case_wide(_g)
CASE_NAMES = tuple(CASES)
DETERMINISM_CASES = ("entry-split", "batch3", "n65-g63")


@lru_cache(maxsize=None)
def case(name: str) -> dict:
    cs = dict(theta=100.0, clip="sqrt", codes=None, n_batches=1, nan_rows=(), zero_genes=(), resid_only=False)
    cs.update(CASES[name]())
    x = cs["x"]
    assert x.has_canonical_format
    for a in (x.data, x.indices, x.indptr):
        a.setflags(write=False)
    return cs


def assert_table_covers_the_issue():
    ns = {case(k)["x"].shape[0] for k in CASE_NAMES}
    gs = {case(k)["x"].shape[1] for k in CASE_NAMES}
    assert ns >= {1, 2, 63, 64, 65} and gs >= {1, 63, 65, 1023, 1024, 1025, 2049}
    split = case("entry-split")["x"].tocsc()
    per_gene = np.diff(split.indptr)
    assert per_gene[0] > 2 * PR_CHUNK and per_gene[0] % PR_CHUNK and (per_gene[1:] <= 3).all() and len(per_gene) == 201
    for name, want in (("u1", 1), ("u-all-distinct", 70), (f"u{PR_BLOCK - 1}", PR_BLOCK - 1), (f"u{PR_BLOCK + 1}", PR_BLOCK + 1)):
        assert len(np.unique(np.asarray(case(name)["x"].sum(axis=1)).ravel())) == want, name
    sp = case("special-genes")["x"].tocsc()
    assert np.diff(sp.indptr)[1] == 65 and np.diff(sp.indptr)[2] == 1 and np.diff(sp.indptr)[3] == 0
    b3 = case("batch3")
    assert np.bincount(b3["codes"]).min() == 1 and b3["x"].toarray()[b3["codes"] == 1, 5].sum() == 0
    for g in (1023, 1024, 1025, 2049):
        ln = np.diff(case(f"wide-g{g}")["x"].indptr)
        assert ln[0] == 0 and ln[1] == 1 and ln[2] == g and len(ln) > PR_ROWS


# ---------------------------------------------------------------------------------------------------------------------
# Callers of the entry points through the raw C ABI: numpy in, numpy out, outputs prefilled with NaN, the residual matrix
# between guard words.  `mem`: tests/emu/harness.py:HostMem or graph_kernel_cases.DeviceMem.
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 32   # elements before and after the residual matrix (a multiple of 16 bytes: the alignment of the matrix is kept)


class PearsonAbi:
    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def gene_var(self, x, gene_sum, cell_total, total, inv_theta, clip, tot_u, mult_u, n_batch, *, codes=None, batch=0, n_rows=None,
                 g=None, nnz=None, n_u=None, null=(), ws_short=0):
        """x: scipy CSR [n, g] (its CSC copy is handed over) -> (rc, var float64 [g] prefilled with NaN)"""
        m, z = self.mem, C.c_void_p(0)
        t = sparse.csc_matrix(x)
        bufs = {"t_indptr": m.put(t.indptr, np.int64), "t_rows": m.put(t.indices, np.int32), "t_data": m.put(t.data, np.float32),
                "gene_sum": m.put(gene_sum, np.float64), "cell_total": m.put(cell_total, np.float64),
                "tot_u": m.put(tot_u, np.float64), "mult_u": m.put(mult_u, np.float64),
                "var": m.full(max(x.shape[1], 1), np.float64, np.nan)}
        d_codes = None if codes is None else m.put(codes, np.int32)
        gx = x.shape[1] if g is None else g
        nz = x.nnz if nnz is None else nnz
        nbytes = int(self.lib.scamd_pp_pearson_workspace_bytes(x.shape[1], x.nnz))   # (of the true sizes, whatever is passed)
        ws = m.full(max(nbytes - ws_short, 1), np.uint8, 0xAB)

        def p(name):
            return z if name in null else m.ptr(bufs[name])

        rc = self.lib.scamd_pp_pearson_gene_var_f32(p("t_indptr"), p("t_rows"), p("t_data"), x.shape[0] if n_rows is None else n_rows, gx,
                                                    nz, p("gene_sum"), p("cell_total"), float(total), float(inv_theta), float(clip),
                                                    p("tot_u"), p("mult_u"), len(tot_u) if n_u is None else n_u, int(n_batch),
                                                    z if d_codes is None else m.ptr(d_codes), int(batch), p("var"),
                                                    z if "workspace" in null else m.ptr(ws), max(nbytes - ws_short, 0), m.stream)
        m.sync()
        return rc, m.get(bufs["var"])[:x.shape[1]]

    def residuals(self, x, gene_sum, cell_total, total, inv_theta, clip, *, out_f64=True, n=None, g=None, nnz=None, null=()):
        """-> (rc, out [n, g] prefilled with NaN, the guard words before and after it: True when untouched)"""
        m, z = self.mem, C.c_void_p(0)
        nr, gx = x.shape
        dt = np.float64 if out_f64 else np.float32
        bufs = {"indptr": m.put(x.indptr, np.int64), "indices": m.put(x.indices, np.int32), "data": m.put(x.data, np.float32),
                "gene_sum": m.put(gene_sum, np.float64), "cell_total": m.put(cell_total, np.float64)}
        flat = np.full(nr * gx + 2 * GUARD, np.nan, dtype=dt)
        flat[:GUARD], flat[GUARD + nr * gx:] = -77.0, -77.0
        out = m.put(flat, dt)

        def p(name):
            return z if name in null else m.ptr(bufs[name])

        po = C.c_void_p(m.ptr(out).value + GUARD * np.dtype(dt).itemsize)
        rc = self.lib.scamd_pp_pearson_residuals_f32(p("indptr"), p("indices"), p("data"), nr if n is None else n, gx if g is None else g,
                                                     x.nnz if nnz is None else nnz, p("gene_sum"), p("cell_total"), float(total),
                                                     float(inv_theta), float(clip), z if "out" in null else po, int(out_f64), m.stream)
        m.sync()
        got = m.get(out)
        guards_ok = bool((got[:GUARD] == -77.0).all() and (got[GUARD + nr * gx:] == -77.0).all())
        return rc, got[GUARD:GUARD + nr * gx].reshape(nr, gx), guards_ok


# ---------------------------------------------------------------------------------------------------------------------
# The checker: one case through both entry points.  `worst` collects the largest observed error / bound ratios.
# ---------------------------------------------------------------------------------------------------------------------
worst = {"var": 0.0, "resid64": 0.0}


def _sums(dense):
    return dense.sum(axis=0), dense.sum(axis=1)


def _clip_of(cs, n):
    return float(np.sqrt(n)) if cs["clip"] == "sqrt" else float(cs["clip"])


def run_gene_var(abi: PearsonAbi, cs: dict, x, *, collapse: bool, what=""):
    """-> var [n_batches, g]: every batch through the entry point, checked against the restatement within `var_bound`"""
    dense = x.toarray().astype(np.float64)
    stored = np.zeros(dense.shape, dtype=bool)
    stored[np.repeat(np.arange(x.shape[0]), np.diff(x.indptr)), x.indices] = True
    n, g = dense.shape
    codes = cs["codes"]
    clip = _clip_of(cs, n if codes is None else int((codes == 0).sum()))   # (the first batch's sqrt(n) for every batch)
    t_all = dense.sum(axis=1)
    out = []
    for b in range(cs["n_batches"]):
        rows = np.ones(n, bool) if codes is None else codes == b
        sub = dense[rows]
        s = sub.sum(axis=0)
        own = t_all[rows]
        if collapse:
            tot_u, mult_u = np.unique(own, return_counts=True)
        else:
            tot_u, mult_u = own, np.ones(len(own))
        rc, var = abi.gene_var(x, s, t_all, s.sum(), 1.0 / cs["theta"], clip, tot_u, mult_u.astype(np.float64), len(own), codes=codes,
                               batch=b)
        assert rc == 0, (what, b, rc)
        want = restate_gene_var(dense, cs["theta"], clip, codes, b)
        assert np.array_equal(np.isnan(var), np.isnan(want)), (what, b, "NaN pattern", var, want)
        assert np.all(var[s == 0] == 0), (what, b, "a gene with sum 0")
        live = (s != 0) & ~np.isnan(want)
        if live.any():
            tol = var_bound(sub[:, live], stored[rows][:, live], cs["theta"], clip, len(tot_u))
            err = np.abs(var[live] - want[live])
            assert np.all(err <= tol), (what, b, "beyond the bound by", float((err - tol).max()), int(np.argmax(err - tol)))
            ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)
            worst["var"] = max(worst["var"], float(ratio.max()))
        out.append(var)
    return np.array(out)


def run_residuals(abi: PearsonAbi, cs: dict, x, *, out_f64: bool, what=""):
    dense = x.toarray().astype(np.float64)
    n, g = dense.shape
    clip = _clip_of(cs, n)
    s, t = _sums(dense)
    rc, out, guards_ok = abi.residuals(x, s, t, s.sum(), 1.0 / cs["theta"], clip, out_f64=out_f64)
    assert rc == 0 and guards_ok, (what, rc, "guard words" if not guards_ok else "")
    want = restate_residuals(dense, cs["theta"], clip)
    nan_rows = np.zeros(n, bool)
    nan_rows[list(cs["nan_rows"])] = True
    live_cols = s != 0   # (a gene with sum 0: mu = 0 and 0 / 0 in every cell, in the restatement and in the kernel alike)
    assert np.array_equal(np.isnan(out), np.isnan(want)), (what, "NaN pattern / a cell that was not written")
    assert np.isnan(out[nan_rows]).all() and not np.isnan(out[~nan_rows][:, live_cols]).any(), what
    ok = ~np.isnan(want)
    err = np.abs(out.astype(np.float64) - want)
    if out_f64:
        tol = residual_tolerance(dense, cs["theta"])
        assert np.all(err[ok] <= tol[ok]), (what, float((err[ok] - tol[ok]).max()))
        with np.errstate(all="ignore"):
            ratio = np.where(tol[ok] > 0, err[ok] / tol[ok], 0.0)
        worst["resid64"] = max(worst["resid64"], float(ratio.max(initial=0.0)))
    else:
        tol = np.spacing(np.abs(want[ok]).astype(np.float32)).astype(np.float64)
        assert np.all(err[ok] <= tol), (what, float((err[ok] - tol).max()))
    if cs["clip"] == 0.0:
        assert np.all(out[ok] == 0), (what, "clip 0")
    return out


def run_case(abi: PearsonAbi, name: str, label=""):
    cs = case(name)
    x = cs["x"]
    what = f"{label} {name}"
    n = x.shape[0]
    res = {}
    if not cs["resid_only"]:
        res["var"] = run_gene_var(abi, cs, x, collapse=True, what=what)
        if n <= 300:
            run_gene_var(abi, cs, x, collapse=False, what=what + " plain")
        if cs["clip"] == 0.0:
            assert np.all(res["var"] == 0), (what, "clip 0")
        if cs["nan_rows"]:
            live = np.asarray(x.sum(axis=0)).ravel() != 0
            assert np.isnan(res["var"][0][live]).all(), (what, "a cell with total 0")
        if name in DETERMINISM_CASES:
            again = run_gene_var(abi, cs, x, collapse=True, what=what + " second run")
            assert again.tobytes() == res["var"].tobytes(), (what, "two runs differ")
            perm = np.random.default_rng(5).permutation(n)
            cs_p = dict(cs, codes=None if cs["codes"] is None else cs["codes"][perm])
            xp = sparse.csr_matrix(x[perm])
            xp.sort_indices()
            moved = run_gene_var(abi, cs_p, xp, collapse=True, what=what + " permuted rows")
            assert moved.tobytes() == res["var"].tobytes(), (what, "a permutation of the rows changes the bits")
    for f64 in ((True, False) if (cs["resid_only"] or n <= 65) else (n % 2 == 0,)):
        res[f64] = run_residuals(abi, cs, x, out_f64=f64, what=f"{what} f64={f64}")
    if name in DETERMINISM_CASES or cs["resid_only"]:
        f64 = True if True in res else False
        again = run_residuals(abi, cs, x, out_f64=f64, what=what + " second run")
        assert again.tobytes() == res[f64].tobytes(), (what, "two runs of the residual matrix differ")
    return cs, res


def run_argument_checks(abi: PearsonAbi, launches=None):
    """the documented codes; a rejected call starts no kernel and writes nothing"""
    x = _counts(np.random.default_rng(3), 20, 16)
    dense = x.toarray().astype(np.float64)
    s, t = _sums(dense)
    tot_u, mult_u = np.unique(t, return_counts=True)
    mult_u = mult_u.astype(np.float64)
    before = launches() if launches else 0
    base = (x, s, t, s.sum(), 0.01, 4.0, tot_u, mult_u, 20)
    for kw, code in ((dict(null=("t_indptr",)), EINVAL), (dict(null=("t_rows",)), EINVAL), (dict(null=("t_data",)), EINVAL),
                     (dict(null=("gene_sum",)), EINVAL), (dict(null=("cell_total",)), EINVAL), (dict(null=("tot_u",)), EINVAL),
                     (dict(null=("mult_u",)), EINVAL), (dict(null=("var",)), EINVAL), (dict(null=("workspace",)), EWORKSPACE),
                     (dict(ws_short=256), EWORKSPACE), (dict(n_rows=-1), EINVAL), (dict(g=-1), EINVAL), (dict(nnz=-1), EINVAL),
                     (dict(n_u=-1), EINVAL), (dict(n_u=21), EINVAL), (dict(g=1 << 31), EINVAL), (dict(n_rows=1 << 31), EINVAL)):
        rc, var = abi.gene_var(*base, **kw)
        assert rc == code, (kw, rc)
        assert np.isnan(var).all(), kw
    rc, var = abi.gene_var(x, s, t, s.sum(), 0.01, 4.0, tot_u, mult_u, 25)   # more cells in the batch than rows
    assert rc == EINVAL and np.isnan(var).all()
    for theta_inv, clip in ((-1.0, 4.0), (0.01, -1.0)):
        rc, var = abi.gene_var(x, s, t, s.sum(), theta_inv, clip, tot_u, mult_u, 20)
        assert rc == EINVAL and np.isnan(var).all()
        rc, out, ok = abi.residuals(x, s, t, s.sum(), theta_inv, clip)
        assert rc == EINVAL and ok and np.isnan(out).all()
    for kw in (dict(null=("indptr",)), dict(null=("indices",)), dict(null=("data",)), dict(null=("gene_sum",)),
               dict(null=("cell_total",)), dict(null=("out",)), dict(n=-1), dict(g=-1), dict(nnz=-1), dict(g=1 << 31)):
        rc, out, ok = abi.residuals(x, s, t, s.sum(), 0.01, 4.0, **kw)
        assert rc == EINVAL and ok and np.isnan(out).all(), (kw, rc)
    if launches:
        assert launches() == before, "an argument check let a kernel start"
    rc, out, ok = abi.residuals(x, s, t, s.sum(), 0.01, 4.0, n=0)   # nothing to write
    assert rc == 0 and ok and np.isnan(out).all()
    rc, var = abi.gene_var(x, s, t, s.sum(), 0.01, 4.0, tot_u, mult_u, 20, g=0)
    assert rc == 0 and np.isnan(var).all()


# ---------------------------------------------------------------------------------------------------------------------
# CPU stand-in for the three backend calls of `experimental.pp` (the front-end tests): the restatement itself.
# ---------------------------------------------------------------------------------------------------------------------
class CpuStubPearsonBackend(CpuStubPPBackend):
    @staticmethod
    def _dense(m):
        d = np.zeros(m.shape, dtype=np.float64)
        d[m.rows, m.indices] = m.data
        return d

    def row_totals64(self, m):
        return self._dense(m).sum(axis=1)

    def pearson_gene_var(self, m, gene_sum, cell_total, total, *, inv_theta, clip, batch_codes=None, batch_id=0, n_batch=None):
        d = self._dense(m)
        rows = np.ones(len(d), bool) if batch_codes is None else np.asarray(batch_codes) == batch_id
        assert n_batch is None or n_batch == rows.sum()
        assert np.allclose(gene_sum, d[rows].sum(axis=0), rtol=1e-12, atol=0) and total == gene_sum.sum()
        with np.errstate(all="ignore"):
            return restate_gene_var(d[rows], 1.0 / inv_theta if inv_theta else np.inf, clip)

    def pearson_residuals(self, m, gene_sum, cell_total, total, *, inv_theta, clip, out_f64=True):
        r = restate_residuals(self._dense(m), 1.0 / inv_theta if inv_theta else np.inf, clip)
        return r.astype(np.float64 if out_f64 else np.float32)
