"""What the calls of `experimental.pp` share: which host matrices travel to the device (and as what), and the two device passes of
csrc/pearson.hip behind `_csr_device.default_backend()`.

Accepted: CSR, CSC or dense; float32, integers and booleans that float32 holds exactly (|x| <= 2^24), float64 that float32 holds
exactly.  Refused: a backed matrix, dask, other float64, wider integers (`NotImplementedError`); non-finite values
(`ValueError`: the reference lets them spread into every gene)."""
from __future__ import annotations

import numpy as np
from scipy import sparse

from ...preprocessing import _csr_device


def _refuse_lazy(x, what: str) -> None:
    if getattr(x, "is_backed", False) or type(x).__module__.split(".")[0] == "h5py":
        raise NotImplementedError(f"{what}: the matrix is on disk (backed): streaming a backed matrix is not offered, load it first "
                                  "(`.to_memory()`, or read without backed='r')")
    if type(x).__module__.split(".")[0] == "dask":
        raise NotImplementedError(f"{what}: dask arrays are not offered, `.compute()` first")


def _as_float32(values: np.ndarray, what: str) -> np.ndarray:
    dt = values.dtype
    if dt.kind in "iu":
        if values.size and max(int(values.max()), -int(values.min())) > 2 ** 24:
            raise NotImplementedError(f"{what}: {dt} values beyond 2^24 in magnitude do not travel as float32 exactly")
        return values.astype(np.float32)
    if dt.kind == "b" or dt == np.float16:
        return values.astype(np.float32)
    if dt not in (np.float32, np.float64):
        raise NotImplementedError(f"{what}: values of dtype {dt}")
    if not np.isfinite(values).all():
        raise ValueError(f"{what}: the matrix holds values that are not finite (NaN or infinity)")
    if dt == np.float32:
        return values
    narrow = values.astype(np.float32)
    if not np.array_equal(narrow, values):
        raise NotImplementedError(f"{what}: float64 values that float32 does not hold exactly are not offered (the matrix travels as "
                                  "float32); cast with `.astype(np.float32)` if that is meant")
    return narrow


def host_matrix(x, what: str):
    """-> (the matrix with float32 values: scipy CSR / CSC or a 2-d ndarray, dtype of the input)"""
    _refuse_lazy(x, what)
    if sparse.issparse(x):
        if x.format not in ("csr", "csc"):
            x = x.tocsr()
        if max(x.shape) >= 2 ** 31:
            raise NotImplementedError(f"{what} is offered below 2^31 rows and columns")
        values = _as_float32(np.asarray(x.data), what)
        return type(x)((values, x.indices, x.indptr), shape=x.shape), x.dtype
    dense = np.asarray(x)
    if dense.ndim != 2:
        raise ValueError(f"{what} needs a 2-d matrix, got {dense.ndim} dimensions")
    return _as_float32(np.ascontiguousarray(dense), what), dense.dtype


def upload(x, what: str):
    """-> (backend, the resident CSR float32 matrix, dtype of the input)"""
    mat, dtype = host_matrix(x, what)
    be = _csr_device.default_backend()
    return be, be.upload(mat), dtype
