"""The case table of tests/eigensolver_cases.py on ONE build of the library: per case the path counters and the sha256 of every
output array and of the info words, one line each -- two builds computed the same iff their outputs of this script are equal.
  python tools/eigensolver_ab.py --emu [libscanpy_amd_emu.so]    the host emulator (default: this tree's build)
  python tools/eigensolver_ab.py --gpu [libscanpy_amd.so]        the product library on the device (default: this tree's)
tools/eigensolver_ab.sh runs it on two builds, each in a fresh process, and compares."""
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "emu")]
import eigensolver_cases as E  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def main():
    mode, path = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else None)
    launches = lambda: -1  # noqa: E731
    if mode == "--emu":
        import harness as H

        lib = H.load(path=path)
        launches = lib.emu_launches
        eigh = lambda a, k: H.eigh_topk(lib, a, k)  # noqa: E731
        pca = lambda x, k: H.pca_csr(lib, x, k)  # noqa: E731
        spectral = lambda a, dim: H.spectral_embedding(lib, a, dim)  # noqa: E731
    else:
        import ctypes as C

        import torch

        from scanpy_amd import _kernels as K
        from scanpy_amd import _lib

        if path:
            _lib.LIB_PATH = Path(path).resolve()
        dev = lambda a, t: torch.from_numpy(np.array(a, dtype=t, order="C", copy=True)).cuda()  # noqa: E731
        csr = lambda x: (dev(x.indptr, np.int64), dev(x.indices, np.int32), dev(x.data, np.float32))  # noqa: E731
        words = lambda d, keys: np.array([float(np.sum(d[k])) if k != "ritz_values" else float(np.sum(d[k])) for k in keys])  # noqa: E731

        def eigh(a, k):
            lam, v, info = K.eigh_topk(dev(a, np.float64), k)
            return lam.cpu().numpy(), v.cpu().numpy(), info, words(info, sorted(info))

        def pca(x, k):
            out = K.pca_csr(*csr(x), x.shape[0], x.shape[1], k)
            got = {key: t.cpu().numpy() for key, t in zip(("scores", "components", "variance", "variance_ratio", "mean"), out)}
            got["info_dict"], got["info"] = out[5], words(out[5], sorted(out[5]))
            return got

        def spectral(a, dim):
            v, info = K.spectral_embedding(*csr(a), a.shape[0], dim)
            return v.cpu().numpy(), info, np.array([info[k] for k in sorted(info) if k != "ritz_values"] + info["ritz_values"], dtype=np.float64)

        _ = C
    for name in E.DENSE_CASES:
        a, k, _, _ = E.dense_input(name)
        n0 = launches()
        lam, v, info, raw = eigh(a, k)
        print(f"{name}: {info} launches={launches() - n0} lam={sha(lam)} v={sha(v)} info={sha(raw)}", flush=True)
    n0 = launches()
    got = pca(E.pca_input(), E.PCA_SHAPE[2])
    info = got.get("info_dict", None)
    if info is None:
        info = H.dense_info(got["info"])
    print(f"two_batches: {info} launches={launches() - n0} " + " ".join(
        f"{key}={sha(got[key])}" for key in ("scores", "components", "variance", "variance_ratio", "mean", "info")), flush=True)
    for name in E.SPECTRAL_CASES:
        a, dim = E.spectral_input(name)[:2]
        n0 = launches()
        v, info, raw = spectral(a, dim)
        print(f"{name}: {info} launches={launches() - n0} v={sha(v)} info={sha(raw)}", flush=True)


if __name__ == "__main__":
    main()
