#!/usr/bin/env python3
"""Generate the committed golden fixtures under tests/golden/ from the reference tree.

Run ONCE in the build container (where /root/reference is mounted); the GPU box never
sees /root/reference, so everything the tests need is written here as small .npz files.

Sources (all under /root/reference):
  * tests/test_pca.py:34-59          -> pca_toy.npz          (A_list, A_pca, A_svd)
  * tests/test_neighbors.py:23-48    -> neighbors_toy.npz    (X, distances_euclidean,
                                                              connectivities_umap, transitions*)
  * src/scanpy/datasets/10x_pbmc68k_reduced.zarr.zip
                                      -> pbmc68k_reduced.npz (X, counts CSR, obs n_counts, stored
                                         distances / connectivities CSR, X_pca, louvain codes)
  * tests/_scripts/seurat_hvg.csv, tests/_scripts/cell_ranger_hvg.csv
                                      -> hvg_golden.npz       (the Seurat / Cell Ranger outputs that
                                         tests/test_highly_variable_genes.py:367-422 compares against)
  * tests/test_scaling.py:13-72       -> scale_toy.npz        (X_original, X_scaled_*, X_centered_*, mask cases)
  * data files the reader tests open, copied byte for byte (REFERENCE_DATA): the Cell Ranger / Visium files of
    tests/_data/10x_data and tests/_data/visium_data, the zarr-v2 store tests/_data/10x-10k-subset.zarr, and the
    zarr-v3 zip above cut into parts below the 1 MiB limit of a committed file (10x_pbmc68k_reduced.zarr.zip.part<i>)
  * the line count of every reference file that include/scanpy_amd.h, INTEGRATION.md and DESIGN.md cite
                                      -> reference_line_counts.json (tests/test_reference_citations_cpu.py)

The reference cannot be imported here (needs Python >= 3.12), so the literal arrays are
pulled out of the test modules with `ast`, and the zarr-v3 store is decoded by hand
(zip member -> `sharding_indexed` shard -> trailing (offset,nbytes) index -> zstd chunk).
"""
from __future__ import annotations

import ast
import json
import sys
import zipfile
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent


def literal_arrays(pyfile: Path, names: set[str]) -> dict[str, np.ndarray]:
    """Evaluate top-level `name = <literal or np.array(literal)>` assignments."""
    tree = ast.parse(pyfile.read_text())
    out = {}
    for node in tree.body:
        if not isinstance(node, ast.Assign) or len(node.targets) != 1:
            continue
        tgt = node.targets[0]
        if not isinstance(tgt, ast.Name) or tgt.id not in names:
            continue
        val = node.value
        if isinstance(val, ast.Call):  # np.array([...])
            val = val.args[0]
        out[tgt.id] = np.array(ast.literal_eval(val), dtype=np.float64)
    missing = names - out.keys()
    if missing:
        raise SystemExit(f"{pyfile}: did not find {sorted(missing)}")
    return out


# --------------------------------------------------------------------------------------
# minimal zarr-v3 reader: regular chunk grid of shard files, each holding a C-ordered grid of
# inner chunks; inner codecs bytes(little)+zstd; shard index at the end =
# n_inner x (offset u64, nbytes u64) + crc32c
# --------------------------------------------------------------------------------------
def _zstd_decompress(buf: bytes, nbytes: int) -> bytes:
    import pyarrow as pa

    return pa.Codec("zstd").decompress(buf, decompressed_size=nbytes).to_pybytes()


def read_zarr_array(z: zipfile.ZipFile, path: str) -> np.ndarray:
    meta = json.loads(z.read(f"{path}/zarr.json"))
    shape = tuple(meta["shape"])
    dtype = np.dtype(meta["data_type"])
    chunk = tuple(meta["chunk_grid"]["configuration"]["chunk_shape"])
    (codec,) = meta["codecs"]
    assert codec["name"] == "sharding_indexed", codec["name"]
    inner = tuple(codec["configuration"]["chunk_shape"])
    assert [c["name"] for c in codec["configuration"]["codecs"]] == ["bytes", "zstd"]
    assert codec["configuration"]["index_location"] == "end"
    out = np.full(shape, meta["fill_value"], dtype=dtype)
    grid = [-(-s // c) for s, c in zip(shape, chunk)]
    per_shard = [c // i for c, i in zip(chunk, inner)]  # inner chunks per shard, per axis
    n_inner = int(np.prod(per_shard))
    inner_bytes = int(np.prod(inner)) * dtype.itemsize
    for sidx in np.ndindex(*grid):
        key = f"{path}/c/" + "/".join(map(str, sidx))
        raw = z.read(key)
        index = np.frombuffer(raw[-(16 * n_inner + 4) : -4], dtype="<u8").reshape(n_inner, 2)
        for flat, iidx in enumerate(np.ndindex(*per_shard)):
            off, nb = index[flat]
            if off == np.iinfo(np.uint64).max:  # empty inner chunk -> fill value
                continue
            buf = _zstd_decompress(raw[int(off) : int(off + nb)], inner_bytes)
            block = np.frombuffer(buf, dtype=dtype.newbyteorder("<")).reshape(inner)
            lo = [s * c + i * ic for s, c, i, ic in zip(sidx, chunk, iidx, inner)]
            sl = tuple(slice(l, min(l + ic, s)) for l, ic, s in zip(lo, inner, shape))
            if any(s.start >= s.stop for s in sl):
                continue
            out[sl] = block[tuple(slice(0, s.stop - s.start) for s in sl)]
    return out


def read_csr(z: zipfile.ZipFile, path: str) -> dict[str, np.ndarray]:
    meta = json.loads(z.read(f"{path}/zarr.json"))
    assert meta["attributes"]["encoding-type"] == "csr_matrix"
    return dict(
        data=read_zarr_array(z, f"{path}/data"),
        indices=read_zarr_array(z, f"{path}/indices"),
        indptr=read_zarr_array(z, f"{path}/indptr"),
        shape=np.array(meta["attributes"]["shape"], dtype=np.int64),
    )


REFERENCE_DATA = [
    "10x_data/1.2.0/filtered_gene_bc_matrices/hg19_chr21/genes.tsv",
    "10x_data/1.2.0/filtered_gene_bc_matrices/hg19_chr21/barcodes.tsv",
    "10x_data/1.2.0/filtered_gene_bc_matrices/hg19_chr21/matrix.mtx",
    "10x_data/1.2.0/filtered_gene_bc_matrices_h5.h5",
    "10x_data/1.2.0/multiple_genomes.h5",
    "10x_data/3.0.0/filtered_feature_bc_matrix/matrix.mtx.gz",
    "10x_data/3.0.0/filtered_feature_bc_matrix/features.tsv.gz",
    "10x_data/3.0.0/filtered_feature_bc_matrix/barcodes.tsv.gz",
    "10x_data/3.0.0/filtered_feature_bc_matrix.h5",
    "visium_data/2.1.0/raw_probe_bc_matrix.h5",
    "10x-10k-subset.zarr",
]
ZIP_PART_BYTES = 900_000


def repack_lzma(npz: Path) -> None:
    src = zipfile.ZipFile(npz)
    members = [(i.filename, src.read(i.filename)) for i in src.infolist()]
    src.close()
    with zipfile.ZipFile(npz, "w", compression=zipfile.ZIP_LZMA) as z:
        for name, raw in members:
            z.writestr(name, raw)


def copy_reference_data() -> None:
    import shutil

    for rel in REFERENCE_DATA:
        src, dst = REF / "tests/_data" / rel, OUT / rel
        dst.parent.mkdir(parents=True, exist_ok=True)
        if src.is_dir():
            shutil.copytree(src, dst, dirs_exist_ok=True)
        else:
            shutil.copyfile(src, dst)
    raw = (REF / "src/scanpy/datasets/10x_pbmc68k_reduced.zarr.zip").read_bytes()
    for i in range(0, len(raw), ZIP_PART_BYTES):
        (OUT / f"10x_pbmc68k_reduced.zarr.zip.part{i // ZIP_PART_BYTES}").write_bytes(raw[i:i + ZIP_PART_BYTES])


def citation_line_counts() -> None:
    import re

    root = OUT.parent.parent
    cite = re.compile(r"(?<![\w/.])((?:src/scanpy|tests)/[\w/]+\.py):(\d+)(?:-(\d+))?")  # as the test's CITE
    paths = sorted({m[0] for doc in ("include/scanpy_amd.h", "INTEGRATION.md", "DESIGN.md")
                    for m in cite.findall((root / doc).read_text())})
    counts = {p: len((REF / p).read_text().splitlines()) for p in paths if (REF / p).is_file()}
    (OUT / "reference_line_counts.json").write_text(json.dumps(counts, indent=1, sort_keys=True) + "\n")


def main() -> None:
    if not REF.exists():
        raise SystemExit("/root/reference not present: fixtures can only be regenerated in the build container")

    pca = literal_arrays(REF / "tests/test_pca.py", {"A_list", "A_pca", "A_svd"})
    np.savez(OUT / "pca_toy.npz", **pca)

    nb_names = {
        "X",
        "distances_euclidean",
        "distances_euclidean_all",
        "connectivities_umap",
        "transitions_sym_umap",
        "transitions_umap",
        "connectivities_gauss_knn",
        "connectivities_jaccard",
    }
    nb = literal_arrays(REF / "tests/test_neighbors.py", nb_names)
    nb["n_neighbors"] = np.array(3)  # tests/test_neighbors.py:24 (includes the point itself)
    np.savez(OUT / "neighbors_toy.npz", **nb)

    z = zipfile.ZipFile(REF / "src/scanpy/datasets/10x_pbmc68k_reduced.zarr.zip")
    fx = {}
    fx["X"] = read_zarr_array(z, "X")
    for name, path in [("counts", "layers/counts"), ("distances", "obsp/distances"), ("connectivities", "obsp/connectivities")]:
        for k, v in read_csr(z, path).items():
            fx[f"{name}_{k}"] = v
    fx["X_pca"] = read_zarr_array(z, "obsm/X_pca")
    fx["louvain_codes"] = read_zarr_array(z, "obs/louvain/codes")
    fx["bulk_labels_codes"] = read_zarr_array(z, "obs/bulk_labels/codes")
    fx["highly_variable"] = read_zarr_array(z, "var/highly_variable")
    fx["n_neighbors"] = read_zarr_array(z, "uns/neighbors/params/n_neighbors")
    fx["obs_n_counts"] = read_zarr_array(z, "obs/n_counts")
    np.savez_compressed(OUT / "pbmc68k_reduced.npz", **fx)
    repack_lzma(OUT / "pbmc68k_reduced.npz")  # deflate leaves it above 1 MiB; np.load reads LZMA members too

    import pandas as pd

    hvg = {}
    for tag, f in (("seurat", "seurat_hvg.csv"), ("cell_ranger", "cell_ranger_hvg.csv")):
        df = pd.read_csv(REF / "tests/_scripts" / f, index_col=0)
        for col in ("means", "dispersions", "dispersions_norm"):
            hvg[f"{tag}_{col}"] = df[col].to_numpy(dtype=np.float64)
        hvg[f"{tag}_highly_variable"] = df["highly_variable"].to_numpy(dtype=bool)
    np.savez_compressed(OUT / "hvg_golden.npz", **hvg)

    sc_names = {"X_original", "X_scaled_original", "X_centered_original", "X_scaled_original_clipped", "X_for_mask",
                "X_scaled_for_mask", "X_centered_for_mask", "X_scaled_for_mask_clipped"}
    np.savez(OUT / "scale_toy.npz", **literal_arrays(REF / "tests/test_scaling.py", sc_names))

    # Seurat's vst table for pbmc3k (tests/_scripts/seurat_extract_hvg_v3.r wrote it): per gene the mean, the
    # variance and `variance.expected` = 10 ** (R's loess(log10(variance) ~ log10(mean), span = 0.3) fitted values),
    # the known answers of scanpy_amd/preprocessing/_loess.py; plus the 2000 genes Seurat's SelectIntegrationFeatures
    # picked with a batch covariate (tests/test_highly_variable_genes.py:462-491)
    import pandas as pd

    vst = pd.read_csv(REF / "tests/_scripts/seurat_hvg_v3.csv.gz", index_col=0)
    np.savez_compressed(OUT / "loess_seurat_v3.npz", mean=vst["mean"].to_numpy(), variance=vst["variance"].to_numpy(),
                        variance_expected=vst["variance.expected"].to_numpy(),
                        variance_standardized=vst["variance.standardized"].to_numpy())

    copy_reference_data()
    citation_line_counts()

    for f in ("pca_toy.npz", "neighbors_toy.npz", "pbmc68k_reduced.npz", "hvg_golden.npz", "scale_toy.npz"):
        print(f, (OUT / f).stat().st_size, "bytes")


if __name__ == "__main__":
    sys.exit(main())
