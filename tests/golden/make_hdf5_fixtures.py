"""Store DeepRank2's own test files as fixtures under ``tests/golden/``.

    python tests/golden/make_hdf5_fixtures.py <DeepRank2 checkout>/tests/data

For each file of ``FILES`` under ``<data>/hdf5`` this writes
``tests/golden/hdf5/<name>.hdf5.gz``: every numeric dataset of the file, as
``deeprank2_amd.io.hdf5.read_files`` returns it (entry order, names, dtypes
and values unchanged; the string datasets ``_name`` / ``_chain_id``, which the
package never reads, are left out), written again with
``deeprank2_amd.io.hdf5.write_graphs`` (contiguous datasets, none of the
original files' free space) and gzipped, which brings each under the size
limit for a committed file.  ``tests/_util.py:golden_hdf5_dir`` unpacks them
for the tests.  The script checks that each fixture reads back equal to its
source.

The pre-trained VanillaNetwork checkpoint
(``<data>/pretrained/testing_graph_model.pth.tar``) is a pickle that holds
classes and code objects beside its data, so it is not copied.  Only its data
is stored, read with ``deeprank2_amd.io.checkpoint.load_checkpoint`` (which
runs nothing from the file): the tensors of ``model_state`` and
``optimizer_state`` in ``tests/golden/pretrained/testing_graph_model.npz``,
and every other entry (settings, means / devs, the transforms' source
strings, the optimizer's param groups; ``data_type``, ``optimizer`` and
``lossfunction`` as class names) in ``testing_graph_model.json``.
``tests/_util.py:golden_pretrained`` writes a checkpoint in the reference's
format from the two for the tests.
"""

from __future__ import annotations

import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "deeprank-gnn-2_amd"))

from deeprank2_amd.io.checkpoint import load_checkpoint  # noqa: E402
from deeprank2_amd.io.hdf5 import read_files, write_graphs  # noqa: E402

# the files whose entries the tests read (1ATN_ppi, test, test_no_target) or
# that store MCL clusters (variants)
FILES = ("1ATN_ppi", "test", "test_no_target", "variants")
LIMIT = 1 << 20


def same(a, b):
    assert list(a) == list(b)
    for e in a:
        assert list(a[e]) == list(b[e]), e
        for k in a[e]:
            x, y = np.asarray(a[e][k]), np.asarray(b[e][k])
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (e, k)


def main(data):
    out = os.path.join(HERE, "hdf5")
    os.makedirs(out, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        for name in FILES:
            src = read_files([os.path.join(data, "hdf5", f"{name}.hdf5")])[0]
            if isinstance(src, Exception):
                raise src
            plain = os.path.join(td, f"{name}.hdf5")
            write_graphs(plain, src)
            back = read_files([plain])[0]
            if isinstance(back, Exception):
                raise back
            same(src, back)
            dst = os.path.join(out, f"{name}.hdf5.gz")
            with open(plain, "rb") as f, open(dst, "wb") as g, gzip.GzipFile(filename="", mode="wb", fileobj=g, compresslevel=9, mtime=0) as z:
                shutil.copyfileobj(f, z)
            size = os.path.getsize(dst)
            print(f"{name}: {len(src)} entries, {os.path.getsize(plain)} bytes -> {size} gzipped")
            assert size < LIMIT, name
    store_checkpoint(os.path.join(data, "pretrained", "testing_graph_model.pth.tar"), os.path.join(HERE, "pretrained", "testing_graph_model"))


def store_checkpoint(src, stem):
    st = load_checkpoint(src)
    arrays = {f"model_state/{k}": v.numpy() for k, v in st.pop("model_state").items()}
    opt = st.pop("optimizer_state")
    for i, d in opt["state"].items():
        arrays.update({f"optimizer_state/{i}/{k}": v.numpy() for k, v in d.items()})
    meta = {k: v for k, v in st.items() if k not in ("means", "devs", "classes_to_index")}
    meta["means"] = {k: float(v) for k, v in st["means"].items()}
    meta["devs"] = {k: float(v) for k, v in st["devs"].items()}
    meta["classes_to_index"] = [[k, v] for k, v in st["classes_to_index"].items()]  # int keys
    meta["param_groups"] = opt["param_groups"]
    os.makedirs(os.path.dirname(stem), exist_ok=True)
    np.savez(stem + ".npz", **arrays)
    with open(stem + ".json", "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(f"checkpoint: {len(arrays)} tensors, {len(meta)} entries")


if __name__ == "__main__":
    if len(sys.argv) != 2:  # noqa: PLR2004
        sys.stderr.write(__doc__)
        sys.exit(2)
    main(sys.argv[1])
