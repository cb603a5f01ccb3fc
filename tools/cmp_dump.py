"""Compare two dumps of tools/pass_dump.py (two .npz files, or two directories
of them as --matrix writes) array by array: byte identity (the exit status is
1 unless every array is byte-identical), and how far apart the values are
where they differ.

    python tools/cmp_dump.py <a.npz | dir_a> <b.npz | dir_b>
"""
import numpy as np, os, sys


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    same = sorted(a.files) == sorted(b.files)
    for k in a.files:
        x, y = a[k], b[k]
        ident = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        same = same and ident
        d = np.abs(x - y)
        bad = np.argwhere(~np.isclose(x, y, rtol=1e-4, atol=1e-6 * (np.abs(x).max() + 1e-30)))
        print(k, x.shape, "bytes identical" if ident else "BYTES DIFFER", "max abs diff", float(np.nanmax(d)) if d.size else 0, "bad rows", sorted(set(bad[:, 0].tolist()))[:20] if bad.size else [])
    return same


if os.path.isdir(sys.argv[1]):
    names = sorted(os.listdir(sys.argv[1]))
    ok = names == sorted(os.listdir(sys.argv[2])) and len(names) > 0
    for n in names:
        print("==", n)
        ok = cmp(os.path.join(sys.argv[1], n), os.path.join(sys.argv[2], n)) and ok
    print("ALL BYTE-IDENTICAL" if ok else "DIFFERENCES", len(names), "dumps")
else:
    ok = cmp(sys.argv[1], sys.argv[2])
sys.exit(0 if ok else 1)
