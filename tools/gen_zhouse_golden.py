"""Record ``tests/golden/zhouse_arnoldi.npz``: H and V of the unmodified reference's complex ``Arnoldi(ortho='house')``, with
their inputs (data only).  Needs the reference tree (``oracle.refshim``); run from the repository root:

    python tools/gen_zhouse_golden.py

Two cases: a random sparse complex operator with ``n = 37`` / 12 steps and ``n = 257`` / 40 steps (density about 6 entries
per row plus a shifted diagonal), a random complex start vector.  The operator is stored as its CSR arrays, H whole, and of V
the columns ``<tag>_Vcols``: all 13 of the small case, every fifth of the large one (0, 5 ... 40 - the columns are built one
from the other, and the whole block of the large case alone would be 168 KB of incompressible data)."""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("a", 37, 12, 101), ("b", 257, 40, 102))


def make_case(n, seed):
    rng = np.random.default_rng(seed)
    nnz = 6 * n
    rows, cols = rng.integers(0, n, nnz), rng.integers(0, n, nnz)
    vals = rng.standard_normal(nnz) + 1j * rng.standard_normal(nnz)
    A = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    A = (A + sp.diags(np.full(n, 4.0 + 1.0j))).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return A, v.reshape(-1, 1)


def main():
    from oracle import refshim
    krypy = refshim.load()
    out = {}
    for tag, n, steps, seed in CASES:
        A, v = make_case(n, seed)
        ar = krypy.utils.Arnoldi(A, v, maxiter=steps, ortho="house")
        for _ in range(steps):
            ar.advance()
        V, H = ar.get()
        orth = np.linalg.norm(np.eye(steps + 1) - V.conj().T.dot(V), 2)
        print("case %s: n = %d, %d steps, ||I - V^H V||_2 = %.2e" % (tag, n, steps, orth))
        cols = np.arange(steps + 1) if n * (steps + 1) <= 1000 else np.arange(0, steps + 1, 5)
        out.update({tag + "_Vcols": cols.astype(np.int32), tag + "_data": A.data, tag + "_indices": A.indices.astype(np.int32),
                    tag + "_indptr": A.indptr.astype(np.int32), tag + "_v": v, tag + "_H": np.array(H),
                    tag + "_V": np.array(V)[:, cols], tag + "_steps": np.int64(steps)})
    path = os.path.join(ROOT, "tests", "golden", "zhouse_arnoldi.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
