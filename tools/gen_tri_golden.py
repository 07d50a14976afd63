"""Record ``tests/golden/tri_precond.npz``: the residual norms of the unmodified reference's GMRES with an incomplete-LU left
preconditioner given as a host callable, with the inputs (data only).  Needs the reference tree (``oracle.refshim``); run from
the repository root:

    python tools/gen_tri_golden.py

One case: the five-point Laplacian on a 24 x 17 grid plus a convection term (unsymmetric), ``ilu = spilu(A, drop_tol=1e-3,
fill_factor=5)`` with SuperLU's default column ordering, ``Ml = LinearOperator(ilu.solve)``, a seeded random right-hand side,
``tol = 1e-8``.  Stored: A, the factors L and U (CSR arrays), perm_r, perm_c, b, the reference's resnorms and final iterate."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX, NY = 24, 17


def make_case():
    ex, ey = np.ones(NX), np.ones(NY)
    Tx = sp.diags([-ex[:-1] * 1.3, 2 * ex, -ex[:-1] * 0.7], [-1, 0, 1])
    Ty = sp.diags([-ey[:-1], 2 * ey, -ey[:-1]], [-1, 0, 1])
    A = (sp.kron(Tx, sp.identity(NY)) + sp.kron(sp.identity(NX), Ty)).tocsc()
    b = np.random.default_rng(2417).standard_normal((NX * NY, 1))
    return A, b


def _csr(tag, M, out):
    M = sp.csr_matrix(M)
    M.sort_indices()
    out.update({tag + "_data": M.data, tag + "_indices": M.indices.astype(np.int32), tag + "_indptr": M.indptr.astype(np.int32)})


def main():
    from oracle import refshim
    krypy = refshim.load()
    A, b = make_case()
    ilu = spla.spilu(A, drop_tol=1e-3, fill_factor=5)
    n = A.shape[0]
    Ml = krypy.utils.LinearOperator((n, n), float, dot=lambda X: ilu.solve(X))
    ls = krypy.linsys.LinearSystem(A, b, Ml=Ml)
    sol = krypy.linsys.Gmres(ls, tol=1e-8, maxiter=100)
    res = np.array(sol.resnorms)
    print("n = %d, nnz(L) = %d, nnz(U) = %d, %d iterations, last resnorm %.2e, perm_r identity: %s, perm_c identity: %s" % (
        n, ilu.L.nnz, ilu.U.nnz, len(res) - 1, res[-1], np.array_equal(ilu.perm_r, np.arange(n)),
        np.array_equal(ilu.perm_c, np.arange(n))))
    out = {"perm_r": np.asarray(ilu.perm_r, dtype=np.int32), "perm_c": np.asarray(ilu.perm_c, dtype=np.int32), "b": b,
           "resnorms": res, "xk": np.array(sol.xk), "n": np.int64(n)}
    _csr("A", A, out)
    _csr("L", ilu.L, out)
    _csr("U", ilu.U, out)
    path = os.path.join(ROOT, "tests", "golden", "tri_precond.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
