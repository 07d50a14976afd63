"""Record ``tests/golden/cheb_precond.npz``: the residual norms and final iterates of the unmodified reference's CG, MINRES and
GMRES with the Chebyshev polynomial preconditioner given as a host callable, with the inputs (data only).  Needs the reference
tree (``oracle.refshim``); run from the repository root:

    python tools/gen_cheb_golden.py

One case: the five-point Laplacian on a 24 x 17 grid, ``M = LinearOperator(dot=oracle)`` with the oracle of
tests/support/cheb_ref.py at ``lmax = 8.8``, ``ratio = 30``, ``degree = 4``, a seeded random right-hand side, ``tol = 1e-9``.
Stored: A (CSR arrays), b, lmax, ratio, degree, the coefficients, and per solver the reference's resnorms and final iterate."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.support import cheb_cases as cc                               # noqa: E402
from tests.support.cheb_ref import cheb_apply_ref, cheb_coefficients     # noqa: E402

NX, NY = 24, 17
LMAX, RATIO, DEGREE = 8.8, 30.0, 4


def make_case():
    A = cc.lap2d(NX, NY)
    b = np.random.default_rng(2417).standard_normal((NX * NY, 1))
    return A, b


def main():
    from oracle import refshim
    krypy = refshim.load()
    A, b = make_case()
    n = A.shape[0]
    coef = cheb_coefficients(LMAX / RATIO, LMAX, DEGREE)
    M = krypy.utils.LinearOperator((n, n), float, dot=lambda X: cheb_apply_ref(A, X, coef))
    out = {"A_data": A.data, "A_indices": A.indices.astype(np.int32), "A_indptr": A.indptr.astype(np.int32), "b": b,
           "n": np.int64(n), "lmax": np.float64(LMAX), "ratio": np.float64(RATIO), "degree": np.int64(DEGREE), "coef": coef}
    for name in ("Cg", "Minres", "Gmres"):
        ls = krypy.linsys.LinearSystem(A, b, M=M, self_adjoint=True, positive_definite=True)
        sol = getattr(krypy.linsys, name)(ls, tol=1e-9)
        res = np.array(sol.resnorms)
        print("%-6s %d iterations, last resnorm %.2e" % (name, len(res) - 1, res[-1]))
        out["resnorms_" + name.lower()] = res
        out["xk_" + name.lower()] = np.array(sol.xk)
    path = os.path.join(ROOT, "tests", "golden", "cheb_precond.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
