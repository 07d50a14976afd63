"""The NumPy test double with the GMRES polynomial preconditioner added - TEST INFRASTRUCTURE ONLY (tests/test_poly_host.py).
``poly_update`` / ``poly_apply`` follow ``Context.poly_update`` / ``Context.poly_apply`` of ``krypy_amd/_hip.py`` with the
oracle's array expressions (tests/support/poly_ref.py) in place of the kernels."""
import numpy as np

from krypy_amd._hip import BackendError
from tests.support.idrs_numpy_context import IdrsNumpyContext
from tests.support.numpy_context import _same
from tests.support.poly_ref import poly_apply_ref


def _same_col(A, acol, B, bcol):
    return A is not None and A is B and acol == bcol


def check_table(steps):
    """What kh_poly_apply refuses in a table, with its messages."""
    n = steps.shape[0]
    if n < 1:
        raise BackendError("kh_poly_apply: 0 steps, at least 1 expected")
    for k in range(n):
        kd, close = steps[k, 0], steps[k, 3] != 0.0
        if kd not in (0.0, 1.0, 2.0, 3.0):
            raise BackendError("kh_poly_apply: step %d has kind %g, 0 (LIN), 1 (QA), 2 (QB) or 3 (SCALE) expected" % (k, kd))
        if kd == 1.0 and close:
            raise BackendError("kh_poly_apply: step %d closes on a QA step (a real root closes behind LIN or QB)" % k)
        if kd == 3.0 and (n != 1 or close):
            raise BackendError("kh_poly_apply: step %d is a SCALE step that does not stand alone" % k)
        if kd == 2.0 and (k == 0 or steps[k - 1, 0] != 1.0):
            raise BackendError("kh_poly_apply: step %d is a QB step not preceded by QA" % k)


class PolyNumpyContext(IdrsNumpyContext):
    """(on the double that has BiCGStab and IDR(s): the solvers this preconditioner serves)"""

    def poly_update(self, In, incol, P, pcol, Y, ycol, SO, socol, kind, c, a2=0.0, cl=0.0, first=False, close=False):
        self._count("poly_update")
        if _same("poly_update", *[B for B in (In, Y, SO, P) if B is not None]):
            raise BackendError("poly_update: real operator on %s blocks" % (In.dtype,))
        kind, c, a2, cl = int(kind), float(c), float(a2), float(cl)
        if kind not in (0, 1, 2, 3):
            raise BackendError("kh_poly_update: kind %d, 0 (LIN), 1 (QA), 2 (QB) or 3 (SCALE) expected" % kind)
        if (kind in (1, 3) and close) or (kind == 2 and first):
            raise BackendError("kh_poly_update: close on a QA step" if kind == 1 else
                               "kh_poly_update: close on a SCALE step" if kind == 3 else
                               "kh_poly_update: a QB step cannot be the first")
        cols = [(In, incol), (Y, ycol)] + ([(SO, socol)] if kind != 3 else []) + ([(P, pcol)] if kind == 2 else [])
        for B, _ in cols:
            if B is None:
                raise BackendError("kh_poly_update: NULL block")
            if B.n != In.n:
                raise BackendError("kh_poly_update: block of length %d, expected %d" % (B.n, In.n))
        for i in range(len(cols)):
            for j in range(i):
                if _same_col(cols[i][0], cols[i][1], cols[j][0], cols[j][1]):
                    raise BackendError("kh_poly_update: in, prod, y and s/out must be different columns")
        vin = In.a[:, incol]
        if kind == 3:
            Y.a[:, ycol] = c * vin
            return
        s = SO.a[:, socol].copy()
        if kind == 0:
            u = c * vin
            y = u if first else Y.a[:, ycol] + u
            out = vin - (c * s)
        elif kind == 1:
            out = (a2 * vin) - s
            u = c * out
            y = u if first else Y.a[:, ycol] + u
        else:
            out = P.a[:, pcol] - (c * s)
            y = None
        if close:
            y = (Y.a[:, ycol] if y is None else y) + (cl * out)
        if y is not None:
            Y.a[:, ycol] = y
        SO.a[:, socol] = out

    def poly_apply(self, A, steps, X, xcol, Y, ycol, ncols, S):
        self._count("poly_apply")
        if _same("poly_apply", X, Y, S) or A.dtype.kind == "c":
            raise BackendError("poly_apply: %s operator on %s blocks (real operators on real blocks only)" % (A.dtype, X.dtype))
        steps = np.asarray(steps, dtype=np.float64)
        if steps.ndim != 2 or steps.shape[1] != 5:
            raise BackendError("poly_apply: an (nsteps, 5) table of steps expected, got shape %s" % (steps.shape,))
        if A.kind == "diag":
            raise BackendError("kh_poly_apply: A is a diagonal operator")
        if A.shape[0] != A.shape[1] or X.n != A.shape[0] or Y.n != X.n or S.n != X.n:
            raise BackendError("kh_poly_apply: block of length %d, expected %d" % (X.n, A.shape[0]))
        if S.ncols < 3:
            raise BackendError("kh_poly_apply: the scratch block has %d columns, 3 needed" % S.ncols)
        if X is Y and xcol < ycol + ncols and ycol < xcol + ncols:
            raise BackendError("kh_poly_apply: x and y overlap (x is read after y is first written)")
        if S is X or S is Y:
            raise BackendError("kh_poly_apply: the scratch block overlaps x or y")
        check_table(steps)
        S.a[:] = np.nan                          # the scratch holds anything afterwards
        Y.a[:, ycol: ycol + ncols] = poly_apply_ref(A.mat, X.a[:, xcol: xcol + ncols].copy(), steps)
