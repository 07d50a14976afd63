"""The NumPy test double with the Chebyshev preconditioner added - TEST INFRASTRUCTURE ONLY (tests/test_cheb_host.py).
``cheb_update`` / ``cheb_apply`` follow ``Context.cheb_update`` / ``Context.cheb_apply`` of ``krypy_amd/_hip.py`` with the
oracle's array expressions (tests/support/cheb_ref.py) in place of the kernels."""
import numpy as np

from krypy_amd._hip import BackendError
from tests.support.cheb_ref import cheb_apply_ref
from tests.support.numpy_context import NumpyContext, _same


def _dinv(Dinv, what):
    if Dinv is None:
        return None
    if Dinv.kind != "diag" or Dinv.dtype.kind == "c":
        raise BackendError("%s: Dinv is not a real diagonal operator" % what)
    return Dinv.mat


def _rv(col):
    """The (re, im) view of a column of a complex block (a writable view), the column itself when real."""
    return col.view(np.float64) if col.dtype.kind == "c" else col


class ChebNumpyContext(NumpyContext):
    def cheb_update(self, AZ, azcol, R, rcol, Dinv, D, dcol, Zin, zincol, Zout, zoutcol, a, b, first=False):
        self._count("cheb_update")
        _same("cheb_update", *[B for B in (R, D, Zout, None if first else AZ, None if first else Zin) if B is not None])
        sc = _dinv(Dinv, "cheb_update")
        r = _rv(R.a[:, rcol])
        if sc is not None and sc.size != r.size:
            raise BackendError("kh_cheb_update: Dinv has length %d, the blocks %d" % (sc.size, r.size))
        if first:
            t = r.copy()
            if sc is not None:
                t = t * sc
            d = float(b) * t
            z = d
        else:
            t = r - _rv(AZ.a[:, azcol])
            if sc is not None:
                t = t * sc
            d = (float(a) * _rv(D.a[:, dcol])) + (float(b) * t)
            z = _rv(Zin.a[:, zincol]) + d
        _rv(D.a[:, dcol])[:] = d
        _rv(Zout.a[:, zoutcol])[:] = z

    def cheb_apply(self, A, Dinv, coef, X, xcol, Y, ycol, ncols, S):
        self._count("cheb_apply")
        if (A.dtype.kind == "c") != _same("cheb_apply", X, Y, S):
            raise BackendError("cheb_apply: %s operator on %s blocks" % (A.dtype, X.dtype))
        coef = np.asarray(coef, dtype=np.float64)
        if coef.ndim != 2 or coef.shape[1] != 2 or coef.shape[0] < 1:
            raise BackendError("cheb_apply: an (m, 2) array of coefficients expected, got shape %s" % (coef.shape,))
        if A.kind == "diag" or A.shape[0] != A.shape[1] or X.n != A.shape[0] or Y.n != X.n or S.n != X.n:
            raise BackendError("kh_cheb_apply: dimension mismatch")
        if S.ncols < 3:
            raise BackendError("kh_cheb_apply: the scratch block has %d columns, 3 needed" % S.ncols)
        if X is Y and xcol < ycol + ncols and ycol < xcol + ncols:
            raise BackendError("kh_cheb_apply: x and y overlap (r is read in every step)")
        if S is X or S is Y:
            raise BackendError("kh_cheb_apply: the scratch block overlaps x or y")
        sc = _dinv(Dinv, "cheb_apply")
        if sc is not None:
            if sc.size != (2 if X.dtype.kind == "c" else 1) * X.n:
                raise BackendError("kh_cheb_apply: Dinv has length %d" % sc.size)
            sc = sc[::2] if X.dtype.kind == "c" else sc
        S.a[:] = np.nan                          # the scratch holds anything afterwards
        Y.a[:, ycol: ycol + ncols] = cheb_apply_ref(A.mat, X.a[:, xcol: xcol + ncols].copy(), coef, sc)
