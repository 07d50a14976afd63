"""The NumPy test double with the triangular solves added - TEST INFRASTRUCTURE ONLY (tests/test_tri_host.py).
``tri`` / ``tri_solve`` follow ``Context.tri`` / ``Context.tri_solve`` of ``krypy_amd/_hip.py`` with the oracle's sequential
substitution (tests/support/tri_ref.py) in place of the kernels."""
import numpy as np
import scipy.sparse as sp

from krypy_amd._hip import BackendError
from tests.support.numpy_context import NumpyContext, _bdt, _same
from tests.support.tri_ref import tri_solve_ref


class NumpyTriangular(object):
    def __init__(self, ctx, T, lower, unit_diagonal, dtype):
        self.ctx, self.T, self.lower, self.unit_diagonal = ctx, T, bool(lower), bool(unit_diagonal)
        self.dtype, self.shape, self.nnz, self.handle = dtype, T.shape, T.nnz, self


class TriNumpyContext(NumpyContext):
    def tri(self, T, lower, unit_diagonal=False, dtype=None):
        T = sp.csr_matrix(T)
        dt = _bdt(T.dtype if dtype is None else np.result_type(T.dtype, dtype))
        if not T.has_sorted_indices:
            raise BackendError("kh_tri_create: unsorted column indices")
        C = T.tocoo()
        if np.any(C.row < C.col) if lower else np.any(C.row > C.col):
            raise BackendError("kh_tri_create: entry on the wrong side of the diagonal")
        if not unit_diagonal and np.any(T.diagonal() == 0):
            raise BackendError("kh_tri_create: zero or missing diagonal entry")
        self._count("tri")
        return NumpyTriangular(self, T.astype(dt), lower, unit_diagonal, dt)

    def tri_solve(self, t, X, xcol, Y, ycol, ncols=1):
        self._count("tri_solve")
        if (t.dtype.kind == "c") != _same("tri_solve", X, Y):
            raise BackendError("tri_solve: %s operator on %s blocks" % (t.dtype, X.dtype))
        assert X.n == t.shape[0] and Y.n == t.shape[0]
        for c in range(ncols):
            Y.a[:, ycol + c] = tri_solve_ref(t.T, X.a[:, xcol + c].copy(), t.lower, t.unit_diagonal)
