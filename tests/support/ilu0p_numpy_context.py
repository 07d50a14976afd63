"""The NumPy test double with the persistent ILU(0) preconditioner added - TEST INFRASTRUCTURE ONLY (tests/test_ilu0p_host.py).
``ilu0_handle`` / ``ilu0_refactor`` / ``ilu0_solve`` follow the methods of ``Context`` in ``krypy_amd/_hip.py`` with the oracle
(tests/support/ilu0p_ref.py) in place of the kernels; the plan figures of ``info()`` come from the NumPy restatement of the level
analysis (tests/support/tri_ref.py)."""
import numpy as np
import scipy.sparse as sp

from krypy_amd._hip import BackendError
from tests.support.ilu0_numpy_context import Ilu0NumpyContext
from tests.support.ilu0p_ref import Ilu0pRef, permuted
from tests.support.numpy_context import _bdt, _same
from tests.support.tri_ref import levels_ref


def _launches(cnt, narrow):
    wide = nar = 0
    run = False
    for c in cnt:
        if c <= narrow:
            nar += 0 if run else 1
            run = True
        else:
            wide += 1
            run = False
    return wide, nar


class NumpyIlu0(object):
    def __init__(self, ctx, pattern, perm, dtype):
        self.ctx, self.pattern, self.perm, self.dtype = ctx, pattern, perm, dtype
        self.shape, self.nnz, self.handle = pattern.shape, pattern.nnz, self
        self.ref = None
        Ap, _ = permuted(pattern, perm)
        self.cnt_l = levels_ref(sp.tril(Ap, -1).tocsr(), True)[1]
        self.cnt_u = levels_ref(sp.triu(Ap, 0).tocsr(), False)[1]
        self.longest = int(np.diff(Ap.indptr).max())

    @property
    def factored(self):
        return self.ref is not None and self.ref.bad < 0

    def info(self):
        fw, fn = _launches(self.cnt_l, self.ctx.narrow_rows)
        uw, un = _launches(self.cnt_u, self.ctx.narrow_rows)
        return dict(n=self.shape[0], nnz=self.nnz, levels=len(self.cnt_l), wide_launches=fw, narrow_launches=fn,
                    levels_l=len(self.cnt_l), levels_u=len(self.cnt_u), solve_wide_launches=fw + uw, solve_narrow_launches=fn + un,
                    slots_l=0, slots_u=0, permuted=self.perm is not None, factored=self.factored, device_bytes=0)

    def values(self):
        if not self.factored:
            raise BackendError("kh_ilu0_values failed (status -2): kh_ilu0_values: the handle is not factored")
        return np.array(self.ref.values)


class Ilu0pNumpyContext(Ilu0NumpyContext):
    def ilu0_handle(self, A_pattern, perm=None, dtype=np.float64):
        P = sp.csr_matrix(A_pattern)
        n = P.shape[0]
        if P.shape[0] != P.shape[1]:
            raise BackendError("ilu0_handle: a square matrix expected, got %s" % (P.shape,))
        for i in range(n):
            cols = P.indices[P.indptr[i]: P.indptr[i + 1]]
            if np.any(np.diff(cols) <= 0):
                raise BackendError("kh_ilu0_create failed (status -2): unsorted or duplicate column indices in row %d" % i)
            if i not in cols:
                raise BackendError("kh_ilu0_create failed (status -2): row %d has no diagonal entry" % i)
        if perm is not None and not np.array_equal(np.sort(perm), np.arange(n)):
            raise BackendError("kh_ilu0_create failed (status -2): perm is not a permutation of 0 .. n-1")
        self._count("ilu0_handle")
        pattern = sp.csr_matrix((np.ones(P.nnz), P.indices.copy(), P.indptr.copy()), shape=P.shape)
        return NumpyIlu0(self, pattern, None if perm is None else np.array(perm), _bdt(dtype))

    def ilu0_refactor(self, h, data):
        data = np.asarray(data)
        if data.dtype.kind == "c" and h.dtype.kind != "c":
            raise BackendError("ilu0_refactor: complex values for a real handle")
        if data.shape != (h.nnz,):
            raise BackendError("ilu0_refactor: %s values for a pattern of %d entries" % (data.shape, h.nnz))
        self._count("ilu0_refactor")
        A = sp.csr_matrix((data.astype(h.dtype), h.pattern.indices, h.pattern.indptr), shape=h.shape)
        h.ref = Ilu0pRef(A, h.perm)
        wide, nar = _launches(h.cnt_l, self.narrow_rows)
        return dict(n=h.shape[0], nnz=h.nnz, levels=len(h.cnt_l), wide_launches=wide, narrow_launches=nar,
                    widest_level=int(h.cnt_l.max()), longest_row=h.longest, first_broken_row=h.ref.bad)

    def ilu0_solve(self, h, X, xcol, Y, ycol, ncols=1):
        self._count("ilu0_solve")
        if (h.dtype.kind == "c") != _same("ilu0_solve", X, Y):
            raise BackendError("ilu0_solve: %s preconditioner on %s blocks" % (h.dtype, X.dtype))
        if not h.factored:
            raise BackendError("kh_ilu0_solve failed (status -2): kh_ilu0_solve: the handle is not factored")
        assert X.n == h.shape[0] and Y.n == h.shape[0]
        for c in range(ncols):
            Y.a[:, ycol + c] = h.ref.solve(X.a[:, xcol + c].copy())
