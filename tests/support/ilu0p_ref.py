"""Oracle of the persistent ILU(0) preconditioner - TEST INFRASTRUCTURE ONLY, shares no code with the package.

``Ilu0pRef(A, perm)`` is ``ilu0_ref`` (tests/support/ilu0_ref.py) on ``Ap = A[perm][:, perm]`` and then the sequential
substitutions of tests/support/tri_ref.py with the gather and the scatter written out:  ``x[perm] = U^{-1} L^{-1} b[perm]``.
``values`` holds the factored values at the positions of the CALLER's value array (``values[src[q]] = lu[q]`` for entry ``q``
of ``Ap``), ``bad`` the first broken row in the numbering of ``Ap`` (-1: none)."""
import numpy as np
import scipy.sparse as sp

from tests.support.ilu0_ref import ilu0_ref
from tests.support.tri_ref import tri_solve_ref


def permuted(A, perm=None):
    """``(Ap, src)``: ``A[perm][:, perm]`` as canonical CSR with stored zeros kept, and for every entry of ``Ap`` its position in
    ``A.data`` - found by sending position tags through SciPy's own indexing, not by restating the library's loop."""
    A = sp.csr_matrix(A)
    assert A.has_canonical_format
    T = sp.csr_matrix((np.arange(1.0, A.nnz + 1.0), A.indices, A.indptr), shape=A.shape)
    if perm is not None:
        T = T[perm][:, perm].tocsr()
    T.sort_indices()
    src = T.data.astype(np.int64) - 1
    return sp.csr_matrix((A.data[src], T.indices.copy(), T.indptr.copy()), shape=A.shape), src


class Ilu0pRef(object):
    def __init__(self, A, perm=None):
        n = A.shape[0]
        self.perm = np.arange(n) if perm is None else np.asarray(perm)
        self.Ap, self.src = permuted(A, perm)
        self.L, self.U, lu, self.bad = ilu0_ref(self.Ap)
        self.values = np.empty_like(lu)
        self.values[self.src] = lu
        self.values.setflags(write=False)

    def solve(self, b):
        """``x`` with ``x[perm] = U^{-1} L^{-1} b[perm]`` for one vector or the columns of an ``(n, k)`` array."""
        b = np.asarray(b)
        B = b.reshape(self.Ap.shape[0], -1)
        Z = tri_solve_ref(self.U, tri_solve_ref(self.L, B[self.perm], True, True), False)
        X = np.zeros_like(Z)
        X[self.perm] = Z
        return X.reshape(b.shape) if b.ndim == 1 else X
