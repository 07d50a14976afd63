"""The NumPy test double with the ILU(0) factorisation added - TEST INFRASTRUCTURE ONLY (tests/test_ilu0_host.py).
``ilu0`` follows ``Context.ilu0`` of ``krypy_amd/_hip.py`` with the oracle's sequential loop (tests/support/ilu0_ref.py) in place
of the kernels; the plan figures of ``info`` come from the NumPy restatement of the level analysis (tests/support/tri_ref.py)."""
import numpy as np
import scipy.sparse as sp

from krypy_amd._hip import BackendError
from tests.support.ilu0_ref import ilu0_ref
from tests.support.numpy_context import _bdt
from tests.support.tri_numpy_context import TriNumpyContext
from tests.support.tri_ref import levels_ref


class Ilu0NumpyContext(TriNumpyContext):
    narrow_rows = 1024

    def ilu0(self, A, dtype=None):
        A = sp.csr_matrix(A)
        dt = _bdt(A.dtype if dtype is None else np.result_type(A.dtype, dtype))
        if A.shape[0] != A.shape[1]:
            raise BackendError("ilu0: a square matrix expected, got %s" % (A.shape,))
        n = A.shape[0]
        for i in range(n):
            cols = A.indices[A.indptr[i]: A.indptr[i + 1]]
            if np.any(np.diff(cols) <= 0):
                raise BackendError("kh_ilu0_factor failed (status -2): unsorted or duplicate column indices in row %d" % i)
            if i not in cols:
                raise BackendError("kh_ilu0_factor failed (status -2): row %d has no diagonal entry" % i)
        self._count("ilu0")
        _, _, lu, bad = ilu0_ref(A.astype(dt))
        _, cnt = levels_ref(sp.tril(A, -1).tocsr(), True)
        wide = nar = 0
        run = False
        for c in cnt:
            if c <= self.narrow_rows:
                nar += 0 if run else 1
                run = True
            else:
                wide += 1
                run = False
        return lu, dict(n=n, nnz=A.nnz, levels=len(cnt), wide_launches=wide, narrow_launches=nar, widest_level=int(cnt.max()),
                        longest_row=int(np.diff(A.indptr).max()), first_broken_row=bad)
