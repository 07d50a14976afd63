"""The NumPy test double with the sparse approximate inverse added - TEST INFRASTRUCTURE ONLY (tests/test_spai_host.py).
``spai`` follows ``Context.spai`` of ``krypy_amd/_hip.py`` with the oracle's sequential loop (tests/support/spai_ref.py) in place of
the kernel; the launch figures of ``info`` restate the rule of krypy_amd/csrc/spai.hip."""
import numpy as np
import scipy.sparse as sp

from krypy_amd._hip import BackendError
from tests.support.numpy_context import NumpyContext
from tests.support.spai_ref import spai_ref


def launch_figures(n, qmax, cplx):
    """(lanes per row, workgroups, LDS bytes per workgroup): 8 lanes up to 8 entries, 16 up to 16, above that 32 (real) or 64
    (complex); 256 threads per workgroup, fewer rows where their work space (P S q + q + 2 P q doubles, S = q | 1, P = 2 for
    complex data) would pass 64 KiB."""
    W = 8 if qmax <= 8 else 16 if qmax <= 16 else 64 if cplx else 32
    if qmax == 0:
        return W, 0, 0
    P = 2 if cplx else 1
    doubles = P * (qmax | 1) * qmax + qmax + 2 * P * qmax
    rows = 256 // W
    while rows > 1 and rows * doubles * 8 > 65536:
        rows -= 1
    return W, -(-n // rows), rows * doubles * 8


class SpaiNumpyContext(NumpyContext):
    def spai(self, A, P):
        A, P = sp.csr_matrix(A), sp.csr_matrix(P)
        if A.shape[0] != A.shape[1] or P.shape != A.shape:
            raise BackendError("spai: a square matrix and a pattern of its shape expected, got %s and %s" % (A.shape, P.shape))
        for what, X in (("A", A), ("the pattern", P)):
            for i in range(X.shape[0]):
                if np.any(np.diff(X.indices[X.indptr[i]: X.indptr[i + 1]]) <= 0):
                    raise BackendError("kh_spai_build failed (status -2): unsorted or duplicate column indices in row %d of %s" % (i, what))
        q = np.diff(P.indptr)
        if q.size and q.max() > 32:
            raise BackendError("kh_spai_build failed (status -2): pattern row %d has %d entries, at most 32 are supported"
                               % (int(np.flatnonzero(q > 32)[0]), int(q.max())))
        self._count("spai")
        M, bad = spai_ref(A, P)
        qmax = int(q.max()) if q.size else 0
        W, wgs, lds = launch_figures(A.shape[0], qmax, M.dtype.kind == "c")
        return M.data, dict(n=A.shape[0], pnnz=P.nnz, qmax=qmax, group_width=W, workgroups=wgs, lds_bytes=lds, first_broken_row=bad)
