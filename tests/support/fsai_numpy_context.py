"""The NumPy test double with the factorized sparse approximate inverse added - TEST INFRASTRUCTURE ONLY
(tests/test_fsai_host.py).  ``fsai`` follows ``Context.fsai`` of ``krypy_amd/_hip.py`` with the oracle's sequential loop
(tests/support/fsai_ref.py) in place of the kernel.  Of the launch figures of ``info`` only what does not depend on the measured
choice of lanes per row is restated: see ``launch_figures``."""
import numpy as np
import scipy.sparse as sp

from krypy_amd._hip import BackendError
from tests.support.fsai_ref import fsai_ref
from tests.support.numpy_context import NumpyContext


def launch_figures(n, qmax, cplx, W):
    """(workgroups, LDS bytes per workgroup) for ``W`` lanes per row: 256 threads per workgroup, fewer rows where their work space
    (P S q + q + 2 P q doubles, S = q | 1, P = 2 for complex data) would pass 64 KiB."""
    P = 2 if cplx else 1
    doubles = P * (qmax | 1) * qmax + qmax + 2 * P * qmax
    rows = 256 // W
    while rows > 1 and rows * doubles * 8 > 65536:
        rows -= 1
    return -(-n // rows), rows * doubles * 8


class FsaiNumpyContext(NumpyContext):
    WIDTH = 16          # any of 8 / 16 / 32 / 64: no test may depend on the device's choice

    def fsai(self, A, P):
        A, P = sp.csr_matrix(A), sp.csr_matrix(P)
        if A.shape[0] != A.shape[1] or P.shape != A.shape:
            raise BackendError("fsai: a square matrix and a pattern of its shape expected, got %s and %s" % (A.shape, P.shape))
        for what, X in (("A", A), ("the pattern", P)):
            for i in range(X.shape[0]):
                if np.any(np.diff(X.indices[X.indptr[i]: X.indptr[i + 1]]) <= 0):
                    raise BackendError("kh_fsai_build failed (status -2): unsorted or duplicate column indices in row %d of %s" % (i, what))
        q = np.diff(P.indptr)
        for i in range(P.shape[0]):
            if q[i] < 1:
                raise BackendError("kh_fsai_build failed (status -2): pattern row %d is empty, it has to end in the diagonal" % i)
            if P.indices[P.indptr[i + 1] - 1] != i:
                raise BackendError("kh_fsai_build failed (status -2): pattern row %d ends in column %d, a lower-triangular pattern "
                                   "with the diagonal is expected" % (i, P.indices[P.indptr[i + 1] - 1]))
            if q[i] > 32:
                raise BackendError("kh_fsai_build failed (status -2): pattern row %d has %d entries, at most 32 are supported" % (i, q[i]))
        self._count("fsai")
        U, d, bad = fsai_ref(A, P)
        qmax = int(q.max())
        wgs, lds = launch_figures(A.shape[0], qmax, U.dtype.kind == "c", self.WIDTH)
        return U.data, d, dict(n=A.shape[0], pnnz=P.nnz, qmax=qmax, group_width=self.WIDTH, workgroups=wgs, lds_bytes=lds,
                               first_broken_row=bad)
