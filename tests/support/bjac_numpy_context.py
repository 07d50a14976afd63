"""The NumPy test double with the block-Jacobi preconditioner added - TEST INFRASTRUCTURE ONLY (tests/test_bjac_host.py).
``bjac_create`` / ``bjac_update`` / ``bjac_apply`` / ``bjac_values`` follow the methods of ``Context`` in ``krypy_amd/_hip.py``
with the oracle (tests/support/bjac_ref.py) in place of the kernels; the checks and their messages restate
krypy_amd/csrc/bjac.h."""
import numpy as np
import scipy.sparse as sp

from krypy_amd._hip import BackendError
from tests.support.bjac_ref import apply_ref, bjac_ref, group_width
from tests.support.numpy_context import NumpyContext, _bdt, _same


class NumpyBjac(object):
    def __init__(self, ctx, A, blkptr):
        self.ctx, self.shape, self.nnz, self.dtype = ctx, A.shape, A.nnz, _bdt(A.dtype)
        self.blkptr, self.handle = blkptr, self
        self.indptr, self.indices = A.indptr.copy(), A.indices.copy()
        self.build(A.data)

    def build(self, data):
        A = sp.csr_matrix((np.asarray(data, dtype=self.dtype), self.indices, self.indptr), shape=self.shape)
        self.values, self.blocks, self.bad = bjac_ref(A, self.blkptr)

    def info(self):
        mmax = int(np.diff(self.blkptr).max())
        W = group_width(mmax)
        nblk = self.blkptr.size - 1
        tiles = -(-nblk // (64 // W))
        return dict(n=self.shape[0], nnz=self.nnz, nblk=nblk, max_block=mmax, group_width=W, workgroups=-(-tiles // 4),
                    device_bytes=0, first_broken_block=self.bad)


class BjacNumpyContext(NumpyContext):
    def bjac_create(self, A, blkptr):
        A = sp.csr_matrix(A)
        n = A.shape[0]
        if A.shape[0] != A.shape[1]:
            raise BackendError("bjac_create: a square matrix expected, got %s" % (A.shape,))
        blk = np.asarray(blkptr)
        if blk.ndim != 1 or blk.size < 2 or blk.dtype.kind not in "iu":
            raise BackendError("bjac_create: blkptr must be an integer array of at least two entries")
        who = "kh_bjac_create failed (status -2): kh_bjac_create: "
        for i in range(n):
            if np.any(np.diff(A.indices[A.indptr[i]: A.indptr[i + 1]]) <= 0):
                raise BackendError(who + "unsorted or duplicate indices in row %d" % i)
        if blk[0] != 0:
            raise BackendError(who + "blkptr does not start at 0 (block 0)")
        m = np.diff(blk.astype(np.int64))
        for g in range(m.size):
            if m[g] < 1:
                raise BackendError(who + "blkptr is not strictly increasing at block %d" % g)
            if m[g] > 32:
                raise BackendError(who + "block %d has %d rows, more than 32" % (g, m[g]))
            if blk[g + 1] > n:
                raise BackendError(who + "block %d ends at %d, behind n = %d" % (g, blk[g + 1], n))
        if blk[-1] != n:
            raise BackendError(who + "blkptr ends at %d, not at n = %d (block %d)" % (blk[-1], n, m.size - 1))
        self._count("bjac_create")
        h = NumpyBjac(self, A, blk.astype(np.int32))
        return h, h.info()

    def bjac_update(self, h, data):
        data = np.asarray(data)
        if data.dtype.kind == "c" and h.dtype.kind != "c":
            raise BackendError("bjac_update: complex values for a real handle")
        if data.shape != (h.nnz,):
            raise BackendError("bjac_update: %s values for a pattern of %d entries" % (data.shape, h.nnz))
        self._count("bjac_update")
        h.build(data)
        return h.info()

    def bjac_apply(self, h, X, xcol, Y, ycol, ncols=1):
        self._count("bjac_apply")
        if (h.dtype.kind == "c") != _same("bjac_apply", X, Y):
            raise BackendError("kh_bjac_apply failed (status -2): a real handle meets complex blocks / a complex handle real ones")
        if X is Y and abs(xcol - ycol) < ncols:
            raise BackendError("kh_bjac_apply failed (status -2): columns of one block overlap")
        assert X.n == h.shape[0] and Y.n == h.shape[0]
        for c in range(ncols):
            Y.a[:, ycol + c] = apply_ref(h.blocks, h.blkptr, X.a[:, xcol + c])

    def bjac_values(self, h):
        return np.array(h.values)
