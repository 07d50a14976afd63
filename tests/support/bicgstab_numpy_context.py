"""The NumPy test double with the BiCGStab entries added - TEST INFRASTRUCTURE ONLY (tests/test_bicgstab_host.py).
``bicgstab_dir`` / ``_half`` / ``_full`` / ``_step`` follow the signatures of ``krypy_amd/_hip.py``'s ``Context`` with the
expressions of tests/support/bicgstab_ref.py in place of the kernels and ``numpy.dot`` for the sums."""
import numpy as np

from krypy_amd._hip import BackendError
from tests.support import bicgstab_ref as ref
from tests.support.numpy_context import NumpyContext, _same


def _real(what, *blocks):
    if _same(what, *blocks):
        raise BackendError("%s: real blocks expected" % what)
    n = blocks[0].n
    if any(b.n != n for b in blocks):
        raise BackendError("kh_%s: length mismatch" % what)


def _distinct(what, written, read):
    for name, W, w in written:
        for R, r in read:
            if W is R and w == r:
                raise BackendError("kh_%s: %s (written) must be a column of its own" % (what, name))


class BicgstabNumpyContext(NumpyContext):
    def _dot(self, a, b):
        return float(self._allreduce(np.array([np.dot(a, b)]))[0])

    def bicgstab_dir(self, R, rcol, P, pcol, V, vcol, beta, omega):
        self._count("bicgstab_dir")
        _real("bicgstab_dir", R, P, V)
        _distinct("bicgstab_dir", [("p", P, pcol)], [(R, rcol), (V, vcol)])
        P.a[:, pcol] = ref.dir_ref(R.a[:, rcol], P.a[:, pcol], V.a[:, vcol], float(beta), float(omega))

    def bicgstab_half(self, RT, rtcol, R, rcol, V, vcol, S, scol, rho):
        self._count("bicgstab_half")
        _real("bicgstab_half", RT, R, V, S)
        _distinct("bicgstab_half", [("s", S, scol)], [(RT, rtcol), (R, rcol), (V, vcol)])
        sigma = self._dot(RT.a[:, rtcol], V.a[:, vcol])
        self._alpha, s = ref.half_ref(R.a[:, rcol], V.a[:, vcol], float(rho), sigma)
        S.a[:, scol] = s
        return sigma, self._dot(s, s), ref.flags_of(rho, sigma, 0.0, 1.0, 1.0)

    def bicgstab_full(self, RT, rtcol, R, rcol, P, pcol, S, scol, T, tcol, YK, ycol, theta_known=False):
        self._count("bicgstab_full")
        _real("bicgstab_full", RT, R, P, S, T, YK)
        read = [(RT, rtcol), (P, pcol), (S, scol), (T, tcol)]
        _distinct("bicgstab_full", [("r", R, rcol)], read + [(YK, ycol)])
        _distinct("bicgstab_full", [("yk", YK, ycol)], read)
        s, t = S.a[:, scol], T.a[:, tcol]
        theta = self._theta = self._theta if theta_known else self._dot(t, s)      # (the scratch scalar of the context)
        phi = self._dot(t, t)
        _, y, r = ref.full_ref(P.a[:, pcol], s, t, YK.a[:, ycol], self._alpha, theta, phi)
        YK.a[:, ycol] = y
        R.a[:, rcol] = r
        rho_new = self._dot(RT.a[:, rtcol], r)
        return theta, phi, rho_new, self._dot(r, r), ref.flags_of(1.0, 1.0, theta, phi, rho_new)

    def bicgstab_step(self, A, RT, rtcol, R, rcol, P, pcol, V, vcol, S, scol, T, tcol, YK, ycol, first, beta, omega_prev,
                      rho):
        self._count("bicgstab_step")
        blocks = [(RT, rtcol), (R, rcol), (P, pcol), (V, vcol), (S, scol), (T, tcol), (YK, ycol)]
        _real("bicgstab_step", *[b for b, _ in blocks])
        if A.dtype.kind == "c":
            raise BackendError("kh_bicgstab_step: real operator expected")
        if A.shape != (R.n, R.n):
            raise BackendError("kh_bicgstab_step: length mismatch (operator)")
        for i, (B, c) in enumerate(blocks):
            _distinct("bicgstab_step", [("column %d" % i, B, c)], blocks[i + 1:])
        calls = dict(self.calls)
        if not first:
            self.bicgstab_dir(R, rcol, P, pcol, V, vcol, beta, omega_prev)
        V.a[:, vcol] = self._matvec(A, P.a[:, pcol])
        sigma, ss, f0 = self.bicgstab_half(RT, rtcol, R, rcol, V, vcol, S, scol, rho)
        T.a[:, tcol] = self._matvec(A, S.a[:, scol])
        theta, phi, rho_new, rr, f1 = self.bicgstab_full(RT, rtcol, R, rcol, P, pcol, S, scol, T, tcol, YK, ycol)
        self.calls = calls                     # one entry point: the pieces are not counted
        return sigma, ss, theta, phi, rho_new, rr, f0 | f1
