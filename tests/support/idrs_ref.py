"""IDR(s) with bi-orthogonalisation in NumPy, expression for expression as ``include/krylov_hip.h`` states the iteration -
TEST INFRASTRUCTURE ONLY.

Every elementwise expression is written as the kernels evaluate it (the library is built without contraction, so with the
same scalars NumPy and the device produce the same bits), and the small forward substitutions run in Python floats in the
kernels' order.  ``csolve`` / ``asolve`` / ``omega_scalars`` are the kernels' prologues, ``dir_ref`` / ``orth_ref`` /
``omega_ref`` their vector passes; ``Stepper`` strings them into positions on a scalar block with the device's layout
(``krypy_amd._hip.IDRS_LAYOUT``), and ``solve_ref`` is the whole solver with a pluggable inner product
(``bicgstab_ref.DOTS``)."""
import math

import numpy as np

from krypy_amd._hip import IDRS_LAYOUT as L
from krypy_amd._hip import IDRS_NSCAL, IDRS_RUN_MAX, IDRS_SMAX
from tests.support.bicgstab_ref import DOTS, quot  # noqa: F401  (DOTS: re-exported for the cases)

PIVOT_ZERO, OMEGA_CLAMPED, OMEGA_ZERO, NONFINITE = 1, 2, 4, 8
KAPPA = 0.7
SM = IDRS_SMAX


def new_scalars():
    sc = np.zeros(IDRS_NSCAL)
    for i in range(SM):
        sc[L["M"] + i * SM + i] = 1.0
    sc[L["OM"]] = 1.0
    return sc


def M_of(sc, i, j):
    return float(sc[L["M"] + i * SM + j])


# ---- the prologues: small scalars in the kernels' order ---------------------------------------------------------------
def csolve(sc, k, s):
    """k_idr_dir: c_i = (f_i - sum_{j=k}^{i-1} M_ij c_j) / M_ii for i = k .. s-1 (entries below k: 0) and the flags"""
    c = [0.0] * s
    for i in range(k, s):
        acc = float(sc[L["F"] + i])
        for j in range(k, i):
            acc = acc - M_of(sc, i, j) * c[j]
        c[i] = quot(acc, M_of(sc, i, i))
    mkk = M_of(sc, k, k)
    return c, (PIVOT_ZERO if (not math.isfinite(mkk) or mkk == 0.0) else 0)


def asolve(sc, k, s):
    """k_idr_orth: a (entries 0 .. k-1), the new column M[k:, k] (a list from row k on), beta, the new f[k+1:], flags"""
    h = [float(x) for x in sc[L["H"]: L["H"] + s]]
    a = [0.0] * k
    for i in range(k):
        acc = h[i]
        for j in range(i):
            acc = acc - M_of(sc, i, j) * a[j]
        a[i] = quot(acc, M_of(sc, i, i))
    col = []
    for i in range(k, s):
        m = h[i]
        for j in range(k):
            m = m - M_of(sc, i, j) * a[j]
        col.append(m)
    beta = quot(float(sc[L["F"] + k]), col[0])
    fnew = [float(sc[L["F"] + i]) - beta * col[i - k] for i in range(k + 1, s)]
    flags = 0
    if not math.isfinite(col[0]) or col[0] == 0.0:
        flags |= PIVOT_ZERO
    if not all(math.isfinite(x) for x in h):
        flags |= NONFINITE
    return a, col, beta, fnew, flags


def omega_scalars(theta, phi, rr):
    """k_idr_omega: om with the kappa correction, and the flags"""
    theta, phi, rr = float(theta), float(phi), float(rr)
    om = quot(theta, phi)
    with np.errstate(all="ignore"):
        rho = float(np.float64(theta) / (np.sqrt(np.float64(phi)) * np.sqrt(np.float64(rr))))
    if abs(rho) < KAPPA:
        om = quot(om * KAPPA, abs(rho))
    flags = 0
    if not (math.isfinite(theta) and math.isfinite(phi)):
        flags |= NONFINITE
    if phi == 0.0:
        flags |= OMEGA_CLAMPED
    if om == 0.0 and rr > 0.0:
        flags |= OMEGA_ZERO
    return om, flags


def flags_of(kind, sc_before, k=0, s=1):
    """the flags a step of ``kind`` ('dir', 'orth', 'omega') raises from the scalar block as it stands before it"""
    if kind == "dir":
        return csolve(sc_before, k, s)[1]
    if kind == "orth":
        return asolve(sc_before, k, s)[4]
    return omega_scalars(sc_before[L["THETA"]], sc_before[L["PHI"]], sc_before[L["RR"]])[1]


# ---- the vector passes --------------------------------------------------------------------------------------------------
def dir_ref(r, G, U, k, s, c, om):
    """u_k = om (r - sum_{i>=k} c_i g_i) + sum_{i>=k} c_i u_i, one term at a time (i = k reads the old u_k)"""
    v = r.copy()
    for i in range(k, s):
        v = v - c[i] * G[:, i]
    u = om * v
    for i in range(k, s):
        u = u + c[i] * U[:, i]
    return u


def orth_ref(t, G, U, r, y, k, a, beta):
    """g_k, u_k, r, y of position k from the operator product t"""
    g, u = t.copy(), U[:, k].copy()
    for i in range(k):
        g = g - a[i] * G[:, i]
        u = u - a[i] * U[:, i]
    return g, u, r - beta * g, y + beta * u


def omega_ref(r, t, y, om):
    """y, r of position s"""
    return y + om * r, r - om * t


# ---- positions on a state -------------------------------------------------------------------------------------------------
class Stepper(object):
    """P, G, U (n x s), r, y, t and the scalar block; ``dot(a, b)`` is the inner product.  The methods are the device's
    entry points: ``dir``, ``orth``, ``omega`` (each returns what the device would record) with the stop word honoured."""

    def __init__(self, P, G, U, r, y, t, sc, dot=np.dot):
        self.P, self.G, self.U, self.r, self.y, self.t, self.sc, self.dot = P, G, U, r, y, t, sc, dot
        self.s = P.shape[1]

    def init(self):
        self.sc[:] = new_scalars()
        for i in range(self.s):
            self.sc[L["F"] + i] = self.dot(self.P[:, i], self.r)
        self.sc[L["RR"]] = self.dot(self.r, self.r)
        return float(self.sc[L["RR"]])

    def stopped(self):
        return self.sc[L["STOP"]] != 0.0

    def clear_stop(self):
        self.sc[L["STOP"]] = self.sc[L["COUNT"]] = 0.0

    def _raise(self, bits):
        self.sc[L["FLAGS"]] = float(int(self.sc[L["FLAGS"]]) | bits)

    def _block_dot(self, w):
        for i in range(self.s):
            self.sc[L["H"] + i] = self.dot(self.P[:, i], w)

    def _rr(self, rr, pos, bnorm, tol):
        sc, s = self.sc, self.s
        bits = int(sc[L["FLAGS"]])
        if not math.isfinite(rr):
            bits |= NONFINITE
        if pos < s:
            x1, x2 = M_of(sc, pos, pos), float(sc[L["F"] + pos])
        else:
            x1, x2 = float(sc[L["THETA"]]), float(sc[L["PHI"]])
            for i in range(s):
                if not math.isfinite(sc[L["H"] + i]):
                    bits |= NONFINITE
                sc[L["F"] + i] = sc[L["H"] + i]
        idx = int(sc[L["COUNT"]])
        with np.errstate(all="ignore"):
            stop = bits != 0 or bool(np.sqrt(np.float64(rr)) / np.float64(bnorm) <= tol)
        rec = (float(rr), x1, x2, bits)
        if idx < IDRS_RUN_MAX:
            sc[L["REC"] + 4 * idx: L["REC"] + 4 * idx + 4] = rec
        if idx + 1 >= IDRS_RUN_MAX:
            stop = True
        sc[L["RR"]], sc[L["FLAGS"]], sc[L["COUNT"]] = rr, 0.0, idx + 1
        if stop:
            sc[L["STOP"]] = 1.0
        return rec

    def dir(self, k):
        if self.stopped():
            return
        c, flags = csolve(self.sc, k, self.s)
        self.sc[L["C"] + k: L["C"] + self.s] = c[k:]
        if flags:
            self._raise(flags)
        self.U[:, k] = dir_ref(self.r, self.G, self.U, k, self.s, c, float(self.sc[L["OM"]]))

    def orth(self, k, bnorm, tol):
        """from t = A^ u_k on"""
        self._block_dot(self.t)
        if self.stopped():
            return None
        sc, s = self.sc, self.s
        a, col, beta, fnew, flags = asolve(sc, k, s)
        if flags:
            self._raise(flags)
        sc[L["A"]: L["A"] + k] = a
        sc[L["BETA"]] = beta
        for i in range(k, s):
            sc[L["M"] + i * SM + k] = col[i - k]
        sc[L["F"] + k + 1: L["F"] + s] = fnew
        self.G[:, k], self.U[:, k], self.r[:], self.y[:] = orth_ref(self.t, self.G, self.U, self.r, self.y, k, a, beta)
        return self._rr(float(self.dot(self.r, self.r)), k, bnorm, tol)

    def omega(self, bnorm, tol):
        """from t = A^ r on"""
        sc = self.sc
        sc[L["THETA"]], sc[L["PHI"]] = self.dot(self.t, self.r), self.dot(self.t, self.t)
        if self.stopped():
            self._block_dot(self.r)
            return None
        om, flags = omega_scalars(sc[L["THETA"]], sc[L["PHI"]], sc[L["RR"]])
        if flags:
            self._raise(flags)
        sc[L["OM"]] = om
        self.y[:], self.r[:] = omega_ref(self.r, self.t, self.y, om)
        self._block_dot(self.r)
        return self._rr(float(self.dot(self.r, self.r)), self.s, bnorm, tol)

    def position(self, pos, apply, bnorm, tol):
        """one whole position with the operator ``apply`` (a stopped state is left as it is, up to t and h)"""
        if pos < self.s:
            self.dir(pos)
            self.t[:] = apply(self.U[:, pos])
            return self.orth(pos, bnorm, tol)
        self.t[:] = apply(self.r)
        return self.omega(bnorm, tol)


class Result(object):
    def __init__(self):
        self.resnorms, self.trace, self.iter, self.x, self.breakdown = [], [], 0, None, None


def solve_ref(A, b, tol, maxiter, s=4, shadow=None, seed=0, Ml=None, Mr=None, x0=None, dot=np.dot):
    """IDR(s) on ``Ml A Mr`` from ``x0``; ``resnorms[k] = sqrt(<r_k, r_k>) / ||Ml b||`` of the recurrence's residual after
    k operator applications.  Stops at the tolerance, at ``maxiter`` or at a breakdown (``breakdown``: the flags)."""
    from krypy_amd.utils import idrs_shadow
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = b.size
    ml = (lambda x: x) if Ml is None else (lambda x: Ml.dot(x))
    mr = (lambda x: x) if Mr is None else (lambda x: Mr.dot(x))

    def apply(x):
        return ml(A.dot(mr(x)))

    x0 = np.zeros(n) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(-1)
    out = Result()
    bnorm = math.sqrt(float(dot(ml(b), ml(b))))
    if bnorm == 0.0:
        out.resnorms, out.x = [0.0], np.zeros(n)
        return out
    r = ml(b - A.dot(x0)) if np.any(x0) else ml(b)
    P = np.asfortranarray(idrs_shadow(n, s, seed) if shadow is None else shadow, dtype=np.float64)
    st = Stepper(P, np.zeros((n, s), order="F"), np.zeros((n, s), order="F"), r.copy(), np.zeros(n), np.zeros(n),
                 np.zeros(IDRS_NSCAL), dot)
    st.init()
    out.resnorms.append(math.sqrt(float(dot(r, r))) / bnorm)
    pos = 0
    while out.resnorms[-1] > tol and out.iter < maxiter:
        st.clear_stop()
        rr, x1, x2, flags = st.position(pos, apply, bnorm, tol)
        out.trace.append((out.iter, pos, rr, x1, x2, flags))
        resnorm = math.sqrt(abs(rr)) / bnorm
        if flags and not resnorm <= tol:
            out.breakdown = flags
            break
        out.resnorms.append(resnorm)
        out.iter += 1
        pos = (pos + 1) % (s + 1)
    out.x = x0 + mr(st.y)
    return out
