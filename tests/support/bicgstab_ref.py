"""BiCGStab in NumPy, expression for expression as ``include/krylov_hip.h`` states the iteration - TEST INFRASTRUCTURE ONLY.

Every elementwise expression is written as the kernels evaluate it (the library is built without contraction, so with the
same scalars NumPy and the device produce the same bits).  ``step_ref`` takes the reduced sums as arguments, so that it can
be fed the device's own; ``solve_ref`` is the whole solver with a pluggable inner product (``DOTS``: four summation
orders, whose spread is what separates rounding from error in the whole-solve tests)."""
import math

import numpy as np

NONFINITE_SIGMA, ALPHA_CLAMPED, OMEGA_CLAMPED, RHO_ZERO = 1, 2, 4, 8


def quot(a, b):
    """IEEE ``a / b``, clamped to 0 when it is not finite (alpha and omega on the device)"""
    with np.errstate(all="ignore"):
        q = np.float64(a) / np.float64(b)
    return float(q) if np.isfinite(q) else 0.0


def flags_of(rho, sigma, theta, phi, rho_new):
    f = 0
    with np.errstate(all="ignore"):
        if not np.isfinite(sigma):
            f |= NONFINITE_SIGMA
        elif np.isfinite(rho) and not np.isfinite(np.float64(rho) / np.float64(sigma)):
            f |= ALPHA_CLAMPED
        if not np.isfinite(np.float64(theta) / np.float64(phi)):
            f |= OMEGA_CLAMPED
    if not np.isfinite(rho_new) or rho_new == 0.0:
        f |= RHO_ZERO
    return f


def dir_ref(r, p, v, beta, omega):
    return r + beta * (p - omega * v)


def half_ref(r, v, rho, sigma):
    alpha = quot(rho, sigma)
    return alpha, r - alpha * v


def full_ref(p, s, t, y, alpha, theta, phi):
    omega = quot(theta, phi)
    return omega, (y + alpha * p) + omega * s, s - omega * t


def step_ref(state, scalars, v=None, t=None):
    """One iteration from ``state`` (``apply``: x -> A^ x, and the vectors ``r, p, v, y``) with the scalars AND sums of
    ``scalars`` (``first, beta, omega_prev, rho, sigma, theta, phi``).  ``v`` / ``t``: operator products to use instead of
    ``apply`` (an operator whose kernel does not promise SciPy's bits).  Returns the new ``p, v, s, t, y, r, alpha, omega``."""
    p = state["p"] if scalars["first"] else dir_ref(state["r"], state["p"], state["v"], scalars["beta"], scalars["omega_prev"])
    v = state["apply"](p) if v is None else v
    alpha, s = half_ref(state["r"], v, scalars["rho"], scalars["sigma"])
    t = state["apply"](s) if t is None else t
    omega, y, r = full_ref(p, s, t, state["y"], alpha, scalars["theta"], scalars["phi"])
    return dict(p=p, v=v, s=s, t=t, y=y, r=r, alpha=alpha, omega=omega)


# ---- four summation orders of the inner product ---------------------------------------------------------------------
def dot_reversed(a, b):
    return float(np.dot(a[::-1], b[::-1]))


def dot_fsum(a, b):
    return math.fsum((a * b).tolist())


def dot_strided(a, b, parts=256):
    return float(np.sum(np.array([np.dot(a[i::parts], b[i::parts]) for i in range(parts)])))


DOTS = {"numpy": np.dot, "reversed": dot_reversed, "fsum": dot_fsum, "strided256": dot_strided}


class Result(object):
    def __init__(self):
        self.resnorms, self.trace, self.iter, self.x, self.breakdown = [], [], 0, None, None


def solve_ref(A, b, tol, maxiter, Ml=None, Mr=None, x0=None, dot=np.dot):
    """BiCGStab on ``Ml A Mr`` from ``x0``; ``resnorms[k] = sqrt(<r_k, r_k>) / ||Ml b||`` of the recurrence's residual.
    Stops at the tolerance, at ``maxiter`` or at a breakdown (``breakdown``: the flags, with the iterate of that point)."""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = b.size
    ml = (lambda x: x) if Ml is None else (lambda x: Ml.dot(x))
    mr = (lambda x: x) if Mr is None else (lambda x: Mr.dot(x))

    def apply(x):
        return ml(A.dot(mr(x)))

    x0 = np.zeros(n) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(-1)
    out = Result()
    bnorm = math.sqrt(float(dot(ml(b), ml(b))))
    r = ml(b - A.dot(x0)) if np.any(x0) else ml(b)
    y = np.zeros(n)
    if bnorm == 0.0:
        out.resnorms, out.x = [0.0], np.zeros(n)
        return out
    rt, p, v = r.copy(), r.copy(), np.zeros(n)
    rho = float(dot(rt, r))
    out.resnorms.append(math.sqrt(float(dot(r, r))) / bnorm)
    rho_prev = alpha = omega = 0.0
    while out.resnorms[-1] > tol and out.iter < maxiter:
        k = out.iter
        beta = 0.0
        if k > 0:
            with np.errstate(all="ignore"):
                beta = float((np.float64(rho) / np.float64(rho_prev)) * (np.float64(alpha) / np.float64(omega)))
            if not np.isfinite(beta):
                out.breakdown = OMEGA_CLAMPED
                break
            p = dir_ref(r, p, v, beta, omega)
        v = apply(p)
        sigma = float(dot(rt, v))
        alpha, s = half_ref(r, v, rho, sigma)
        ss = float(dot(s, s))
        t = apply(s)
        theta, phi = float(dot(t, s)), float(dot(t, t))
        omega, y, r = full_ref(p, s, t, y, alpha, theta, phi)
        rho_new, rr = float(dot(rt, r)), float(dot(r, r))
        f = flags_of(rho, sigma, theta, phi, rho_new)
        out.trace.append((k, rho, sigma, ss, theta, phi, rho_new, rr, f))
        resnorm = math.sqrt(rr) / bnorm
        if f & (NONFINITE_SIGMA | ALPHA_CLAMPED | RHO_ZERO) and not resnorm <= tol:
            out.breakdown = f
            break
        out.resnorms.append(resnorm)
        rho_prev, rho = rho, rho_new
        out.iter += 1
    out.x = x0 + mr(y)
    return out
