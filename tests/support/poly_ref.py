"""Oracle of the GMRES polynomial preconditioner - TEST INFRASTRUCTURE ONLY, shares no code with the package.

``roots_ref`` restates the roots (``d`` steps of modified Gram-Schmidt Arnoldi with a pluggable inner product, the harmonic
Ritz values ``eigvals(H_d + h_{d+1,d}^2 f e_d^T)``, ``f = H_d^{-H} e_d``, in modified Leja order), ``steps_ref`` the table and
``poly_apply_ref`` the application as NumPy array expressions in exactly the device's order (every multiply and add rounded on
its own; the product is ``A.dot``, SciPy's ``csr_matvec`` for a sparse ``A``):

    LIN   (kind 0):  s = A prod;  y = y + (c * prod);                  prod = prod - (c * s)
    QA    (kind 1):  s = A prod;  t = (a2 * prod) - s;  y = y + (c * t)
    QB    (kind 2):  s = A t;                                          prod = prod - (c * s)
    SCALE (kind 3):  y = c * x
    the first step: y = (c * ...) itself;   close: y = y + (cl * prod) with the new prod
"""
import math

import numpy as np


def arnoldi_ref(A, v, d, dot=np.dot):
    """``(H, k)``: the ``(k + 1, k)`` Hessenberg matrix of ``k <= d`` modified Gram-Schmidt Arnoldi steps (k < d: invariant)."""
    v = np.asarray(v, dtype=float).reshape(-1)
    n = v.size
    V = np.zeros((n, d + 1))
    H = np.zeros((d + 1, d))
    V[:, 0] = v / math.sqrt(dot(v, v))
    for k in range(d):
        w = np.asarray(A.dot(V[:, k])).reshape(-1)
        for j in range(k + 1):
            H[j, k] = dot(V[:, j], w)
            w = w - H[j, k] * V[:, j]
        H[k + 1, k] = math.sqrt(dot(w, w))
        if H[k + 1, k] <= 1e-14 * np.linalg.norm(H[:k + 2, :k + 1]):
            return H[:k + 2, :k + 1], k + 1, True
        V[:, k + 1] = w / H[k + 1, k]
    return H, d, False


def harmonic_ritz_ref(H, k, invariant=False):
    if invariant:
        return np.linalg.eigvals(H[:k, :k])
    Hd = H[:k, :k]
    e = np.zeros(k)
    e[k - 1] = 1.0
    f = np.linalg.solve(Hd.T, e)
    G = np.array(Hd)
    G[:, k - 1] = G[:, k - 1] + (H[k, k - 1] * H[k, k - 1]) * f
    return np.linalg.eigvals(G)


def _lg(x):
    return math.log(x) if x > 0.0 else -math.inf


def leja_ref(theta):
    """Modified Leja order: real roots and the Im > 0 members compete; largest modulus first, then the largest sum of
    log-distances to everything placed; the first of equals wins; the conjugate follows at once."""
    todo = [complex(t) for t in theta if complex(t).imag >= 0.0]
    done = []
    while todo:
        if not done:
            key = [abs(t) for t in todo]
        else:
            key = []
            for t in todo:
                acc = 0.0
                for mu in done:
                    acc = acc + _lg(abs(t - mu))
                key.append(acc)
        j = 0
        for i in range(1, len(todo)):
            if key[i] > key[j]:
                j = i
        t = todo.pop(j)
        done.append(t)
        if t.imag != 0.0:
            done.append(t.conjugate())
    return np.array(done, dtype=complex)


def roots_ref(A, d, v=None, seed=0, dot=np.dot):
    n = A.shape[0]
    if v is None:
        v = np.random.default_rng(seed).standard_normal((n, 1))
    H, k, inv = arnoldi_ref(A, v, min(d, n), dot)
    return leja_ref(harmonic_ritz_ref(H, k, inv or k < d))


def log10_pof_max_ref(theta):
    worst = -math.inf
    for k in range(len(theta)):
        acc = 0.0
        for i in range(len(theta)):
            if i != k:
                acc = acc + _lg(abs(1.0 - complex(theta[k]) / complex(theta[i])))
        worst = max(worst, acc / math.log(10.0))
    return worst


def steps_ref(roots):
    """The table of (kind, c, a2, close, cl) for ordered roots, in Python floats."""
    th = [complex(t) for t in roots]
    d = len(th)
    out = []
    i = 0
    while i < d:
        if th[i].imag == 0.0:
            inv = 1 / th[i].real
            if d == 1:
                out.append([3.0, inv, 0.0, 0.0, 0.0])
            elif i == d - 1:
                out[-1][3] = 1.0
                out[-1][4] = inv
            else:
                out.append([0.0, inv, 0.0, 0.0, 0.0])
            i += 1
        else:
            a, b = th[i].real, th[i].imag
            assert th[i + 1] == th[i].conjugate()
            c = 1 / ((a * a) + (b * b))
            out.append([1.0, c, 2 * a, 0.0, 0.0])
            if i + 2 < d:
                out.append([2.0, c, 0.0, 0.0, 0.0])
            i += 2
    return np.array(out, dtype=np.float64).reshape(len(out), 5)


def poly_apply_ref(A, x, steps):
    """``p(A) x`` for one vector or the columns of an ``(n, k)`` array; ``steps`` is the table."""
    x = np.asarray(x, dtype=np.float64)
    X = np.ascontiguousarray(x.reshape(x.shape[0], -1).T)
    Y = np.empty_like(X)
    for col in range(X.shape[0]):
        prod = X[col].copy()
        y = t = None
        for k, (kind, c, a2, close, cl) in enumerate(steps):
            kind, c, a2, cl = int(kind), float(c), float(a2), float(cl)
            if kind == 3:
                y = c * prod
                continue
            if kind == 0:
                s = np.asarray(A.dot(prod)).reshape(-1)
                u = c * prod
                y = u if k == 0 else y + u
                prod = prod - (c * s)
            elif kind == 1:
                s = np.asarray(A.dot(prod)).reshape(-1)
                t = (a2 * prod) - s
                u = c * t
                y = u if k == 0 else y + u
            else:
                s = np.asarray(A.dot(t)).reshape(-1)
                prod = prod - (c * s)
            if close != 0.0:
                y = y + (cl * prod)
        Y[col] = y
    out = np.ascontiguousarray(Y.T)
    return out.reshape(x.shape) if x.ndim == 1 else out
