"""Oracle of the Chebyshev polynomial preconditioner - TEST INFRASTRUCTURE ONLY, shares no code with the package.

``cheb_coefficients`` and ``cheb_apply_ref`` restate the operator to the bit: the coefficients in Python floats,

    theta = (lmax + lmin) / 2;  delta = (lmax - lmin) / 2;  sigma = theta / delta
    rho_0 = 1 / sigma;          (a_0, b_0) = (0.0, 1 / theta)
    rho_k = 1 / (2 * sigma - rho_{k-1});   (a_k, b_k) = (rho_k * rho_{k-1}, 2 * rho_k / delta)

and the ``m`` steps as NumPy array expressions in exactly this order (every multiply and add rounded on its own; the product
is ``A.dot``, SciPy's ``csr_matvec`` for a sparse ``A``):

    step 0:        t = r;           [t = t * dinv];  d = b_0 * t;              z = d
    step k >= 1:   t = r - A z;     [t = t * dinv];  d = (a_k * d) + (b_k * t); z = z + d

For complex data the scalars and ``dinv`` are real and everything except ``A z`` acts on the (re, im) view."""
import numpy as np


def cheb_coefficients(lmin, lmax, m):
    lmin, lmax = float(lmin), float(lmax)
    theta = (lmax + lmin) / 2
    delta = (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    out = [(0.0, 1 / theta)]
    for _ in range(1, m):
        rho_new = 1 / (2 * sigma - rho)
        out.append((rho_new * rho, 2 * rho_new / delta))
        rho = rho_new
    return np.array(out, dtype=np.float64).reshape(m, 2)


def _view(x):
    """The (re, im) view of a complex vector, the vector itself when real."""
    return x.view(np.float64) if x.dtype.kind == "c" else x


def cheb_apply_ref(A, r, coef, dinv=None):
    """``p(A) r`` for one vector or the columns of an ``(n, k)`` array; ``coef`` is the ``(m, 2)`` array of ``(a_k, b_k)``."""
    r = np.asarray(r)
    cplx = r.dtype.kind == "c" or getattr(A, "dtype", np.dtype(float)).kind == "c"
    dt = np.complex128 if cplx else np.float64
    R = np.ascontiguousarray(r.reshape(r.shape[0], -1).astype(dt).T)       # one contiguous row per column of r
    Z = np.empty_like(R)
    sc = None
    if dinv is not None:
        sc = np.asarray(dinv, dtype=np.float64)
        sc = np.repeat(sc, 2) if cplx else sc
    for c in range(R.shape[0]):
        rv = _view(R[c])
        t = rv.copy()
        if sc is not None:
            t = t * sc
        d = float(coef[0][1]) * t
        z = d.copy()
        for k in range(1, len(coef)):
            a, b = float(coef[k][0]), float(coef[k][1])
            zc = z.view(np.complex128) if cplx else z
            az = _view(np.ascontiguousarray(np.asarray(A.dot(zc)).reshape(-1).astype(dt)))
            t = rv - az
            if sc is not None:
                t = t * sc
            d = (a * d) + (b * t)
            z = z + d
        Z[c] = z.view(np.complex128) if cplx else z
    out = np.ascontiguousarray(Z.T)
    return out.reshape(r.shape) if r.ndim == 1 else out
