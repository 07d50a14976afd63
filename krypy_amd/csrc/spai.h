// Sparse approximate inverse on a fixed pattern (static-pattern SPAI): the validation and the arithmetic of one row (spai.hip holds
// the kernel and the C entry points).  Plain C++, no HIP call: the header compiles alone (tests/support/spai_main.cpp builds it
// with the host sanitizers and runs it on the CPU).
//
// Row i of M minimises || e_i^T - m^T A[J, :] ||_2 over the entries m of the pattern columns J = (J_0 < ... < J_{q-1}), q <= 32: the
// normal equations G m = r with G_ab = sum_c conj(A[J_a, c]) A[J_b, c], r_a = conj(A[J_a, i]), solved by a root-free Cholesky
// factorisation G = L D L^H.  THE CONTRACT (every multiply, add and divide rounds on its own; complex product (ac - bd, ad + bc);
// a complex value times or over a real d: part by part):
//   G_ab (a >= b): two-pointer merge of the CSR rows J_a, J_b in ascending column, s = +0; s = s + conj(x) * y
//   L, d: the factorisation of sai_row.h with X = G
//   y_a = r_a - sum_{k < a} L_ak * y_k (k ascending);  z_a = y_a / d_a;  m_a = z_a - sum_{k > a} conj(L_ka) * m_k (k ascending,
//   a = q-1 .. 0)
// A row breaks down when some d_j is not > 0 or not finite; the arithmetic goes on and the SMALLEST such row is reported.  A part of
// m_a that is a NaN is STORED as the quiet NaN 0x7ff8000000000000 (sai_row.h says why): host and device agree in every bit of a
// broken row too.
//
// row<Z>() deals that work to the W lanes of a group in phases with a barrier between them (Exec::phase).  Every G_ab, L_ij, y_a
// and m_a is the work of one lane in the order above, so the result does not depend on W:
//   gram     pair t = a (a + 1) / 2 + b to lane t mod W;  r_a to lane a mod W
//   P1(j)    y_a = y_a - L_{a,j-1} * y_{j-1} for a >= j, lane a mod W (the forward substitution, column by column: every y_a still
//            receives its terms in ascending k), then P1(j) of sai_row.h
//   P2(j)    that of sai_row.h (the same loop as in fsai.h; sai_row.h says why it stands in both)
//   back     lane 0: z and the back substitution, m written to the output
// The loops that hold a barrier run to `qloop`, the longest pattern row of the CALL, with j < q as a predicate: all lanes of a
// workgroup reach every barrier.  Work space of one row: the layout of sai_row.h with X = G and x = r / y.
#pragma once
#include "sai_row.h"

namespace khspai {

using namespace khsai;      // QMAX, Csr, row_doubles, ...: what every row-by-row builder shares

// lanes per pattern row for a call whose longest pattern row has qmax entries - measured (KERNELS.md 4.24: N = 10^6, q = 5, 13, 25,
// widths 8 / 16 / 32 / 64): short rows want many rows per workgroup and barrier, long ones lanes for the q (q + 1) / 2 merges
inline int group_width(int64_t qmax, bool cplx) { return qmax <= 8 ? 8 : qmax <= 16 ? 16 : cplx ? 64 : 32; }

// Checks A and the pattern.  Returns "" and the longest pattern row, or what is wrong (the row named).
inline std::string validate(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int64_t pnnz, const int32_t* pindptr,
                            const int32_t* pindices, int64_t* qmax) {
    const std::string why = validate_patterns(n, nnz, indptr, indices, pnnz, pindptr, pindices, qmax);
    if (!why.empty()) return why;
    if (*qmax > QMAX)
        for (int64_t i = 0; i < n; ++i)
            if (pindptr[i + 1] - pindptr[i] > QMAX)
                return "pattern row " + str(i) + " has " + str(pindptr[i + 1] - pindptr[i]) + " entries, at most " + str(QMAX) + " are supported";
    return "";
}

// Row i of M on the W lanes of `ex` (a lane calls phase(f) with f(lane); phase() ends with the barrier).  J: the q pattern columns
// of the row, w: row_doubles(qloop) of work space, m: where the q values go (Z: pairs).  Returns true when a d_j this lane
// computed is not > 0 or not finite (the host form: any lane).  q = 0: nothing is read or written, every barrier is reached.
template <bool Z, class Exec>
KH_SAI_HD inline bool row(const Csr& A, const int32_t* J, int q, int qloop, int32_t i, double* w, double* m, int W, Exec& ex) {
    const Planes<Z> ws(w, qloop);
    const int S = ws.S;
    double *Lr = ws.Lr, *Li = ws.Li, *d = ws.d, *vr = ws.vr, *vi = ws.vi, *yr = ws.xr, *yi = ws.xi;
    bool bad = false;

    ex.phase([&](int lane) {          // gram
        const int npair = q * (q + 1) / 2;
        for (int t = lane; t < npair; t += W) {
            int a = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
            while ((a + 1) * (a + 2) / 2 <= t) ++a;
            while (a * (a + 1) / 2 > t) --a;
            const int b = t - a * (a + 1) / 2;
            int32_t pa = A.indptr[J[a]], pb = A.indptr[J[b]];
            const int32_t ea = A.indptr[J[a] + 1], eb = A.indptr[J[b] + 1];
            double sr = 0.0, si = 0.0;
            while (pa < ea && pb < eb) {
                const int32_t ca = A.indices[pa], cb = A.indices[pb];
                if (ca == cb) {
                    if (!Z) {
                        sr = sr + A.data[pa] * A.data[pb];
                    } else {
                        const double xr = A.data[2 * (int64_t)pa], xi = -A.data[2 * (int64_t)pa + 1];      // conj
                        const double ur = A.data[2 * (int64_t)pb], ui = A.data[2 * (int64_t)pb + 1];
                        sr = sr + (xr * ur - xi * ui);
                        si = si + (xr * ui + xi * ur);
                    }
                    ++pa;
                    ++pb;
                } else if (ca < cb) ++pa;
                else ++pb;
            }
            Lr[a * S + b] = sr;
            if (Z) Li[a * S + b] = si;
        }
        for (int a = lane; a < q; a += W) {
            double rr = 0.0, ri = 0.0;
            for (int32_t p = A.indptr[J[a]]; p < A.indptr[J[a] + 1]; ++p) {
                const int32_t c = A.indices[p];
                if (c >= i) {
                    if (c == i) {
                        rr = Z ? A.data[2 * (int64_t)p] : A.data[p];
                        if (Z) ri = -A.data[2 * (int64_t)p + 1];
                    }
                    break;
                }
            }
            yr[a] = rr;
            if (Z) yi[a] = ri;
        }
    });

    for (int j = 0; j < qloop; ++j) {
        ex.phase([&](int lane) {          // P1(j)
            if (j >= q) return;
            if (j > 0)
                for (int a = j + (lane - j % W + W) % W; a < q; a += W) {      // a >= j, a mod W == lane
                    const double lr = Lr[a * S + j - 1], kr = yr[j - 1];
                    if (!Z) {
                        yr[a] = yr[a] - lr * kr;
                    } else {
                        const double li = Li[a * S + j - 1], ki = yi[j - 1];
                        yr[a] = yr[a] - (lr * kr - li * ki);
                        yi[a] = yi[a] - (lr * ki + li * kr);
                    }
                }
            for (int r = j + lane; r < q; r += W) {
                double sr = Lr[r * S + j], si = Z ? Li[r * S + j] : 0.0;
                for (int k = 0; k < j; ++k) {
                    const double lr = Lr[r * S + k], cr = vr[k];
                    if (!Z) {
                        sr = sr - lr * cr;
                    } else {
                        const double li = Li[r * S + k], ci = -vi[k];      // conj
                        sr = sr - (lr * cr - li * ci);
                        si = si - (lr * ci + li * cr);
                    }
                }
                if (r == j) {
                    d[j] = sr;
                    bad = bad || broken(sr);
                } else {
                    Lr[r * S + j] = sr;
                    if (Z) Li[r * S + j] = si;
                }
            }
        });
        ex.phase([&](int lane) {          // P2(j)
            if (j >= q) return;
            const double dj = d[j];
            for (int r = j + 1 + lane; r < q; r += W) {
                const double lr = Lr[r * S + j] / dj;
                Lr[r * S + j] = lr;
                if (r == j + 1) vr[j] = lr * dj;
                if (Z) {
                    const double li = Li[r * S + j] / dj;
                    Li[r * S + j] = li;
                    if (r == j + 1) vi[j] = li * dj;
                }
            }
            if (j + 1 < q)
                for (int k = lane; k < j; k += W) {
                    vr[k] = Lr[(j + 1) * S + k] * d[k];
                    if (Z) vi[k] = Li[(j + 1) * S + k] * d[k];
                }
        });
    }

    ex.phase([&](int lane) {
        if (lane != 0) return;
        for (int a = q - 1; a >= 0; --a) {
            double sr = yr[a] / d[a], si = Z ? yi[a] / d[a] : 0.0;
            for (int k = a + 1; k < q; ++k) {
                const double lr = Lr[k * S + a];
                if (!Z) {
                    sr = sr - lr * m[k];
                } else {
                    const double li = -Li[k * S + a], mr = m[2 * k], mi = m[2 * k + 1];      // conj
                    sr = sr - (lr * mr - li * mi);
                    si = si - (lr * mi + li * mr);
                }
            }
            if (!Z) {
                m[a] = stored(sr);
            } else {
                m[2 * a] = stored(sr);
                m[2 * a + 1] = stored(si);
            }
        }
    });
    return bad;
}

// All rows on the host with W emulated lanes per row (cplx: (re, im) pairs).  Returns the smallest row that broke down, or -1.
// work: row_doubles(qloop, cplx) doubles.
inline int64_t build_host(int64_t n, const Csr& A, const int32_t* pindptr, const int32_t* pindices, int qloop, int W, bool cplx,
                          double* work, double* m_out) {
    return khsai::build_host(n, pindptr, W, [&](int64_t i, int32_t p0, int q, HostLanes& ex) {
        return cplx ? row<true>(A, pindices + p0, q, qloop, (int32_t)i, work, m_out + 2 * (int64_t)p0, W, ex)
                    : row<false>(A, pindices + p0, q, qloop, (int32_t)i, work, m_out + p0, W, ex);
    });
}

}  // namespace khspai
