// Factorized sparse approximate inverse on a fixed lower-triangular pattern (static-pattern FSAI): the validation and the
// arithmetic of one row (fsai.hip holds the kernel and the C entry points).  Plain C++, no HIP call: the header compiles alone
// (tests/support/fsai_main.cpp builds it with the host sanitizers and runs it on the CPU).
//
// For a Hermitian positive definite A = L L^H, G ~ L^-1 on the pattern, so that M = G^H G is Hermitian positive definite by
// construction.  Row i with the pattern columns J = (J_0 < ... < J_{q-1} = i), 1 <= q <= 32, is u / sqrt(d_i), where u solves
// A[J, J] y = e_last up to the scale y_last = 1 / d_i: A[J, J] = L D L^H by a root-free Cholesky factorisation, then L^T u = e_last.
// This header computes u and d_i; the square root and the division by it are the caller's (utils.fsai does them in NumPy).
// THE CONTRACT (every multiply, add and divide rounds on its own; complex product (ac - bd, ad + bc); a complex value times or
// over a real d: part by part):
//   S_ab (a >= b) = the stored A[J_a, J_b], or +0 where row J_a has no entry in column J_b: bits copied, no arithmetic - the merge of
//                   the sorted CSR row J_a with J.  Only the LOWER triangle of A is ever read.
//   L, d: the factorisation of sai_row.h with X = S
//   u_{q-1} = 1;   u_a = s with s = +0; s = s - L_ka * u_k (k = a + 1 .. q - 1 ascending, a = q - 2 .. 0)
// The back substitution takes L UNCONJUGATED (L^T u = e_last): that is what makes (G A)[i, J_b] = 0 for b < q - 1 with complex data.
// Outputs: u at the CSR positions of the pattern and d_i = d_{q-1}, one real value per row; a part that is a NaN is stored as the one
// quiet NaN 0x7ff8000000000000 (khsai::stored).  A row breaks down when some d_j is not > 0 or not finite (A[J, J] is not positive
// definite); the arithmetic goes on and the SMALLEST such row is reported.
//
// row<Z>() deals that work to the W lanes of a group in phases with a barrier between them (Exec::phase).  Every S_ab, L_ij and u_a
// is the work of one lane in the order above, so the result does not depend on W:
//   gather   matrix row a (the merge of CSR row J_a with J_0 .. J_a) to lane a mod W
//   P1(j), P2(j)   those of sai_row.h (the same loop as in spai.h without its forward column; sai_row.h says why it stands in both)
//   back     lane 0: the back substitution, u and d_i written to the output
// The loops that hold a barrier run to `qloop`, the longest pattern row of the CALL, with j < q as a predicate: all lanes of a
// workgroup reach every barrier.  Work space of one row: the layout of sai_row.h with X = S and x = u.
#pragma once
#include "sai_row.h"

namespace khfsai {

using namespace khsai;      // QMAX, Csr, row_doubles, ...: what every row-by-row builder shares

// lanes per pattern row for a call whose longest pattern row has qmax entries - measured (KERNELS.md 4.26: N = 10^6, q = 3, 7, 13,
// 21, widths 8 / 16 / 32 / 64, real and complex).  The thresholds of khspai::group_width carry over for short rows; the gather here is
// q merges, not q (q + 1) / 2, so 64 lanes per row never pay, not even with complex data (q = 21: 14.7 ms with 32 lanes, 16.1 with 64)
inline int group_width(int64_t qmax) { return qmax <= 8 ? 8 : qmax <= 16 ? 16 : 32; }

// Checks A and the pattern.  Returns "" and the longest pattern row, or what is wrong (the row named).
inline std::string validate(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int64_t pnnz, const int32_t* pindptr,
                            const int32_t* pindices, int64_t* qmax) {
    const std::string why = validate_patterns(n, nnz, indptr, indices, pnnz, pindptr, pindices, qmax);
    if (!why.empty()) return why;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t q = pindptr[i + 1] - pindptr[i];
        if (q < 1) return "pattern row " + str(i) + " is empty, it has to end in the diagonal";
        if (pindices[pindptr[i + 1] - 1] != i)
            return "pattern row " + str(i) + " ends in column " + str(pindices[pindptr[i + 1] - 1]) + ", a lower-triangular pattern with the diagonal is expected";
        if (q > QMAX) return "pattern row " + str(i) + " has " + str(q) + " entries, at most " + str(QMAX) + " are supported";
    }
    return "";
}

// Row i of the factor on the W lanes of `ex` (a lane calls phase(f) with f(lane); phase() ends with the barrier).  J: the q pattern
// columns of the row (J[q - 1] = i), w: row_doubles(qloop) of work space, u_out: where the q values go (Z: pairs), d_out: where d_i
// goes.  Returns true when a d_j this lane computed is not > 0 or not finite (the host form: any lane).  q = 0: nothing is read or
// written, every barrier is reached.
template <bool Z, class Exec>
KH_SAI_HD inline bool row(const Csr& A, const int32_t* J, int q, int qloop, double* w, double* u_out, double* d_out, int W, Exec& ex) {
    const Planes<Z> ws(w, qloop);
    const int S = ws.S;
    double *Lr = ws.Lr, *Li = ws.Li, *d = ws.d, *vr = ws.vr, *vi = ws.vi, *ur = ws.xr, *ui = ws.xi;
    bool bad = false;

    ex.phase([&](int lane) {          // gather
        for (int a = lane; a < q; a += W) {
            for (int b = 0; b <= a; ++b) {
                Lr[a * S + b] = 0.0;
                if (Z) Li[a * S + b] = 0.0;
            }
            int32_t p = A.indptr[J[a]];
            const int32_t e = A.indptr[J[a] + 1];
            int b = 0;
            while (p < e && b <= a) {
                const int32_t c = A.indices[p], jb = J[b];
                if (c == jb) {
                    Lr[a * S + b] = Z ? A.data[2 * (int64_t)p] : A.data[p];
                    if (Z) Li[a * S + b] = A.data[2 * (int64_t)p + 1];
                    ++p;
                    ++b;
                } else if (c < jb) ++p;
                else ++b;
            }
        }
    });

    for (int j = 0; j < qloop; ++j) {
        ex.phase([&](int lane) {          // P1(j)
            if (j >= q) return;
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

    ex.phase([&](int lane) {          // back: L^T u = e_last, L unconjugated
        if (lane != 0 || q < 1) return;
        ur[q - 1] = 1.0;
        if (Z) ui[q - 1] = 0.0;
        for (int a = q - 2; a >= 0; --a) {
            double sr = 0.0, si = 0.0;
            for (int k = a + 1; k < q; ++k) {
                const double lr = Lr[k * S + a];
                if (!Z) {
                    sr = sr - lr * ur[k];
                } else {
                    const double li = Li[k * S + a], xr = ur[k], xi = ui[k];
                    sr = sr - (lr * xr - li * xi);
                    si = si - (lr * xi + li * xr);
                }
            }
            ur[a] = sr;
            if (Z) ui[a] = si;
        }
        for (int a = 0; a < q; ++a) {
            if (!Z) {
                u_out[a] = stored(ur[a]);
            } else {
                u_out[2 * a] = stored(ur[a]);
                u_out[2 * a + 1] = stored(ui[a]);
            }
        }
        *d_out = stored(d[q - 1]);
    });
    return bad;
}

// All rows on the host with W emulated lanes per row (cplx: (re, im) pairs).  Returns the smallest row that broke down, or -1.
// work: row_doubles(qloop, cplx) doubles.
inline int64_t build_host(int64_t n, const Csr& A, const int32_t* pindptr, const int32_t* pindices, int qloop, int W, bool cplx,
                          double* work, double* u_out, double* d_out) {
    return khsai::build_host(n, pindptr, W, [&](int64_t i, int32_t p0, int q, HostLanes& ex) {
        return cplx ? row<true>(A, pindices + p0, q, qloop, work, u_out + 2 * (int64_t)p0, d_out + i, W, ex)
                    : row<false>(A, pindices + p0, q, qloop, work, u_out + p0, d_out + i, W, ex);
    });
}

}  // namespace khfsai
