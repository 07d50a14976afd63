// Sparse approximate inverse on a fixed pattern (static-pattern SPAI): the validation and the arithmetic of one row (spai.hip holds
// the kernel and the C entry points).  Plain C++, no HIP call: the header compiles alone (tests/support/spai_main.cpp builds it
// with the host sanitizers and runs it on the CPU).
//
// Row i of M minimises || e_i^T - m^T A[J, :] ||_2 over the entries m of the pattern columns J = (J_0 < ... < J_{q-1}), q <= 32: the
// normal equations G m = r with G_ab = sum_c conj(A[J_a, c]) A[J_b, c], r_a = conj(A[J_a, i]), solved by a root-free Cholesky
// factorisation G = L D L^H.  THE CONTRACT (every multiply, add and divide rounds on its own; complex product (ac - bd, ad + bc);
// a complex value times or over a real d: part by part):
//   G_ab (a >= b): two-pointer merge of the CSR rows J_a, J_b in ascending column, s = +0; s = s + conj(x) * y
//   for j = 0 .. q-1:   v_k = L_jk * d_k (k < j);   s = G_jj; s = s - L_jk * conj(v_k) (k < j ascending);   d_j = Re(s)
//                       for i > j:  s = G_ij; s = s - L_ik * conj(v_k) (k < j ascending);  L_ij = s / d_j
//   y_a = r_a - sum_{k < a} L_ak * y_k (k ascending);  z_a = y_a / d_a;  m_a = z_a - sum_{k > a} conj(L_ka) * m_k (k ascending,
//   a = q-1 .. 0)
// A row breaks down when some d_j is not > 0 or not finite; the arithmetic goes on and the SMALLEST such row is reported.  IEEE 754
// leaves the sign and payload of a NaN that an invalid operation produces to the hardware (inf - inf is 0x7ff8... on gfx950 and
// 0xfff8... on x86), so a part of m_a that is a NaN is STORED as the quiet NaN 0x7ff8000000000000: host and device then agree in
// every bit of a broken row too (infinities keep their sign; a NaN never turns into anything else on the way).
//
// row<Z>() deals that work to the W lanes of a group in phases with a barrier between them (Exec::phase).  Every G_ab, L_ij, y_a
// and m_a is the work of one lane in the order above, so the result does not depend on W:
//   gram     pair t = a (a + 1) / 2 + b to lane t mod W;  r_a to lane a mod W
//   P1(j)    y_a = y_a - L_{a,j-1} * y_{j-1} for a >= j, lane a mod W (the forward substitution, column by column: every y_a still
//            receives its terms in ascending k);  T_ij = G_ij - sum_{k<j} L_ik conj(v_k) for i >= j, lane (i - j) mod W;  d_j
//   P2(j)    L_ij = T_ij / d_j for i > j, lane (i - j - 1) mod W; that lane of row j + 1 also writes v_j = L_{j+1,j} * d_j;
//            v_k = L_{j+1,k} * d_k for k < j, lane k mod W: the v of column j + 1
//   back     lane 0: z and the back substitution, m written to the output
// The loops that hold a barrier run to `qloop`, the longest pattern row of the CALL, with j < q as a predicate: all lanes of a
// workgroup reach every barrier.  Work space of one row (doubles, P = 1 real / 2 complex planes, S = qloop | 1 the row stride -
// odd, so the lanes of P1, one matrix row each, read 32 different LDS banks with 64-bit reads):
//   [P * S * qloop] G / T / L in place, lower triangle   [qloop] d   [P * qloop] v   [P * qloop] r / y
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <string>

#if defined(__HIPCC__)
#define KH_SPAI_HD __host__ __device__
#else
#define KH_SPAI_HD
#endif

namespace khspai {

constexpr int QMAX = 32;

KH_SPAI_HD inline int stride(int qloop) { return qloop | 1; }
// doubles of one row's work space
KH_SPAI_HD inline int64_t row_doubles(int qloop, bool cplx) {
    const int P = cplx ? 2 : 1;
    return (int64_t)P * stride(qloop) * qloop + qloop + 2 * (int64_t)P * qloop;
}
// lanes per pattern row for a call whose longest pattern row has qmax entries - measured (KERNELS.md 4.24: N = 10^6, q = 5, 13, 25,
// widths 8 / 16 / 32 / 64): short rows want many rows per workgroup and barrier, long ones lanes for the q (q + 1) / 2 merges
inline int group_width(int64_t qmax, bool cplx) { return qmax <= 8 ? 8 : qmax <= 16 ? 16 : cplx ? 64 : 32; }

// one CSR pattern: sorted, duplicate-free, columns in [0, n).  `what` names it in the message ("A" / "the pattern").
inline std::string check_pattern(const char* what, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int64_t* longest) {
    auto str = [](int64_t v) { return std::to_string((long long)v); };
    if (nnz < 0 || nnz > (int64_t)0x7fffffff) return std::string("nnz = ") + str(nnz) + " of " + what + " out of range (int32 row pointers)";
    if (!indptr || (nnz > 0 && !indices)) return std::string("NULL array of ") + what;
    if (indptr[0] != 0 || indptr[n] != nnz) return std::string("indptr[0] != 0 or indptr[n] != nnz of ") + what;
    *longest = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = indptr[i], b = indptr[i + 1];
        if (a > b || b > nnz) return std::string("indptr of ") + what + " not ascending at row " + str(i);
        for (int64_t p = a; p < b; ++p) {
            const int64_t c = indices[p];
            if (c < 0 || c >= n) return "column " + str(c) + " out of range in row " + str(i) + " of " + what;
            if (p > a && indices[p - 1] >= c)
                return std::string(indices[p - 1] == c ? "duplicate" : "unsorted") + " column indices in row " + str(i) + " of " + what;
        }
        if (b - a > *longest) *longest = b - a;
    }
    return "";
}

// Checks A and the pattern.  Returns "" and the longest pattern row, or what is wrong (the row named).
inline std::string validate(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int64_t pnnz, const int32_t* pindptr,
                            const int32_t* pindices, int64_t* qmax) {
    auto str = [](int64_t v) { return std::to_string((long long)v); };
    if (n < 1 || n > (int64_t)0x7fffffff - 64) return "n = " + str(n) + " out of range";
    int64_t longest = 0;
    std::string why = check_pattern("A", n, nnz, indptr, indices, &longest);
    if (!why.empty()) return why;
    why = check_pattern("the pattern", n, pnnz, pindptr, pindices, qmax);
    if (!why.empty()) return why;
    if (*qmax > QMAX)
        for (int64_t i = 0; i < n; ++i)
            if (pindptr[i + 1] - pindptr[i] > QMAX)
                return "pattern row " + str(i) + " has " + str(pindptr[i + 1] - pindptr[i]) + " entries, at most " + str(QMAX) + " are supported";
    return "";
}

struct Csr {
    const int32_t* indptr;
    const int32_t* indices;
    const double* data;      // Z: (re, im) pairs
};

// The lanes of one group on the host, one after the other; the end of the loop is the barrier.
struct HostLanes {
    int W;
    template <class F>
    void phase(F f) {
        for (int l = 0; l < W; ++l) f(l);
    }
};

KH_SPAI_HD inline bool broken(double d) { return !(d > 0.0) || !(d <= DBL_MAX); }
// what is stored for x: a NaN as the one quiet NaN 0x7ff8000000000000
KH_SPAI_HD inline double stored(double x) { return x != x ? __builtin_nan("") : x; }

// Row i of M on the W lanes of `ex` (a lane calls phase(f) with f(lane); phase() ends with the barrier).  J: the q pattern columns
// of the row, w: row_doubles(qloop) of work space, m: where the q values go (Z: pairs).  Returns true when a d_j this lane
// computed is not > 0 or not finite (the host form: any lane).  q = 0: nothing is read or written, every barrier is reached.
template <bool Z, class Exec>
KH_SPAI_HD inline bool row(const Csr& A, const int32_t* J, int q, int qloop, int32_t i, double* w, double* m, int W, Exec& ex) {
    const int S = stride(qloop), P = Z ? 2 : 1;
    double* Lr = w;                                  // [a * S + b], lower triangle
    double* Li = w + (Z ? S * qloop : 0);
    double* d = w + P * S * qloop;
    double* vr = d + qloop;
    double* vi = vr + (Z ? qloop : 0);
    double* yr = vr + P * qloop;
    double* yi = yr + (Z ? qloop : 0);
    bool bad = false;

    ex.phase([&](int lane) {
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
    int64_t bad = -1;
    HostLanes ex{W};
    for (int64_t i = 0; i < n; ++i) {
        const int32_t p0 = pindptr[i];
        const int q = pindptr[i + 1] - p0;
        const bool broke = cplx ? row<true>(A, pindices + p0, q, qloop, (int32_t)i, work, m_out + 2 * (int64_t)p0, W, ex)
                                : row<false>(A, pindices + p0, q, qloop, (int32_t)i, work, m_out + p0, W, ex);
        if (broke && bad < 0) bad = i;
    }
    return bad;
}

}  // namespace khspai
