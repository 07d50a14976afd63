// What the approximate inverses built row by row on a fixed pattern share (spai.h: static-pattern SPAI, fsai.h: static-pattern FSAI):
// the validation of A and the pattern, the work space of one row, the contract of the root-free Cholesky factorisation
// X = L D L^H of the row's small Hermitian matrix and the loop over the rows on the host.  Plain C++, no HIP call: the header
// compiles alone.
//
// Each method gathers the lower triangle of its X (q x q, q <= 32: a Gram matrix or a submatrix of A), factors it and substitutes
// back.  THE CONTRACT of the factorisation (every multiply, add and divide rounds on its own; complex product (ac - bd, ad + bc); a
// complex value times or over a real d: part by part):
//   for j = 0 .. q-1:   v_k = L_jk * d_k (k < j);   s = X_jj; s = s - L_jk * conj(v_k) (k < j ascending);   d_j = Re(s)
//                       for i > j:  s = X_ij; s = s - L_ik * conj(v_k) (k < j ascending);  L_ij = s / d_j
// A row breaks down when some d_j is not > 0 or not finite; the arithmetic goes on.  IEEE 754 leaves the sign and payload of a NaN
// that an invalid operation produces to the hardware (inf - inf is 0x7ff8... on gfx950 and 0xfff8... on x86), so a part of a result
// that is a NaN is STORED as the quiet NaN 0x7ff8000000000000 (stored()): host and device then agree in every bit of a broken row
// too (infinities keep their sign; a NaN never turns into anything else on the way).
//
// Both row<Z>() deal that work to the W lanes of a group in two phases per column, with a barrier after each (Exec::phase).  Every
// L_ij and d_j is the work of one lane in the order above, so the result does not depend on W:
//   P1(j)    T_ij = X_ij - sum_{k<j} L_ik conj(v_k) for i >= j, lane (i - j) mod W;  d_j
//   P2(j)    L_ij = T_ij / d_j for i > j, lane (i - j - 1) mod W; that lane of row j + 1 also writes v_j = L_{j+1,j} * d_j;
//            v_k = L_{j+1,k} * d_k for k < j, lane k mod W: the v of column j + 1
// The loop runs to `qloop`, the longest pattern row of the CALL, with j < q as a predicate: all lanes of a workgroup reach every
// barrier.  THE LOOP ITSELF STANDS IN BOTH HEADERS, line for line but for the forward-substitution column at the head of SPAI's
// P1(j): as a function template of this header (with that column as a callable, as a compile-time option, the flag returned or
// passed by reference, always_inline or not) the compiler carried the breakdown flag through the loop with three more scalar
// mask instructions per column and two more SGPRs, and k_spai measured 0.3 to 0.7 % slower (profiles/sai_refactor_bench.log).
// Work space of one row (doubles, P = 1 real / 2 complex planes, S = qloop | 1 the row stride - odd, so the lanes of P1, one
// matrix row each, read 32 different LDS banks with 64-bit reads):
//   [P * S * qloop] X / T / L in place, lower triangle   [qloop] d   [P * qloop] v   [P * qloop] x, the method's own vector
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <string>

#if defined(__HIPCC__)
#define KH_SAI_HD __host__ __device__
#else
#define KH_SAI_HD
#endif

namespace khsai {

constexpr int QMAX = 32;

KH_SAI_HD inline int stride(int qloop) { return qloop | 1; }
// doubles of one row's work space
KH_SAI_HD inline int64_t row_doubles(int qloop, bool cplx) {
    const int P = cplx ? 2 : 1;
    return (int64_t)P * stride(qloop) * qloop + qloop + 2 * (int64_t)P * qloop;
}

inline std::string str(int64_t v) { return std::to_string((long long)v); }

// one CSR pattern: sorted, duplicate-free, columns in [0, n).  `what` names it in the message ("A" / "the pattern").
inline std::string check_pattern(const char* what, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int64_t* longest) {
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

// The checks every method makes first: n, A and the pattern.  Returns "" and the longest pattern row, or what is wrong.
inline std::string validate_patterns(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int64_t pnnz,
                                     const int32_t* pindptr, const int32_t* pindices, int64_t* qmax) {
    if (n < 1 || n > (int64_t)0x7fffffff - 64) return "n = " + str(n) + " out of range";
    const std::string why = check_pattern("A", n, nnz, indptr, indices, qmax);
    return why.empty() ? check_pattern("the pattern", n, pnnz, pindptr, pindices, qmax) : why;
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

KH_SAI_HD inline bool broken(double d) { return !(d > 0.0) || !(d <= DBL_MAX); }
// what is stored for x: a NaN as the one quiet NaN 0x7ff8000000000000
KH_SAI_HD inline double stored(double x) { return x != x ? __builtin_nan("") : x; }

// the work space w of one row (row_doubles(qloop) doubles) by its planes; the imaginary planes of real data alias the real ones
// and are never touched
template <bool Z>
struct Planes {
    int S;                                       // the row stride of L
    double *Lr, *Li, *d, *vr, *vi, *xr, *xi;     // L: [a * S + b], lower triangle; x: the method's vector, SPAI's r / y, FSAI's u
    KH_SAI_HD Planes(double* w, int qloop)
        : S(stride(qloop)),
          Lr(w),
          Li(w + (Z ? S * qloop : 0)),
          d(w + (Z ? 2 : 1) * S * qloop),
          vr(d + qloop),
          vi(vr + (Z ? qloop : 0)),
          xr(vr + (Z ? 2 : 1) * qloop),
          xi(xr + (Z ? qloop : 0)) {}
};

// All rows on the host with W emulated lanes per row: row(i, p0, q, ex) computes pattern row i, the q entries from position p0,
// and returns whether it broke down.  Returns the smallest row that broke down, or -1.
template <class Row>
inline int64_t build_host(int64_t n, const int32_t* pindptr, int W, Row row) {
    int64_t bad = -1;
    HostLanes ex{W};
    for (int64_t i = 0; i < n; ++i) {
        const int32_t p0 = pindptr[i];
        if (row(i, p0, pindptr[i + 1] - p0, ex) && bad < 0) bad = i;
    }
    return bad;
}

}  // namespace khsai
