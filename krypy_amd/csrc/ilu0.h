// ILU(0) factorisation by level scheduling and the greedy multicolour ordering: the HOST analysis and the arithmetic of one row
// (ilu0.hip holds the kernels and the C entry points).  Plain C++, no HIP call: the header compiles alone
// (tests/support/ilu0_analysis_main.cpp builds it with the host sanitizers and runs it on the CPU).
//
// The factorisation, in place on a copy a of the values of a CSR matrix with sorted, duplicate-free indices and a structural
// diagonal in every row (stored zeros are part of the pattern):
//   for i = 0 .. n-1:
//     for the entries p of row i with k = col[p] < i, ascending:
//       a[p] = a[p] / a[dpos[k]]                                  (the finished pivot of row k)
//       for the entries q of row i behind p: if (k, col[q]) is an entry r of row k:  a[q] = a[q] - a[p] * a[r]
// Product and difference round separately; complex: (ac - bd, ad + bc) and NumPy's quotient (Smith's formula, ratio and scale
// once - the code of tri_slice<true> in tri.hip).  Row i reads rows k < i of its own pattern only, so its dependency graph is
// that of tril(A, -1): level[i] = 1 + max level[k], and the plan is khtri::analyse's on the strict lower pattern - rows grouped
// by level, inside a level by (strict lower length descending, row index ascending), slices of 64 rows that never span two
// levels, narrow runs and wide levels decided by the same narrow_rows.  A row breaks down when its finished pivot is zero or not
// finite; factor_host / the kernels report the SMALLEST such row (a row that inherits a NaN has a larger index than the row that
// produced it) and go on, as the sequential loop does.
#pragma once
#include <float.h>
#include <math.h>

#include "tri.h"

#if defined(__HIPCC__)
#define KH_ILU0_HD __host__ __device__
#else
#define KH_ILU0_HD
#endif

namespace khilu0 {

struct Plan {
    int64_t n = 0, nnz = 0, nlevels = 0, widest = 0, longest = 0, nslices = 0;
    int64_t n_wide = 0, n_narrow = 0;
    std::vector<int32_t> dpos;         // [n] position of the diagonal entry of every row
    std::vector<int32_t> level;        // [n]
    std::vector<int32_t> order;        // [n] rows in level order
    std::vector<int32_t> lev_ptr;      // [nlevels + 1] into order
    std::vector<int32_t> lev_slice;    // [nlevels + 1] first slice of every level
    std::vector<int32_t> row_id;       // [nslices * 64] one thread per entry, -1: no row
    std::vector<khtri::Launch> launches;
};

// Checks the CSR pattern and builds the plan.  Returns "" or what is wrong (the row named).
inline std::string analyse(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int64_t narrow_rows, Plan& p) {
    auto str = [](int64_t v) { return std::to_string((long long)v); };
    if (n < 1 || n > (int64_t)0x7fffffff - 2 * khtri::SLICE) return "n = " + str(n) + " out of range";
    if (nnz < 0 || nnz > (int64_t)0x7fffffff) return "nnz = " + str(nnz) + " out of range (int32 row pointers)";
    if (!indptr || !indices) return "NULL array";
    if (indptr[0] != 0 || indptr[n] != nnz) return "indptr[0] != 0 or indptr[n] != nnz";
    p = Plan();
    p.n = n;
    p.nnz = nnz;
    p.dpos.assign((size_t)n, -1);
    std::vector<int32_t> lptr((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = indptr[i], b = indptr[i + 1];
        if (a > b || b > nnz) return "indptr not ascending at row " + str(i);
        int32_t below = 0;
        for (int64_t q = a; q < b; ++q) {
            const int64_t c = indices[q];
            if (c < 0 || c >= n) return "column " + str(c) + " out of range in row " + str(i);
            if (q > a && indices[q - 1] >= c)
                return std::string(indices[q - 1] == c ? "duplicate" : "unsorted") + " column indices in row " + str(i);
            if (c == i) p.dpos[(size_t)i] = (int32_t)q;
            below += c < i;
        }
        if (p.dpos[(size_t)i] < 0) return "row " + str(i) + " has no diagonal entry";
        lptr[(size_t)i + 1] = lptr[(size_t)i] + below;
        p.longest = std::max<int64_t>(p.longest, b - a);
    }
    // the strict lower pattern through the triangular solves' analysis (a unit diagonal: the values are never looked at)
    std::vector<int32_t> lidx((size_t)lptr[(size_t)n]);
    for (int64_t i = 0; i < n; ++i)
        std::copy(indices + indptr[i], indices + p.dpos[(size_t)i], lidx.begin() + lptr[(size_t)i]);
    std::vector<double> zeros(lidx.size(), 0.0);
    khtri::Plan t;
    const std::string why = khtri::analyse(n, (int64_t)lidx.size(), lptr.data(), lidx.data(), zeros.data(), 1, true, true, narrow_rows, t);
    if (!why.empty()) return why;
    p.nlevels = t.nlevels;
    p.widest = t.widest;
    p.nslices = t.nslices;
    p.n_wide = t.n_wide;
    p.n_narrow = t.n_narrow;
    p.level.swap(t.level);
    p.order.swap(t.order);
    p.lev_ptr.swap(t.lev_ptr);
    p.lev_slice.swap(t.lev_slice);
    p.row_id.swap(t.row_id);
    p.launches.swap(t.launches);
    return "";
}

// Row i of the factorisation (Z: a holds (re, im) pairs).  The tail of row i is merged with the part of row k behind its diagonal
// by two pointers.  a is read and written through a plain pointer on purpose: in a kernel the rows k were written by earlier
// launches or by other waves of the workgroup before the last barrier.  Returns true when the finished pivot is zero or not
// finite.
template <bool Z>
KH_ILU0_HD inline bool factor_row(const int32_t* indptr, const int32_t* indices, const int32_t* dpos, int32_t i, double* a) {
    const int32_t qend = indptr[i + 1], di = dpos[i];
    for (int32_t p = indptr[i]; p < di; ++p) {
        const int32_t k = indices[p], dk = dpos[k], rend = indptr[k + 1];
        int32_t q = p + 1, r = dk + 1;
        if (!Z) {
            const double l = a[p] / a[dk];
            a[p] = l;
            while (q < qend && r < rend) {
                const int32_t cq = indices[q], cr = indices[r];
                if (cq == cr) {
                    a[q] = a[q] - l * a[r];
                    ++q;
                    ++r;
                } else if (cq < cr) ++q;
                else ++r;
            }
        } else {
            const double nx = a[2 * (int64_t)p], ny = a[2 * (int64_t)p + 1], dx = a[2 * (int64_t)dk], dy = a[2 * (int64_t)dk + 1];
            const bool big_re = fabs(dx) >= fabs(dy);
            const double rat = big_re ? dy / dx : dx / dy;
            const double scl = 1.0 / (big_re ? (dx + dy * rat) : (dy + dx * rat));
            double lx, ly;
            if (big_re) {
                lx = (nx + ny * rat) * scl;
                ly = (ny - nx * rat) * scl;
            } else {
                lx = (nx * rat + ny) * scl;
                ly = (ny * rat - nx) * scl;
            }
            a[2 * (int64_t)p] = lx;
            a[2 * (int64_t)p + 1] = ly;
            while (q < qend && r < rend) {
                const int32_t cq = indices[q], cr = indices[r];
                if (cq == cr) {
                    const double ux = a[2 * (int64_t)r], uy = a[2 * (int64_t)r + 1];
                    const double vx = a[2 * (int64_t)q], vy = a[2 * (int64_t)q + 1];
                    a[2 * (int64_t)q] = vx - (lx * ux - ly * uy);
                    a[2 * (int64_t)q + 1] = vy - (lx * uy + ly * ux);
                    ++q;
                    ++r;
                } else if (cq < cr) ++q;
                else ++r;
            }
        }
    }
    if (!Z) {
        const double d = a[di];
        return d == 0.0 || !(fabs(d) <= DBL_MAX);
    }
    const double dx = a[2 * (int64_t)di], dy = a[2 * (int64_t)di + 1];
    return (dx == 0.0 && dy == 0.0) || !(fabs(dx) <= DBL_MAX) || !(fabs(dy) <= DBL_MAX);
}

// The kernels' arithmetic on the host, walking the plan in launch order (w = 1: real, w = 2: (re, im) pairs).  Returns the
// smallest row that broke down, or -1.
inline int64_t factor_host(const Plan& p, const int32_t* indptr, const int32_t* indices, int w, double* a) {
    int64_t bad = -1;
    for (const khtri::Launch& L : p.launches)
        for (int64_t at = (int64_t)L.slice0 * khtri::SLICE; at < (int64_t)(L.slice0 + L.nslices) * khtri::SLICE; ++at) {
            const int32_t i = p.row_id[(size_t)at];
            if (i < 0) continue;
            const bool broke = w == 2 ? factor_row<true>(indptr, indices, p.dpos.data(), i, a)
                                      : factor_row<false>(indptr, indices, p.dpos.data(), i, a);
            if (broke && (bad < 0 || i < bad)) bad = i;
        }
    return bad;
}

// Greedy colouring of the graph given as a CSR pattern (the caller passes the pattern of A + A^T; a diagonal entry is ignored):
// rows in ascending order, each takes the smallest colour no already-coloured neighbour holds.  The multicolour ordering is the
// stable sort of the rows by colour.  Returns "" or what is wrong.
inline std::string multicolor(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int32_t* color,
                              int64_t* ncolors) {
    auto str = [](int64_t v) { return std::to_string((long long)v); };
    if (n < 1 || n > (int64_t)0x7fffffff) return "n = " + str(n) + " out of range";
    if (nnz < 0 || nnz > (int64_t)0x7fffffff) return "nnz = " + str(nnz) + " out of range (int32 row pointers)";
    if (!indptr || (nnz > 0 && !indices) || !color || !ncolors) return "NULL array";
    if (indptr[0] != 0 || indptr[n] != nnz) return "indptr[0] != 0 or indptr[n] != nnz";
    std::vector<int32_t> seen;         // seen[c] == i: a neighbour of row i holds colour c
    int32_t nc = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = indptr[i], b = indptr[i + 1];
        if (a > b || b > nnz) return "indptr not ascending at row " + str(i);
        for (int64_t q = a; q < b; ++q) {
            const int64_t c = indices[q];
            if (c < 0 || c >= n) return "column " + str(c) + " out of range in row " + str(i);
            if (c < i) seen[(size_t)color[c]] = (int32_t)i;
        }
        int32_t mine = 0;
        while (mine < nc && seen[(size_t)mine] == (int32_t)i) ++mine;
        if (mine == nc) {
            seen.push_back(-1);
            nc += 1;
        }
        color[i] = mine;
    }
    *ncolors = nc;
    return "";
}

}  // namespace khilu0
