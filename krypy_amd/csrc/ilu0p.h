// Persistent ILU(0) preconditioner: everything that depends on the PATTERN alone - the HOST analysis of kh_ilu0_create - and the
// arithmetic of one row of the two permuted triangular stages (ilu0p.hip holds the kernels and the C entry points).  Plain C++, no
// HIP call: the header compiles alone (tests/support/ilu0p_main.cpp builds it with the host sanitizers and runs it on the CPU).
//
// For a CSR pattern of A with sorted, duplicate-free indices and a structural diagonal in every row, and an ordering perm (new row
// r = old row perm[r]; none: the natural order):
//   Ap = A[perm][:, perm]   its pattern with sorted indices; src[q] = the position in the CALLER's value array of entry q of Ap
//                           (stored zeros stay in the pattern); dpos[r] = the position of the diagonal of row r.
//   L, U                    the khtri plans of the two factors - L: the strict lower pattern of Ap, unit diagonal; U: the diagonal and
//                           what is right of it - exactly what khtri::analyse makes of them (the values are filled on the device).
//                           The plan of L IS the plan of the factorisation: khilu0::analyse passes the same strict lower pattern to
//                           the same function, so row_id, lev_slice and the launches serve both.
//   fmap                    ONE map for ONE device array img = [ slots of L | slots of U | one diagonal per lane of U ]: the position
//                           in Ap's value array an element takes its value from, -1: a padding slot or a lane without a row, never
//                           written (it keeps 0, the diagonal 1, from the creation).
// The solve: Y[perm[i]] = (U^{-1} L^{-1} b')_i with b'_i = X[perm[i]].  The L stage reads X[perm[row]] and writes t[row]; the U stage
// runs in place on the scratch column t (its own right-hand side t[row], operands t[col] of earlier levels) and stores every
// finished entry to t[row] AND to Y[perm[row]].  Per row the arithmetic is that of tri.hip, to the bit: ascending column order,
// product and difference rounded separately, Smith's quotient for complex.
#pragma once
#include "ilu0.h"

namespace khilu0p {

// one sliced-ELL image: pointers into host vectors or device memory
struct Tri {
    const double* vals;
    const double* diag;        // U only
    const int32_t* cols;
    const int64_t* slice_base;
    const int32_t* slice_slots;
    const int32_t* row_id;
    const int32_t* row_len;
};

// Lane `lane` of slice s of one stage (Z: (re, im) pairs; P: through perm; UPPER: the U stage).  x is read in the L stage only, y
// written in the U stage only; t is read through a plain pointer on purpose: other waves of the workgroup wrote those entries
// before the last barrier.
template <bool Z, bool P, bool UPPER>
KH_ILU0_HD inline void solve_lane(const Tri& T, const int32_t* perm, int64_t s, int lane, const double* x, double* t, double* y) {
    const int64_t at = s * khtri::SLICE + lane;
    const int32_t row = T.row_id[at];
    const int32_t len = row >= 0 ? T.row_len[at] : 0;
    const int32_t ns = T.slice_slots[s];          // the same for the 64 lanes of a slice
    const int64_t base = T.slice_base[s];
    const int32_t out = row >= 0 ? (P ? perm[row] : row) : 0;
    if (!Z) {
        double acc = row >= 0 ? (UPPER ? t[row] : x[out]) : 0.0;
        for (int32_t k = 0; k < ns; ++k) {
            if (k < len) {
                const int64_t q = base + (int64_t)k * khtri::SLICE + lane;
                acc = acc - T.vals[q] * t[T.cols[q]];
            }
        }
        if (row >= 0) {
            if (UPPER) {
                acc = acc / T.diag[at];
                y[out] = acc;
            }
            t[row] = acc;
        }
    } else {
        double accx = 0.0, accy = 0.0;
        if (row >= 0) {
            const double* b = UPPER ? t + 2 * (int64_t)row : x + 2 * (int64_t)out;
            accx = b[0];
            accy = b[1];
        }
        for (int32_t k = 0; k < ns; ++k) {
            if (k < len) {
                const int64_t q = base + (int64_t)k * khtri::SLICE + lane;
                const int64_t c = T.cols[q];
                const double ax = T.vals[2 * q], ay = T.vals[2 * q + 1], bx = t[2 * c], by = t[2 * c + 1];
                accx = accx - (ax * bx - ay * by);
                accy = accy - (ax * by + ay * bx);
            }
        }
        if (row >= 0) {
            if (UPPER) {
                const double dx = T.diag[2 * at], dy = T.diag[2 * at + 1];
                const bool big_re = fabs(dx) >= fabs(dy);
                const double rat = big_re ? dy / dx : dx / dy;
                const double scl = 1.0 / (big_re ? (dx + dy * rat) : (dy + dx * rat));
                double zx, zy;
                if (big_re) {
                    zx = (accx + accy * rat) * scl;
                    zy = (accy - accx * rat) * scl;
                } else {
                    zx = (accx * rat + accy) * scl;
                    zy = (accy * rat - accx) * scl;
                }
                accx = zx;
                accy = zy;
                y[2 * (int64_t)out] = accx;
                y[2 * (int64_t)out + 1] = accy;
            }
            t[2 * (int64_t)row] = accx;
            t[2 * (int64_t)row + 1] = accy;
        }
    }
}

struct Plan {
    int64_t n = 0, nnz = 0, longest = 0;
    bool permuted = false;
    std::vector<int32_t> perm;                     // [n], empty in the natural order
    std::vector<int32_t> indptr, indices, src;     // Ap; src: [nnz] into the caller's value array
    std::vector<int32_t> dpos;                     // [n]
    khtri::Plan L, U;                              // vals released, U.diag = 1: the device fills them through fmap
    std::vector<int32_t> fmap;                     // [total()]
    int64_t off_u() const { return L.slots; }
    int64_t off_d() const { return L.slots + U.slots; }
    int64_t total() const { return L.slots + U.slots + U.nslices * khtri::SLICE; }
    Tri tri_l(const double* img, int w) const {
        return Tri{img, nullptr, L.cols.data(), L.slice_base.data(), L.slice_slots.data(), L.row_id.data(), L.row_len.data()};
    }
    Tri tri_u(const double* img, int w) const {
        return Tri{img + off_u() * w, img + off_d() * w, U.cols.data(), U.slice_base.data(), U.slice_slots.data(), U.row_id.data(),
                   U.row_len.data()};
    }
};

// Checks pattern and ordering (the offending row named, in the caller's numbering) and builds everything above.  Returns "" or
// what is wrong.
inline std::string analyse(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const int32_t* perm,
                           int64_t narrow_rows, Plan& p) {
    auto str = [](int64_t v) { return std::to_string((long long)v); };
    if (n < 1 || n > (int64_t)0x7fffffff - 2 * khtri::SLICE) return "n = " + str(n) + " out of range";
    if (nnz < 0 || nnz > (int64_t)0x7fffffff) return "nnz = " + str(nnz) + " out of range (int32 row pointers)";
    if (!indptr || !indices) return "NULL array";
    if (indptr[0] != 0 || indptr[n] != nnz) return "indptr[0] != 0 or indptr[n] != nnz";
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = indptr[i], b = indptr[i + 1];
        if (a > b || b > nnz) return "indptr not ascending at row " + str(i);
        bool diag = false;
        for (int64_t q = a; q < b; ++q) {
            const int64_t c = indices[q];
            if (c < 0 || c >= n) return "column " + str(c) + " out of range in row " + str(i);
            if (q > a && indices[q - 1] >= c)
                return std::string(indices[q - 1] == c ? "duplicate" : "unsorted") + " column indices in row " + str(i);
            diag = diag || c == i;
        }
        if (!diag) return "row " + str(i) + " has no diagonal entry";
    }
    p = Plan();
    p.n = n;
    p.nnz = nnz;
    p.permuted = perm != nullptr;
    p.indptr.assign((size_t)n + 1, 0);
    p.indices.resize((size_t)nnz);
    p.src.resize((size_t)nnz);
    if (perm) {
        std::vector<int32_t> inv((size_t)n, -1);
        for (int64_t r = 0; r < n; ++r) {
            const int64_t o = perm[r];
            if (o < 0 || o >= n || inv[(size_t)o] >= 0) return "perm is not a permutation of 0 .. n-1 (entry " + str(r) + ")";
            inv[(size_t)o] = (int32_t)r;
        }
        p.perm.assign(perm, perm + n);
        std::vector<std::pair<int32_t, int32_t>> row;      // (new column, position in A)
        for (int64_t r = 0; r < n; ++r) {
            const int64_t o = perm[r];
            row.clear();
            for (int32_t q = indptr[o]; q < indptr[o + 1]; ++q) row.push_back({inv[(size_t)indices[q]], q});
            std::sort(row.begin(), row.end());
            int64_t at = p.indptr[(size_t)r];
            for (const auto& e : row) {
                p.indices[(size_t)at] = e.first;
                p.src[(size_t)at++] = e.second;
            }
            p.indptr[(size_t)r + 1] = (int32_t)at;
        }
    } else {
        std::copy(indptr, indptr + n + 1, p.indptr.begin());
        std::copy(indices, indices + nnz, p.indices.begin());
        for (int64_t q = 0; q < nnz; ++q) p.src[(size_t)q] = (int32_t)q;
    }
    // dpos and the two triangles of Ap, each with the positions its entries have in Ap
    p.dpos.assign((size_t)n, -1);
    std::vector<int32_t> lptr((size_t)n + 1, 0), uptr((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
        int32_t d = p.indptr[(size_t)r];
        while (p.indices[(size_t)d] != r) ++d;             // present: the diagonal of row perm[r] of A
        p.dpos[(size_t)r] = d;
        lptr[(size_t)r + 1] = lptr[(size_t)r] + (d - p.indptr[(size_t)r]);
        uptr[(size_t)r + 1] = uptr[(size_t)r] + (p.indptr[(size_t)r + 1] - d);
        p.longest = std::max<int64_t>(p.longest, p.indptr[(size_t)r + 1] - p.indptr[(size_t)r]);
    }
    std::vector<int32_t> lidx((size_t)lptr[(size_t)n]), lpos(lidx.size()), uidx((size_t)uptr[(size_t)n]), upos(uidx.size());
    for (int64_t r = 0; r < n; ++r) {
        int32_t l = lptr[(size_t)r], u = uptr[(size_t)r];
        for (int32_t q = p.indptr[(size_t)r]; q < p.indptr[(size_t)r + 1]; ++q) {
            if (q < p.dpos[(size_t)r]) {
                lidx[(size_t)l] = p.indices[(size_t)q];
                lpos[(size_t)l++] = q;
            } else {
                uidx[(size_t)u] = p.indices[(size_t)q];
                upos[(size_t)u++] = q;
            }
        }
    }
    {   // the plans: values that pass khtri's checks (a unit diagonal never looks; U needs non-zero diagonals), then released
        std::vector<double> ones(std::max(lidx.size(), uidx.size()), 1.0);
        std::string why = khtri::analyse(n, (int64_t)lidx.size(), lptr.data(), lidx.data(), ones.data(), 1, true, true, narrow_rows, p.L);
        if (!why.empty()) return why;
        why = khtri::analyse(n, (int64_t)uidx.size(), uptr.data(), uidx.data(), ones.data(), 1, false, false, narrow_rows, p.U);
        if (!why.empty()) return why;
        std::vector<double>().swap(p.L.vals);
        std::vector<double>().swap(p.U.vals);
    }
    // the fill map, slot by slot as khtri::analyse places the off-diagonal entries of a row (ascending column order)
    p.fmap.assign((size_t)p.total(), -1);
    auto image = [&](const khtri::Plan& t, const std::vector<int32_t>& ptr, const std::vector<int32_t>& idx,
                     const std::vector<int32_t>& pos, int64_t off, bool with_diag) {
        for (int64_t s = 0; s < t.nslices; ++s)
            for (int lane = 0; lane < khtri::SLICE; ++lane) {
                const int32_t i = t.row_id[(size_t)s * khtri::SLICE + lane];
                if (i < 0) continue;
                int64_t k = 0;
                for (int32_t q = ptr[(size_t)i]; q < ptr[(size_t)i + 1]; ++q) {
                    if (idx[(size_t)q] == i) {
                        if (with_diag) p.fmap[(size_t)(p.off_d() + s * khtri::SLICE + lane)] = pos[(size_t)q];
                        continue;
                    }
                    p.fmap[(size_t)(off + t.slice_base[(size_t)s] + k * khtri::SLICE + lane)] = pos[(size_t)q];
                    k += 1;
                }
            }
    };
    image(p.L, lptr, lidx, lpos, 0, false);
    image(p.U, uptr, uidx, upos, p.off_u(), true);
    return "";
}

// What the gather kernel does: a[q] = staged[src[q]].
inline void gather_host(const Plan& p, int w, const double* staged, double* a) {
    for (int64_t q = 0; q < p.nnz; ++q)
        for (int c = 0; c < w; ++c) a[q * w + c] = staged[(int64_t)p.src[(size_t)q] * w + c];
}

// The factorisation on the host, walking the plan of L in launch order (khilu0::factor_host on the shared plan).  Returns the
// smallest row of Ap that broke down, or -1.
inline int64_t factor_host(const Plan& p, int w, double* a) {
    int64_t bad = -1;
    for (const khtri::Launch& L : p.L.launches)
        for (int64_t at = (int64_t)L.slice0 * khtri::SLICE; at < (int64_t)(L.slice0 + L.nslices) * khtri::SLICE; ++at) {
            const int32_t i = p.L.row_id[(size_t)at];
            if (i < 0) continue;
            const bool broke = w == 2 ? khilu0::factor_row<true>(p.indptr.data(), p.indices.data(), p.dpos.data(), i, a)
                                      : khilu0::factor_row<false>(p.indptr.data(), p.indices.data(), p.dpos.data(), i, a);
            if (broke && (bad < 0 || i < bad)) bad = i;
        }
    return bad;
}

// What the fill kernel does.  img: [total() * w], 0 in the slots and 1 in the diagonals before the first fill.
inline void fill_host(const Plan& p, int w, const double* a, double* img) {
    for (int64_t e = 0; e < p.total(); ++e) {
        const int32_t q = p.fmap[(size_t)e];
        if (q >= 0)
            for (int c = 0; c < w; ++c) img[e * w + c] = a[(int64_t)q * w + c];
    }
}

// The two stages on the host, walking both plans in launch order with gather and scatter (t: the scratch column; x may be y).
inline void solve_host(const Plan& p, int w, const double* img, const double* x, double* t, double* y) {
    const Tri tl = p.tri_l(img, w), tu = p.tri_u(img, w);
    const int32_t* perm = p.permuted ? p.perm.data() : nullptr;
    for (int stage = 0; stage < 2; ++stage) {
        const khtri::Plan& t3 = stage ? p.U : p.L;
        for (const khtri::Launch& L : t3.launches)
            for (int64_t s = L.slice0; s < (int64_t)L.slice0 + L.nslices; ++s)
                for (int lane = 0; lane < khtri::SLICE; ++lane) {
                    if (w == 2) {
                        if (perm) stage ? solve_lane<true, true, true>(tu, perm, s, lane, x, t, y) : solve_lane<true, true, false>(tl, perm, s, lane, x, t, y);
                        else stage ? solve_lane<true, false, true>(tu, perm, s, lane, x, t, y) : solve_lane<true, false, false>(tl, perm, s, lane, x, t, y);
                    } else {
                        if (perm) stage ? solve_lane<false, true, true>(tu, perm, s, lane, x, t, y) : solve_lane<false, true, false>(tl, perm, s, lane, x, t, y);
                        else stage ? solve_lane<false, false, true>(tu, perm, s, lane, x, t, y) : solve_lane<false, false, false>(tl, perm, s, lane, x, t, y);
                    }
                }
    }
}

}  // namespace khilu0p
