// Stand-alone check of the persistent ILU(0) preconditioner's host analysis and row arithmetic (krypy_amd/csrc/ilu0p.h) - TEST
// INFRASTRUCTURE ONLY.  tests/test_ilu0p_host.py compiles this file with the host compiler and -fsanitize=address,undefined and runs
// it on the CPU: ilu0p.h is plain C++ without a HIP call.  Every case, ordering and narrow_rows in {0, 64, 1024} prints one line
//     <name>/<ordering>/<narrow_rows> levels=<..> levels_l=<..> levels_u=<..> wide=<..> narrow=<..> solve_wide=<..> solve_narrow=<..>
//         pattern=<ok|BAD> plan=<ok|BAD> images=<ok|BAD> solve=<ok|BAD>
// pattern: the pattern of Ap = A[perm][:, perm] and src against a plain loop over a sorted map;  plan: dpos and the factorisation's
// plan against khilu0::analyse on Ap;  images: for real and complex values, the images of L and U filled through the map against
// the vals / diag khtri::analyse produces for the split factors, bit for bit (and the plans' index arrays);  solve: the host walk of
// both stages in launch order, with gather and scatter, out of place and in place, against the row-by-row substitution, bit for
// bit.  Every refused input prints "<name> refused: <why>".
#include <stdio.h>
#include <string.h>

#include <map>
#include <utility>

#include "ilu0p.h"

struct Csr {
    int64_t n = 0;
    std::vector<int32_t> indptr, indices;
    std::vector<double> data;
};
typedef std::map<std::pair<int32_t, int32_t>, double> Entries;

static uint64_t g_state = 12345;
static double rnd() {      // uniform in [-1, 1)
    g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)((g_state >> 11) & ((1ULL << 52) - 1)) / (double)(1ULL << 51) - 1.0;
}
static int32_t rndint(int32_t n) { return (int32_t)((rnd() + 1.0) * 0.5 * n) % n; }

static Csr csr(int64_t n, const Entries& e) {
    Csr A;
    A.n = n;
    A.indptr.assign((size_t)n + 1, 0);
    for (const auto& kv : e) {
        A.indptr[(size_t)kv.first.first + 1] += 1;
        A.indices.push_back(kv.first.second);
        A.data.push_back(kv.second);
    }
    for (int64_t i = 0; i < n; ++i) A.indptr[(size_t)i + 1] += A.indptr[(size_t)i];
    return A;
}

static bool same(const double* a, const double* b, size_t count) { return count == 0 || memcmp(a, b, count * sizeof(double)) == 0; }
template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// (re, im) of the quotient as NumPy rounds it (Smith's formula, ratio and scale once)
static void zdiv(double ax, double ay, double dx, double dy, double* zx, double* zy) {
    if (fabs(dx) >= fabs(dy)) {
        const double rat = dy / dx, scl = 1.0 / (dx + dy * rat);
        *zx = (ax + ay * rat) * scl;
        *zy = (ay - ax * rat) * scl;
    } else {
        const double rat = dx / dy, scl = 1.0 / (dy + dx * rat);
        *zx = (ax * rat + ay) * scl;
        *zy = (ay * rat - ax) * scl;
    }
}

// x[perm[i]] = (U^{-1} L^{-1} b')_i, b'_i = b[perm[i]]: row by row on the CSR arrays of Ap with the factored values a
static void substitute(const khilu0p::Plan& p, const std::vector<int32_t>& perm, int w, const std::vector<double>& a,
                       const std::vector<double>& b, std::vector<double>& x) {
    const int64_t n = p.n;
    std::vector<double> z((size_t)n * w);
    for (int64_t i = 0; i < n; ++i) {
        double sx = b[(size_t)perm[(size_t)i] * w], sy = w == 2 ? b[(size_t)perm[(size_t)i] * 2 + 1] : 0.0;
        for (int32_t q = p.indptr[(size_t)i]; q < p.dpos[(size_t)i]; ++q) {
            const size_t c = (size_t)p.indices[(size_t)q];
            if (w == 1) sx = sx - a[(size_t)q] * z[c];
            else {
                const double ax = a[2 * (size_t)q], ay = a[2 * (size_t)q + 1], bx = z[2 * c], by = z[2 * c + 1];
                sx = sx - (ax * bx - ay * by);
                sy = sy - (ax * by + ay * bx);
            }
        }
        z[(size_t)i * w] = sx;
        if (w == 2) z[(size_t)i * 2 + 1] = sy;
    }
    for (int64_t i = n - 1; i >= 0; --i) {
        double sx = z[(size_t)i * w], sy = w == 2 ? z[(size_t)i * 2 + 1] : 0.0;
        const int32_t d = p.dpos[(size_t)i];
        for (int32_t q = d + 1; q < p.indptr[(size_t)i + 1]; ++q) {
            const size_t c = (size_t)p.indices[(size_t)q];
            if (w == 1) sx = sx - a[(size_t)q] * z[c];
            else {
                const double ax = a[2 * (size_t)q], ay = a[2 * (size_t)q + 1], bx = z[2 * c], by = z[2 * c + 1];
                sx = sx - (ax * bx - ay * by);
                sy = sy - (ax * by + ay * bx);
            }
        }
        if (w == 1) sx = sx / a[(size_t)d];
        else zdiv(sx, sy, a[2 * (size_t)d], a[2 * (size_t)d + 1], &sx, &sy);
        z[(size_t)i * w] = sx;
        if (w == 2) z[(size_t)i * 2 + 1] = sy;
        for (int c = 0; c < w; ++c) x[(size_t)perm[(size_t)i] * w + c] = z[(size_t)i * w + c];
    }
}

static int run(const char* name, const char* ordering, const Csr& A, const std::vector<int32_t>* perm) {
    int badcases = 0;
    const int64_t n = A.n, nnz = (int64_t)A.indices.size();
    for (int64_t narrow : {(int64_t)0, (int64_t)64, (int64_t)1024}) {
        khilu0p::Plan p;
        const std::string why = khilu0p::analyse(n, nnz, A.indptr.data(), A.indices.data(), perm ? perm->data() : nullptr, narrow, p);
        if (!why.empty()) {
            printf("%s refused: %s\n", name, why.c_str());
            return 0;
        }
        std::vector<int32_t> pm((size_t)n), inv((size_t)n);
        for (int64_t r = 0; r < n; ++r) pm[(size_t)r] = perm ? (*perm)[(size_t)r] : (int32_t)r;
        for (int64_t r = 0; r < n; ++r) inv[(size_t)pm[(size_t)r]] = (int32_t)r;
        // ---- the permuted pattern and src: a sorted map per row ----
        bool pattern = p.permuted == (perm != nullptr) && p.indptr[0] == 0 && p.indptr[(size_t)n] == nnz;
        for (int64_t r = 0; r < n && pattern; ++r) {
            std::map<int32_t, int32_t> row;
            for (int32_t q = A.indptr[(size_t)pm[(size_t)r]]; q < A.indptr[(size_t)pm[(size_t)r] + 1]; ++q) row[inv[(size_t)A.indices[(size_t)q]]] = q;
            int32_t at = p.indptr[(size_t)r];
            pattern = pattern && p.indptr[(size_t)r + 1] - at == (int32_t)row.size();
            for (const auto& kv : row) {
                pattern = pattern && p.indices[(size_t)at] == kv.first && p.src[(size_t)at] == kv.second;
                at += 1;
            }
            pattern = pattern && p.indices[(size_t)p.dpos[(size_t)r]] == r;
        }
        // ---- the factorisation's plan: khilu0::analyse on Ap ----
        khilu0::Plan k;
        bool plan = khilu0::analyse(n, nnz, p.indptr.data(), p.indices.data(), narrow, k).empty();
        plan = plan && same(k.dpos, p.dpos) && same(k.row_id, p.L.row_id) && same(k.lev_slice, p.L.lev_slice) && same(k.order, p.L.order) &&
               k.nlevels == p.L.nlevels && k.n_wide == p.L.n_wide && k.n_narrow == p.L.n_narrow && k.widest == p.L.widest &&
               k.longest == p.longest && k.launches.size() == p.L.launches.size();
        for (size_t l = 0; plan && l < k.launches.size(); ++l) {
            const khtri::Launch &x = k.launches[l], &y = p.L.launches[l];
            plan = x.narrow == y.narrow && x.lev0 == y.lev0 && x.nlev == y.nlev && x.slice0 == y.slice0 && x.nslices == y.nslices &&
                   x.threads == y.threads;
        }
        bool images = true, solve = true;
        for (int w = 1; w <= 2; ++w) {
            // values in the CALLER's positions; complex: a seeded imaginary part, + 0.5 i on the diagonal
            std::vector<double> data((size_t)nnz * w), a((size_t)nnz * w), a2;
            for (int64_t i = 0; i < n; ++i)
                for (int32_t q = A.indptr[(size_t)i]; q < A.indptr[(size_t)i + 1]; ++q) {
                    data[(size_t)q * w] = A.data[(size_t)q];
                    if (w == 2) data[(size_t)q * 2 + 1] = 0.2 * A.data[(size_t)q] * rnd() + (A.indices[(size_t)q] == i ? 0.5 : 0.0);
                }
            khilu0p::gather_host(p, w, data.data(), a.data());
            for (int64_t q = 0; q < nnz; ++q) images = images && same(&a[(size_t)q * w], &data[(size_t)p.src[(size_t)q] * w], (size_t)w);
            a2 = a;
            const int64_t bad = khilu0p::factor_host(p, w, a.data());
            images = images && bad == -1 && bad == khilu0::factor_host(k, p.indptr.data(), p.indices.data(), w, a2.data()) && same(a, a2);
            // the images through the map ...
            std::vector<double> img((size_t)p.total() * w, 0.0);
            for (int64_t e = p.off_d(); e < p.total(); ++e) img[(size_t)e * w] = 1.0;
            khilu0p::fill_host(p, w, a.data(), img.data());
            // ... against khtri::analyse on the split factors with their values
            Csr L, U;
            L.indptr.assign((size_t)n + 1, 0);
            U.indptr.assign((size_t)n + 1, 0);
            for (int64_t r = 0; r < n; ++r) {
                for (int32_t q = p.indptr[(size_t)r]; q < p.indptr[(size_t)r + 1]; ++q) {
                    Csr& T = q < p.dpos[(size_t)r] ? L : U;
                    T.indices.push_back(p.indices[(size_t)q]);
                    for (int c = 0; c < w; ++c) T.data.push_back(a[(size_t)q * w + c]);
                }
                L.indptr[(size_t)r + 1] = (int32_t)L.indices.size();
                U.indptr[(size_t)r + 1] = (int32_t)U.indices.size();
            }
            khtri::Plan tl, tu;
            images = images && khtri::analyse(n, (int64_t)L.indices.size(), L.indptr.data(), L.indices.data(), L.data.data(), w, true, true, narrow, tl).empty();
            images = images && khtri::analyse(n, (int64_t)U.indices.size(), U.indptr.data(), U.indices.data(), U.data.data(), w, false, false, narrow, tu).empty();
            images = images && tl.slots == p.L.slots && tu.slots == p.U.slots && tu.nslices == p.U.nslices &&
                     (int64_t)tl.vals.size() == p.L.slots * w && (int64_t)tu.diag.size() == p.U.nslices * khtri::SLICE * w;
            if (images) {
                images = same(img.data(), tl.vals.data(), tl.vals.size()) && same(img.data() + p.off_u() * w, tu.vals.data(), tu.vals.size()) &&
                         same(img.data() + p.off_d() * w, tu.diag.data(), tu.diag.size());
                images = images && same(tl.cols, p.L.cols) && same(tl.row_id, p.L.row_id) && same(tl.row_len, p.L.row_len) &&
                         same(tl.slice_base, p.L.slice_base) && same(tl.slice_slots, p.L.slice_slots) && same(tl.lev_slice, p.L.lev_slice);
                images = images && same(tu.cols, p.U.cols) && same(tu.row_id, p.U.row_id) && same(tu.row_len, p.U.row_len) &&
                         same(tu.slice_base, p.U.slice_base) && same(tu.slice_slots, p.U.slice_slots) && same(tu.lev_slice, p.U.lev_slice) &&
                         tu.launches.size() == p.U.launches.size() && tl.launches.size() == p.L.launches.size();
            }
            // ---- both stages in launch order against the row-by-row substitution ----
            std::vector<double> b((size_t)n * w), want((size_t)n * w, 0.0), y((size_t)n * w, -7.0), t((size_t)n * w, -9.0);
            for (double& v : b) v = rnd();
            substitute(p, pm, w, a, b, want);
            khilu0p::solve_host(p, w, img.data(), b.data(), t.data(), y.data());
            solve = solve && same(y, want);
            khilu0p::solve_host(p, w, img.data(), b.data(), t.data(), b.data());      // in place
            solve = solve && same(b, want);
        }
        printf("%s/%s/%lld levels=%lld levels_l=%lld levels_u=%lld wide=%lld narrow=%lld solve_wide=%lld solve_narrow=%lld pattern=%s plan=%s "
               "images=%s solve=%s\n", name, ordering, (long long)narrow, (long long)k.nlevels, (long long)p.L.nlevels, (long long)p.U.nlevels,
               (long long)p.L.n_wide, (long long)p.L.n_narrow, (long long)(p.L.n_wide + p.U.n_wide), (long long)(p.L.n_narrow + p.U.n_narrow),
               pattern ? "ok" : "BAD", plan ? "ok" : "BAD", images ? "ok" : "BAD", solve ? "ok" : "BAD");
        badcases += (pattern && plan && images && solve) ? 0 : 1;
    }
    return badcases;
}

static void refused(const char* name, const Csr& A, const std::vector<int32_t>* perm) {
    khilu0p::Plan p;
    const std::string why = khilu0p::analyse(A.n, (int64_t)A.indices.size(), A.indptr.data(), A.indices.data(), perm ? perm->data() : nullptr, 1024, p);
    printf("%s %s: %s\n", name, why.empty() ? "ACCEPTED" : "refused", why.c_str());
}

static std::vector<int32_t> random_permutation(int32_t n) {
    std::vector<int32_t> p((size_t)n);
    for (int32_t i = 0; i < n; ++i) p[(size_t)i] = i;
    for (int32_t i = n - 1; i > 0; --i) std::swap(p[(size_t)i], p[(size_t)rndint(i + 1)]);
    return p;
}

// the rows sorted by the colours of the greedy colouring of A + A^T
static std::vector<int32_t> multicolour(int64_t n, const Entries& e) {
    Entries sym = e;
    for (const auto& kv : e) sym[{kv.first.second, kv.first.first}] = 1.0;
    const Csr G = csr(n, sym);
    std::vector<int32_t> color((size_t)n, -1), perm;
    int64_t nc = 0;
    if (!khilu0::multicolor(n, (int64_t)G.indices.size(), G.indptr.data(), G.indices.data(), color.data(), &nc).empty()) return perm;
    for (int32_t c = 0; c < nc; ++c)
        for (int64_t i = 0; i < n; ++i)
            if (color[(size_t)i] == c) perm.push_back((int32_t)i);
    return perm;
}

// five-point (with upwind convection inside the grid lines) or nine-point stencil on nx x ny, point (ix, iy) has index ix * ny + iy
static Entries stencil(int nx, int ny, bool nine, double wind) {
    Entries e;
    for (int ix = 0; ix < nx; ++ix)
        for (int iy = 0; iy < ny; ++iy) {
            const int32_t p = ix * ny + iy;
            e[{p, p}] = (nine ? 8.0 : 4.0) + wind + 0.001 * iy;
            for (int dx = -1; dx <= 1; ++dx)
                for (int dy = -1; dy <= 1; ++dy) {
                    if ((dx == 0 && dy == 0) || (!nine && dx != 0 && dy != 0)) continue;
                    const int jx = ix + dx, jy = iy + dy;
                    if (jx < 0 || jx >= nx || jy < 0 || jy >= ny) continue;
                    e[{p, jx * ny + jy}] = -1.0 - (dx == 0 && dy == -1 ? wind : 0.0) - 0.0001 * (ix + 2 * dy);
                }
        }
    return e;
}

// tridiagonal plus one random off-band entry per row, strictly diagonally dominant
static Entries band_plus_one(int32_t n) {
    Entries e;
    for (int32_t i = 0; i < n; ++i) {
        e[{i, i}] = 3.5 + 0.01 * (i % 17);
        if (i > 0) e[{i, i - 1}] = -1.0 + 0.1 * rnd();
        if (i + 1 < n) e[{i, i + 1}] = -1.0 + 0.1 * rnd();
        const int32_t j = rndint(n);
        if (j < i - 1 || j > i + 1) e[{i, j}] = 0.5 * rnd();
    }
    return e;
}

// about `per_row` entries per row at random columns (unsymmetric pattern), the diagonal dominant
static Entries random_pattern(int32_t n, int per_row) {
    Entries e;
    for (int32_t i = 0; i < n; ++i) {
        for (int k = 0; k + 1 < per_row; ++k) {
            const int32_t j = rndint(n);
            if (j != i) e[{i, j}] = rnd();
        }
        e[{i, i}] = per_row + 1.0 + rnd();
    }
    return e;
}

int main() {
    int bad = 0;
    char name[64];
    for (int32_t n : {1, 2, 63, 64, 65, 129, 4097}) {
        const Entries e = band_plus_one(n);
        const std::vector<int32_t> perm = random_permutation(n);
        snprintf(name, sizeof name, "band%d", (int)n);
        bad += run(name, "natural", csr(n, e), nullptr);
        bad += run(name, "random", csr(n, e), &perm);
    }
    {
        const Entries e = random_pattern(20001, 7);
        const std::vector<int32_t> perm = multicolour(20001, e);
        bad += run("random20001", "natural", csr(20001, e), nullptr);
        bad += run("random20001", "multicolor", csr(20001, e), &perm);
    }
    {
        const Entries e = stencil(37, 23, false, 0.8);
        const std::vector<int32_t> perm = multicolour(37 * 23, e);
        bad += run("convection", "natural", csr(37 * 23, e), nullptr);
        bad += run("convection", "multicolor", csr(37 * 23, e), &perm);
        const Entries e9 = stencil(37, 23, true, 0.0);
        const std::vector<int32_t> perm9 = multicolour(37 * 23, e9);
        bad += run("nine_point", "multicolor", csr(37 * 23, e9), &perm9);
    }
    {   // refused inputs
        const Entries e = band_plus_one(300);
        const Csr A = csr(300, e);
        std::vector<int32_t> twice = random_permutation(300), outside = twice;
        twice[17] = twice[3];
        outside[200] = 300;
        refused("perm_duplicate", A, &twice);
        refused("perm_out_of_range", A, &outside);
        Csr B = A, C = A;
        C.indices[(size_t)C.indptr[1] + 1] = C.indices[(size_t)C.indptr[1]];
        refused("duplicate", C, nullptr);
        std::swap(B.indices[(size_t)B.indptr[1]], B.indices[(size_t)B.indptr[1] + 1]);
        refused("unsorted", B, nullptr);
        Entries g = e;
        g.erase({7, 7});
        refused("missing_diagonal", csr(300, g), nullptr);
    }
    return bad ? 1 : 0;
}
