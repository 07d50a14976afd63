// Stand-alone check of the ILU(0) analysis, its host arithmetic and the greedy colouring (krypy_amd/csrc/ilu0.h) - TEST
// INFRASTRUCTURE ONLY.  tests/test_ilu0_host.py compiles this file with the host compiler and -fsanitize=address,undefined and runs
// it on the CPU: ilu0.h is plain C++ without a HIP call.  Every case and every narrow_rows in {0, 64, 1024} prints one line
//     <name>/<narrow_rows> levels=<..> widest=<..> longest=<..> wide=<..> narrow=<..> bad=<first broken row> factor=<ok|BAD>
// where factor=ok says: factor_host (the plan walked in launch order, real and complex values) gave the bits of the plain
// row-by-row loop written out below, every row sits in the plan exactly once and the launches cover the levels in order.  Every
// colouring prints "<name> colors=<..> valid=<ok|BAD> order <rows sorted by colour>", every refused input "<name> refused: <why>".
#include <stdio.h>
#include <string.h>

#include <map>
#include <utility>

#include "ilu0.h"

struct Csr {
    int64_t n = 0;
    std::vector<int32_t> indptr, indices;
    std::vector<double> data;
};
typedef std::map<std::pair<int32_t, int32_t>, double> Entries;

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

// P A P^T for the ordering perm (new row r = old row perm[r])
static Entries permuted(const Entries& e, const std::vector<int32_t>& perm) {
    std::vector<int32_t> inv(perm.size());
    for (size_t r = 0; r < perm.size(); ++r) inv[(size_t)perm[r]] = (int32_t)r;
    Entries out;
    for (const auto& kv : e) out[{inv[(size_t)kv.first.first], inv[(size_t)kv.first.second]}] = kv.second;
    return out;
}

static Entries symmetrised(const Entries& e) {
    Entries out = e;
    for (const auto& kv : e) out[{kv.first.second, kv.first.first}] = 1.0;
    return out;
}

// five-point (nine = false) or nine-point stencil on nx x ny, point (ix, iy) has index ix * ny + iy; wind: upwind convection
// inside the grid lines
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

// the plain loop, row by row, every partner entry looked up by column (no merge, no plan).  Returns the first broken row.
static int64_t plain(const Csr& A, int w, std::vector<double>& a) {
    const int64_t n = A.n;
    std::vector<int32_t> dpos((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t q = A.indptr[(size_t)i]; q < A.indptr[(size_t)i + 1]; ++q)
            if (A.indices[(size_t)q] == i) dpos[(size_t)i] = q;
    int64_t bad = -1;
    for (int64_t i = 0; i < n; ++i) {
        for (int32_t p = A.indptr[(size_t)i]; p < A.indptr[(size_t)i + 1] && A.indices[(size_t)p] < i; ++p) {
            const int32_t k = A.indices[(size_t)p], dk = dpos[(size_t)k];
            double lx, ly = 0.0;
            if (w == 1) {
                lx = a[(size_t)p] / a[(size_t)dk];
                a[(size_t)p] = lx;
            } else {
                const double ax = a[2 * (size_t)p], ay = a[2 * (size_t)p + 1], dx = a[2 * (size_t)dk], dy = a[2 * (size_t)dk + 1];
                if (fabs(dx) >= fabs(dy)) {
                    const double rat = dy / dx, scl = 1.0 / (dx + dy * rat);
                    lx = (ax + ay * rat) * scl;
                    ly = (ay - ax * rat) * scl;
                } else {
                    const double rat = dx / dy, scl = 1.0 / (dy + dx * rat);
                    lx = (ax * rat + ay) * scl;
                    ly = (ay * rat - ax) * scl;
                }
                a[2 * (size_t)p] = lx;
                a[2 * (size_t)p + 1] = ly;
            }
            for (int32_t q = p + 1; q < A.indptr[(size_t)i + 1]; ++q)
                for (int32_t r = A.indptr[(size_t)k]; r < A.indptr[(size_t)k + 1]; ++r) {
                    if (A.indices[(size_t)r] != A.indices[(size_t)q]) continue;
                    if (w == 1) a[(size_t)q] = a[(size_t)q] - lx * a[(size_t)r];
                    else {
                        const double ux = a[2 * (size_t)r], uy = a[2 * (size_t)r + 1];
                        a[2 * (size_t)q] = a[2 * (size_t)q] - (lx * ux - ly * uy);
                        a[2 * (size_t)q + 1] = a[2 * (size_t)q + 1] - (lx * uy + ly * ux);
                    }
                }
        }
        bool broke = true;
        for (int c = 0; c < w; ++c) broke = broke && a[(size_t)w * (size_t)dpos[(size_t)i] + c] == 0.0;
        for (int c = 0; c < w; ++c) broke = broke || !(fabs(a[(size_t)w * (size_t)dpos[(size_t)i] + c]) <= DBL_MAX);
        if (broke && bad < 0) bad = i;
    }
    return bad;
}

static int run(const char* name, const Csr& A) {
    int badcases = 0;
    for (int64_t narrow : {(int64_t)0, (int64_t)64, (int64_t)1024}) {
        khilu0::Plan p;
        const std::string why = khilu0::analyse(A.n, (int64_t)A.indices.size(), A.indptr.data(), A.indices.data(), narrow, p);
        if (!why.empty()) {
            printf("%s refused: %s\n", name, why.c_str());
            return 0;
        }
        bool ok = true;
        int64_t first = -1;
        for (int w = 1; w <= 2; ++w) {
            std::vector<double> a((size_t)w * A.data.size()), b;
            for (size_t q = 0; q < A.data.size(); ++q) {
                a[(size_t)w * q] = A.data[q];
                if (w == 2) a[2 * q + 1] = 0.2 * A.data[q] * (double)((int)((q * 7919) % 13) - 6) / 6.0 + (A.data[q] > 1.5 ? 0.5 : 0.0);
            }
            b = a;
            const int64_t bad_a = khilu0::factor_host(p, A.indptr.data(), A.indices.data(), w, a.data());
            const int64_t bad_b = plain(A, w, b);
            ok = ok && bad_a == bad_b;
            for (size_t q = 0; q < a.size(); ++q)      // the same bits; behind a breakdown a NaN for a NaN (its payload is the CPU's business)
                ok = ok && (memcmp(&a[q], &b[q], sizeof(double)) == 0 || (a[q] != a[q] && b[q] != b[q]));
            if (w == 1) first = bad_a;
        }
        std::vector<int> seen((size_t)A.n, 0);
        for (int32_t r : p.row_id)
            if (r >= 0) seen[(size_t)r] += 1;
        for (int v : seen) ok = ok && v == 1;
        int32_t lev = 0, sl = 0;
        for (const khtri::Launch& L : p.launches) {
            ok = ok && L.lev0 == lev && L.slice0 == sl && L.threads >= 64 && L.threads <= 1024 && L.threads % 64 == 0;
            lev += L.nlev;
            sl += L.nslices;
        }
        ok = ok && lev == p.nlevels && sl == p.nslices && (int64_t)p.launches.size() == p.n_wide + p.n_narrow &&
             (int64_t)p.row_id.size() == p.nslices * khtri::SLICE;
        printf("%s/%lld levels=%lld widest=%lld longest=%lld wide=%lld narrow=%lld bad=%lld factor=%s\n", name, (long long)narrow,
               (long long)p.nlevels, (long long)p.widest, (long long)p.longest, (long long)p.n_wide, (long long)p.n_narrow,
               (long long)first, ok ? "ok" : "BAD");
        badcases += ok ? 0 : 1;
    }
    return badcases;
}

// colours the pattern of A + A^T, checks the colouring and returns the ordering (stable sort of the rows by colour)
static std::vector<int32_t> colour(const char* name, int64_t n, const Entries& e, int* bad) {
    const Csr G = csr(n, symmetrised(e));
    std::vector<int32_t> color((size_t)n, -1), perm;
    int64_t nc = 0;
    const std::string why = khilu0::multicolor(n, (int64_t)G.indices.size(), G.indptr.data(), G.indices.data(), color.data(), &nc);
    if (!why.empty()) {
        printf("%s refused: %s\n", name, why.c_str());
        return perm;
    }
    bool ok = true;
    for (int64_t i = 0; i < n; ++i) {
        ok = ok && color[(size_t)i] >= 0 && color[(size_t)i] < nc;
        for (int32_t q = G.indptr[(size_t)i]; q < G.indptr[(size_t)i + 1]; ++q)      // no stored off-diagonal entry joins two rows of one colour
            ok = ok && (G.indices[(size_t)q] == i || color[(size_t)G.indices[(size_t)q]] != color[(size_t)i]);
    }
    for (int32_t c = 0; c < nc; ++c)
        for (int64_t i = 0; i < n; ++i)
            if (color[(size_t)i] == c) perm.push_back((int32_t)i);
    printf("%s colors=%lld valid=%s order", name, (long long)nc, ok ? "ok" : "BAD");
    for (int32_t r : perm) printf(" %d", (int)r);
    printf("\n");
    *bad += ok ? 0 : 1;
    return perm;
}

int main() {
    int bad = 0;
    const int nx = 37, ny = 23, n = nx * ny;
    {
        Entries dense, tri, diag;
        for (int32_t i = 0; i < 12; ++i)
            for (int32_t j = 0; j < 12; ++j) dense[{i, j}] = i == j ? 14.0 + 0.1 * i : -1.0 + 0.01 * ((i * 5 + j * 3) % 17);
        for (int32_t i = 0; i < 300; ++i) {
            tri[{i, i}] = 2.5 + 0.01 * i;
            diag[{i, i}] = 1.0 + i;
            if (i > 0) tri[{i, i - 1}] = -1.0;
            if (i + 1 < 300) tri[{i, i + 1}] = -1.0 - 0.001 * i;
        }
        bad += run("dense12", csr(12, dense));
        bad += run("tridiagonal", csr(300, tri));
        bad += run("diagonal", csr(300, diag));
        // one row with 200 entries left of the diagonal among short ones, a stored zero inside the pattern
        Entries f = tri;
        for (int32_t j = 0; j < 200; ++j) f[{250, j}] = 0.001 * (j + 1);
        f[{250, 250}] = 5.0;
        f[{100, 50}] = 0.0;
        bad += run("long_row", csr(300, f));
        // breakdown: [[1,1,0],[1,1,1],[0,1,3]] breaks in row 1 and goes on; two independent zero pivots: the smaller row
        Entries z = {{{0, 0}, 1.0}, {{0, 1}, 1.0}, {{1, 0}, 1.0}, {{1, 1}, 1.0}, {{1, 2}, 1.0}, {{2, 1}, 1.0}, {{2, 2}, 3.0}};
        bad += run("breakdown3", csr(3, z));
        Entries two = tri;
        two[{200, 200}] = 0.0;
        two.erase({200, 199});
        two.erase({199, 200});
        two[{7, 7}] = 0.0;
        two.erase({7, 6});
        two.erase({6, 7});
        bad += run("two_zero_pivots", csr(300, two));
        // refused inputs
        Csr A = csr(300, tri), B = A, C = A, D = A;
        std::swap(B.indices[3], B.indices[4]);
        bad += run("unsorted", B);
        C.indices[4] = C.indices[3];
        bad += run("duplicate", C);
        D.indices[4] = 300;
        bad += run("out_of_range", D);
        Entries g = tri;
        g.erase({7, 7});
        bad += run("missing_diagonal", csr(300, g));
    }
    for (int conv = 0; conv < 2; ++conv) {
        const Entries e = stencil(nx, ny, false, conv ? 0.8 : 0.0);
        bad += run(conv ? "convection_natural" : "lap2d_natural", csr(n, e));
        const std::vector<int32_t> perm = colour(conv ? "convection_colouring" : "lap2d_colouring", n, e, &bad);
        bad += run(conv ? "convection_multicolor" : "lap2d_multicolor", csr(n, permuted(e, perm)));
    }
    {
        const Entries e = stencil(19, 14, true, 0.0);
        bad += run("nine_point_natural", csr(19 * 14, e));
        const std::vector<int32_t> perm = colour("nine_point_colouring", 19 * 14, e, &bad);
        bad += run("nine_point_multicolor", csr(19 * 14, permuted(e, perm)));
    }
    return bad ? 1 : 0;
}
