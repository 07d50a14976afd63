// Stand-alone check of the level analysis of the sparse triangular solves (krypy_amd/csrc/tri.h) - TEST INFRASTRUCTURE ONLY.
// tests/test_tri_host.py compiles this file with the host compiler and -fsanitize=address,undefined and runs it on the CPU:
// tri.h is plain C++ without a HIP call.  Every case prints one line
//     <name> levels=<..> widest=<..> longest=<..> slots=<..> wide=<..> narrow=<..> first=<rows of level 0> solve=<ok|BAD>
// (the test holds the hand-counted numbers), followed for the default plans by "order <name> <rows in plan order>", every refused
// input one line "<name> refused: <message>".
#include <stdio.h>
#include <string.h>

#include <map>
#include <utility>

#include "tri.h"

struct Csr {
    int64_t n = 0;
    std::vector<int32_t> indptr, indices;
    std::vector<double> data;
};

// CSR of the given triangle (diagonal included) of the matrix given as sorted (row, col) -> value entries
static Csr triangle(int64_t n, const std::map<std::pair<int32_t, int32_t>, double>& e, bool lower) {
    Csr A;
    A.n = n;
    A.indptr.assign((size_t)n + 1, 0);
    for (const auto& kv : e) {
        const int32_t r = kv.first.first, c = kv.first.second;
        if (lower ? c > r : c < r) continue;
        A.indptr[(size_t)r + 1] += 1;
        A.indices.push_back(c);
        A.data.push_back(kv.second);
    }
    for (int64_t i = 0; i < n; ++i) A.indptr[(size_t)i + 1] += A.indptr[(size_t)i];
    return A;
}

// five-point Laplacian on nx x ny; perm[p] = index of grid point p
static std::map<std::pair<int32_t, int32_t>, double> lap2d(int nx, int ny, const std::vector<int32_t>& perm) {
    std::map<std::pair<int32_t, int32_t>, double> e;
    for (int ix = 0; ix < nx; ++ix)
        for (int iy = 0; iy < ny; ++iy) {
            const int32_t p = perm[(size_t)(ix * ny + iy)];
            e[{p, p}] = 4.0;
            if (ix > 0) e[{p, perm[(size_t)((ix - 1) * ny + iy)]}] = -1.0;
            if (ix + 1 < nx) e[{p, perm[(size_t)((ix + 1) * ny + iy)]}] = -1.0;
            if (iy > 0) e[{p, perm[(size_t)(ix * ny + iy - 1)]}] = -1.0;
            if (iy + 1 < ny) e[{p, perm[(size_t)(ix * ny + iy + 1)]}] = -1.0 - 0.001 * iy;
        }
    return e;
}

static int run(const char* name, const Csr& A, bool lower, bool unit, int64_t narrow, bool print_order = false) {
    khtri::Plan p;
    const std::string why =
        khtri::analyse(A.n, (int64_t)A.indices.size(), A.indptr.data(), A.indices.data(), A.data.data(), 1, lower, unit, narrow, p);
    if (!why.empty()) {
        printf("%s refused: %s\n", name, why.c_str());
        return 0;
    }
    // the plan's arithmetic against the row-by-row substitution on the CSR input: the same bits
    std::vector<double> b((size_t)A.n), x((size_t)A.n, 0.0), y((size_t)A.n, 0.0);
    for (int64_t i = 0; i < A.n; ++i) b[(size_t)i] = 1.0 + 0.37 * (double)((i * 7919) % 101) - 0.011 * (double)(i % 13);
    khtri::solve_host(p, unit, b.data(), x.data());
    for (int64_t s = 0; s < A.n; ++s) {
        const int64_t i = lower ? s : A.n - 1 - s;
        double acc = b[(size_t)i], d = 1.0;
        for (int32_t q = A.indptr[(size_t)i]; q < A.indptr[(size_t)i + 1]; ++q) {
            if (A.indices[(size_t)q] == i) d = A.data[(size_t)q];
            else acc = acc - A.data[(size_t)q] * y[(size_t)A.indices[(size_t)q]];
        }
        y[(size_t)i] = unit ? acc : acc / d;
    }
    const bool same = memcmp(x.data(), y.data(), sizeof(double) * (size_t)A.n) == 0;
    // every row exactly once, the launches cover all levels in order
    std::vector<int> seen((size_t)A.n, 0);
    bool ok = same;
    for (int32_t r : p.row_id)
        if (r >= 0) seen[(size_t)r] += 1;
    for (int v : seen) ok = ok && v == 1;
    int32_t lev = 0, sl = 0;
    for (const khtri::Launch& L : p.launches) {
        ok = ok && L.lev0 == lev && L.slice0 == sl && L.threads >= 64 && L.threads <= 1024 && L.threads % 64 == 0;
        lev += L.nlev;
        sl += L.nslices;
    }
    ok = ok && lev == p.nlevels && sl == p.nslices && (int64_t)p.launches.size() == p.n_wide + p.n_narrow;
    printf("%s levels=%lld widest=%lld longest=%lld slots=%lld wide=%lld narrow=%lld first=%d solve=%s\n", name, (long long)p.nlevels,
           (long long)p.widest, (long long)p.longest, (long long)p.slots, (long long)p.n_wide, (long long)p.n_narrow,
           (int)(p.lev_ptr[1] - p.lev_ptr[0]), ok ? "ok" : "BAD");
    if (print_order) {      // the rows in plan order
        printf("order %s", name);
        for (int32_t r : p.order) printf(" %d", (int)r);
        printf("\n");
    }
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    const int nx = 37, ny = 23, n = nx * ny;
    std::vector<int32_t> natural((size_t)n), redblack((size_t)n);
    int32_t nred = 0, nblack = 0;
    for (int p = 0; p < n; ++p) nred += ((p / ny + p % ny) % 2 == 0);
    {
        int32_t r = 0;
        for (int p = 0; p < n; ++p) {
            natural[(size_t)p] = p;
            if ((p / ny + p % ny) % 2 == 0) redblack[(size_t)p] = r++;
            else redblack[(size_t)p] = nred + nblack++;
        }
    }
    const auto nat = lap2d(nx, ny, natural), rb = lap2d(nx, ny, redblack);
    bad += run("natural_lower", triangle(n, nat, true), true, false, 1024, true);
    bad += run("natural_upper", triangle(n, nat, false), false, false, 1024, true);
    bad += run("natural_lower_wide", triangle(n, nat, true), true, false, 0);
    bad += run("natural_lower_mixed", triangle(n, nat, true), true, false, 16);
    bad += run("redblack_lower", triangle(n, rb, true), true, false, 1024, true);
    bad += run("redblack_upper", triangle(n, rb, false), false, true, 64, true);
    {
        std::map<std::pair<int32_t, int32_t>, double> e;
        for (int32_t i = 0; i < 300; ++i) {
            e[{i, i}] = 2.0 + 0.01 * i;
            if (i > 0) e[{i, i - 1}] = -1.0;
        }
        bad += run("bidiagonal", triangle(300, e, true), true, false, 1024);
        std::map<std::pair<int32_t, int32_t>, double> d;
        for (int32_t i = 0; i < 300; ++i) d[{i, i}] = 1.0 + i;
        bad += run("diagonal", triangle(300, d, true), true, false, 1024);
        // one row of 200 entries among short ones
        std::map<std::pair<int32_t, int32_t>, double> f = e;
        for (int32_t j = 0; j < 200; ++j) f[{250, j}] = 0.001 * (j + 1);
        bad += run("long_row", triangle(300, f, true), true, false, 1024, true);
        // refused inputs
        Csr A = triangle(300, e, true);
        bad += run("wrong_side", A, false, false, 1024);
        Csr B = A;
        std::swap(B.indices[1], B.indices[2]);
        bad += run("unsorted", B, true, false, 1024);
        Csr C = A;
        C.indices[2] = C.indices[1];
        bad += run("duplicate", C, true, false, 1024);
        Csr D = A;
        D.data[(size_t)D.indptr[6] - 1] = 0.0;
        bad += run("zero_diagonal", D, true, false, 1024);
        bad += run("zero_diagonal_unit", D, true, true, 1024);
        std::map<std::pair<int32_t, int32_t>, double> g = e;
        g.erase({7, 7});
        bad += run("missing_diagonal", triangle(300, g, true), true, false, 1024);
    }
    return bad ? 1 : 0;
}
