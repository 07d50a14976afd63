// Stand-alone host program around krypy_amd/csrc/fsai.h - TEST INFRASTRUCTURE ONLY (tests/test_fsai_host.py compiles it with
// -fsanitize=address,undefined and runs it as a child process).  For every case, real and complex, it computes all rows
//   - with plain_row_r / plain_row_z below: the contract as ONE sequential loop, written here without the header's phases, and
//   - with khfsai::build_host() on W = 1 / 8 / 16 / 32 / 64 emulated lanes, the split the kernel makes,
// and compares the bits of u and d (memcmp: a NaN must be the very same NaN).  One line per case and W:
//   <case>/<r|z>/<W> q=<longest pattern row> bad=<first broken row> bits=<ok|DIFFER>
// then one line per refused input:  <name> refused: <message>.  Exit status 1 when any bits differ.
// The cases' matrices and the comparison are in sai_main.h, shared with spai_main.cpp.
#include "fsai.h"

#include "sai_main.h"

namespace {

// five-point Laplacian minus `shift` on the diagonal
Mat laplacian(int nx, int ny, double shift) {
    Triplets t;
    for (int ix = 0; ix < nx; ++ix)
        for (int iy = 0; iy < ny; ++iy) {
            const int32_t i = ix * ny + iy;
            t.push_back({{i, i}, 4.0 - shift});
            if (iy > 0) t.push_back({{i, i - 1}, -1.0});
            if (iy + 1 < ny) t.push_back({{i, i + 1}, -1.0});
            if (ix > 0) t.push_back({{i, i - ny}, -1.0});
            if (ix + 1 < nx) t.push_back({{i, i + ny}, -1.0});
        }
    return from_triplets((int64_t)nx * ny, t);
}

// a symmetric band of half-width hw with seeded values and a dominant diagonal
Mat band(int n, int hw) {
    Triplets t;
    for (int i = 0; i < n; ++i) {
        t.push_back({{i, i}, 3.0 * hw + 1.0 + lcg()});
        for (int j = std::max(0, i - hw); j < i; ++j) {
            const double v = lcg();
            t.push_back({{i, j}, v});
            t.push_back({{j, i}, v});
        }
    }
    return from_triplets(n, t);
}

Mat diagonal(int n) {
    Triplets t;
    for (int i = 0; i < n; ++i) t.push_back({{i, i}, 0.5 + 0.25 * i});
    return from_triplets(n, t);
}

// the lower triangle of a pattern with the diagonal added
Mat lower(const Mat& P) {
    Triplets t;
    for (int32_t i = 0; i < P.n; ++i) {
        bool diag = false;
        for (int32_t p = P.ptr[(size_t)i]; p < P.ptr[(size_t)i + 1]; ++p)
            if (P.idx[(size_t)p] <= i) {
                t.push_back({{i, P.idx[(size_t)p]}, 1.0});
                diag = diag || P.idx[(size_t)p] == i;
            }
        if (!diag) t.push_back({{i, i}, 1.0});
    }
    return from_triplets(P.n, t);
}

// Hermitian: the lower triangle gets a seeded imaginary part, the upper one its conjugate, the diagonal stays real
Mat complex_case(const Mat& A) {
    Mat Z = A;
    Z.val.assign(2 * A.val.size(), 0.0);
    for (int32_t i = 0; i < A.n; ++i)
        for (int32_t p = A.ptr[(size_t)i]; p < A.ptr[(size_t)i + 1]; ++p) Z.val[2 * (size_t)p] = A.val[(size_t)p];
    for (int32_t i = 0; i < A.n; ++i)
        for (int32_t p = A.ptr[(size_t)i]; p < A.ptr[(size_t)i + 1]; ++p) {
            const int32_t j = A.idx[(size_t)p];
            if (j >= i) continue;
            const double im = 0.3 * lcg() * A.val[(size_t)p];
            Z.val[2 * (size_t)p + 1] = im;
            for (int32_t r = A.ptr[(size_t)j]; r < A.ptr[(size_t)j + 1]; ++r)
                if (A.idx[(size_t)r] == i) Z.val[2 * (size_t)r + 1] = -im;
        }
    return Z;
}

// A[r, c] by a linear search of row r: the bits, or +0
bool find(const Mat& A, int32_t r, int32_t c, int32_t* at) {
    for (int32_t p = A.ptr[(size_t)r]; p < A.ptr[(size_t)r + 1]; ++p)
        if (A.idx[(size_t)p] == c) {
            *at = p;
            return true;
        }
    return false;
}

// The contract, complex form, one sequential loop.
bool plain_row_z(const Mat& A, const int32_t* J, int q, double* u, double* dout) {
    std::vector<C> S((size_t)q * q), L((size_t)q * q), v((size_t)q), uu((size_t)q);
    std::vector<double> d((size_t)q);
    bool bad = false;
    for (int a = 0; a < q; ++a)
        for (int b = 0; b <= a; ++b) {
            int32_t p = 0;
            S[(size_t)a * q + b] = find(A, J[a], J[b], &p) ? C{A.val[2 * (size_t)p], A.val[2 * (size_t)p + 1]} : C{0.0, 0.0};
        }
    for (int j = 0; j < q; ++j) {
        for (int k = 0; k < j; ++k) v[(size_t)k] = {L[(size_t)j * q + k].r * d[(size_t)k], L[(size_t)j * q + k].i * d[(size_t)k]};
        C s = S[(size_t)j * q + j];
        for (int k = 0; k < j; ++k) s = sub(s, mul(L[(size_t)j * q + k], cj(v[(size_t)k])));
        d[(size_t)j] = s.r;
        bad = bad || !(s.r > 0.0) || !(s.r <= DBL_MAX);
        for (int t = j + 1; t < q; ++t) {
            s = S[(size_t)t * q + j];
            for (int k = 0; k < j; ++k) s = sub(s, mul(L[(size_t)t * q + k], cj(v[(size_t)k])));
            L[(size_t)t * q + j] = {s.r / d[(size_t)j], s.i / d[(size_t)j]};
        }
    }
    uu[(size_t)q - 1] = {1.0, 0.0};
    for (int a = q - 2; a >= 0; --a) {
        C s{0.0, 0.0};
        for (int k = a + 1; k < q; ++k) s = sub(s, mul(L[(size_t)k * q + a], uu[(size_t)k]));          // L unconjugated
        uu[(size_t)a] = s;
    }
    for (int a = 0; a < q; ++a) {
        u[2 * a] = canon(uu[(size_t)a].r);
        u[2 * a + 1] = canon(uu[(size_t)a].i);
    }
    *dout = canon(d[(size_t)q - 1]);
    return bad;
}

// The real form spelled out separately (in the complex form x - (+-0 * +-0) may turn a -0 real part into +0).
bool plain_row_r(const Mat& A, const int32_t* J, int q, double* u, double* dout) {
    std::vector<double> S((size_t)q * q), L((size_t)q * q), v((size_t)q), d((size_t)q), uu((size_t)q);
    bool bad = false;
    for (int a = 0; a < q; ++a)
        for (int b = 0; b <= a; ++b) {
            int32_t p = 0;
            S[(size_t)a * q + b] = find(A, J[a], J[b], &p) ? A.val[(size_t)p] : 0.0;
        }
    for (int j = 0; j < q; ++j) {
        for (int k = 0; k < j; ++k) v[(size_t)k] = L[(size_t)j * q + k] * d[(size_t)k];
        double s = S[(size_t)j * q + j];
        for (int k = 0; k < j; ++k) s = s - L[(size_t)j * q + k] * v[(size_t)k];
        d[(size_t)j] = s;
        bad = bad || !(s > 0.0) || !(s <= DBL_MAX);
        for (int t = j + 1; t < q; ++t) {
            s = S[(size_t)t * q + j];
            for (int k = 0; k < j; ++k) s = s - L[(size_t)t * q + k] * v[(size_t)k];
            L[(size_t)t * q + j] = s / d[(size_t)j];
        }
    }
    uu[(size_t)q - 1] = 1.0;
    for (int a = q - 2; a >= 0; --a) {
        double s = 0.0;
        for (int k = a + 1; k < q; ++k) s = s - L[(size_t)k * q + a] * uu[(size_t)k];
        uu[(size_t)a] = s;
    }
    for (int a = 0; a < q; ++a) u[a] = canon(uu[(size_t)a]);
    *dout = canon(d[(size_t)q - 1]);
    return bad;
}

// ---- the hooks of sai_main.h ----------------------------------------------------------------------------------------------
std::string validate(int64_t n, int64_t nnz, const Mat& A, const Mat& P, int64_t* qmax) {
    return khfsai::validate(n, nnz, A.ptr.data(), A.idx.data(), P.nnz(), P.ptr.data(), P.idx.data(), qmax);
}

Outputs blank_outputs(const Mat& A, const Mat& P, bool cplx) {      // u and d
    return {std::vector<double>((size_t)P.nnz() * (cplx ? 2 : 1) + 1, -7.0), std::vector<double>((size_t)A.n + 1, -7.0)};
}

bool plain_row(const Mat& A, const int32_t* J, int q, int64_t i, int32_t p0, bool cplx, Outputs& want) {
    return cplx ? plain_row_z(A, J, q, want[0].data() + 2 * (size_t)p0, want[1].data() + i)
                : plain_row_r(A, J, q, want[0].data() + p0, want[1].data() + i);
}

int64_t lanes_build(const Mat& A, const Mat& P, int qmax, int W, bool cplx, double* work, Outputs& got) {
    const khfsai::Csr csr{A.ptr.data(), A.idx.data(), A.val.data()};
    return khfsai::build_host(A.n, csr, P.ptr.data(), P.idx.data(), qmax, W, cplx, work, got[0].data(), got[1].data());
}

}  // namespace

int main() {
    lcg_state = 4321;
    const Mat A = laplacian(13, 9, 0.0);
    const Mat A2 = pattern_product(A, A), A3 = pattern_product(A2, A), A4 = pattern_product(A3, A);
    both("grid_tril_A", A, lower(A));            // q <= 3
    both("grid_tril_A2", A, lower(A2));          // q <= 7
    both("grid_tril_A3", A, lower(A3));          // q <= 13
    both("grid_tril_A4", A, lower(A4));          // q <= 21
    both("band_q32", band(70, 31), lower(band(70, 31)));          // rows of 1 .. 32 entries
    both("diagonal", diagonal(9), diagonal(9));
    both("n1", diagonal(1), diagonal(1));
    {   // a missing stored diagonal: S_jj = +0, the pivot of row 5 is minus a sum of squares over positive pivots
        const Mat B = band(12, 2);
        Triplets t;
        for (int32_t i = 0; i < 12; ++i)
            for (int32_t p = B.ptr[(size_t)i]; p < B.ptr[(size_t)i + 1]; ++p)
                if (!(i == 5 && B.idx[(size_t)p] == 5)) t.push_back({{i, B.idx[(size_t)p]}, B.val[(size_t)p]});
        both("missing_diagonal", from_triplets(12, t), lower(B));
    }
    both("indefinite", laplacian(9, 7, 3.0), lower(laplacian(9, 7, 3.0)));          // row 1: d = 1 - (-1 / 1) * (-1) = 0 exactly
    // every validation error
    const Mat LA = lower(A);
    refused_inputs(A, LA, 15, 16);
    {
        refused("upper_entries", A, A);                         // the full pattern of A: row 0 ends in column 9
        Triplets t;
        for (int32_t i = 0; i < A.n; ++i)
            for (int32_t p = LA.ptr[(size_t)i]; p < LA.ptr[(size_t)i + 1]; ++p)
                if (i != 7) t.push_back({{i, LA.idx[(size_t)p]}, 1.0});
        refused("empty_row", A, from_triplets(A.n, t));
        t.clear();
        for (int32_t i = 0; i < A.n; ++i)
            for (int32_t p = LA.ptr[(size_t)i]; p < LA.ptr[(size_t)i + 1]; ++p)
                if (!(i == 11 && LA.idx[(size_t)p] == 11)) t.push_back({{i, LA.idx[(size_t)p]}, 1.0});
        refused("no_diagonal", A, from_triplets(A.n, t));
    }
    refused("q33", band(50, 32), lower(band(50, 32)));
    return failures ? 1 : 0;
}
