// Stand-alone host program around krypy_amd/csrc/spai.h - TEST INFRASTRUCTURE ONLY (tests/test_spai_host.py compiles it with
// -fsanitize=address,undefined and runs it as a child process).  For every case, real and complex, it computes all rows
//   - with plain_row_r / plain_row_z below: the contract as ONE sequential loop, written here without the header's phases, and
//   - with khspai::build_host() on W = 1 / 8 / 16 / 32 / 64 emulated lanes, the split the kernel makes,
// and compares the bits (memcmp: a NaN must be the very same NaN).  One line per case and W:
//   <case>/<r|z>/<W> q=<longest pattern row> bad=<first broken row> bits=<ok|DIFFER>
// then one line per refused input:  <name> refused: <message>.  Exit status 1 when any bits differ.
// The cases' matrices and the comparison are in sai_main.h, shared with fsai_main.cpp.
#include "spai.h"

#include "sai_main.h"

namespace {

// five-point Laplacian with upwind convection inside a grid line
Mat convection(int nx, int ny, double wind) {
    Triplets t;
    for (int ix = 0; ix < nx; ++ix)
        for (int iy = 0; iy < ny; ++iy) {
            const int32_t i = ix * ny + iy;
            t.push_back({{i, i}, 4.0 + wind});
            if (iy > 0) t.push_back({{i, i - 1}, -1.0 - wind});
            if (iy + 1 < ny) t.push_back({{i, i + 1}, -1.0});
            if (ix > 0) t.push_back({{i, i - ny}, -1.0});
            if (ix + 1 < nx) t.push_back({{i, i + ny}, -1.0});
        }
    return from_triplets((int64_t)nx * ny, t);
}

// a band of half-width hw with seeded values and a dominant diagonal
Mat band(int n, int hw) {
    Triplets t;
    for (int i = 0; i < n; ++i)
        for (int j = std::max(0, i - hw); j <= std::min(n - 1, i + hw); ++j) t.push_back({{i, j}, i == j ? 2.0 * hw + 1.0 + lcg() : lcg()});
    return from_triplets(n, t);
}

Mat complex_case(const Mat& A) {
    Mat Z = A;
    Z.val.resize(2 * A.val.size());
    for (size_t p = 0; p < A.val.size(); ++p) {
        Z.val[2 * p] = A.val[p];
        Z.val[2 * p + 1] = 0.3 * lcg() * A.val[p];
    }
    return Z;
}

// The contract, complex form, one sequential loop.  For real data every imaginary part is +0 or -0 and no real part depends on
// one: x - (+-0 * +-0) may turn a -0 real part into +0, so the real form is spelled out separately below.
bool plain_row_z(const Mat& A, const int32_t* J, int q, int32_t i, double* m) {
    auto at = [&](int32_t p) { return C{A.val[2 * (size_t)p], A.val[2 * (size_t)p + 1]}; };
    std::vector<C> G((size_t)q * q), L((size_t)q * q), r((size_t)q), y((size_t)q), v((size_t)q), mm((size_t)q);
    std::vector<double> d((size_t)q);
    bool bad = false;
    for (int a = 0; a < q; ++a) {
        for (int b = 0; b <= a; ++b) {
            int32_t pa = A.ptr[(size_t)J[a]], pb = A.ptr[(size_t)J[b]];
            C s{0.0, 0.0};
            while (pa < A.ptr[(size_t)J[a] + 1] && pb < A.ptr[(size_t)J[b] + 1]) {
                if (A.idx[(size_t)pa] == A.idx[(size_t)pb]) {
                    const C pr = mul(cj(at(pa)), at(pb));
                    s = {s.r + pr.r, s.i + pr.i};
                    ++pa;
                    ++pb;
                } else if (A.idx[(size_t)pa] < A.idx[(size_t)pb]) ++pa;
                else ++pb;
            }
            G[(size_t)a * q + b] = s;
        }
        r[(size_t)a] = {0.0, 0.0};
        for (int32_t p = A.ptr[(size_t)J[a]]; p < A.ptr[(size_t)J[a] + 1]; ++p)
            if (A.idx[(size_t)p] == i) r[(size_t)a] = cj(at(p));
    }
    for (int j = 0; j < q; ++j) {
        for (int k = 0; k < j; ++k) v[(size_t)k] = {L[(size_t)j * q + k].r * d[(size_t)k], L[(size_t)j * q + k].i * d[(size_t)k]};
        C s = G[(size_t)j * q + j];
        for (int k = 0; k < j; ++k) s = sub(s, mul(L[(size_t)j * q + k], cj(v[(size_t)k])));
        d[(size_t)j] = s.r;
        bad = bad || !(s.r > 0.0) || !(s.r <= DBL_MAX);
        for (int t = j + 1; t < q; ++t) {
            s = G[(size_t)t * q + j];
            for (int k = 0; k < j; ++k) s = sub(s, mul(L[(size_t)t * q + k], cj(v[(size_t)k])));
            L[(size_t)t * q + j] = {s.r / d[(size_t)j], s.i / d[(size_t)j]};
        }
    }
    for (int a = 0; a < q; ++a) {
        C s = r[(size_t)a];
        for (int k = 0; k < a; ++k) s = sub(s, mul(L[(size_t)a * q + k], y[(size_t)k]));
        y[(size_t)a] = s;
    }
    for (int a = q - 1; a >= 0; --a) {
        C s{y[(size_t)a].r / d[(size_t)a], y[(size_t)a].i / d[(size_t)a]};
        for (int k = a + 1; k < q; ++k) s = sub(s, mul(cj(L[(size_t)k * q + a]), mm[(size_t)k]));
        mm[(size_t)a] = s;
        m[2 * a] = canon(s.r);
        m[2 * a + 1] = canon(s.i);
    }
    return bad;
}

bool plain_row_r(const Mat& A, const int32_t* J, int q, int32_t i, double* m) {
    std::vector<double> G((size_t)q * q), L((size_t)q * q), r((size_t)q), y((size_t)q), v((size_t)q), d((size_t)q);
    bool bad = false;
    for (int a = 0; a < q; ++a) {
        for (int b = 0; b <= a; ++b) {
            int32_t pa = A.ptr[(size_t)J[a]], pb = A.ptr[(size_t)J[b]];
            double s = 0.0;
            while (pa < A.ptr[(size_t)J[a] + 1] && pb < A.ptr[(size_t)J[b] + 1]) {
                if (A.idx[(size_t)pa] == A.idx[(size_t)pb]) {
                    s = s + A.val[(size_t)pa] * A.val[(size_t)pb];
                    ++pa;
                    ++pb;
                } else if (A.idx[(size_t)pa] < A.idx[(size_t)pb]) ++pa;
                else ++pb;
            }
            G[(size_t)a * q + b] = s;
        }
        r[(size_t)a] = 0.0;
        for (int32_t p = A.ptr[(size_t)J[a]]; p < A.ptr[(size_t)J[a] + 1]; ++p)
            if (A.idx[(size_t)p] == i) r[(size_t)a] = A.val[(size_t)p];
    }
    for (int j = 0; j < q; ++j) {
        for (int k = 0; k < j; ++k) v[(size_t)k] = L[(size_t)j * q + k] * d[(size_t)k];
        double s = G[(size_t)j * q + j];
        for (int k = 0; k < j; ++k) s = s - L[(size_t)j * q + k] * v[(size_t)k];
        d[(size_t)j] = s;
        bad = bad || !(s > 0.0) || !(s <= DBL_MAX);
        for (int t = j + 1; t < q; ++t) {
            s = G[(size_t)t * q + j];
            for (int k = 0; k < j; ++k) s = s - L[(size_t)t * q + k] * v[(size_t)k];
            L[(size_t)t * q + j] = s / d[(size_t)j];
        }
    }
    for (int a = 0; a < q; ++a) {
        double s = r[(size_t)a];
        for (int k = 0; k < a; ++k) s = s - L[(size_t)a * q + k] * y[(size_t)k];
        y[(size_t)a] = s;
    }
    for (int a = q - 1; a >= 0; --a) {
        double s = y[(size_t)a] / d[(size_t)a];
        for (int k = a + 1; k < q; ++k) s = s - L[(size_t)k * q + a] * m[k];
        m[a] = canon(s);
    }
    return bad;
}

// ---- the hooks of sai_main.h ----------------------------------------------------------------------------------------------
std::string validate(int64_t n, int64_t nnz, const Mat& A, const Mat& P, int64_t* qmax) {
    return khspai::validate(n, nnz, A.ptr.data(), A.idx.data(), P.nnz(), P.ptr.data(), P.idx.data(), qmax);
}

Outputs blank_outputs(const Mat&, const Mat& P, bool cplx) { return {std::vector<double>((size_t)P.nnz() * (cplx ? 2 : 1) + 1, -7.0)}; }

bool plain_row(const Mat& A, const int32_t* J, int q, int64_t i, int32_t p0, bool cplx, Outputs& want) {
    return cplx ? plain_row_z(A, J, q, (int32_t)i, want[0].data() + 2 * (size_t)p0) : plain_row_r(A, J, q, (int32_t)i, want[0].data() + p0);
}

int64_t lanes_build(const Mat& A, const Mat& P, int qmax, int W, bool cplx, double* work, Outputs& got) {
    const khspai::Csr csr{A.ptr.data(), A.idx.data(), A.val.data()};
    return khspai::build_host(A.n, csr, P.ptr.data(), P.idx.data(), qmax, W, cplx, work, got[0].data());
}

}  // namespace

int main() {
    lcg_state = 12345;
    const Mat A = convection(13, 9, 0.4);
    both("grid_pattern_A", A, A);                              // q <= 5
    both("grid_pattern_A2", A, pattern_product(A, A));        // q <= 13
    const Mat B = band(70, 3);
    both("band_q31", B, band(70, 15));                         // q up to 31: the 32-lane kernel's range, rows of 16 .. 31
    both("band_q32", band(40, 16), [] {                        // one row of exactly 32 entries among short ones
        Mat P = band(40, 1);
        Triplets t;
        for (int32_t i = 0; i < 40; ++i)
            for (int32_t p = P.ptr[(size_t)i]; p < P.ptr[(size_t)i + 1]; ++p)
                if (i != 20) t.push_back({{i, P.idx[(size_t)p]}, 1.0});
        for (int32_t c = 3; c < 35; ++c) t.push_back({{20, c}, 1.0});
        return from_triplets(40, t);
    }());
    {   // an empty pattern row, and a pattern without the diagonal
        Mat P = A;
        Triplets t;
        for (int32_t i = 0; i < A.n; ++i)
            for (int32_t p = A.ptr[(size_t)i]; p < A.ptr[(size_t)i + 1]; ++p)
                if (i != 7 && A.idx[(size_t)p] != i) t.push_back({{i, A.idx[(size_t)p]}, 1.0});
        both("no_diagonal_empty_row", A, from_triplets(A.n, t));
    }
    {   // breakdowns, exact by construction: rows 3 and 4 of A identical (d = 0 exactly for every pattern row that holds both), row 9 zero
        Mat D = band(12, 1);
        for (int32_t p = D.ptr[4]; p < D.ptr[5]; ++p) D.val[(size_t)p] = 0.0;
        Triplets t;
        for (int32_t i = 0; i < 12; ++i)
            for (int32_t p = D.ptr[(size_t)i]; p < D.ptr[(size_t)i + 1]; ++p)
                if (i != 3 && i != 4) t.push_back({{i, D.idx[(size_t)p]}, i == 9 ? 0.0 : D.val[(size_t)p]});
        for (int32_t i = 3; i <= 4; ++i)
            for (int32_t c = 2; c <= 5; ++c) t.push_back({{i, c}, 1.0 + 0.25 * c});
        both("breakdown", from_triplets(12, t), D);
    }
    refused_inputs(A, A, 5, 6);
    refused("q33", band(50, 16), band(50, 16));
    return failures ? 1 : 0;
}
