// What the stand-alone host programs spai_main.cpp and fsai_main.cpp share - TEST INFRASTRUCTURE ONLY: a CSR matrix and its
// builders, the complex helpers of the plain sequential loops, and the comparison of such a loop with the header's build_host()
// on W = 1 / 8 / 16 / 32 / 64 emulated lanes.  A main includes its method's header (spai.h / fsai.h) first and defines the hooks
// declared below; the plain loops themselves stay in the mains and use nothing of the product but what is passed to them.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sai_row.h"

namespace {

struct Mat {
    int64_t n = 0;
    std::vector<int32_t> ptr, idx;
    std::vector<double> val;      // real: one per entry; complex: pairs
    int64_t nnz() const { return (int64_t)idx.size(); }
};

typedef std::vector<std::pair<std::pair<int32_t, int32_t>, double>> Triplets;

uint64_t lcg_state = 0;      // a main sets its seed first
double lcg() {      // uniform in (-1, 1), deterministic
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((lcg_state >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 52) - 1.0;
}

// entries (row, col, value) -> CSR, sorted (the entries are unique)
Mat from_triplets(int64_t n, Triplets t) {
    std::sort(t.begin(), t.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    Mat m;
    m.n = n;
    m.ptr.assign((size_t)n + 1, 0);
    for (const auto& e : t) {
        m.ptr[(size_t)e.first.first + 1] += 1;
        m.idx.push_back(e.first.second);
        m.val.push_back(e.second);
    }
    for (int64_t i = 0; i < n; ++i) m.ptr[(size_t)i + 1] += m.ptr[(size_t)i];
    return m;
}

// the pattern of A * B (values 1)
Mat pattern_product(const Mat& A, const Mat& B) {
    Triplets t;
    for (int32_t i = 0; i < A.n; ++i) {
        std::vector<int32_t> cols;
        for (int32_t p = A.ptr[(size_t)i]; p < A.ptr[(size_t)i + 1]; ++p) {
            const int32_t k = A.idx[(size_t)p];
            cols.insert(cols.end(), B.idx.begin() + B.ptr[(size_t)k], B.idx.begin() + B.ptr[(size_t)k + 1]);
        }
        std::sort(cols.begin(), cols.end());
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        for (int32_t c : cols) t.push_back({{i, c}, 1.0});
    }
    return from_triplets(A.n, t);
}

struct C {
    double r, i;
};
C mul(C a, C b) { return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
C cj(C a) { return {a.r, -a.i}; }
C sub(C a, C b) { return {a.r - b.r, a.i - b.i}; }
double canon(double x) { return x != x ? __builtin_nan("") : x; }          // a NaN is stored as 0x7ff8000000000000

// ---- the hooks: what a main defines for its method ---------------------------------------------------------------------
typedef std::vector<std::vector<double>> Outputs;      // the output arrays of all rows, each with one guard element at its end
// the method's validate() on A (with n and nnz as given) and the pattern P
std::string validate(int64_t n, int64_t nnz, const Mat& A, const Mat& P, int64_t* qmax);
// the output arrays of a case, every element -7
Outputs blank_outputs(const Mat& A, const Mat& P, bool cplx);
// pattern row i (its q columns J, from position p0 of the pattern) by the plain sequential loop; true: it broke down
bool plain_row(const Mat& A, const int32_t* J, int q, int64_t i, int32_t p0, bool cplx, Outputs& want);
// all rows by the header's build_host() on W lanes; the smallest row that broke down, or -1
int64_t lanes_build(const Mat& A, const Mat& P, int qmax, int W, bool cplx, double* work, Outputs& got);
// the complex matrix that a real case is also run with
Mat complex_case(const Mat& A);

int failures = 0;

void run_case(const char* name, const Mat& A, const Mat& P, bool cplx) {
    int64_t qmax = 0;
    const std::string why = validate(A.n, A.nnz(), A, P, &qmax);
    if (!why.empty()) {
        printf("%s/%s refused: %s\n", name, cplx ? "z" : "r", why.c_str());
        failures += 1;
        return;
    }
    Outputs want = blank_outputs(A, P, cplx);
    int64_t bad_want = -1;
    for (int64_t i = 0; i < A.n; ++i) {
        const int32_t p0 = P.ptr[(size_t)i];
        if (plain_row(A, P.idx.data() + p0, P.ptr[(size_t)i + 1] - p0, i, p0, cplx, want) && bad_want < 0) bad_want = i;
    }
    for (int W : {1, 8, 16, 32, 64}) {
        std::vector<double> work((size_t)khsai::row_doubles((int)qmax, cplx), -3.0);
        Outputs got = blank_outputs(A, P, cplx);
        const int64_t bad = lanes_build(A, P, (int)qmax, W, cplx, work.data(), got);
        bool same = bad == bad_want;
        for (size_t o = 0; o < got.size(); ++o) same = same && memcmp(got[o].data(), want[o].data(), sizeof(double) * got[o].size()) == 0;
        printf("%s/%s/%d q=%lld bad=%lld bits=%s\n", name, cplx ? "z" : "r", W, (long long)qmax, (long long)bad, same ? "ok" : "DIFFER");
        if (!same) failures += 1;
    }
}

void both(const char* name, const Mat& A, const Mat& P) {
    run_case(name, A, P, false);
    run_case(name, complex_case(A), P, true);
}

void refused(const char* name, const Mat& A, const Mat& P, int64_t n_override = -1, int64_t nnz_override = -1) {
    int64_t qmax = 0;
    const std::string why = validate(n_override >= 0 ? n_override : A.n, nnz_override >= 0 ? nnz_override : A.nnz(), A, P, &qmax);
    printf("%s %s: %s\n", name, why.empty() ? "ACCEPTED" : "refused", why.c_str());
    if (why.empty()) failures += 1;
}

// every validation error of the checks that the methods share, on A and on the pattern P (whose rows `unsorted_row` and
// `duplicate_row` have two entries or more)
void refused_inputs(const Mat& A, const Mat& P, int unsorted_row, int duplicate_row) {
    refused("n_zero", A, P, 0);
    refused("n_too_large", A, P, (int64_t)1 << 31);
    refused("nnz_too_large", A, P, -1, (int64_t)1 << 31);
    Mat U = A, Up = P;
    std::swap(U.idx[(size_t)U.ptr[5]], U.idx[(size_t)U.ptr[5] + 1]);
    std::swap(Up.idx[(size_t)Up.ptr[(size_t)unsorted_row]], Up.idx[(size_t)Up.ptr[(size_t)unsorted_row] + 1]);
    refused("unsorted_A", U, P);
    refused("unsorted_pattern", A, Up);
    Mat D = A, Dp = P;
    D.idx[(size_t)D.ptr[6] + 1] = D.idx[(size_t)D.ptr[6]];
    Dp.idx[(size_t)Dp.ptr[(size_t)duplicate_row] + 1] = Dp.idx[(size_t)Dp.ptr[(size_t)duplicate_row]];
    refused("duplicate_A", D, P);
    refused("duplicate_pattern", A, Dp);
    Mat O = A, Op = P;
    O.idx[(size_t)O.ptr[8] - 1] = (int32_t)A.n;
    Op.idx[(size_t)Op.ptr[8] - 1] = (int32_t)A.n;
    refused("out_of_range_A", O, P);
    refused("out_of_range_pattern", A, Op);
    Mat N = A;
    N.idx[(size_t)N.ptr[2]] = -1;
    refused("negative_column", N, P);
    Mat Q = A;
    Q.ptr[3] = Q.ptr[2] - 1;
    refused("indptr_not_ascending", Q, P);
}

}  // namespace
