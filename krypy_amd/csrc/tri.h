// Sparse triangular solve by level scheduling: the HOST analysis (tri.hip holds the kernels and the C entry points).
// Plain C++, no HIP call: the header compiles alone (tests/support/tri_analysis_main.cpp builds it with the host
// sanitizers and runs it on the CPU).
//
//   level[i] = 1 + max(level[j]) over the off-diagonal entries (i, j) of row i (0-based here: a row without any is level
//   0), one pass, ascending for a lower and descending for an upper triangle.  Rows of one level do not depend on each
//   other.  They are grouped by level with a counting sort and ordered inside a level by (row length descending, row
//   index ascending), cut into SLICES of 64 rows - one wavefront, a slice never spans two levels - and stored as sliced
//   ELL: slot-major, vals[base + k * 64 + lane] / cols[...], padded to the slice's longest row (its first).  Per lane:
//   the row id (-1: no row), the number of off-diagonal entries, the diagonal.  A padding slot holds column 0 and value
//   0 and is never read: the kernels skip it by predicate (k < len).
//
// Launch plan: a maximal run of consecutive levels with at most `narrow_rows` rows each is ONE launch of ONE workgroup
// that walks the levels with a barrier between them (narrow run); every other level is one launch of as many workgroups
// as its slices need (wide).  No launch ever waits for another workgroup.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace khtri {

constexpr int SLICE = 64;            // rows per slice: one wave64
constexpr int WIDE_WAVES = 4;        // slices per workgroup of a wide launch
constexpr int NARROW_MAX_THREADS = 1024;
constexpr int64_t NARROW_ROWS_DEFAULT = 1024;

struct Launch {
    int narrow;          // 1: one workgroup walks levels [lev0, lev0 + nlev); 0: level lev0, one wave per slice
    int32_t lev0, nlev;
    int32_t slice0, nslices;
    int threads;         // workgroup size
};

struct Plan {
    int64_t n = 0, nnz = 0, nlevels = 0, widest = 0, longest = 0, slots = 0, nslices = 0;
    int64_t n_wide = 0, n_narrow = 0;
    std::vector<int32_t> level;        // [n]
    std::vector<int32_t> order;        // [n] rows in level order
    std::vector<int32_t> lev_ptr;      // [nlevels + 1] into order
    std::vector<int32_t> lev_slice;    // [nlevels + 1] first slice of every level
    std::vector<int64_t> slice_base;   // [nslices] first slot of the slice
    std::vector<int32_t> slice_slots;  // [nslices] slots per lane (the slice's longest row)
    std::vector<int32_t> row_id;       // [nslices * 64], -1: lane without a row
    std::vector<int32_t> row_len;      // [nslices * 64] off-diagonal entries of the lane's row
    std::vector<int32_t> cols;         // [slots]
    std::vector<double> vals;          // [slots * w]
    std::vector<double> diag;          // [nslices * 64 * w] (1 where there is no row / for a unit diagonal)
    std::vector<Launch> launches;
};

// Checks the CSR input and builds the plan.  w = 1: real data, w = 2: (re, im) pairs.  Returns "" or what is wrong.
inline std::string analyse(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int w,
                           bool lower, bool unit, int64_t narrow_rows, Plan& p) {
    auto str = [](int64_t v) { return std::to_string((long long)v); };
    if (n < 1 || n > (int64_t)0x7fffffff - 2 * SLICE) return "n = " + str(n) + " out of range";
    if (nnz < 0 || nnz > (int64_t)0x7fffffff) return "nnz = " + str(nnz) + " out of range (int32 row pointers)";
    if (!indptr || (nnz > 0 && (!indices || !data))) return "NULL array";
    if (indptr[0] != 0 || indptr[n] != nnz) return "indptr[0] != 0 or indptr[n] != nnz";
    p = Plan();
    p.n = n;
    p.nnz = nnz;
    // ---- validation, off-diagonal counts ----
    std::vector<int32_t> len((size_t)n), dpos((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = indptr[i], b = indptr[i + 1];
        if (a > b || b > nnz) return "indptr not ascending at row " + str(i);
        int32_t cnt = 0;
        for (int64_t q = a; q < b; ++q) {
            const int64_t c = indices[q];
            if (c < 0 || c >= n) return "column " + str(c) + " out of range in row " + str(i);
            if (q > a && indices[q - 1] >= c)
                return std::string(indices[q - 1] == c ? "duplicate" : "unsorted") + " column indices in row " + str(i);
            if (c == i) dpos[(size_t)i] = (int32_t)q;
            else if (lower ? c > i : c < i)
                return "entry (" + str(i) + ", " + str(c) + ") on the wrong side of the diagonal of " + (lower ? "a lower" : "an upper") +
                       " triangle";
            else cnt += 1;
        }
        if (!unit) {
            const int32_t q = dpos[(size_t)i];
            if (q < 0) return "row " + str(i) + " has no diagonal entry (unit_diag = 0)";
            bool zero = true;
            for (int c = 0; c < w; ++c) zero = zero && data[(int64_t)q * w + c] == 0.0;
            if (zero) return "zero diagonal entry in row " + str(i) + " (unit_diag = 0)";
        }
        len[(size_t)i] = cnt;
        p.longest = std::max<int64_t>(p.longest, cnt);
    }
    // ---- levels ----
    p.level.assign((size_t)n, 0);
    int32_t maxlev = 0;
    for (int64_t s = 0; s < n; ++s) {
        const int64_t i = lower ? s : n - 1 - s;
        int32_t lv = 0;
        for (int64_t q = indptr[i]; q < indptr[i + 1]; ++q)
            if (indices[q] != i) lv = std::max(lv, p.level[(size_t)indices[q]] + 1);
        p.level[(size_t)i] = lv;
        maxlev = std::max(maxlev, lv);
    }
    p.nlevels = (int64_t)maxlev + 1;
    // ---- order: a stable counting sort by row length (descending), then a stable one by level ----
    std::vector<int32_t> bylen((size_t)n);
    {
        std::vector<int64_t> cnt((size_t)p.longest + 2, 0);
        for (int64_t i = 0; i < n; ++i) cnt[(size_t)(p.longest - len[(size_t)i]) + 1] += 1;
        for (size_t k = 1; k < cnt.size(); ++k) cnt[k] += cnt[k - 1];
        for (int64_t i = 0; i < n; ++i) bylen[(size_t)cnt[(size_t)(p.longest - len[(size_t)i])]++] = (int32_t)i;
    }
    p.lev_ptr.assign((size_t)p.nlevels + 1, 0);
    for (int64_t i = 0; i < n; ++i) p.lev_ptr[(size_t)p.level[(size_t)i] + 1] += 1;
    for (int64_t l = 0; l < p.nlevels; ++l) {
        p.widest = std::max<int64_t>(p.widest, p.lev_ptr[(size_t)l + 1]);
        p.lev_ptr[(size_t)l + 1] += p.lev_ptr[(size_t)l];
    }
    p.order.assign((size_t)n, 0);
    {
        std::vector<int32_t> at(p.lev_ptr.begin(), p.lev_ptr.end() - 1);
        for (int64_t s = 0; s < n; ++s) {
            const int32_t i = bylen[(size_t)s];
            p.order[(size_t)at[(size_t)p.level[(size_t)i]]++] = i;
        }
    }
    // ---- slices ----
    p.lev_slice.assign((size_t)p.nlevels + 1, 0);
    for (int64_t l = 0; l < p.nlevels; ++l) {
        const int64_t rows = p.lev_ptr[(size_t)l + 1] - p.lev_ptr[(size_t)l];
        p.lev_slice[(size_t)l + 1] = p.lev_slice[(size_t)l] + (int32_t)((rows + SLICE - 1) / SLICE);
    }
    p.nslices = p.lev_slice[(size_t)p.nlevels];
    p.slice_base.assign((size_t)p.nslices, 0);
    p.slice_slots.assign((size_t)p.nslices, 0);
    p.row_id.assign((size_t)p.nslices * SLICE, -1);
    p.row_len.assign((size_t)p.nslices * SLICE, 0);
    p.diag.assign((size_t)p.nslices * SLICE * w, 0.0);
    for (size_t k = 0; k < p.diag.size(); k += w) p.diag[k] = 1.0;
    int64_t slots = 0;
    for (int64_t l = 0; l < p.nlevels; ++l) {
        for (int64_t s = p.lev_slice[(size_t)l]; s < p.lev_slice[(size_t)l + 1]; ++s) {
            const int64_t r0 = p.lev_ptr[(size_t)l] + (s - p.lev_slice[(size_t)l]) * SLICE;
            const int64_t r1 = std::min<int64_t>(r0 + SLICE, p.lev_ptr[(size_t)l + 1]);
            const int32_t ns = len[(size_t)p.order[(size_t)r0]];      // the longest row of the slice comes first
            p.slice_base[(size_t)s] = slots;
            p.slice_slots[(size_t)s] = ns;
            slots += (int64_t)ns * SLICE;
            for (int64_t r = r0; r < r1; ++r) {
                const int32_t i = p.order[(size_t)r];
                const size_t lane = (size_t)(s * SLICE + (r - r0));
                p.row_id[lane] = i;
                p.row_len[lane] = len[(size_t)i];
                if (!unit)
                    for (int c = 0; c < w; ++c) p.diag[lane * w + c] = data[(int64_t)dpos[(size_t)i] * w + c];
            }
        }
    }
    p.slots = slots;
    p.cols.assign((size_t)slots, 0);
    p.vals.assign((size_t)slots * w, 0.0);
    for (int64_t s = 0; s < p.nslices; ++s) {
        for (int lane = 0; lane < SLICE; ++lane) {
            const int32_t i = p.row_id[(size_t)s * SLICE + lane];
            if (i < 0) continue;
            int64_t k = 0;
            for (int64_t q = indptr[i]; q < indptr[i + 1]; ++q) {      // ascending column order
                if (indices[q] == i) continue;
                const int64_t at = p.slice_base[(size_t)s] + k * SLICE + lane;
                p.cols[(size_t)at] = indices[q];
                for (int c = 0; c < w; ++c) p.vals[(size_t)at * w + c] = data[q * w + c];
                k += 1;
            }
        }
    }
    // ---- launches ----
    if (narrow_rows < 0) narrow_rows = 0;
    for (int64_t l = 0; l < p.nlevels;) {
        auto rows = [&](int64_t m) { return (int64_t)(p.lev_ptr[(size_t)m + 1] - p.lev_ptr[(size_t)m]); };
        Launch L;
        if (rows(l) <= narrow_rows) {
            int64_t e = l, wmax = 0;
            while (e < p.nlevels && rows(e) <= narrow_rows) wmax = std::max(wmax, rows(e++));
            L.narrow = 1;
            L.lev0 = (int32_t)l;
            L.nlev = (int32_t)(e - l);
            L.slice0 = p.lev_slice[(size_t)l];
            L.nslices = p.lev_slice[(size_t)e] - L.slice0;
            L.threads = (int)std::min<int64_t>(NARROW_MAX_THREADS, (wmax + SLICE - 1) / SLICE * SLICE);
            p.n_narrow += 1;
            l = e;
        } else {
            L.narrow = 0;
            L.lev0 = (int32_t)l;
            L.nlev = 1;
            L.slice0 = p.lev_slice[(size_t)l];
            L.nslices = p.lev_slice[(size_t)l + 1] - L.slice0;
            L.threads = WIDE_WAVES * SLICE;
            p.n_wide += 1;
            l += 1;
        }
        p.launches.push_back(L);
    }
    return "";
}

// The arithmetic of the kernels on the host, walking the plan in launch order (the stand-alone program checks it against a
// row-by-row substitution on the CSR input; real data only).
inline void solve_host(const Plan& p, bool unit, const double* b, double* x) {
    for (int64_t s = 0; s < p.nslices; ++s)
        for (int lane = 0; lane < SLICE; ++lane) {
            const size_t at = (size_t)s * SLICE + lane;
            const int32_t i = p.row_id[at];
            if (i < 0) continue;
            double acc = b[i];
            for (int32_t k = 0; k < p.slice_slots[(size_t)s]; ++k)
                if (k < p.row_len[at]) {
                    const size_t q = (size_t)(p.slice_base[(size_t)s] + (int64_t)k * SLICE + lane);
                    acc = acc - p.vals[q] * x[p.cols[q]];
                }
            x[i] = unit ? acc : acc / p.diag[at];
        }
}

}  // namespace khtri
