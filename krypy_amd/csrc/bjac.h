// Block-Jacobi preconditioner (kh_bjac_*): the contract, the layout of the inverses on the device and the host side of the checks.
// The kernels are in bjac.hip.
//
// A partition of 0 .. n into nblk consecutive ranges blkptr[0 .. nblk] (blkptr[0] = 0, blkptr[nblk] = n, strictly increasing,
// every size m_g = blkptr[g + 1] - blkptr[g] in 1 .. 32).  One group width W holds for a handle: the smallest of 1, 2, 4, 8, 16,
// 32 that is at least max m_g.  Lane i of a group of W lanes owns row i of its block; a wave holds 64 / W blocks (a "tile").
//
// Build.  Lane i < m_g walks row blkptr[g] + i of A (sorted, duplicate-free indices; stored zeros kept): the entries with columns
// in [blkptr[g], blkptr[g + 1]) are the dense block, absent entries are 0.  The block is inverted in place by Gauss-Jordan
// elimination with row pivoting; mag(x) = |re x| + |im x|.  Every multiply, add and divide is rounded on its own (the library is
// built without contraction); complex products are (ac - bd, ad + bc), 1 / a is Smith's formula with the numerator (1, 0), ratio
// and scale once, as in kh_ztri_create / kh_zilu0_factor:
//
//   for k = 0 .. m-1:
//       p = the smallest i >= k with the largest mag(a[i][k]), a NaN magnitude counting as +inf;  piv[k] = p
//       the block is BROKEN if mag(a[p][k]) is 0 or not finite (the arithmetic goes on as IEEE makes it)
//       swap rows k and p
//       d = 1 / a[k][k]
//       a[k][j] = a[k][j] * d  for j != k ;  a[k][k] = d
//       for every i != k:  f = a[i][k] ;  a[i][j] = a[i][j] - f * a[k][j]  for j != k ;  a[i][k] = -(f * d)
//   for k = m-1 .. 0:  swap columns k and piv[k]
//
// The result does not depend on how lanes and registers are used: the row of a lane is a register array whose every index is a
// compile-time constant under the template on W, rows travel between lanes by shuffles of width W, the pivot search is a
// butterfly over a TOTAL order (magnitude, then the smaller row), the column swaps are folded into the addresses of the stores.
//
// Storage.  Element (i, j) of block g is entry  ((g / (64/W)) * W + j) * 64 + (g % (64/W)) * W + i  of the array of inverses
// (complex: of (re, im) pairs): a wave's load of column j of its 64 / W blocks is one contiguous line of 64 entries.  The build
// writes 0 into the padding (i or j >= m_g, blocks past nblk in the last tile); nobody reads it back.
//
// Apply, y = D^-1 x.  Lane i < m_g loads x[blkptr[g] + i] and forms y_i = ((0 + a[i][0] x_0) + a[i][1] x_1) + ... for
// j = 0 .. m_g - 1, rising j, separate multiply and add - bit for bit the CSR SpMV of the block-diagonal matrix that stores all
// m_g^2 entries of every block.  Lanes with i >= m_g and groups with g >= nblk load and store nothing.
#pragma once
#include <stdint.h>

#include <string>

namespace khbjac {

constexpr int MAX_BLOCK = 32;
constexpr int WAVE = 64;

// the smallest of 1, 2, 4, 8, 16, 32 that is at least mmax
inline int group_width(int64_t mmax) {
    int W = 1;
    while (W < mmax) W *= 2;
    return W;
}

// tiles of 64 / W blocks
inline int64_t tiles(int64_t nblk, int W) { return (nblk + WAVE / W - 1) / (WAVE / W); }

// entries (doubles, or (re, im) pairs) of the array of inverses
inline int64_t entries(int64_t nblk, int W) { return tiles(nblk, W) * W * WAVE; }

// where element (i, j) of block g sits
inline int64_t at(int64_t g, int i, int j, int W) {
    const int per = WAVE / W;
    return ((g / per) * W + j) * WAVE + (g % per) * W + i;
}

// Checks A's pattern and the partition.  Returns "" or what is wrong (the row or the block named); *mmax: the largest block.
inline std::string validate(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int64_t nblk, const int32_t* blkptr,
                            int64_t* mmax) {
    auto str = [](int64_t v) { return std::to_string((long long)v); };
    if (n < 1 || n > (int64_t)0x7fffffff) return "n = " + str(n) + " out of range";
    if (nnz < 0 || nnz > (int64_t)0x7fffffff) return "nnz = " + str(nnz) + " out of range (int32 row pointers)";
    if (nblk < 1 || nblk > n) return "nblk = " + str(nblk) + " out of range for n = " + str(n);
    if (indptr == nullptr || blkptr == nullptr || (nnz > 0 && indices == nullptr)) return "NULL array";
    if (indptr[0] != 0 || indptr[n] != nnz) return "indptr does not run from 0 to nnz";
    for (int64_t i = 0; i < n; ++i) {
        if (indptr[i + 1] < indptr[i] || indptr[i + 1] > nnz) return "indptr decreases or leaves the arrays at row " + str(i);
        for (int32_t p = indptr[i]; p < indptr[i + 1]; ++p) {
            if (indices[p] < 0 || indices[p] >= n) return "column " + str(indices[p]) + " out of range in row " + str(i);
            if (p > indptr[i] && indices[p] <= indices[p - 1]) return "unsorted or duplicate indices in row " + str(i);
        }
    }
    if (blkptr[0] != 0) return "blkptr does not start at 0 (block 0)";
    int64_t big = 0;
    for (int64_t g = 0; g < nblk; ++g) {
        const int64_t m = (int64_t)blkptr[g + 1] - blkptr[g];
        if (m < 1) return "blkptr is not strictly increasing at block " + str(g);
        if (m > MAX_BLOCK) return "block " + str(g) + " has " + str(m) + " rows, more than " + str(MAX_BLOCK);
        if (blkptr[g + 1] > n) return "block " + str(g) + " ends at " + str(blkptr[g + 1]) + ", behind n = " + str(n);
        big = m > big ? m : big;
    }
    if (blkptr[nblk] != n) return "blkptr ends at " + str(blkptr[nblk]) + ", not at n = " + str(n) + " (block " + str(nblk - 1) + ")";
    *mmax = big;
    return "";
}

// the inverses out of the device layout: dense row-major m_g x m_g arrays, one after another in block order (w = 1: real,
// w = 2: (re, im) pairs)
inline void unpack(const double* inv, int64_t nblk, const int32_t* blkptr, int W, int w, double* out) {
    int64_t o = 0;
    for (int64_t g = 0; g < nblk; ++g) {
        const int m = blkptr[g + 1] - blkptr[g];
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j)
                for (int c = 0; c < w; ++c) out[o++] = inv[at(g, i, j, W) * w + c];
    }
}

}  // namespace khbjac
