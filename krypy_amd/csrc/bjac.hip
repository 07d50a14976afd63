// Block-Jacobi preconditioner on the device (kh_bjac_*): the diagonal blocks of a CSR matrix, given by a partition with blocks of
// at most 32 rows, are gathered and inverted by ONE launch and stay on the device in the layout the apply kernel reads; an
// application y = D^-1 x is one streaming launch per column - fp64 and c128 from one templated implementation.  No reference
// counterpart (the reference takes any callable as M, Ml, Mr).  Contract, arithmetic and layout: bjac.h.
//
// k_bjac_build<Z, W>: one block per group of W lanes, 64 / W blocks per wave, grid-stride over the tiles.  The row of a lane is a
// register array, every index a compile-time constant (the loops over k and j are unrolled on W); a Gauss-Jordan step costs one
// shuffle per column - every lane reads the pivot row from lane p, lane p reads row k, which is the row swap - and a butterfly
// of log2 W steps for the pivot.  The column swaps never move a register: lane c tracks where working column c ends up, and the
// store of column c goes there.  Steps k >= m_g of a smaller block run with their effect masked, so that every lane of a wave
// reaches every shuffle.
//
// k_bjac_apply<Z, W>: a wave loads column j of its 64 / W inverses as one line of 64 entries (W non-temporal loads, all in flight:
// a read-once stream like the CSR kernel's, 87.5 -> 79.6 us at 10^7 rows in blocks of 4, 138.4 -> 118.2 us in blocks of 8), x_j
// reaches the lanes of a group by a shuffle of width W, the sum runs over j < m_g in rising order, y leaves through a
// non-temporal store.  No LDS, no barrier, no scratch; neither kernel waits for another workgroup.
#include <float.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <type_traits>

#include "bjac.h"
#include "kh_internal.h"

using namespace kh;

struct kh_bjac_s {
    kh_ctx ctx = nullptr;
    int64_t n = 0, nnz = 0, nblk = 0, mmax = 0, ntile = 0, entries = 0, bytes = 0, grid = 0, bad = -1;
    int cplx = 0, W = 1;
    std::vector<int32_t> blkptr_host;                       // kh_bjac_values unpacks through it
    std::vector<void*> owned;                               // every device allocation
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int32_t *indptr = nullptr, *indices = nullptr, *blkptr = nullptr, *bad_word = nullptr;
    double *data = nullptr, *inv = nullptr;
};

namespace {

constexpr int32_t NONE = 0x7f7f7f7f;      // what hipMemsetAsync(.., 0x7f, 4) arms the breakdown word with
constexpr int WAVES = BS / khbjac::WAVE;

typedef double v2f64 __attribute__((ext_vector_type(2)));

// ---- the two number types: double, and (re, im) as a plain pair (two registers, nothing the optimiser has to look through) ----
struct __attribute__((aligned(16))) Cx {
    double x, y;
};
__device__ __forceinline__ Cx make_cx(double x, double y) {
    Cx r;
    r.x = x;
    r.y = y;
    return r;
}
template <bool Z>
struct Num {
    typedef double T;
};
template <>
struct Num<true> {
    typedef Cx T;
};

__device__ __forceinline__ double zero_of(double) { return 0.0; }
__device__ __forceinline__ Cx zero_of(Cx) { return make_cx(0.0, 0.0); }
__device__ __forceinline__ double mul(double a, double b) { return a * b; }
__device__ __forceinline__ Cx mul(Cx a, Cx b) { return make_cx(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double add(double a, double b) { return a + b; }
__device__ __forceinline__ Cx add(Cx a, Cx b) { return make_cx(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double sub(double a, double b) { return a - b; }
__device__ __forceinline__ Cx sub(Cx a, Cx b) { return make_cx(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double neg(double a) { return -a; }
__device__ __forceinline__ Cx neg(Cx a) { return make_cx(-a.x, -a.y); }
__device__ __forceinline__ double mag(double a) { return fabs(a); }
__device__ __forceinline__ double mag(Cx a) { return fabs(a.x) + fabs(a.y); }
__device__ __forceinline__ double recip(double a) { return 1.0 / a; }
// Smith's quotient (1, 0) / a: ratio and scale once
__device__ __forceinline__ Cx recip(Cx a) {
    const double nx = 1.0, ny = 0.0;
    const bool big_re = fabs(a.x) >= fabs(a.y);
    const double rat = big_re ? a.y / a.x : a.x / a.y;
    const double scl = 1.0 / (big_re ? (a.x + a.y * rat) : (a.y + a.x * rat));
    if (big_re) return make_cx((nx + ny * rat) * scl, (ny - nx * rat) * scl);
    return make_cx((nx * rat + ny) * scl, (ny * rat - nx) * scl);
}
template <int W>
__device__ __forceinline__ double shfl(double a, int src) {
    return __shfl(a, src, W);
}
template <int W>
__device__ __forceinline__ Cx shfl(Cx a, int src) {
    return make_cx(__shfl(a.x, src, W), __shfl(a.y, src, W));
}
__device__ __forceinline__ double pick(bool c, double a, double b) { return c ? a : b; }
__device__ __forceinline__ Cx pick(bool c, Cx a, Cx b) { return make_cx(c ? a.x : b.x, c ? a.y : b.y); }
// loads and stores of a pair part by part (the two merge into one 16-byte access; a copy of the whole struct would keep the
// register arrays in memory)
__device__ __forceinline__ double load(const double* p) { return *p; }
__device__ __forceinline__ Cx load(const Cx* p) { return make_cx(p->x, p->y); }
__device__ __forceinline__ void store(double* p, double v) { *p = v; }
__device__ __forceinline__ void store(Cx* p, Cx v) {
    p->x = v.x;
    p->y = v.y;
}
__device__ __forceinline__ double load_nt(const double* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ Cx load_nt(const Cx* p) {
    const v2f64 t = __builtin_nontemporal_load(reinterpret_cast<const v2f64*>(p));
    return make_cx(t.x, t.y);
}
__device__ __forceinline__ void store_nt(double* p, double v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store_nt(Cx* p, Cx v) {
    v2f64 t;
    t.x = v.x;
    t.y = v.y;
    __builtin_nontemporal_store(t, reinterpret_cast<v2f64*>(p));
}

// f(integral_constant<int, K>) for K = 0 .. N-1: the index is a constant inside f, whatever the unroller decides
template <int K, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (K < N) {
        f(std::integral_constant<int, K>());
        static_for<K + 1, N>(f);
    }
}

template <bool Z, int W>
__global__ __launch_bounds__(BS) void k_bjac_build(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                   const typename Num<Z>::T* __restrict__ data, const int32_t* __restrict__ blkptr,
                                                   int64_t nblk, int64_t ntile, typename Num<Z>::T* __restrict__ inv, int32_t* bad) {
    typedef typename Num<Z>::T T;
    constexpr int PER = khbjac::WAVE / W;
    const int lane = threadIdx.x & 63, i = lane % W;
    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); tile < ntile; tile += (int64_t)gridDim.x * WAVES) {
        const int64_t g = tile * PER + lane / W;
        int32_t b0 = 0, m = 0;
        if (g < nblk) {
            b0 = blkptr[g];
            m = blkptr[g + 1] - b0;
        }
        // ---- the row of this lane out of A: first entry at or behind b0 by bisection, then a merge walk over the W columns ----
        T a[W];
        {
            int32_t p = 0, pend = 0;
            if (i < m) {
                p = indptr[b0 + i];
                pend = indptr[b0 + i + 1];
                int32_t hi = pend;
                while (p < hi) {
                    const int32_t mid = p + (hi - p) / 2;
                    if (indices[mid] < b0) p = mid + 1;
                    else hi = mid;
                }
            }
#pragma unroll
            for (int j = 0; j < W; ++j) {
                a[j] = zero_of(T());
                if (j < m && p < pend && indices[p] == b0 + j) {
                    a[j] = load(data + p);
                    ++p;
                }
            }
        }
        // ---- Gauss-Jordan with row pivoting ----
        int piv[W];
        bool broken = false;
        static_for<0, W>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const bool act = k < m;
            // the pivot: largest key, then the smaller row - a total order, so every lane of the group ends with the same pair
            const double mk = mag(a[k]);
            double key = (i >= k && i < m) ? (mk != mk ? (double)INFINITY : mk) : -1.0;
            int p = i;
#pragma unroll
            for (int off = W / 2; off >= 1; off /= 2) {
                const double ok = __shfl_xor(key, off, W);
                const int op = __shfl_xor(p, off, W);
                if (ok > key || (ok == key && op < p)) {
                    key = ok;
                    p = op;
                }
            }
            p = act ? p : k;
            piv[k] = p;
            // every lane reads the pivot row from lane p; lane p reads row k and keeps it: the swap
            T row[W];
            const int src = (i == p) ? k : p;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const T t = shfl<W>(a[j], src);
                row[j] = pick(i == p, a[j], t);      // (pick, not ?: - a conditional on two struct lvalues selects an address)
                a[j] = pick(act && i == p, t, a[j]);
            }
            const double pm = mag(row[k]);
            broken = broken || (act && (pm == 0.0 || !(pm <= DBL_MAX)));
            const T d = recip(row[k]);
#pragma unroll
            for (int j = 0; j < W; ++j) row[j] = pick(j == k, d, mul(row[j], d));
            const T f = a[k];
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const T other = pick(j == k, neg(mul(f, d)), sub(a[j], mul(f, row[j])));
                a[j] = pick(act, pick(i == k, row[j], other), a[j]);
            }
        });
        if (broken && i == 0 && g < nblk) atomicMin(bad, (int32_t)g);
        // ---- the column swaps, as addresses: lane c follows working column c to its final place ----
        int pos = i;
        static_for<0, W>([&](auto kc) {
            constexpr int k = W - 1 - decltype(kc)::value;
            pos = (pos == k) ? piv[k] : (pos == piv[k]) ? k : pos;
        });
        T* const out = inv + tile * (W * khbjac::WAVE) + lane;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int dest = __shfl(pos, c, W);
            store(out + (int64_t)dest * khbjac::WAVE, pick(i < m && c < m, a[c], zero_of(T())));
        }
    }
}

template <bool Z, int W>
__global__ __launch_bounds__(BS) void k_bjac_apply(const typename Num<Z>::T* __restrict__ inv, const int32_t* __restrict__ blkptr,
                                                   int64_t nblk, int64_t ntile, const typename Num<Z>::T* __restrict__ x,
                                                   typename Num<Z>::T* __restrict__ y) {
    typedef typename Num<Z>::T T;
    constexpr int PER = khbjac::WAVE / W;
    const int lane = threadIdx.x & 63, i = lane % W;
    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); tile < ntile; tile += (int64_t)gridDim.x * WAVES) {
        const int64_t g = tile * PER + lane / W;
        int32_t b0 = 0, m = 0;
        if (g < nblk) {
            b0 = blkptr[g];
            m = blkptr[g + 1] - b0;
        }
        T xi = zero_of(T());
        if (i < m) xi = load(x + (int64_t)b0 + i);
        const T* const col = inv + tile * (W * khbjac::WAVE) + lane;
        T a[W];
#pragma unroll
        for (int j = 0; j < W; ++j) a[j] = load_nt(col + j * khbjac::WAVE);
        T acc = zero_of(T());
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const T xj = shfl<W>(xi, j);
            acc = pick(j < m, add(acc, mul(a[j], xj)), acc);
        }
        if (i < m) store_nt(y + (int64_t)b0 + i, acc);
    }
}

template <bool Z, int W>
void launch_build_zw(kh_bjac h, unsigned grid) {
    typedef typename Num<Z>::T T;
    hipLaunchKernelGGL((k_bjac_build<Z, W>), dim3(grid), dim3(BS), 0, h->ctx->stream, h->indptr, h->indices,
                       reinterpret_cast<const T*>(h->data), h->blkptr, h->nblk, h->ntile, reinterpret_cast<T*>(h->inv), h->bad_word);
}

template <bool Z, int W>
void launch_apply_zw(kh_bjac h, unsigned grid, const double* x, double* y) {
    typedef typename Num<Z>::T T;
    hipLaunchKernelGGL((k_bjac_apply<Z, W>), dim3(grid), dim3(BS), 0, h->ctx->stream, reinterpret_cast<const T*>(h->inv), h->blkptr,
                       h->nblk, h->ntile, reinterpret_cast<const T*>(x), reinterpret_cast<T*>(y));
}

template <bool Z>
void launch_build(kh_bjac h, unsigned grid) {
    switch (h->W) {
        case 1: launch_build_zw<Z, 1>(h, grid); break;
        case 2: launch_build_zw<Z, 2>(h, grid); break;
        case 4: launch_build_zw<Z, 4>(h, grid); break;
        case 8: launch_build_zw<Z, 8>(h, grid); break;
        case 16: launch_build_zw<Z, 16>(h, grid); break;
        default: launch_build_zw<Z, 32>(h, grid); break;
    }
}

template <bool Z>
void launch_apply(kh_bjac h, unsigned grid, const double* x, double* y) {
    switch (h->W) {
        case 1: launch_apply_zw<Z, 1>(h, grid, x, y); break;
        case 2: launch_apply_zw<Z, 2>(h, grid, x, y); break;
        case 4: launch_apply_zw<Z, 4>(h, grid, x, y); break;
        case 8: launch_apply_zw<Z, 8>(h, grid, x, y); break;
        case 16: launch_apply_zw<Z, 16>(h, grid, x, y); break;
        default: launch_apply_zw<Z, 32>(h, grid, x, y); break;
    }
}

// workgroups of both kernels: one wave per tile, never more than the reduction grid
unsigned bjac_grid(kh_ctx ctx, int64_t ntile) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((ntile + WAVES - 1) / WAVES, ctx->nb));
}

int dev_alloc(kh_bjac h, void** dst, size_t bytes) {
    bytes = std::max<size_t>(bytes, 8);
    const hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) {
        *dst = nullptr;
        return fail(KH_ERR_NOMEM, "kh_bjac_create: hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    }
    h->owned.push_back(*dst);
    h->bytes += (int64_t)bytes;
    return 0;
}

template <typename T>
int to_device(kh_bjac h, T** dst, const T* src, size_t count) {
    KH_TRY(dev_alloc(h, reinterpret_cast<void**>(dst), sizeof(T) * count));
    if (count) KH_HIP(hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return 0;
}

// the build launch on values that are already on the device; refreshes the breakdown word and the counters
int build(kh_bjac h) {
    kh_ctx ctx = h->ctx;
    KH_HIP(hipMemsetAsync(h->bad_word, 0x7f, sizeof(int32_t), ctx->stream));
    KH_HIP(hipEventRecord(h->ev0, ctx->stream));
    const unsigned grid = bjac_grid(ctx, h->ntile);
    if (h->cplx) launch_build<true>(h, grid);
    else launch_build<false>(h, grid);
    KH_HIP(hipGetLastError());
    KH_HIP(hipEventRecord(h->ev1, ctx->stream));
    int32_t bad = NONE;
    KH_HIP(hipMemcpyAsync(&bad, h->bad_word, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    KH_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    KH_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    ctx->bjac_device_us = (int64_t)((double)ms * 1000.0);
    ctx->n_bjac_build += 1;
    h->grid = grid;
    h->bad = bad == NONE ? -1 : (int64_t)bad;
    return 0;
}

int fill_info(kh_bjac h, int64_t info[8]) {
    const int64_t res[8] = {h->n, h->nnz, h->nblk, h->mmax, h->W, h->grid, h->bytes, h->bad};
    for (int i = 0; i < 8; ++i) info[i] = res[i];
    return 0;
}

int bjac_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t nblk,
                const int32_t* blkptr, kh_bjac* out, int64_t info[8], int cplx) {
    const char* who = cplx ? "kh_zbjac_create" : "kh_bjac_create";
    KH_ARG(ctx != nullptr && out != nullptr && info != nullptr, "%s: NULL", who);
    if (kh_multi(ctx) || ctx->comm != nullptr)
        return fail(KH_ERR_UNSUPPORTED, "%s: the context has a communicator - the blocks of a sharded matrix are not implemented", who);
    kh_bjac h = nullptr;
    try {
        int64_t mmax = 0;
        const std::string why = khbjac::validate(n, nnz, indptr, indices, nblk, blkptr, &mmax);
        KH_ARG(why.empty(), "%s: %s", who, why.c_str());
        KH_ARG(nnz == 0 || data != nullptr, "%s: NULL array", who);
        h = new kh_bjac_s();
        h->ctx = ctx;
        h->n = n;
        h->nnz = nnz;
        h->nblk = nblk;
        h->mmax = mmax;
        h->cplx = cplx != 0;
        h->W = khbjac::group_width(mmax);
        h->ntile = khbjac::tiles(nblk, h->W);
        h->entries = khbjac::entries(nblk, h->W);
        h->blkptr_host.assign(blkptr, blkptr + nblk + 1);
        const size_t w = cplx ? 2 : 1;
        auto body = [&]() -> int {
            KH_TRY(to_device(h, &h->indptr, indptr, (size_t)n + 1));
            KH_TRY(to_device(h, &h->indices, indices, (size_t)nnz));
            KH_TRY(to_device(h, &h->data, data, (size_t)nnz * w));
            KH_TRY(to_device(h, &h->blkptr, blkptr, (size_t)nblk + 1));
            KH_TRY(dev_alloc(h, reinterpret_cast<void**>(&h->inv), sizeof(double) * w * (size_t)h->entries));
            KH_TRY(dev_alloc(h, reinterpret_cast<void**>(&h->bad_word), sizeof(int32_t)));
            KH_HIP(hipEventCreate(&h->ev0));
            KH_HIP(hipEventCreate(&h->ev1));
            return build(h);
        };
        const int rc = body();
        if (rc != 0) {          // nothing half-built stays behind
            kh_bjac_free(h);
            return rc;
        }
    } catch (const std::bad_alloc&) {
        if (h) kh_bjac_free(h);
        return fail(KH_ERR_NOMEM, "%s: out of host memory", who);
    }
    *out = h;
    return fill_info(h, info);
}

int check_col(kh_vec v, int64_t col, int64_t ncols, int64_t rn, const char* what) {
    KH_ARG(v != nullptr, "kh_bjac_apply(%s): NULL block", what);
    KH_ARG(col >= 0 && ncols >= 0 && col + ncols <= v->ncols, "kh_bjac_apply(%s): columns [%lld, %lld) of a block with %lld", what,
           (long long)col, (long long)(col + ncols), (long long)v->ncols);
    KH_ARG(v->n == rn, "kh_bjac_apply(%s): the block has %lld doubles per column, the preconditioner needs %lld (n does not match, or "
                       "a real handle meets complex blocks / a complex handle real ones)",
           what, (long long)v->n, (long long)rn);
    return 0;
}

}  // namespace

extern "C" {

int kh_bjac_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t nblk,
                   const int32_t* blkptr, kh_bjac* out, int64_t info[8]) {
    return bjac_create(ctx, n, nnz, indptr, indices, data, nblk, blkptr, out, info, 0);
}

int kh_zbjac_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                    int64_t nblk, const int32_t* blkptr, kh_bjac* out, int64_t info[8]) {
    return bjac_create(ctx, n, nnz, indptr, indices, data_re_im, nblk, blkptr, out, info, 1);
}

int kh_bjac_free(kh_bjac h) {
    if (!h) return 0;
    (void)hipStreamSynchronize(h->ctx->stream);
    for (void* p : h->owned) (void)hipFree(p);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
    return 0;
}

int kh_bjac_update(kh_bjac h, const double* data) {
    KH_ARG(h != nullptr, "kh_bjac_update: NULL");
    KH_ARG(h->nnz == 0 || data != nullptr, "kh_bjac_update: NULL array");
    const size_t bytes = sizeof(double) * (h->cplx ? 2 : 1) * (size_t)h->nnz;
    if (bytes) KH_HIP(hipMemcpyAsync(h->data, data, bytes, hipMemcpyHostToDevice, h->ctx->stream));
    return build(h);
}

int kh_bjac_info(kh_bjac h, int64_t info[8]) {
    KH_ARG(h != nullptr && info != nullptr, "kh_bjac_info: NULL");
    return fill_info(h, info);
}

int kh_bjac_apply(kh_ctx ctx, kh_bjac h, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol, int64_t ncols) {
    KH_ARG(ctx != nullptr && h != nullptr, "kh_bjac_apply: NULL");
    KH_ARG(h->ctx == ctx, "kh_bjac_apply: the handle belongs to another context");
    const int64_t rn = h->cplx ? 2 * h->n : h->n;
    KH_TRY(check_col(X, xcol, ncols, rn, "x"));
    KH_TRY(check_col(Y, ycol, ncols, rn, "y"));
    // a lane reads entries of x that other lanes' stores to y would overwrite: not in place
    KH_ARG(!(X == Y && (xcol < ycol ? ycol - xcol : xcol - ycol) < ncols),
           "kh_bjac_apply: columns [%lld, %lld) and [%lld, %lld) of one block overlap", (long long)xcol, (long long)(xcol + ncols),
           (long long)ycol, (long long)(ycol + ncols));
    const unsigned grid = bjac_grid(ctx, h->ntile);
    for (int64_t c = 0; c < ncols; ++c) {
        if (h->cplx) launch_apply<true>(h, grid, X->col(xcol + c), Y->col(ycol + c));
        else launch_apply<false>(h, grid, X->col(xcol + c), Y->col(ycol + c));
        KH_HIP(hipGetLastError());
        ctx->n_bjac_apply += 1;
    }
    chain_blk_touch(ctx, Y);
    return 0;
}

int kh_bjac_values(kh_bjac h, double* out) {
    KH_ARG(h != nullptr && out != nullptr, "kh_bjac_values: NULL");
    const int w = h->cplx ? 2 : 1;
    try {
        std::vector<double> inv((size_t)h->entries * w);
        KH_HIP(hipStreamSynchronize(h->ctx->stream));
        KH_HIP(hipMemcpy(inv.data(), h->inv, sizeof(double) * inv.size(), hipMemcpyDeviceToHost));
        khbjac::unpack(inv.data(), h->nblk, h->blkptr_host.data(), h->W, w, out);
    } catch (const std::bad_alloc&) {
        return fail(KH_ERR_NOMEM, "kh_bjac_values: out of host memory");
    }
    return 0;
}

}  // extern "C"
