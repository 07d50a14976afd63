// Persistent ILU(0) preconditioner on the device (kh_ilu0_*): the analysis runs once per pattern (ilu0p.h, on the host), a
// refactorisation for new values is one upload and a few launches, the factors never come back to the host, the two triangular
// images are filled by a kernel and the ordering is folded into the solves - fp64 and c128.  No reference counterpart (the
// reference takes any callable as M, Ml, Mr).
//
// kh_ilu0_refactor, on the context's stream:
//   k_ilu0p_gather          a[q] = staged[src[q]]: the caller's values into the order of Ap = A[perm][:, perm]; arms the breakdown word
//   k_ilu0p_wide / _narrow  the factorisation of ilu0.hip - khilu0::factor_row, one thread per row, the plan of L - in place on a
//   k_ilu0p_fill            img[e] = a[fmap[e]] for every stored slot of the two sliced-ELL images and every diagonal of U; padding
//                           slots and lanes without a row are not written
// kh_ilu0_solve, per column: the launches of L's plan, then the launches of U's plan (k_ilu0p_solve_wide / _narrow, the row
// arithmetic khilu0p::solve_lane).  The L stage reads X[perm[row]] and writes t[row]; the U stage works in place on t and stores
// every finished entry to t[row] and Y[perm[row]].  All L launches precede all U launches in the stream, so X and Y may be the same
// column.
//
// The one-workgroup kernels hand rows (the factorisation) and entries of t (the solves) from one level to the next through
// __syncthreads(): a workgroup-scope release / acquire between waves of one workgroup, on one compute unit and one L1 - the hand-off
// k_tri_narrow and k_ilu0_narrow rely on.  a and t are read through plain pointers: no const __restrict__, no non-temporal loads.  No
// kernel here waits for another workgroup: no flags, no spins, no grid-wide barrier.  Their loop bounds do not depend on the thread:
// every thread reaches every barrier.
#include <new>

#include "ilu0p.h"
#include "kh_internal.h"

using namespace kh;

struct kh_ilu0_s {
    kh_ctx ctx = nullptr;
    int64_t n = 0, nnz = 0, longest = 0, widest = 0, nlevels = 0;
    int cplx = 0, permuted = 0, factored = 0;
    int64_t total = 0, slots_l = 0, slots_u = 0, levels_l = 0, levels_u = 0, bytes = 0;
    int64_t f_wide = 0, f_narrow = 0, s_wide = 0, s_narrow = 0;
    std::vector<khtri::Launch> launches_l, launches_u;      // L's are the factorisation's too
    std::vector<int32_t> src;                               // host copy: kh_ilu0_values scatters through it
    std::vector<void*> owned;                               // every device allocation
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Ap, the plan and the maps
    int32_t *indptr = nullptr, *indices = nullptr, *dpos = nullptr, *dsrc = nullptr, *fmap = nullptr, *perm = nullptr;
    int32_t *l_cols = nullptr, *l_slots = nullptr, *l_row_id = nullptr, *l_row_len = nullptr, *l_lev_slice = nullptr;
    int32_t *u_cols = nullptr, *u_slots = nullptr, *u_row_id = nullptr, *u_row_len = nullptr, *u_lev_slice = nullptr;
    int64_t *l_base = nullptr, *u_base = nullptr;
    // values
    double *a = nullptr, *staged = nullptr, *img = nullptr, *t = nullptr;
    int32_t* bad = nullptr;
};

namespace {

constexpr int32_t NONE = 0x7fffffff;

template <bool Z>
__global__ __launch_bounds__(BS) void k_ilu0p_gather(double* __restrict__ a, const double* __restrict__ staged,
                                                     const int32_t* __restrict__ src, int64_t nnz, int32_t* bad) {
    const int64_t q = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (q == 0) *bad = NONE;
    if (q < nnz) {
        if (Z) reinterpret_cast<double2*>(a)[q] = reinterpret_cast<const double2*>(staged)[src[q]];
        else a[q] = staged[src[q]];
    }
}

template <bool Z>
__global__ __launch_bounds__(BS) void k_ilu0p_fill(double* __restrict__ img, const double* __restrict__ a,
                                                   const int32_t* __restrict__ fmap, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (e < total) {
        const int32_t q = fmap[e];
        if (q >= 0) {
            if (Z) reinterpret_cast<double2*>(img)[e] = reinterpret_cast<const double2*>(a)[q];
            else img[e] = a[q];
        }
    }
}

struct FactorDev {
    const int32_t* indptr;
    const int32_t* indices;
    const int32_t* dpos;
    const int32_t* row_id;
    int32_t* bad;
};

template <bool Z>
__device__ __forceinline__ void factor_lane(const FactorDev& d, int64_t at, double* a) {
    const int32_t i = d.row_id[at];
    if (i >= 0 && khilu0::factor_row<Z>(d.indptr, d.indices, d.dpos, i, a)) atomicMin(d.bad, i);
}

// slices [slice0, slice0 + nslices) of ONE level: thread t of the grid takes entry slice0 * 64 + t of row_id
template <bool Z>
__global__ __launch_bounds__(khtri::WIDE_WAVES* khtri::SLICE) void k_ilu0p_wide(FactorDev d, int32_t slice0, int32_t nslices, double* a) {
    const int64_t t = (int64_t)blockIdx.x * (khtri::WIDE_WAVES * khtri::SLICE) + threadIdx.x;
    if (t < (int64_t)nslices * khtri::SLICE) factor_lane<Z>(d, (int64_t)slice0 * khtri::SLICE + t, a);
}

// levels [lev0, lev0 + nlev) in ONE workgroup
template <bool Z>
__global__ __launch_bounds__(khtri::NARROW_MAX_THREADS) void k_ilu0p_narrow(FactorDev d, const int32_t* __restrict__ lev_slice,
                                                                            int32_t lev0, int32_t nlev, double* a) {
    for (int32_t l = lev0; l < lev0 + nlev; ++l) {
        const int64_t end = (int64_t)lev_slice[l + 1] * khtri::SLICE;
        for (int64_t at = (int64_t)lev_slice[l] * khtri::SLICE + threadIdx.x; at < end; at += blockDim.x) factor_lane<Z>(d, at, a);
        __syncthreads();      // release / acquire at workgroup scope: this level's rows are visible to the next one
    }
}

// slices [slice0, slice0 + nslices) of ONE level of one stage: workgroup b, wave v takes slice slice0 + b * WIDE_WAVES + v
template <bool Z, bool P, bool UPPER>
__global__ __launch_bounds__(khtri::WIDE_WAVES* khtri::SLICE) void k_ilu0p_solve_wide(khilu0p::Tri T, const int32_t* perm, int32_t slice0,
                                                                                      int32_t nslices, const double* x, double* t, double* y) {
    const int64_t s = (int64_t)blockIdx.x * khtri::WIDE_WAVES + (threadIdx.x >> 6);
    if (s < nslices) khilu0p::solve_lane<Z, P, UPPER>(T, perm, slice0 + s, threadIdx.x & 63, x, t, y);
}

// levels [lev0, lev0 + nlev) of one stage in ONE workgroup
template <bool Z, bool P, bool UPPER>
__global__ __launch_bounds__(khtri::NARROW_MAX_THREADS) void k_ilu0p_solve_narrow(khilu0p::Tri T, const int32_t* perm,
                                                                                  const int32_t* __restrict__ lev_slice, int32_t lev0,
                                                                                  int32_t nlev, const double* x, double* t, double* y) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    for (int32_t l = lev0; l < lev0 + nlev; ++l) {
        const int32_t s1 = lev_slice[l + 1];
        for (int32_t s = lev_slice[l] + wave; s < s1; s += nwaves) khilu0p::solve_lane<Z, P, UPPER>(T, perm, s, lane, x, t, y);
        __syncthreads();      // release / acquire at workgroup scope: this level's t is visible to the next one
    }
}

template <bool Z, bool P, bool UPPER>
void launch_stage(kh_ctx ctx, const std::vector<khtri::Launch>& launches, const khilu0p::Tri& T, const int32_t* perm,
                  const int32_t* lev_slice, const double* x, double* t, double* y) {
    for (const khtri::Launch& L : launches) {
        if (L.narrow) {
            hipLaunchKernelGGL((k_ilu0p_solve_narrow<Z, P, UPPER>), dim3(1), dim3(L.threads), 0, ctx->stream, T, perm, lev_slice, L.lev0,
                               L.nlev, x, t, y);
            ctx->n_ilu0p_narrow += 1;
        } else {
            const unsigned grid = (unsigned)((L.nslices + khtri::WIDE_WAVES - 1) / khtri::WIDE_WAVES);
            hipLaunchKernelGGL((k_ilu0p_solve_wide<Z, P, UPPER>), dim3(grid), dim3(L.threads), 0, ctx->stream, T, perm, L.slice0, L.nslices,
                               x, t, y);
            ctx->n_ilu0p_wide += 1;
        }
    }
}

template <bool Z, bool P>
void launch_column(kh_ctx ctx, kh_ilu0 h, const double* x, double* y) {
    const int w = Z ? 2 : 1;
    const khilu0p::Tri tl{h->img, nullptr, h->l_cols, h->l_base, h->l_slots, h->l_row_id, h->l_row_len};
    const khilu0p::Tri tu{h->img + h->slots_l * w, h->img + (h->slots_l + h->slots_u) * w, h->u_cols, h->u_base, h->u_slots, h->u_row_id,
                          h->u_row_len};
    launch_stage<Z, P, false>(ctx, h->launches_l, tl, h->perm, h->l_lev_slice, x, h->t, y);
    launch_stage<Z, P, true>(ctx, h->launches_u, tu, h->perm, h->u_lev_slice, x, h->t, y);
}

int dev_alloc(kh_ilu0 h, void** dst, size_t bytes) {
    bytes = std::max<size_t>(bytes, 8);
    const hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) {
        *dst = nullptr;
        return fail(KH_ERR_NOMEM, "kh_ilu0_create: hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    }
    h->owned.push_back(*dst);
    h->bytes += (int64_t)bytes;
    return 0;
}

template <typename T>
int to_device(kh_ilu0 h, T** dst, const std::vector<T>& src) {
    KH_TRY(dev_alloc(h, reinterpret_cast<void**>(dst), sizeof(T) * src.size()));
    if (!src.empty()) KH_HIP(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return 0;
}

int check_col(kh_vec v, int64_t col, int64_t ncols, int64_t rn, const char* what) {
    KH_ARG(v != nullptr, "kh_ilu0_solve(%s): NULL block", what);
    KH_ARG(col >= 0 && ncols >= 0 && col + ncols <= v->ncols, "kh_ilu0_solve(%s): columns [%lld, %lld) of a block with %lld", what,
           (long long)col, (long long)(col + ncols), (long long)v->ncols);
    KH_ARG(v->n == rn, "kh_ilu0_solve(%s): the block has %lld doubles per column, the preconditioner needs %lld (n does not match, or "
                       "a real handle meets complex blocks / a complex handle real ones)",
           what, (long long)v->n, (long long)rn);
    return 0;
}

}  // namespace

extern "C" {

int kh_ilu0_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const int32_t* perm, int cplx,
                   kh_ilu0* out) {
    KH_ARG(ctx != nullptr && out != nullptr, "kh_ilu0_create: NULL");
    if (kh_multi(ctx) || ctx->comm != nullptr)
        return fail(KH_ERR_UNSUPPORTED, "kh_ilu0_create: the context has a communicator - a factorisation couples all rows, sharded "
                                        "factorisations are not implemented");
    kh_ilu0 h = nullptr;
    try {
        khilu0p::Plan p;
        const std::string why = khilu0p::analyse(n, nnz, indptr, indices, perm, ctx->tri_narrow_rows, p);
        KH_ARG(why.empty(), "kh_ilu0_create: %s", why.c_str());
        h = new kh_ilu0_s();
        h->ctx = ctx;
        h->n = n;
        h->nnz = nnz;
        h->cplx = cplx != 0;
        h->permuted = p.permuted;
        h->longest = p.longest;
        h->widest = p.L.widest;
        h->nlevels = p.L.nlevels;
        h->total = p.total();
        h->slots_l = p.L.slots;
        h->slots_u = p.U.slots;
        h->levels_l = p.L.nlevels;
        h->levels_u = p.U.nlevels;
        h->f_wide = p.L.n_wide;
        h->f_narrow = p.L.n_narrow;
        h->s_wide = p.L.n_wide + p.U.n_wide;
        h->s_narrow = p.L.n_narrow + p.U.n_narrow;
        h->launches_l = p.L.launches;
        h->launches_u = p.U.launches;
        h->src = p.src;
        const size_t w = cplx ? 2 : 1;
        auto body = [&]() -> int {
            KH_TRY(to_device(h, &h->indptr, p.indptr));
            KH_TRY(to_device(h, &h->indices, p.indices));
            KH_TRY(to_device(h, &h->dpos, p.dpos));
            KH_TRY(to_device(h, &h->dsrc, p.src));
            KH_TRY(to_device(h, &h->fmap, p.fmap));
            if (p.permuted) KH_TRY(to_device(h, &h->perm, p.perm));
            KH_TRY(to_device(h, &h->l_cols, p.L.cols));
            KH_TRY(to_device(h, &h->l_base, p.L.slice_base));
            KH_TRY(to_device(h, &h->l_slots, p.L.slice_slots));
            KH_TRY(to_device(h, &h->l_row_id, p.L.row_id));
            KH_TRY(to_device(h, &h->l_row_len, p.L.row_len));
            KH_TRY(to_device(h, &h->l_lev_slice, p.L.lev_slice));
            KH_TRY(to_device(h, &h->u_cols, p.U.cols));
            KH_TRY(to_device(h, &h->u_base, p.U.slice_base));
            KH_TRY(to_device(h, &h->u_slots, p.U.slice_slots));
            KH_TRY(to_device(h, &h->u_row_id, p.U.row_id));
            KH_TRY(to_device(h, &h->u_row_len, p.U.row_len));
            KH_TRY(to_device(h, &h->u_lev_slice, p.U.lev_slice));
            KH_TRY(dev_alloc(h, reinterpret_cast<void**>(&h->a), sizeof(double) * w * (size_t)nnz));
            KH_TRY(dev_alloc(h, reinterpret_cast<void**>(&h->staged), sizeof(double) * w * (size_t)nnz));
            KH_TRY(dev_alloc(h, reinterpret_cast<void**>(&h->img), sizeof(double) * w * (size_t)h->total));
            KH_TRY(dev_alloc(h, reinterpret_cast<void**>(&h->t), sizeof(double) * w * (size_t)n));
            KH_TRY(dev_alloc(h, reinterpret_cast<void**>(&h->bad), sizeof(int32_t)));
            // what the fill never writes: 0 in the padding slots, 1 in the diagonals of the lanes without a row
            KH_HIP(hipMemset(h->img, 0, sizeof(double) * w * (size_t)h->total));
            std::vector<double> ones((size_t)p.U.nslices * khtri::SLICE * w, 0.0);
            for (size_t k = 0; k < ones.size(); k += w) ones[k] = 1.0;
            KH_HIP(hipMemcpy(h->img + (size_t)p.off_d() * w, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice));
            KH_HIP(hipMemset(h->t, 0, sizeof(double) * w * (size_t)n));
            KH_HIP(hipEventCreate(&h->ev0));
            KH_HIP(hipEventCreate(&h->ev1));
            return 0;
        };
        const int rc = body();
        if (rc != 0) {          // nothing half-built stays behind
            kh_ilu0_free(h);
            return rc;
        }
    } catch (const std::bad_alloc&) {
        if (h) kh_ilu0_free(h);
        return fail(KH_ERR_NOMEM, "kh_ilu0_create: out of host memory in the analysis");
    }
    ctx->n_ilu0p_create += 1;
    *out = h;
    return 0;
}

int kh_ilu0_free(kh_ilu0 h) {
    if (!h) return 0;
    (void)hipStreamSynchronize(h->ctx->stream);
    for (void* p : h->owned) (void)hipFree(p);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
    return 0;
}

int kh_ilu0_refactor(kh_ctx ctx, kh_ilu0 h, const double* data, int64_t info[8]) {
    KH_ARG(ctx != nullptr && h != nullptr && info != nullptr, "kh_ilu0_refactor: NULL");
    KH_ARG(h->ctx == ctx, "kh_ilu0_refactor: the handle belongs to another context");
    KH_ARG(data != nullptr, "kh_ilu0_refactor: NULL array");
    const size_t w = h->cplx ? 2 : 1, bytes = sizeof(double) * w * (size_t)h->nnz;
    h->factored = 0;
    KH_HIP(hipMemcpyAsync(h->staged, data, bytes, hipMemcpyHostToDevice, ctx->stream));
    KH_HIP(hipEventRecord(h->ev0, ctx->stream));
    const unsigned gq = (unsigned)((h->nnz + BS - 1) / BS), ge = (unsigned)((h->total + BS - 1) / BS);
    if (h->cplx) hipLaunchKernelGGL(k_ilu0p_gather<true>, dim3(gq), dim3(BS), 0, ctx->stream, h->a, h->staged, h->dsrc, h->nnz, h->bad);
    else hipLaunchKernelGGL(k_ilu0p_gather<false>, dim3(gq), dim3(BS), 0, ctx->stream, h->a, h->staged, h->dsrc, h->nnz, h->bad);
    const FactorDev d{h->indptr, h->indices, h->dpos, h->l_row_id, h->bad};
    for (const khtri::Launch& L : h->launches_l) {
        if (L.narrow) {
            if (h->cplx)
                hipLaunchKernelGGL(k_ilu0p_narrow<true>, dim3(1), dim3(L.threads), 0, ctx->stream, d, h->l_lev_slice, L.lev0, L.nlev, h->a);
            else
                hipLaunchKernelGGL(k_ilu0p_narrow<false>, dim3(1), dim3(L.threads), 0, ctx->stream, d, h->l_lev_slice, L.lev0, L.nlev, h->a);
            ctx->n_ilu0p_narrow += 1;
        } else {
            const unsigned grid = (unsigned)((L.nslices + khtri::WIDE_WAVES - 1) / khtri::WIDE_WAVES);
            if (h->cplx)
                hipLaunchKernelGGL(k_ilu0p_wide<true>, dim3(grid), dim3(L.threads), 0, ctx->stream, d, L.slice0, L.nslices, h->a);
            else
                hipLaunchKernelGGL(k_ilu0p_wide<false>, dim3(grid), dim3(L.threads), 0, ctx->stream, d, L.slice0, L.nslices, h->a);
            ctx->n_ilu0p_wide += 1;
        }
    }
    if (h->cplx) hipLaunchKernelGGL(k_ilu0p_fill<true>, dim3(ge), dim3(BS), 0, ctx->stream, h->img, h->a, h->fmap, h->total);
    else hipLaunchKernelGGL(k_ilu0p_fill<false>, dim3(ge), dim3(BS), 0, ctx->stream, h->img, h->a, h->fmap, h->total);
    KH_HIP(hipGetLastError());
    KH_HIP(hipEventRecord(h->ev1, ctx->stream));
    int32_t bad = NONE;
    KH_HIP(hipMemcpyAsync(&bad, h->bad, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));      // the only traffic back
    KH_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    KH_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    ctx->ilu0p_refactor_us = (int64_t)((double)ms * 1000.0);
    ctx->ilu0p_h2d_bytes = (int64_t)bytes;
    ctx->ilu0p_d2h_bytes = (int64_t)sizeof(bad);
    ctx->n_ilu0p_refactor += 1;
    h->factored = bad == NONE;
    const int64_t res[8] = {h->n, h->nnz, h->nlevels, h->f_wide, h->f_narrow, h->widest, h->longest, bad == NONE ? -1 : (int64_t)bad};
    for (int i = 0; i < 8; ++i) info[i] = res[i];
    return 0;
}

int kh_ilu0_solve(kh_ctx ctx, kh_ilu0 h, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol, int64_t ncols) {
    KH_ARG(ctx != nullptr && h != nullptr, "kh_ilu0_solve: NULL");
    KH_ARG(h->ctx == ctx, "kh_ilu0_solve: the handle belongs to another context");
    KH_ARG(h->factored, "kh_ilu0_solve: the handle is not factored (never refactored, or the last refactorisation broke down)");
    const int64_t rn = h->cplx ? 2 * h->n : h->n;
    KH_TRY(check_col(X, xcol, ncols, rn, "x"));
    KH_TRY(check_col(Y, ycol, ncols, rn, "y"));
    // the columns are solved one after the other: in one block, shifted ranges that overlap would overwrite a right-hand side
    // before it is read - only the identical range (in place) is safe
    KH_ARG(!(X == Y && xcol != ycol && (xcol < ycol ? ycol - xcol : xcol - ycol) < ncols),
           "kh_ilu0_solve: columns [%lld, %lld) and [%lld, %lld) of one block overlap without being the same", (long long)xcol,
           (long long)(xcol + ncols), (long long)ycol, (long long)(ycol + ncols));
    for (int64_t c = 0; c < ncols; ++c) {
        const double* x = X->col(xcol + c);
        double* y = Y->col(ycol + c);
        if (h->cplx) h->permuted ? launch_column<true, true>(ctx, h, x, y) : launch_column<true, false>(ctx, h, x, y);
        else h->permuted ? launch_column<false, true>(ctx, h, x, y) : launch_column<false, false>(ctx, h, x, y);
        KH_HIP(hipGetLastError());
        ctx->n_ilu0p_solve += 1;
    }
    chain_blk_touch(ctx, Y);
    return 0;
}

int kh_ilu0_values(kh_ilu0 h, double* lu_out) {
    KH_ARG(h != nullptr && lu_out != nullptr, "kh_ilu0_values: NULL");
    KH_ARG(h->factored, "kh_ilu0_values: the handle is not factored (never refactored, or the last refactorisation broke down)");
    const size_t w = h->cplx ? 2 : 1;
    try {
        std::vector<double> a((size_t)h->nnz * w);
        KH_HIP(hipStreamSynchronize(h->ctx->stream));
        KH_HIP(hipMemcpy(a.data(), h->a, sizeof(double) * a.size(), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < (size_t)h->nnz; ++q)
            for (size_t c = 0; c < w; ++c) lu_out[(size_t)h->src[q] * w + c] = a[q * w + c];
    } catch (const std::bad_alloc&) {
        return fail(KH_ERR_NOMEM, "kh_ilu0_values: out of host memory");
    }
    return 0;
}

int kh_ilu0_info(kh_ilu0 h, int64_t out[16]) {
    KH_ARG(h != nullptr && out != nullptr, "kh_ilu0_info: NULL");
    const int64_t res[16] = {h->n, h->nnz, h->nlevels, h->f_wide, h->f_narrow, h->levels_l, h->levels_u, h->s_wide, h->s_narrow,
                             h->slots_l, h->slots_u, h->permuted, h->factored, h->bytes, 0, 0};
    for (int i = 0; i < 16; ++i) out[i] = res[i];
    return 0;
}

}  // extern "C"
