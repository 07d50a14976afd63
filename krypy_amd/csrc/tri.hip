// Sparse triangular solves on the device (kh_tri_*): x = T^{-1} b for a lower / upper triangular CSR matrix, fp64 and c128 -
// what an ILU / IC / SSOR preconditioner applies per iteration (the M, Ml, Mr hooks of krypy/linsys.py; the reference has no
// counterpart, it calls the user's function on host arrays).  Level scheduling over a sliced-ELL copy in level order; the
// analysis and the layout are in tri.h.
//
// One thread per row:  s = b_i;  s = s - t_ij x_j over the off-diagonal entries in ascending column order, multiply and
// subtract rounded separately;  x_i = s / t_ii (x_i = s for a unit diagonal).  Complex: (ac - bd, ad + bc) products and
// NumPy's quotient (Smith's formula, ratio and scale once - as k_zminres_update in zpath.h).  Every x_j a row reads was
// written by an earlier level, so the result is that of the sequential row-by-row substitution bit for bit, in whatever
// order the rows of one level run.
//
// Two kinds of launch (planned at creation):
//   k_tri_wide    one level, one wave per slice, as many workgroups as the level needs; the stream orders the levels.
//   k_tri_narrow  a run of consecutive levels with few rows each, ONE workgroup: every wave takes the slices of the level
//                 in turn, then __syncthreads() - a workgroup-scope release / acquire around the barrier - hands x to the
//                 next level.  Writer and reader are waves of one workgroup, on one compute unit and one L1: the case
//                 workgroup scope covers.
// No kernel here waits for another workgroup: no flags, no spins, no grid-wide barrier.
#include <new>

#include "kh_internal.h"
#include "tri.h"

using namespace kh;

struct kh_tri_s {
    kh_ctx ctx = nullptr;
    int64_t n = 0, nnz = 0;
    int cplx = 0, lower = 0, unit = 0;
    int64_t info[8] = {0};
    std::vector<khtri::Launch> launches;
    // device copy of the plan
    double* vals = nullptr;
    double* diag = nullptr;
    int32_t* cols = nullptr;
    int64_t* slice_base = nullptr;
    int32_t* slice_slots = nullptr;
    int32_t* row_id = nullptr;
    int32_t* row_len = nullptr;
    int32_t* lev_slice = nullptr;
};

namespace {

struct TriDev {
    const double* vals;
    const double* diag;
    const int32_t* cols;
    const int64_t* slice_base;
    const int32_t* slice_slots;
    const int32_t* row_id;
    const int32_t* row_len;
    int unit;
};

// One slice: lane = one row.  b is read from x before y is written (x and y may be the same column); the x_j come from y.
// y is read through a plain pointer on purpose: other waves of the workgroup wrote those entries before the last barrier.
template <bool Z>
__device__ __forceinline__ void tri_slice(const TriDev& t, int64_t s, int lane, const double* x, double* y) {
    const int64_t at = s * khtri::SLICE + lane;
    const int32_t row = t.row_id[at];
    const int32_t len = row >= 0 ? t.row_len[at] : 0;
    const int32_t ns = t.slice_slots[s];          // wave-uniform
    const int64_t base = t.slice_base[s];
    if (!Z) {
        double acc = row >= 0 ? x[row] : 0.0;
        for (int32_t k = 0; k < ns; ++k) {
            if (k < len) {
                const int64_t q = base + (int64_t)k * khtri::SLICE + lane;
                acc = acc - t.vals[q] * y[t.cols[q]];
            }
        }
        if (row >= 0) y[row] = t.unit ? acc : acc / t.diag[at];
    } else {
        const double2* xz = reinterpret_cast<const double2*>(x);
        double2* yz = reinterpret_cast<double2*>(y);
        const double2* vz = reinterpret_cast<const double2*>(t.vals);
        double2 acc = row >= 0 ? xz[row] : make_double2(0.0, 0.0);
        for (int32_t k = 0; k < ns; ++k) {
            if (k < len) {
                const int64_t q = base + (int64_t)k * khtri::SLICE + lane;
                const double2 a = vz[q], b = yz[t.cols[q]];
                acc.x = acc.x - (a.x * b.x - a.y * b.y);
                acc.y = acc.y - (a.x * b.y + a.y * b.x);
            }
        }
        if (row >= 0) {
            if (!t.unit) {
                const double2 d = reinterpret_cast<const double2*>(t.diag)[at];
                const bool big_re = fabs(d.x) >= fabs(d.y);
                const double rat = big_re ? d.y / d.x : d.x / d.y;
                const double scl = 1.0 / (big_re ? (d.x + d.y * rat) : (d.y + d.x * rat));
                double2 z;
                if (big_re) {
                    z.x = (acc.x + acc.y * rat) * scl;
                    z.y = (acc.y - acc.x * rat) * scl;
                } else {
                    z.x = (acc.x * rat + acc.y) * scl;
                    z.y = (acc.y * rat - acc.x) * scl;
                }
                acc = z;
            }
            yz[row] = acc;
        }
    }
}

// slices [slice0, slice0 + nslices) of ONE level: workgroup b, wave v takes slice slice0 + b * WIDE_WAVES + v
template <bool Z>
__global__ __launch_bounds__(khtri::WIDE_WAVES* khtri::SLICE) void k_tri_wide(TriDev t, int32_t slice0, int32_t nslices,
                                                                              const double* x, double* y) {
    const int64_t s = (int64_t)blockIdx.x * khtri::WIDE_WAVES + (threadIdx.x >> 6);
    if (s < nslices) tri_slice<Z>(t, slice0 + s, threadIdx.x & 63, x, y);
}

// levels [lev0, lev0 + nlev) in ONE workgroup; lev_slice[l] .. lev_slice[l + 1] are the slices of level l.  Every thread
// reaches every barrier: the loop bounds do not depend on the thread.
template <bool Z>
__global__ __launch_bounds__(khtri::NARROW_MAX_THREADS) void k_tri_narrow(TriDev t, const int32_t* __restrict__ lev_slice,
                                                                          int32_t lev0, int32_t nlev, const double* x,
                                                                          double* y) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    for (int32_t l = lev0; l < lev0 + nlev; ++l) {
        const int32_t s1 = lev_slice[l + 1];
        for (int32_t s = lev_slice[l] + wave; s < s1; s += nwaves) tri_slice<Z>(t, s, lane, x, y);
        __syncthreads();      // release / acquire at workgroup scope: this level's x is visible to the next one
    }
}

template <typename T>
int to_device(T** dst, const std::vector<T>& src) {
    const size_t bytes = sizeof(T) * std::max<size_t>(src.size(), 1);
    hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess)
        return fail(KH_ERR_NOMEM, "kh_tri_create: hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    if (!src.empty()) KH_HIP(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return 0;
}

int tri_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int lower,
               int unit_diag, int cplx, kh_tri* out) {
    const char* who = cplx ? "kh_ztri_create" : "kh_tri_create";
    KH_ARG(ctx != nullptr && out != nullptr, "%s: NULL", who);
    if (kh_multi(ctx) || ctx->comm != nullptr)
        return fail(KH_ERR_UNSUPPORTED, "%s: the context has a communicator - a triangular solve couples all rows, sharded "
                                        "triangular solves are not implemented", who);
    kh_tri t = nullptr;
    try {
        khtri::Plan p;
        const std::string why = khtri::analyse(n, nnz, indptr, indices, data, cplx ? 2 : 1, lower != 0, unit_diag != 0,
                                               ctx->tri_narrow_rows, p);
        KH_ARG(why.empty(), "%s: %s", who, why.c_str());
        t = new kh_tri_s();
        t->ctx = ctx;
        t->n = n;
        t->nnz = nnz;
        t->cplx = cplx;
        t->lower = lower != 0;
        t->unit = unit_diag != 0;
        const int64_t info[8] = {n, nnz, p.nlevels, p.n_wide, p.n_narrow, p.slots, p.widest, p.longest};
        for (int i = 0; i < 8; ++i) t->info[i] = info[i];
        t->launches = p.launches;
        auto body = [&]() -> int {
            KH_TRY(to_device(&t->vals, p.vals));
            KH_TRY(to_device(&t->diag, p.diag));
            KH_TRY(to_device(&t->cols, p.cols));
            KH_TRY(to_device(&t->slice_base, p.slice_base));
            KH_TRY(to_device(&t->slice_slots, p.slice_slots));
            KH_TRY(to_device(&t->row_id, p.row_id));
            KH_TRY(to_device(&t->row_len, p.row_len));
            KH_TRY(to_device(&t->lev_slice, p.lev_slice));
            return 0;
        };
        const int rc = body();
        if (rc != 0) {          // nothing half-built stays behind
            kh_tri_free(t);
            return rc;
        }
    } catch (const std::bad_alloc&) {
        if (t) kh_tri_free(t);
        return fail(KH_ERR_NOMEM, "%s: out of host memory in the level analysis", who);
    }
    *out = t;
    return 0;
}

int check_col(kh_vec v, int64_t col, int64_t ncols, int64_t rn, const char* what) {
    KH_ARG(v != nullptr, "kh_tri_solve(%s): NULL block", what);
    KH_ARG(col >= 0 && ncols >= 0 && col + ncols <= v->ncols, "kh_tri_solve(%s): columns [%lld, %lld) of a block with %lld", what,
           (long long)col, (long long)(col + ncols), (long long)v->ncols);
    KH_ARG(v->n == rn, "kh_tri_solve(%s): the block has %lld doubles per column, the triangular operator needs %lld (n does not "
                       "match, or a real handle meets complex blocks / a complex handle real ones)",
           what, (long long)v->n, (long long)rn);
    return 0;
}

}  // namespace

extern "C" {

int kh_tri_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int lower,
                  int unit_diag, kh_tri* out) {
    return tri_create(ctx, n, nnz, indptr, indices, data, lower, unit_diag, 0, out);
}

int kh_ztri_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                   int lower, int unit_diag, kh_tri* out) {
    return tri_create(ctx, n, nnz, indptr, indices, data_re_im, lower, unit_diag, 1, out);
}

int kh_tri_free(kh_tri t) {
    if (!t) return 0;
    (void)hipStreamSynchronize(t->ctx->stream);
    (void)hipFree(t->vals);
    (void)hipFree(t->diag);
    (void)hipFree(t->cols);
    (void)hipFree(t->slice_base);
    (void)hipFree(t->slice_slots);
    (void)hipFree(t->row_id);
    (void)hipFree(t->row_len);
    (void)hipFree(t->lev_slice);
    delete t;
    return 0;
}

int kh_tri_info(kh_tri t, int64_t out[8]) {
    KH_ARG(t != nullptr && out != nullptr, "kh_tri_info: NULL");
    for (int i = 0; i < 8; ++i) out[i] = t->info[i];
    return 0;
}

int kh_tri_solve(kh_ctx ctx, kh_tri t, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol, int64_t ncols) {
    KH_ARG(ctx != nullptr && t != nullptr, "kh_tri_solve: NULL");
    KH_ARG(t->ctx == ctx, "kh_tri_solve: the handle belongs to another context");
    const int64_t rn = t->cplx ? 2 * t->n : t->n;
    KH_TRY(check_col(X, xcol, ncols, rn, "x"));
    KH_TRY(check_col(Y, ycol, ncols, rn, "y"));
    // the columns are solved one after the other: in one block, shifted ranges that overlap would overwrite a right-hand side
    // before it is read - only the identical range (in place) is safe
    KH_ARG(!(X == Y && xcol != ycol && (xcol < ycol ? ycol - xcol : xcol - ycol) < ncols),
           "kh_tri_solve: columns [%lld, %lld) and [%lld, %lld) of one block overlap without being the same", (long long)xcol,
           (long long)(xcol + ncols), (long long)ycol, (long long)(ycol + ncols));
    TriDev d{t->vals, t->diag, t->cols, t->slice_base, t->slice_slots, t->row_id, t->row_len, t->unit};
    for (int64_t c = 0; c < ncols; ++c) {
        const double* x = X->col(xcol + c);
        double* y = Y->col(ycol + c);
        for (const khtri::Launch& L : t->launches) {
            if (L.narrow) {
                if (t->cplx)
                    hipLaunchKernelGGL(k_tri_narrow<true>, dim3(1), dim3(L.threads), 0, ctx->stream, d, t->lev_slice, L.lev0, L.nlev,
                                       x, y);
                else
                    hipLaunchKernelGGL(k_tri_narrow<false>, dim3(1), dim3(L.threads), 0, ctx->stream, d, t->lev_slice, L.lev0, L.nlev,
                                       x, y);
                ctx->n_tri_narrow += 1;
            } else {
                const unsigned grid = (unsigned)((L.nslices + khtri::WIDE_WAVES - 1) / khtri::WIDE_WAVES);
                if (t->cplx)
                    hipLaunchKernelGGL(k_tri_wide<true>, dim3(grid), dim3(L.threads), 0, ctx->stream, d, L.slice0, L.nslices, x, y);
                else
                    hipLaunchKernelGGL(k_tri_wide<false>, dim3(grid), dim3(L.threads), 0, ctx->stream, d, L.slice0, L.nslices, x, y);
                ctx->n_tri_wide += 1;
            }
        }
        KH_HIP(hipGetLastError());
        ctx->n_tri_solve += 1;
    }
    chain_blk_touch(ctx, Y);
    return 0;
}

}  // extern "C"
