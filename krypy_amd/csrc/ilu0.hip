// ILU(0) factorisation on the device (kh_ilu0_factor / kh_zilu0_factor) and the greedy multicolour ordering (kh_multicolor, host
// only): the factors the sparse triangular solves of tri.hip apply, built from A alone - fp64 and c128.  No reference counterpart
// (the reference takes any callable as M, Ml, Mr).  The analysis, the plan and the arithmetic of one row are in ilu0.h.
//
// One thread per row, rows in plan order (by level of the strict lower pattern, slices of 64 rows); everything happens in place on
// ONE device array of values.  A row divides each of its entries left of the diagonal by the finished pivot of that column's row
// and subtracts the multiple of that row's upper part from its own tail (two-pointer merge).  Every row it reads belongs to an
// earlier level, so the result is that of the sequential loop bit for bit, in whatever order the rows of one level run.
//
// Two kinds of launch, as for the triangular solves:
//   k_ilu0_wide    one level, 256-thread workgroups, as many as the level needs; the stream orders the levels.
//   k_ilu0_narrow  a run of consecutive levels with few rows each, ONE workgroup with __syncthreads() between the levels - the
//                  workgroup-scope release / acquire around the barrier hands the finished rows to the next level (writer and
//                  reader are waves of one workgroup, on one compute unit and one L1: the hand-off k_tri_narrow relies on).
// The values are read through a plain pointer: no const __restrict__, no non-temporal loads.  No kernel here waits for another
// workgroup: no flags, no spins, no grid-wide barrier.  A breakdown (zero or non-finite pivot) is an atomicMin of the row index
// into one int32, read back once after the last launch.
#include <new>

#include "dev_owned.h"
#include "ilu0.h"

using namespace kh;

namespace {

struct Ilu0Dev {
    const int32_t* indptr;
    const int32_t* indices;
    const int32_t* dpos;
    const int32_t* row_id;
    int32_t* bad;
};

template <bool Z>
__device__ __forceinline__ void ilu0_lane(const Ilu0Dev& d, int64_t at, double* a) {
    const int32_t i = d.row_id[at];
    if (i >= 0 && khilu0::factor_row<Z>(d.indptr, d.indices, d.dpos, i, a)) atomicMin(d.bad, i);
}

// slices [slice0, slice0 + nslices) of ONE level: thread t of the grid takes entry slice0 * 64 + t of row_id
template <bool Z>
__global__ __launch_bounds__(khtri::WIDE_WAVES* khtri::SLICE) void k_ilu0_wide(Ilu0Dev d, int32_t slice0, int32_t nslices, double* a) {
    const int64_t t = (int64_t)blockIdx.x * (khtri::WIDE_WAVES * khtri::SLICE) + threadIdx.x;
    if (t < (int64_t)nslices * khtri::SLICE) ilu0_lane<Z>(d, (int64_t)slice0 * khtri::SLICE + t, a);
}

// levels [lev0, lev0 + nlev) in ONE workgroup; lev_slice[l] .. lev_slice[l + 1] are the slices of level l.  Every thread reaches
// every barrier: the loop bounds do not depend on the thread.
template <bool Z>
__global__ __launch_bounds__(khtri::NARROW_MAX_THREADS) void k_ilu0_narrow(Ilu0Dev d, const int32_t* __restrict__ lev_slice,
                                                                           int32_t lev0, int32_t nlev, double* a) {
    for (int32_t l = lev0; l < lev0 + nlev; ++l) {
        const int64_t end = (int64_t)lev_slice[l + 1] * khtri::SLICE;
        for (int64_t at = (int64_t)lev_slice[l] * khtri::SLICE + threadIdx.x; at < end; at += blockDim.x) ilu0_lane<Z>(d, at, a);
        __syncthreads();      // release / acquire at workgroup scope: this level's rows are visible to the next one
    }
}

int ilu0_factor(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, double* lu_out,
                int64_t info[8], int cplx) {
    const char* who = cplx ? "kh_zilu0_factor" : "kh_ilu0_factor";
    KH_ARG(ctx != nullptr && info != nullptr, "%s: NULL", who);
    if (kh_multi(ctx) || ctx->comm != nullptr)
        return fail(KH_ERR_UNSUPPORTED, "%s: the context has a communicator - a factorisation couples all rows, sharded "
                                        "factorisations are not implemented", who);
    try {
        khilu0::Plan p;
        const std::string why = khilu0::analyse(n, nnz, indptr, indices, ctx->tri_narrow_rows, p);
        KH_ARG(why.empty(), "%s: %s", who, why.c_str());
        KH_ARG(data != nullptr && lu_out != nullptr, "%s: NULL array", who);
        const int w = cplx ? 2 : 1;
        const int32_t none = 0x7fffffff;
        DevArray<int32_t> dev_indptr, dev_indices, dpos, row_id, lev_slice, bad_word;
        DevArray<double> a;
        EventPair ev;
        KH_TRY(to_device(who, dev_indptr, indptr, (size_t)n + 1));
        KH_TRY(to_device(who, dev_indices, indices, (size_t)nnz));
        KH_TRY(to_device(who, a, data, (size_t)nnz * w));
        KH_TRY(to_device(who, dpos, p.dpos.data(), p.dpos.size()));
        KH_TRY(to_device(who, row_id, p.row_id.data(), p.row_id.size()));
        KH_TRY(to_device(who, lev_slice, p.lev_slice.data(), p.lev_slice.size()));
        KH_TRY(to_device(who, bad_word, &none, 1));
        const Ilu0Dev d{dev_indptr.get(), dev_indices.get(), dpos.get(), row_id.get(), bad_word.get()};
        KH_TRY(ev.start(ctx->stream));
        for (const khtri::Launch& L : p.launches) {
            if (L.narrow) {
                if (cplx)
                    hipLaunchKernelGGL(k_ilu0_narrow<true>, dim3(1), dim3(L.threads), 0, ctx->stream, d, lev_slice.get(), L.lev0, L.nlev, a.get());
                else
                    hipLaunchKernelGGL(k_ilu0_narrow<false>, dim3(1), dim3(L.threads), 0, ctx->stream, d, lev_slice.get(), L.lev0, L.nlev, a.get());
                ctx->n_ilu0_narrow += 1;
            } else {
                const unsigned grid = (unsigned)((L.nslices + khtri::WIDE_WAVES - 1) / khtri::WIDE_WAVES);
                if (cplx)
                    hipLaunchKernelGGL(k_ilu0_wide<true>, dim3(grid), dim3(L.threads), 0, ctx->stream, d, L.slice0, L.nslices, a.get());
                else
                    hipLaunchKernelGGL(k_ilu0_wide<false>, dim3(grid), dim3(L.threads), 0, ctx->stream, d, L.slice0, L.nslices, a.get());
                ctx->n_ilu0_wide += 1;
            }
        }
        KH_HIP(hipGetLastError());
        KH_TRY(ev.stop(ctx->stream, &ctx->ilu0_device_us));
        int32_t bad = none;
        KH_HIP(hipMemcpy(&bad, bad_word.get(), sizeof(bad), hipMemcpyDeviceToHost));
        if (nnz) KH_HIP(hipMemcpy(lu_out, a.get(), sizeof(double) * (size_t)nnz * w, hipMemcpyDeviceToHost));
        ctx->n_ilu0_factor += 1;
        const int64_t out[8] = {n, nnz, p.nlevels, p.n_wide, p.n_narrow, p.widest, p.longest, bad == none ? -1 : (int64_t)bad};
        for (int i = 0; i < 8; ++i) info[i] = out[i];
    } catch (const std::bad_alloc&) {
        return fail(KH_ERR_NOMEM, "%s: out of host memory in the level analysis", who);
    }
    return 0;
}

}  // namespace

extern "C" {

int kh_ilu0_factor(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data,
                   double* lu_out, int64_t info[8]) {
    return ilu0_factor(ctx, n, nnz, indptr, indices, data, lu_out, info, 0);
}

int kh_zilu0_factor(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                    double* lu_out_re_im, int64_t info[8]) {
    return ilu0_factor(ctx, n, nnz, indptr, indices, data_re_im, lu_out_re_im, info, 1);
}

int kh_multicolor(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int32_t* color_out, int64_t* ncolors) {
    try {
        const std::string why = khilu0::multicolor(n, nnz, indptr, indices, color_out, ncolors);
        KH_ARG(why.empty(), "kh_multicolor: %s", why.c_str());
    } catch (const std::bad_alloc&) {
        return fail(KH_ERR_NOMEM, "kh_multicolor: out of host memory");
    }
    return 0;
}

}  // extern "C"
