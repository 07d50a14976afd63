// Factorized sparse approximate inverse on a fixed lower-triangular pattern, built on the device (kh_fsai_build / kh_zfsai_build):
// G ~ L^-1 for a Hermitian positive definite A = L L^H, so that M = G^H G is a Hermitian positive definite preconditioner GIVEN AS
// MATRICES, the form kh_apply and the fused steps take - fp64 and c128.  No reference counterpart (the reference takes any callable
// as M, Ml, Mr).  The contract, the split of one row's work over the lanes and the work-space layout are in fsai.h.
//
// k_fsai<Z, W>: one pattern row per group of W lanes, blockDim / W rows per workgroup, ONE launch for all rows.  The submatrix
// A[J, J], its factor L, d, v and u of a row live in LDS (dynamic, sized from the longest pattern row of the call); the phases of
// khfsai::row are separated by __syncthreads().  The loops that hold a barrier run to qloop for every row, shorter rows and the
// rows past n (q = 0) predicated: every thread reaches every barrier.  No kernel waits for another workgroup: no flags, no
// spins.  A breakdown is an atomicMin of the row index into one int32, read back once after the launch.
#include <new>

#include "fsai.h"
#include "kh_internal.h"

using namespace kh;

namespace {

constexpr int FSAI_THREADS = 256;
constexpr int64_t FSAI_LDS_MAX = 64 * 1024;      // static limit of a workgroup without an opt-in

struct DevLanes {
    int lane;
    template <class F>
    __device__ __forceinline__ void phase(F f) {
        f(lane);
        __syncthreads();
    }
};

struct FsaiDev {
    const int32_t* indptr;
    const int32_t* indices;
    const double* data;
    const int32_t* pindptr;
    const int32_t* pindices;
    double* u;
    double* d;
    int32_t* bad;
    int32_t n, qloop, row_doubles;
};

template <bool Z, int W>
__global__ __launch_bounds__(FSAI_THREADS) void k_fsai(FsaiDev d) {
    extern __shared__ double fsai_lds[];
    const int g = threadIdx.x / W;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x / W) + g;
    const bool live = i < d.n;
    const int32_t p0 = live ? d.pindptr[i] : 0;
    const int q = live ? d.pindptr[i + 1] - p0 : 0;
    const khfsai::Csr A{d.indptr, d.indices, d.data};
    DevLanes ex{(int)(threadIdx.x % W)};
    if (khfsai::row<Z>(A, d.pindices + p0, q, d.qloop, fsai_lds + (int64_t)g * d.row_doubles, d.u + (Z ? 2 : 1) * (int64_t)p0,
                       d.d + (live ? i : 0), W, ex))
        atomicMin(d.bad, (int32_t)i);
}

template <int W>
void launch(bool cplx, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const FsaiDev& d) {
    if (cplx) hipLaunchKernelGGL((k_fsai<true, W>), grid, block, lds, stream, d);
    else hipLaunchKernelGGL((k_fsai<false, W>), grid, block, lds, stream, d);
}

// what one call holds on the device; released on every way out
struct FsaiMem {
    int32_t *indptr = nullptr, *indices = nullptr, *pindptr = nullptr, *pindices = nullptr, *bad = nullptr;
    double *data = nullptr, *u = nullptr, *d = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~FsaiMem() {
        (void)hipFree(indptr);
        (void)hipFree(indices);
        (void)hipFree(pindptr);
        (void)hipFree(pindices);
        (void)hipFree(bad);
        (void)hipFree(data);
        (void)hipFree(u);
        (void)hipFree(d);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

template <typename T>
int to_device(const char* who, T** dst, const T* src, size_t count) {
    const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
    hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) {
        *dst = nullptr;
        return fail(KH_ERR_NOMEM, "%s: hipMalloc(%zu bytes): %s", who, bytes, hipGetErrorString(e));
    }
    if (count && src) KH_HIP(hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return 0;
}

int fsai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t pnnz,
               const int32_t* pindptr, const int32_t* pindices, double* u_out, double* d_out, int64_t info[8], int cplx) {
    const char* who = cplx ? "kh_zfsai_build" : "kh_fsai_build";
    KH_ARG(ctx != nullptr && info != nullptr, "%s: NULL", who);
    if (kh_multi(ctx) || ctx->comm != nullptr)
        return fail(KH_ERR_UNSUPPORTED, "%s: the context has a communicator - a row of the factor reads rows of A that other ranks "
                                        "hold, sharded construction is not implemented", who);
    try {
        int64_t qmax = 0;
        const std::string why = khfsai::validate(n, nnz, indptr, indices, pnnz, pindptr, pindices, &qmax);
        KH_ARG(why.empty(), "%s: %s", who, why.c_str());
        KH_ARG((nnz == 0 || data != nullptr) && u_out != nullptr && d_out != nullptr, "%s: NULL array", who);
        const int w = cplx ? 2 : 1;
        const int32_t none = 0x7fffffff;
        const int qloop = (int)qmax;          // >= 1: no pattern row is empty
        const int W = khfsai::group_width(qmax);
        const int64_t row_doubles = khfsai::row_doubles(qloop, cplx != 0);
        int rows = FSAI_THREADS / W;
        while (rows > 1 && rows * row_doubles * (int64_t)sizeof(double) > FSAI_LDS_MAX) --rows;
        const int64_t lds = rows * row_doubles * (int64_t)sizeof(double);
        const int64_t grid = (n + rows - 1) / rows;
        FsaiMem m;
        KH_TRY(to_device(who, &m.indptr, indptr, (size_t)n + 1));
        KH_TRY(to_device(who, &m.indices, indices, (size_t)nnz));
        KH_TRY(to_device(who, &m.data, data, (size_t)nnz * w));
        KH_TRY(to_device(who, &m.pindptr, pindptr, (size_t)n + 1));
        KH_TRY(to_device(who, &m.pindices, pindices, (size_t)pnnz));
        KH_TRY(to_device<double>(who, &m.u, nullptr, (size_t)pnnz * w));
        KH_TRY(to_device<double>(who, &m.d, nullptr, (size_t)n));
        KH_TRY(to_device(who, &m.bad, &none, 1));
        KH_HIP(hipEventCreate(&m.ev0));
        KH_HIP(hipEventCreate(&m.ev1));
        const FsaiDev d{m.indptr, m.indices, m.data, m.pindptr, m.pindices, m.u, m.d, m.bad, (int32_t)n, qloop, (int32_t)row_doubles};
        KH_HIP(hipEventRecord(m.ev0, ctx->stream));
        const dim3 g((unsigned)grid), b((unsigned)(rows * W));
        switch (W) {
            case 8: launch<8>(cplx != 0, g, b, (size_t)lds, ctx->stream, d); break;
            case 16: launch<16>(cplx != 0, g, b, (size_t)lds, ctx->stream, d); break;
            default: launch<32>(cplx != 0, g, b, (size_t)lds, ctx->stream, d); break;
        }
        KH_HIP(hipGetLastError());
        KH_HIP(hipEventRecord(m.ev1, ctx->stream));
        KH_HIP(hipEventSynchronize(m.ev1));
        float ms = 0.f;
        KH_HIP(hipEventElapsedTime(&ms, m.ev0, m.ev1));
        ctx->fsai_device_us = (int64_t)((double)ms * 1000.0);
        int32_t bad = none;
        KH_HIP(hipMemcpy(&bad, m.bad, sizeof(bad), hipMemcpyDeviceToHost));
        KH_HIP(hipMemcpy(u_out, m.u, sizeof(double) * (size_t)pnnz * w, hipMemcpyDeviceToHost));
        KH_HIP(hipMemcpy(d_out, m.d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        ctx->n_fsai_build += 1;
        const int64_t out[8] = {n, pnnz, qmax, W, grid, lds, 0, bad == none ? -1 : (int64_t)bad};
        for (int i = 0; i < 8; ++i) info[i] = out[i];
    } catch (const std::bad_alloc&) {
        return fail(KH_ERR_NOMEM, "%s: out of host memory", who);
    }
    return 0;
}

}  // namespace

extern "C" {

int kh_fsai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t pnnz,
                  const int32_t* pindptr, const int32_t* pindices, double* u_out, double* d_out, int64_t info[8]) {
    return fsai_build(ctx, n, nnz, indptr, indices, data, pnnz, pindptr, pindices, u_out, d_out, info, 0);
}

int kh_zfsai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                   int64_t pnnz, const int32_t* pindptr, const int32_t* pindices, double* u_out_re_im, double* d_out, int64_t info[8]) {
    return fsai_build(ctx, n, nnz, indptr, indices, data_re_im, pnnz, pindptr, pindices, u_out_re_im, d_out, info, 1);
}

}  // extern "C"
