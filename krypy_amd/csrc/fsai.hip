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
#include "fsai.h"
#include "sai_build.h"

using namespace kh;

namespace {

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
__global__ __launch_bounds__(khsai::THREADS) void k_fsai(FsaiDev d) {
    extern __shared__ double fsai_lds[];
    const int g = threadIdx.x / W;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x / W) + g;
    const bool live = i < d.n;
    const int32_t p0 = live ? d.pindptr[i] : 0;
    const int q = live ? d.pindptr[i + 1] - p0 : 0;
    const khfsai::Csr A{d.indptr, d.indices, d.data};
    khsai::DevLanes ex{(int)(threadIdx.x % W)};
    if (khfsai::row<Z>(A, d.pindices + p0, q, d.qloop, fsai_lds + (int64_t)g * d.row_doubles, d.u + (Z ? 2 : 1) * (int64_t)p0,
                       d.d + (live ? i : 0), W, ex))
        atomicMin(d.bad, (int32_t)i);
}

template <int W>
void launch(bool cplx, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const FsaiDev& d) {
    if (cplx) hipLaunchKernelGGL((k_fsai<true, W>), grid, block, lds, stream, d);
    else hipLaunchKernelGGL((k_fsai<false, W>), grid, block, lds, stream, d);
}

int fsai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t pnnz,
               const int32_t* pindptr, const int32_t* pindices, double* u_out, double* d_out, int64_t info[8], int cplx) {
    const char* who = cplx ? "kh_zfsai_build" : "kh_fsai_build";
    const khsai::Call call{ctx, n, nnz, indptr, indices, data, pnnz, pindptr, pindices, info, cplx};
    const khsai::Output outs[] = {{u_out, (size_t)pnnz * (cplx ? 2 : 1)}, {d_out, (size_t)n}};
    int64_t device_us = 0;
    KH_TRY(khsai::build(
        who, "the context has a communicator - a row of the factor reads rows of A that other ranks hold, sharded construction is "
             "not implemented",
        call, outs, &device_us,
        [&](int64_t* qmax, int* W) {
            const std::string why = khfsai::validate(n, nnz, indptr, indices, pnnz, pindptr, pindices, qmax);
            KH_ARG(why.empty(), "%s: %s", who, why.c_str());
            KH_ARG((nnz == 0 || data != nullptr) && u_out != nullptr && d_out != nullptr, "%s: NULL array", who);
            *W = khfsai::group_width(*qmax);          // qmax >= 1: no pattern row is empty
            return 0;
        },
        [&](const khsai::DevArgs& a, int W, dim3 g, dim3 b, size_t lds, hipStream_t stream) {
            const FsaiDev d{a.indptr, a.indices, a.data, a.pindptr, a.pindices, a.out[0], a.out[1], a.bad, a.n, a.qloop, a.row_doubles};
            switch (W) {
                case 8: launch<8>(cplx != 0, g, b, lds, stream, d); break;
                case 16: launch<16>(cplx != 0, g, b, lds, stream, d); break;
                default: launch<32>(cplx != 0, g, b, lds, stream, d); break;
            }
        }));
    ctx->fsai_device_us = device_us;
    ctx->n_fsai_build += 1;
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
