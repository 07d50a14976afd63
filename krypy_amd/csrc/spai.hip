// Sparse approximate inverse on a fixed pattern, built on the device (kh_spai_build / kh_zspai_build): a preconditioner GIVEN AS A
// MATRIX, the form the fused Arnoldi step and kh_apply take - fp64 and c128.  No reference counterpart (the reference takes any
// callable as M, Ml, Mr).  The contract, the split of one row's work over the lanes and the work-space layout are in spai.h.
//
// k_spai<Z, W>: one pattern row per group of W lanes, blockDim / W rows per workgroup, ONE launch for all rows.  The Gram matrix,
// its factor L, d, v and y of a row live in LDS (dynamic, sized from the longest pattern row of the call); the phases of
// khspai::row are separated by __syncthreads().  The loops that hold a barrier run to qloop for every row, shorter rows and the
// rows past n (q = 0) predicated: every thread reaches every barrier.  No kernel waits for another workgroup: no flags, no
// spins.  A breakdown is an atomicMin of the row index into one int32, read back once after the launch.
#include "sai_build.h"
#include "spai.h"

using namespace kh;

namespace {

struct SpaiDev {
    const int32_t* indptr;
    const int32_t* indices;
    const double* data;
    const int32_t* pindptr;
    const int32_t* pindices;
    double* m;
    int32_t* bad;
    int32_t n, qloop, row_doubles;
};

template <bool Z, int W>
__global__ __launch_bounds__(khsai::THREADS) void k_spai(SpaiDev d) {
    extern __shared__ double spai_lds[];
    const int g = threadIdx.x / W;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x / W) + g;
    const bool live = i < d.n;
    const int32_t p0 = live ? d.pindptr[i] : 0;
    const int q = live ? d.pindptr[i + 1] - p0 : 0;
    const khspai::Csr A{d.indptr, d.indices, d.data};
    khsai::DevLanes ex{(int)(threadIdx.x % W)};
    if (khspai::row<Z>(A, d.pindices + p0, q, d.qloop, (int32_t)i, spai_lds + (int64_t)g * d.row_doubles, d.m + (Z ? 2 : 1) * (int64_t)p0, W, ex))
        atomicMin(d.bad, (int32_t)i);
}

template <int W>
void launch(bool cplx, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const SpaiDev& d) {
    if (cplx) hipLaunchKernelGGL((k_spai<true, W>), grid, block, lds, stream, d);
    else hipLaunchKernelGGL((k_spai<false, W>), grid, block, lds, stream, d);
}

int spai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t pnnz,
               const int32_t* pindptr, const int32_t* pindices, double* m_out, int64_t info[8], int cplx) {
    const char* who = cplx ? "kh_zspai_build" : "kh_spai_build";
    const khsai::Call call{ctx, n, nnz, indptr, indices, data, pnnz, pindptr, pindices, info, cplx};
    const khsai::Output outs[] = {{m_out, (size_t)pnnz * (cplx ? 2 : 1)}};
    int64_t device_us = 0;
    KH_TRY(khsai::build(
        who, "the context has a communicator - a row of the approximate inverse reads rows of A that other ranks hold, sharded "
             "construction is not implemented",
        call, outs, &device_us,
        [&](int64_t* qmax, int* W) {
            const std::string why = khspai::validate(n, nnz, indptr, indices, pnnz, pindptr, pindices, qmax);
            KH_ARG(why.empty(), "%s: %s", who, why.c_str());
            KH_ARG((nnz == 0 || data != nullptr) && (pnnz == 0 || m_out != nullptr), "%s: NULL array", who);
            *W = khspai::group_width(*qmax, cplx != 0);
            return 0;
        },
        [&](const khsai::DevArgs& a, int W, dim3 g, dim3 b, size_t lds, hipStream_t stream) {
            const SpaiDev d{a.indptr, a.indices, a.data, a.pindptr, a.pindices, a.out[0], a.bad, a.n, a.qloop, a.row_doubles};
            switch (W) {
                case 8: launch<8>(cplx != 0, g, b, lds, stream, d); break;
                case 16: launch<16>(cplx != 0, g, b, lds, stream, d); break;
                case 32: launch<32>(cplx != 0, g, b, lds, stream, d); break;
                default: launch<64>(cplx != 0, g, b, lds, stream, d); break;
            }
        }));
    ctx->spai_device_us = device_us;
    ctx->n_spai_build += 1;
    return 0;
}

}  // namespace

extern "C" {

int kh_spai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t pnnz,
                  const int32_t* pindptr, const int32_t* pindices, double* m_out, int64_t info[8]) {
    return spai_build(ctx, n, nnz, indptr, indices, data, pnnz, pindptr, pindices, m_out, info, 0);
}

int kh_zspai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                   int64_t pnnz, const int32_t* pindptr, const int32_t* pindices, double* m_out_re_im, int64_t info[8]) {
    return spai_build(ctx, n, nnz, indptr, indices, data_re_im, pnnz, pindptr, pindices, m_out_re_im, info, 1);
}

}  // extern "C"
