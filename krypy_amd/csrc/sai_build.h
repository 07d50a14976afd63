// The device side that the approximate inverses built row by row share (spai.hip, fsai.hip): the lanes of a group as sai_row.h
// wants them, the split of the rows over workgroups and one call from the uploads to the info block.  Each unit keeps its kernel,
// its validation, its width rule and its entry points.
#pragma once
#include <new>

#include "dev_owned.h"
#include "sai_row.h"

namespace khsai {

constexpr int THREADS = 256;
constexpr int64_t LDS_MAX = 64 * 1024;      // static limit of a workgroup without an opt-in

struct DevLanes {
    int lane;
    template <class F>
    __device__ __forceinline__ void phase(F f) {
        f(lane);
        __syncthreads();
    }
};

// what an entry point was given, but for its outputs
struct Call {
    kh_ctx ctx;
    int64_t n, nnz;
    const int32_t *indptr, *indices;
    const double* data;
    int64_t pnnz;
    const int32_t *pindptr, *pindices;
    int64_t* info;
    int cplx;
};

// one output: `count` doubles that the kernel writes and the call copies to `host`
struct Output {
    double* host;
    size_t count;
};

// what the launch is handed: A, the pattern, the outputs and the breakdown word on the device
struct DevArgs {
    const int32_t *indptr, *indices;
    const double* data;
    const int32_t *pindptr, *pindices;
    double* out[2];
    int32_t* bad;
    int32_t n, qloop, row_doubles;
};

// One build.  `sharded`: why a context with a communicator is refused.  check(&qmax, &W) validates the call, its outputs included,
// and gives the longest pattern row and the lanes per row; launch(args, W, grid, block, lds, stream) starts the kernel (not called
// when no pattern row has an entry).  Gives the device time of the launch; fills info[8].
template <size_t NOUT, class Check, class Launch>
int build(const char* who, const char* sharded, const Call& c, const Output (&outs)[NOUT], int64_t* device_us, Check check, Launch launch) {
    static_assert(NOUT <= sizeof(DevArgs::out) / sizeof(double*), "more outputs than DevArgs has room for");
    KH_ARG(c.ctx != nullptr && c.info != nullptr, "%s: NULL", who);
    if (kh_multi(c.ctx) || c.ctx->comm != nullptr) return kh::fail(KH_ERR_UNSUPPORTED, "%s: %s", who, sharded);
    try {
        int64_t qmax = 0;
        int W = 0;
        KH_TRY(check(&qmax, &W));
        const int w = c.cplx ? 2 : 1;
        const int32_t none = 0x7fffffff;
        const int qloop = (int)qmax;
        const int64_t row_doubles = khsai::row_doubles(qloop, c.cplx != 0);
        // pattern rows per workgroup: as many as 256 threads and 64 KiB of LDS hold
        int rows = THREADS / W;
        while (rows > 1 && rows * row_doubles * (int64_t)sizeof(double) > LDS_MAX) --rows;
        const int64_t lds = rows * row_doubles * (int64_t)sizeof(double);
        const int64_t grid = (c.n + rows - 1) / rows;
        kh::DevArray<int32_t> indptr, indices, pindptr, pindices, bad_word;
        kh::DevArray<double> data, out[NOUT];
        kh::EventPair ev;
        KH_TRY(kh::to_device(who, indptr, c.indptr, (size_t)c.n + 1));
        KH_TRY(kh::to_device(who, indices, c.indices, (size_t)c.nnz));
        KH_TRY(kh::to_device(who, data, c.data, (size_t)c.nnz * w));
        KH_TRY(kh::to_device(who, pindptr, c.pindptr, (size_t)c.n + 1));
        KH_TRY(kh::to_device(who, pindices, c.pindices, (size_t)c.pnnz));
        for (size_t o = 0; o < NOUT; ++o) KH_TRY(kh::to_device<double>(who, out[o], nullptr, outs[o].count));
        KH_TRY(kh::to_device(who, bad_word, &none, 1));
        DevArgs a{indptr.get(), indices.get(), data.get(), pindptr.get(), pindices.get(), {}, bad_word.get(),
                  (int32_t)c.n,  qloop,         (int32_t)row_doubles};
        for (size_t o = 0; o < NOUT; ++o) a.out[o] = out[o].get();
        KH_TRY(ev.start(c.ctx->stream));
        if (qloop > 0) {
            launch(a, W, dim3((unsigned)grid), dim3((unsigned)(rows * W)), (size_t)lds, c.ctx->stream);
            KH_HIP(hipGetLastError());
        }
        KH_TRY(ev.stop(c.ctx->stream, device_us));
        int32_t bad = none;
        KH_HIP(hipMemcpy(&bad, bad_word.get(), sizeof(bad), hipMemcpyDeviceToHost));
        for (size_t o = 0; o < NOUT; ++o)
            if (outs[o].count) KH_HIP(hipMemcpy(outs[o].host, out[o].get(), sizeof(double) * outs[o].count, hipMemcpyDeviceToHost));
        const int64_t info[8] = {c.n, c.pnnz, qmax, W, qloop > 0 ? grid : 0, lds, 0, bad == none ? -1 : (int64_t)bad};
        for (int i = 0; i < 8; ++i) c.info[i] = info[i];
    } catch (const std::bad_alloc&) {
        return kh::fail(KH_ERR_NOMEM, "%s: out of host memory", who);
    }
    return 0;
}

}  // namespace khsai
