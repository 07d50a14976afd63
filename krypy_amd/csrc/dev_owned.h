// What ONE call of a builder holds on the device, released on every way out of it: owning device arrays and an owning pair of
// events that times the call's launches (ilu0.hip, and sai_build.h for spai.hip / fsai.hip).  The handles that live across calls
// (tri.hip, ilu0p.hip) keep their own.
#pragma once
#include <algorithm>
#include <memory>

#include "kh_internal.h"

namespace kh {

struct DevFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
template <typename T>
using DevArray = std::unique_ptr<T[], DevFree>;

// allocates `count` elements (at least one) and, with a `src`, uploads them; `who` names the entry point in the message
template <typename T>
int to_device(const char* who, DevArray<T>& dst, const T* src, size_t count) {
    const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
    T* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(KH_ERR_NOMEM, "%s: hipMalloc(%zu bytes): %s", who, bytes, hipGetErrorString(e));
    dst.reset(p);
    if (count && src) KH_HIP(hipMemcpy(p, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return 0;
}

struct EventPair {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    // creates the events and records the first one
    int start(hipStream_t stream) {
        KH_HIP(hipEventCreate(&ev0));
        KH_HIP(hipEventCreate(&ev1));
        KH_HIP(hipEventRecord(ev0, stream));
        return 0;
    }
    // records the second one, waits for it and gives the microseconds between the two
    int stop(hipStream_t stream, int64_t* us) {
        KH_HIP(hipEventRecord(ev1, stream));
        KH_HIP(hipEventSynchronize(ev1));
        float ms = 0.f;
        KH_HIP(hipEventElapsedTime(&ms, ev0, ev1));
        *us = (int64_t)((double)ms * 1000.0);
        return 0;
    }
};

}  // namespace kh
