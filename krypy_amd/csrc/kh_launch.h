// The launch layer of the kernels whose workgroups wait for each other inside the launch (the register-resident Gram-Schmidt
// chain families, the Householder step, the deflation projector): ONE launcher, and the dispatcher that turns a runtime shape
// into a template argument.  Shared by chain_launch.hip, chain_blk.hip, chain_blk2.hip, chain_xr.hip, house.hip, proj_reg.hip
// and - for the attribute-and-launch part only - the panel kernels of krylov_hip.hip.
//
// A plain launch (a cooperative launch goes through a separate hardware queue and costs ~1 ms of cross-queue synchronisation
// per Arnoldi step when interleaved with ordinary kernels).  Residency is what matters for the in-kernel grid reduction, and
// it is identical for plain and cooperative launches: it is checked here against the occupancy of the instantiation, and
// every spin in the kernels is bounded.
#pragma once
#include <type_traits>

#include "kh_internal.h"

namespace kh {

constexpr int KH_MAX_DEVICES = 64;      // devices a process can hold contexts on (kh_ctx_create takes any device)

// What the runtime was told and asked about one kernel on one device: hipFuncSetAttribute is per device, and so is occupancy.
struct KernelOnDevice {
    bool lds_allowed = false;      // MaxDynamicSharedMemorySize has been raised to what this instantiation asks for
    int blocks_per_cu = -1;        // hipOccupancyMaxActiveBlocksPerMultiprocessor at its block size and LDS (-1: not asked yet)
};

// the (kernel, device) entry: one fixed array per instantiation (512 bytes of .bss each, a few hundred KB over all resident
// kernels), indexed by ctx->device; nullptr for a device beyond it - the launchers then return hipErrorInvalidDevice, which
// their callers treat like any refused launch (try_chain: the per-column kernels take vectors of that length)
template <auto Kern>
inline KernelOnDevice* kernel_on_device(kh_ctx ctx) {
    static KernelOnDevice table[KH_MAX_DEVICES];
    return (ctx->device >= 0 && ctx->device < KH_MAX_DEVICES) ? &table[ctx->device] : nullptr;
}

// raises the kernel's dynamic-LDS limit to `lds` bytes on this device, once
template <auto Kern>
inline hipError_t allow_lds(KernelOnDevice* kd, size_t lds) {
    if (lds == 0 || kd->lds_allowed) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) kd->lds_allowed = true;
    return e;
}

// launch with `lds` bytes of dynamic LDS and no residency check: the panel kernels, whose workgroups do not wait for each other
template <auto Kern, class... A>
inline hipError_t launch_lds(kh_ctx ctx, int grid, int block, size_t lds, const A&... args) {
    KernelOnDevice* kd = kernel_on_device<Kern>(ctx);
    if (kd == nullptr) return hipErrorInvalidDevice;
    const hipError_t e = allow_lds<Kern>(kd, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), lds, ctx->stream, args...);
    return hipGetLastError();
}

struct ResidentShape {
    int block;          // threads per workgroup
    int grid;           // workgroups launched: G, G + the row-less ones in front, or 8 G + 8 (one XCD: chain.h, ONEX)
    int cus;            // compute units the G working workgroups must be co-resident on: ctx->ncu, or ctx->ncu / 8 (one XCD)
    size_t lds;         // dynamic LDS bytes
    // G workgroups spread over the chip / on one XCD
    static ResidentShape chip(kh_ctx ctx, int block, int G, size_t lds) { return ResidentShape{block, G, ctx->ncu, lds}; }
    static ResidentShape one_xcd(kh_ctx ctx, int block, int G, size_t lds) { return ResidentShape{block, 8 * G + 8, ctx->ncu / 8, lds}; }
};

// workgroups of `Kern` one compute unit holds at this block size and LDS (asked once per device, after the LDS limit is raised)
template <auto Kern>
inline hipError_t resident_per_cu(kh_ctx ctx, int block, size_t lds, int* out) {
    KernelOnDevice* kd = kernel_on_device<Kern>(ctx);
    if (kd == nullptr) return hipErrorInvalidDevice;
    if (kd->blocks_per_cu < 0) {
        hipError_t e = allow_lds<Kern>(kd, lds);
        if (e != hipSuccess) return e;
        int nb = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kern, block, lds);
        if (e != hipSuccess) return e;
        kd->blocks_per_cu = nb;
    }
    *out = kd->blocks_per_cu;
    return hipSuccess;
}

// The resident launcher: hipErrorCooperativeLaunchTooLarge when the G working workgroups cannot all be resident on s.cus
// compute units (the grid-wide sums would wait for workgroups that never start).  Callers that size something by the
// occupancy figure (the blocked kernels' row-less workgroups) ask resident_per_cu first.
template <auto Kern, class... A>
inline hipError_t launch_resident(kh_ctx ctx, int G, const ResidentShape& s, const A&... args) {
    int per_cu = 0;
    const hipError_t e = resident_per_cu<Kern>(ctx, s.block, s.lds, &per_cu);
    if (e != hipSuccess) return e;
    if ((int64_t)per_cu * s.cus < G) return hipErrorCooperativeLaunchTooLarge;
    hipLaunchKernelGGL(Kern, dim3(s.grid), dim3(s.block), s.lds, ctx->stream, args...);
    return hipGetLastError();
}

// ---- runtime value -> template argument --------------------------------------------------------------------------------
// f(std::integral_constant<int, V>()) for the V of the list that equals v; hipErrorInvalidValue (no instantiation) otherwise.
// Each site lists exactly the values it ships kernels for.
template <int... Vs, class F>
inline hipError_t dispatch_int(int v, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs ? (e = f(std::integral_constant<int, Vs>()), true) : false) || ...);
    return e;
}

template <class F>
inline hipError_t dispatch_bool(bool b, F&& f) {
    return b ? f(std::true_type()) : f(std::false_type());
}

// the diagonals of the banded operator in a fused prologue: 5 or 7 (the callers have checked that it is one of the two)
template <class F>
inline hipError_t dispatch_nd(int nd, F&& f) {
    return nd == 5 ? f(std::integral_constant<int, 5>()) : f(std::integral_constant<int, 7>());
}

}  // namespace kh
