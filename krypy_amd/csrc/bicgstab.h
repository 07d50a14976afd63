// BiCGStab (bicgstab.hip): where the iteration's scalars live on the device, the sanity word the host forms beside them, and the
// two-sum kernel that idrs.hip launches as well.
#pragma once
#include <cmath>

#include "kernels.h"
#include "krylov_hip.h"

namespace kh {

// ctx->scal + SC_TMP + ...: the six sums in the order kh_bicgstab_step returns them (neighbours, so that one copy fetches them
// and one all-reduce takes ss, theta, phi), then the step length k_bicg_half leaves for k_bicg_full
enum { BICG_SIGMA = 0, BICG_SS = 1, BICG_THETA = 2, BICG_PHI = 3, BICG_RHO = 4, BICG_RR = 5, BICG_ALPHA = 6 };

// KH_BICG_* bits of the header, in the spirit of cg_sanity: alpha and omega never visit the host, so what the device clamped
// is told with the sums.  The quotients are the device's own IEEE divisions.
static inline int bicg_sanity_half(double rho, double sigma) {
    int f = 0;
    if (!std::isfinite(sigma)) f |= KH_BICG_NONFINITE_SIGMA;
    else if (std::isfinite(rho) && !std::isfinite(rho / sigma)) f |= KH_BICG_ALPHA_CLAMPED;
    return f;
}
static inline int bicg_sanity_full(double theta, double phi, double rho_new) {
    int f = 0;
    if (!std::isfinite(theta / phi)) f |= KH_BICG_OMEGA_CLAMPED;
    if (!std::isfinite(rho_new) || rho_new == 0.0) f |= KH_BICG_RHO_ZERO;
    return f;
}

// two partials per workgroup, <t, s> in part0 and <t, t> in part1.  2 vector passes: s, t read.  (Here because idrs.hip takes
// the theta and phi of its dimension-reduction step from the same kernel.)
static __global__ __launch_bounds__(BS) void k_bicg_dots(int64_t n, const double* __restrict__ s, const double* __restrict__ t,
                                                         double* __restrict__ part0, double* __restrict__ part1) {
    __shared__ double sm0[4], sm1[4];         // one LDS row per sum: block_sum ends with thread 0 still reading its row
    const int64_t stride = (int64_t)gridDim.x * BS;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        const double tv = t[i];
        a0 = fma(tv, s[i], a0);
        a1 = fma(tv, tv, a1);
    }
    const double r0 = block_sum(a0, sm0);
    const double r1 = block_sum(a1, sm1);
    if (threadIdx.x == 0) {
        part0[blockIdx.x] = r0;
        part1[blockIdx.x] = r1;
    }
}

}  // namespace kh
