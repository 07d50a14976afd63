// BiCGStab (bicgstab.hip): where the iteration's scalars live on the device, and the sanity word the host forms beside them.
#pragma once
#include <cmath>

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

}  // namespace kh
