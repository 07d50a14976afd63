// IDR(s) (idrs.hip): the layout of the scalar state block the caller passes (one column of KH_IDRS_NSCAL doubles; every word is a
// double, the stop word and the counters included, so that the block downloads as one array).
#pragma once
#include "krylov_hip.h"

namespace kh {

constexpr int IDRS_SMAX = KH_IDRS_SMAX;     // columns of the shadow space at most
constexpr int IDRS_RUN_MAX = KH_IDRS_RUN_MAX;   // positions of one kh_idrs_run call at most = step records kept

enum {
    IDRS_M = 0,         // M[i * IDRS_SMAX + j] = <p_i, g_j>, the lower triangle is used (row stride IDRS_SMAX for every s)
    IDRS_F = 64,        // f_i = <p_i, r>
    IDRS_C = 72,        // c of the last k_idr_dir (entries k .. s-1)
    IDRS_H = 80,        // h_i = <p_i, g_k> of the last block dot; at position s the new f before k_idr_rr takes it over
    IDRS_A = 88,        // a of the last k_idr_orth (entries 0 .. k-1)
    IDRS_OM = 96,       // omega
    IDRS_RR = 97,       // <r, r>
    IDRS_THETA = 98,    // <t, r>          (neighbours: one reduction launch and one all-reduce for both)
    IDRS_PHI = 99,      // <t, t>
    IDRS_BETA = 100,    // beta of the last k_idr_orth
    IDRS_FLAGS = 101,   // KH_IDRS_* bits raised by the kernels of the step under way; k_idr_rr records and clears them
    IDRS_TMP = 102,     // a rank's own <r, r> before it is all-reduced (contexts with a communicator)
    IDRS_STOP = 103,    // not 0: every IDR kernel returns at once      (neighbours: one memset clears both, one copy fetches the
    IDRS_COUNT = 104,   // step records written since it was cleared     counter with the records behind it)
    IDRS_REC = 105,     // IDRS_RUN_MAX records (rr, M_kk or theta, f_k or phi, flags)
    IDRS_NSCAL = IDRS_REC + 4 * IDRS_RUN_MAX
};
static_assert(IDRS_NSCAL == KH_IDRS_NSCAL, "krylov_hip.h states the length of the scalar block");
static_assert(IDRS_SMAX * IDRS_SMAX == IDRS_F, "M is IDRS_SMAX x IDRS_SMAX");

}  // namespace kh
