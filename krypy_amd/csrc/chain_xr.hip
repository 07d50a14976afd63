// The register-resident Gram-Schmidt chain (chain.h) on N ranks: every grid-wide sum of the launch also crosses the RANKS, inside
// the XCD leaders' hand-over (grid_sum<true>: one tagged store per peer mailbox and a rank-ordered gather, xr_dev.h).  A
// reference-order Arnoldi step (utils.py:1012-1034) on a slab of 2.5 M ... 14.68 M rows is then the sharded SpMV + ONE launch
// of ours: no all-reduce call, the local basis read once - where the one-reduction and the panel forms read it twice and the
// blocked kernel (chain_blk2.h) ends at 2.5 M rows.  A translation unit of its own (the instantiations with the cross-rank
// stage are compiled here; chain_launch.hip holds the one-GPU ones).
//
// Which kernel: 16 ... 40 rows per lane the LDS-parking kernel (k_mgs_chain_lds: padded vectors, or up to 24 rows masked),
// else the plain kernel; 48 / 56 rows (the last 8 / 16 rows of w in LDS: config 5's 12.5 M-row slabs) the long-vector kernel.
// Every rank takes the shape of ITS slab - the number of sums (k + 1 links and the norm) is the same on all of them, and that
// is all the exchange protocol cares about; eligibility is decided by the caller for the LONGEST slab of the run, so that all
// ranks decide alike, and from there on a refusal is an error (a rank-local fallback would change the pattern of collectives
// its peers see).  Results: the one-GPU chain kernels' arithmetic with the partial sums of the ranks added in rank order - the
// same bits on every rank, run to run; against one GPU the sums are taken in another order (1e-10 parity, tests/test_gpu_chain_xr.py).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "kh_internal.h"
#include "chain.h"
#include "chain_long.h"
#include "kh_launch.h"

namespace kh {

// rows per lane (16 ... 56) and workgroups for a slab of n doubles: the fewest rows whose grid fits the compute units the
// shape is chosen for (all of them; tests: kh_ctx_set "chain_xr_cus").  Short slabs take 16 rows on fewer workgroups.
bool chain_xr_shape(kh_ctx ctx, int64_t n, int* r2_out, int* g_out) {
    if (n < 2) return false;
    const int cus = ctx->chain_xr_cus > 0 ? std::min(ctx->chain_xr_cus, ctx->ncu) : ctx->ncu;
    if (cus > CH_GMAX / 2) return false;              // (grid_sum's XCD-leader form: 2 G granules, one per thread)
    const int64_t n2 = (n + 1) >> 1;
    static const int kR2[] = {16, 24, 32, 40, 48, 56};
    for (int c : kR2) {
        const int64_t g = (n2 + (int64_t)c * CH_BS - 1) / ((int64_t)c * CH_BS);
        if (g <= cus) {
            *r2_out = c;
            *g_out = (int)g;
            return true;
        }
    }
    return false;
}

// the kernels of chain.h / chain_long.h with the cross-rank stage (XR = true) on the resident launcher (kh_launch.h)
template <int R2, bool MASKED, int WL>
static hipError_t launch_xr_plain(kh_ctx ctx, int G, const ChainArgs& a) {
    return launch_resident<k_mgs_chain<R2, MASKED, false, 0, WL, false, true>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, (size_t)WL * CH_BS * sizeof(double2)), a);
}

static hipError_t launch_xr_long(kh_ctx ctx, int G, const ChainArgs& a) {
    return launch_resident<k_mgs_chain_long<0, true>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, ChainShapeLong::LDS_BYTES), a);
}

template <int R2, bool MASKED>
static hipError_t launch_xr_lds(kh_ctx ctx, int G, const ChainArgs& a) {
    return launch_resident<k_mgs_chain_lds<R2, MASKED, false, 0, true>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, ChainShapeLds<R2, false>::LDS_BYTES), a);
}

// One Arnoldi step k of basis block V (columns 0 .. k, reference order, one sweep; w holds this rank's rows of A v_k - after
// the projector of a deflated step) with every sum across the ranks inside the launch: coefficients into hdev[0 .. k], the
// norm into hdev[k + 1], v_{k+1} stored.  Returns 1 when launched, negative on error - never 0: the caller has established
// eligibility for the longest slab of the run, every rank alike.
int chain_xr_step(kh_ctx ctx, kh_vec V, const double* w, int64_t wld, int64_t k, double* hdev, int slot, double* hpin, int hcount) {
    const int64_t n = V->n;
    int r2 = 0, G = 0;
    if (!ctx->xr_on) return fail(KH_ERR_COMM, "chain_xr_step: the xr transport is off");
    if (!chain_xr_shape(ctx, n, &r2, &G))
        return fail(KH_ERR_COMM, "Gram-Schmidt chain with in-kernel cross-rank sums: a slab of %lld rows is not served here although "
                                 "the run's longest slab was found eligible", (long long)n);
    KH_TRY(chain_epoch_check(ctx));
    const int nsums = (int)(k + 2);                       // k + 1 links and the norm
    if (ctx->xr_epoch > 0xfff00000u - (unsigned)nsums)
        return fail(KH_ERR_COMM, "xr: the epoch counter of the cross-rank exchange is exhausted; create a new context");
    const int64_t chunk2 = (int64_t)r2 * CH_BS;
    const int64_t need_ld = (int64_t)G * chunk2 * 2;
    const bool padded = V->ld >= need_ld && wld >= need_ld;
    ChainArgs a;
    chain_args_init(ctx, a, V, w, chunk2, k, hdev, slot, hpin, hcount);
    for (int r = 0; r < ctx->xr_nranks; ++r) a.xr.peer[r] = ctx->xr_peer[r];
    a.xr.rank = ctx->xr_rank;
    a.xr.nranks = ctx->xr_nranks;
    a.xr.epoch0 = ctx->xr_epoch;
    a.xr.timeout_ticks = (long long)(ctx->xr_timeout_ms > 0 ? ctx->xr_timeout_ms : 60000) * 100000ll;
    // the LDS-parking kernel where it exists without spilled registers: padded vectors up to 40 rows, masked ones up to 24
    const bool use_lds = ctx->chain_lds && r2 <= 40 && (padded || r2 <= 24);
    hipError_t e;
    // (rows of w in LDS: 8 of 48, 16 of 56)
    auto plain = [&](auto r, auto wl) {
        return dispatch_bool(!padded, [&](auto m) { return launch_xr_plain<decltype(r)::value, decltype(m)::value, decltype(wl)::value>(ctx, G, a); });
    };
    using std::integral_constant;
    if (r2 <= 40 && use_lds) {
        // (the masked LDS instantiations exist up to 24 rows: use_lds says padded beyond)
        if (r2 <= 24)
            e = dispatch_int<16, 24>(r2, [&](auto r) {
                return dispatch_bool(!padded, [&](auto m) { return launch_xr_lds<decltype(r)::value, decltype(m)::value>(ctx, G, a); });
            });
        else
            e = dispatch_int<32, 40>(r2, [&](auto r) { return launch_xr_lds<decltype(r)::value, false>(ctx, G, a); });
    } else if (r2 <= 40) {
        e = dispatch_int<16, 24, 32, 40>(r2, [&](auto r) { return plain(r, integral_constant<int, 0>()); });
    } else if (r2 == 48) {
        e = (ctx->chain_long && ctx->chain_lds && padded) ? launch_xr_long(ctx, G, a) : hipErrorUnknown;
        if (e != hipSuccess) {          // (switched off, an unpadded block, or the 128 KB of dynamic LDS refused: both reads from memory)
            (void)hipGetLastError();
            e = plain(integral_constant<int, 48>(), integral_constant<int, 8>());
        } else {
            ctx->n_chain_long += 1;
        }
    } else {
        e = plain(integral_constant<int, 56>(), integral_constant<int, 16>());
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(KH_ERR_HIP, "Gram-Schmidt chain with in-kernel cross-rank sums: the launch failed (%s); no rank-local fallback on a "
                                "communicator", hipGetErrorString(e));
    }
    ctx->xr_epoch += (unsigned)nsums;
    ctx->n_xr += nsums;
    ctx->n_chain_xr += 1;
    ctx->n_chain_lds += use_lds ? 1 : 0;
    return chain_launched(ctx, slot, a, nsums);
}

}  // namespace kh
