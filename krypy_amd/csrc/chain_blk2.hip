// Launcher of the eight-wave blocked Gram-Schmidt kernel with the cross-rank stage (chain_blk2.h): a translation unit of
// its own.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "kh_internal.h"
#include "chain_blk2.h"
#include "kh_launch.h"

namespace kh {

static constexpr size_t BLK_GRAN_WORDS = (size_t)2 * CH_GMAX * BLK_NVS * 2;
static constexpr size_t BLK_GRAN2_WORDS = (size_t)2 * BLK_NG2 * BLK_NVS * 2;

// rows of 16 B per lane (4, 5 or 6), workgroups WITH rows and whether wave 0 is a communication wave (448 lanes with rows instead of
// 512) for a vector of n doubles: the fewest rows whose grid fits the chip - beside the workgroups without rows when there is room
// for them; with a communication wave where that fits (KRYPY_AMD_BLK2_CW: 1 = where it fits, 0 = never), else without
bool chain_blk2_shape(kh_ctx ctx, int64_t n, int* r2_out, int* g_out, int* cw_out, bool one_slot) {
    if (n < 2 || ctx->ncu > CH_GMAX / 2) return false;
    const int64_t n2 = (n + 1) >> 1;
    const int room = ctx->ncu - (ctx->blk_nx > 0 ? ctx->blk_nx : 0);
    // In order of measured speed: a communication wave and up to 6 rows per lane (no spills), the same with 7 rows (92 B of
    // scratch per lane), then all 512 lanes with rows (6 rows: 320 B of scratch).  Within each: first with room left for the
    // workgroups without rows, then without (6 rows without them beat 7 rows with them: 6,030 against 5,710 it/s at 1.36 M rows).
    // Last, when the caller takes them: 8 ... 11 rows per lane with ONE block in registers (communication wave, no spills).
    const int tiers[4][3] = {{1, 4, 6}, {1, 7, ctx->blk2_cw_maxrows}, {0, 4, 6}, {1, 8, 11}};       // {communication wave, rows from, rows to}
    const int ntier = (one_slot && ctx->blk2_cw) ? 4 : 3;
    for (int t = ctx->blk2_cw ? 0 : 2; t < ntier; ++t) {
        const int cw = tiers[t][0];
        const int nwork = cw ? CH_BS - 64 : CH_BS;
        for (int pass = 0; pass < 2; ++pass) {
            const int cap = pass == 0 ? room : ctx->ncu;
            for (int r2 = tiers[t][1]; r2 <= tiers[t][2]; ++r2) {
                const int64_t g = (n2 + (int64_t)r2 * nwork - 1) / ((int64_t)r2 * nwork);
                if (g >= 1 && g <= cap) {
                    *r2_out = r2;
                    *g_out = (int)g;
                    if (cw_out) *cw_out = cw;
                    return true;
                }
            }
        }
    }
    return false;
}

template <int R2, bool MASKED, bool XR, bool CW, bool ONE = false>
static hipError_t launch_blk2(kh_ctx ctx, int G, const ChainArgs& a, BlkBufs bf, const XrDev& xr) {
    constexpr auto kern = k_mgs_chain_blk2<R2, MASKED, XR, CW, ONE>;
    int per_cu = 0;
    const hipError_t e = resident_per_cu<kern>(ctx, CH_BS, 0, &per_cu);
    if (e != hipSuccess) return e;
    // workgroups WITHOUT rows in front of the G with rows (chain_blk.h, BlkBufs::nx): when the chip has room for them
    bf.nx = 0;
    if (ctx->blk_nx > 0 && (int64_t)per_cu * ctx->ncu >= G + ctx->blk_nx && G + ctx->blk_nx <= CH_GMAX / 2 && G > BLK_PFLAT * (64 / BLK_BC))
        bf.nx = ctx->blk_nx;
    if (bf.nx > 0) ctx->n_blk_rowless += 1;
    return launch_resident<kern>(ctx, G, ResidentShape{CH_BS, G + bf.nx, ctx->ncu, 0}, a, bf, xr);      // the sums need every workgroup resident
}

// One Arnoldi step k of basis block V (columns 0 .. k, reference order, one sweep; w holds A v_k) on the eight-wave blocked
// kernel: coefficients into hdev[0 .. k], the norm into hdev[k + 1], v_{k+1} stored.  multi: the sums cross the ranks through
// the xr mailboxes inside the launch (no all-reduce call in the step).  Returns 1 when launched, 0 when this shape is not
// served (one GPU only: on a communicator the caller has established eligibility for the longest slab of the run and a
// refusal here is an ERROR - a rank-local fallback would change the pattern of collectives its peers see), negative on error.
int chain_blk2_step(kh_ctx ctx, kh_vec V, const double* w, int64_t wld, int64_t k, double* hdev, int slot, double* hpin, int hcount,
                    bool multi) {
    const int64_t n = V->n;
    int r2 = 0, G = 0, cwi = 0;
    if (!ctx->chain_blk2 || !ctx->chain_configured || !chain_blk2_shape(ctx, n, &r2, &G, &cwi, ctx->blk2_one >= (multi ? 1 : 2)) ||
        k + 3 > BLK_TABCOLS ||
        ((n & 1) && (V->ld <= n || wld <= n)) || (!multi && ctx->blk2_refused_n == n)) {
        if (multi) return fail(KH_ERR_COMM, "blocked Gram-Schmidt with in-kernel cross-rank sums: a slab of %lld rows is not served "
                                            "here although the run's longest slab was found eligible", (long long)n);
        return 0;
    }
    if (multi && !ctx->xr_on) return fail(KH_ERR_COMM, "chain_blk2_step: the xr transport is off");
    KH_TRY(chain_epoch_check(ctx));
    const bool cw = cwi != 0;
    const int64_t chunk2 = (int64_t)r2 * (cw ? CH_BS - 64 : CH_BS);
    const int64_t need_ld = (int64_t)G * chunk2 * 2;
    const bool padded = V->ld >= need_ld && wld >= need_ld;
    BlkBufs bf;
    bf.gtab = chain_blk_table(ctx);
    if (bf.gtab == nullptr) return fail(KH_ERR_NOMEM, "chain_blk2: no memory for the Gram table");
    bf.gran = ctx->blk_gran;
    bf.gran2 = ctx->blk_gran + BLK_GRAN_WORDS;
    bf.res = ctx->blk_gran + BLK_GRAN_WORDS + BLK_GRAN2_WORDS;
    bf.nx = 0;
    // the Gram table (own-block entries: kind 2): valid when this is the next step of the sequence that owns it, otherwise
    // its rows are rebuilt from the basis.  The decision follows (blk_V, blk_next, blk_kind), i.e. the sequence of calls
    // every rank makes alike; on a communicator the panel products are summed across the ranks like any inner product.
    if (!(ctx->blk_V == V && ctx->blk_next == k && ctx->blk_kind == 2)) {
        for (int64_t j = 1; j <= k; ++j) {
            const int64_t b0 = (j / KH_BLK_BC) * KH_BLK_BC;
            if (j > b0) {
                double* row = bf.gtab + j * KH_BLK_TW + KH_BLK_BC;
                KH_TRY(dot_panel_raw(ctx, V, b0, j - b0, V->col(j), row));
                if (multi) KH_TRY(comm_allreduce_dev(ctx, row, j - b0));
            }
        }
        ctx->blk_V = V;
        ctx->blk_next = k;
        ctx->blk_kind = 2;
        ctx->n_blk_rebuild += 1;
    }
    ChainArgs a;
    chain_args_init(ctx, a, V, w, chunk2, k, hdev, slot, hpin, hcount);
    const int nsums = (a.ncol + BLK_BC - 1) / BLK_BC + 1;
    XrDev xr;
    memset(&xr, 0, sizeof(xr));
    if (multi) {
        if (ctx->xr_epoch > 0xfff00000u - (unsigned)nsums)
            return fail(KH_ERR_COMM, "xr: the epoch counter of the cross-rank exchange is exhausted; create a new context");
        for (int r = 0; r < ctx->xr_nranks; ++r) xr.peer[r] = ctx->xr_peer[r];
        xr.rank = ctx->xr_rank;
        xr.nranks = ctx->xr_nranks;
        xr.epoch0 = ctx->xr_epoch;
        xr.timeout_ticks = (long long)(ctx->xr_timeout_ms > 0 ? ctx->xr_timeout_ms : 60000) * 100000ll;
    }
    hipError_t e;
    // 4 ... 6 rows per lane: two blocks in registers, with or without the communication wave; 7: with it only; 8 ... 11: ONE block
    auto launch = [&](auto r, auto c, auto one) {
        return dispatch_bool(multi, [&](auto x) {
            return dispatch_bool(!padded, [&](auto m) {
                return launch_blk2<decltype(r)::value, decltype(m)::value, decltype(x)::value, decltype(c)::value, decltype(one)::value>(ctx, G, a, bf, xr);
            });
        });
    };
    if (r2 <= 6) e = dispatch_int<4, 5, 6>(r2, [&](auto r) { return dispatch_bool(cw, [&](auto c) { return launch(r, c, std::false_type()); }); });
    else if (r2 == 7) e = launch(std::integral_constant<int, 7>(), std::true_type(), std::false_type());
    else e = dispatch_int<8, 9, 10, 11>(r2, [&](auto r) { return launch(r, std::true_type(), std::true_type()); });
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->blk_next = -1;
        if (multi)
            return fail(KH_ERR_HIP, "blocked Gram-Schmidt with in-kernel cross-rank sums: the launch failed (%s); no rank-local "
                                    "fallback on a communicator", hipGetErrorString(e));
        ctx->blk2_refused_n = n;          // (occupancy ...: not tried - nor its table rebuilt - again for vectors of this length)
        return 0;
    }
    ctx->blk_V = V;
    ctx->blk_next = k + 1;
    ctx->blk_kind = 2;
    if (multi) {
        ctx->xr_epoch += (unsigned)nsums;
        ctx->n_xr += nsums;
    }
    ctx->n_chain_blk2 += 1;
    return chain_launched(ctx, slot, a, nsums);
}

}  // namespace kh
