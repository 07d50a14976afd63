// Householder Arnoldi in one launch per step (house.h): the launcher of k_house_chain and the entry pair
// kh_house_step_begin / _end.  A translation unit of its own - the twelve instantiations are compiled here.
//
// Shapes: the rows-per-lane classes of the plain chain family on one GPU, 4 ... 40 double2 rows per lane, each as the
// predicate-free kernel (every block padded to whole workgroup chunks: kh_vec_alloc) and as the MASKED one (short or
// unpadded vectors, a partial last workgroup).  Everything else is declined with KH_HOUSE_NOT_SERVED and the host layer
// applies the reflectors one by one as before: longer vectors (w would need LDS beside the registers), a communicator,
// k + 1 >= N (no reflector is left to make), k + 2 > 1024 (the raw H entries are taken from workgroup 0's first row), more
// workgroups than the XCD-leader form of the sums takes (256), a refused launch (occupancy: remembered for that length).
//
// A timed-out sum (the error word, or the "chain_fault" fake) is reported by kh_house_step_end as KH_HOUSE_TIMED_OUT: the
// kernel has not touched A v_k, so the host re-runs the step on the per-reflector path, which overwrites column k + 1 of both
// blocks and beta[k + 1].  The error word is cleared there and the family is armed again for the next step; the third
// timeout in one context leaves it off (kh_ctx_set "house_chain" 1 starts the count again) - the chain kernels' limit.
#include <hip/hip_runtime.h>
#include <string.h>

#include "krylov_steps.h"
#include "house.h"

namespace kh {

template <int R2, bool MASKED>
static hipError_t launch_house(kh_ctx ctx, int G, HouseArgs& a) {
    // (cached per process like launch_chain's: one context = one device = one process, single-threaded by the contract
    // of krylov_hip.h; a second device of another kind in the same process would need the figure per context)
    static int blocks_per_cu = -1;
    auto kern = k_house_chain<R2, MASKED>;
    if (blocks_per_cu < 0) {
        int nb = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, CH_BS, 0);
        if (e != hipSuccess) return e;
        blocks_per_cu = nb;
    }
    // a plain launch whose grid is checked against the occupancy of the instantiation (krylov_hip.hip: launch_chain)
    if ((int64_t)blocks_per_cu * ctx->ncu < G) return hipErrorCooperativeLaunchTooLarge;
    hipLaunchKernelGGL(kern, dim3(G), dim3(CH_BS), 0, ctx->stream, a);
    return hipGetLastError();
}

}  // namespace kh

using namespace kh;

extern "C" {

int kh_house_step_begin(kh_ctx ctx, kh_vec Hv, kh_vec Beta, kh_vec V, kh_vec W, int64_t wcol, int64_t k, int slot) {
    KH_ARG(ctx && Hv && Beta && V && W, "kh_house_step_begin: NULL argument");
    KH_ARG(slot >= 0 && slot < KH_NSLOT, "kh_house_step_begin: slot %d not in [0,%d)", slot, KH_NSLOT);
    KH_ARG(k >= 0 && k + 1 < V->ncols && k + 1 < Hv->ncols,
           "kh_house_step_begin: k=%lld needs %lld columns, the basis has %lld, the reflector block %lld", (long long)k,
           (long long)(k + 2), (long long)V->ncols, (long long)Hv->ncols);
    KH_ARG(Beta->ncols >= 1 && Beta->n >= k + 2, "kh_house_step_begin: the beta array holds %lld entries, step %lld writes entry %lld",
           (long long)Beta->n, (long long)k, (long long)(k + 1));
    KH_TRY(check_vec(W, wcol, 1, "kh_house_step_begin(W)"));
    KH_ARG(Hv->n == V->n && W->n == V->n, "kh_house_step_begin: lengths differ");
    RoctxScope range_(ctx, "kh_house_step_begin k=%lld", (long long)k);
    const int64_t n = V->n;
    if (!ctx->house_chain || ctx->house_recoveries >= KH_CHAIN_MAX_RECOVERIES || kh_multi(ctx)) return KH_HOUSE_NOT_SERVED;
    if (k + 1 >= n || k + 2 > 2 * CH_BS || n == ctx->house_refused_n) return KH_HOUSE_NOT_SERVED;
    int r2 = 0, G = 0;
    if (!chain_geometry(ctx, n, &r2, &G) || r2 > 40 || 2 * G > CH_BS) return KH_HOUSE_NOT_SERVED;
    // (an odd n is handled as n + 1: row n must exist behind every column)
    if ((n & 1) && (V->ld <= n || Hv->ld <= n || W->ld <= n)) return KH_HOUSE_NOT_SERVED;
    KH_TRY(ensure_hcap(ctx, k + 1 + HOUSE_NSCAL));
    KH_TRY(chain_epoch_check(ctx));
    const int64_t chunk2 = (int64_t)r2 * CH_BS;
    // predicate-free kernel iff every block involved is padded to G whole chunks
    const int64_t need_ld = (int64_t)G * chunk2 * 2;
    const bool padded = V->ld >= need_ld && Hv->ld >= need_ld && W->ld >= need_ld;
    HouseArgs a;
    memset(&a, 0, sizeof(a));
    a.n2 = (n + 1) >> 1;
    a.chunk2 = chunk2;
    a.U = Hv->d;
    a.ldu = Hv->ld;
    a.unext = Hv->col(k + 1);
    a.beta = Beta->d;
    a.w_in = W->col(wcol);
    a.vnext = V->col(k + 1);
    a.k = (int)k;
    a.gran = ctx->chain_gran;
    a.xcc_res = ctx->chain_xcc;
    a.xcc_leader = reinterpret_cast<unsigned*>(ctx->chain_xcc + 128);
    a.epoch0 = ctx->chain_epoch;
    a.err = ctx->chain_err;
    a.debug = ctx->chain_fault ? 4 : 0;      // kh_ctx_set("chain_fault", 1): the next launch behaves like a timed-out one
    a.hpin = ctx->hslot_pin[slot];
    a.errpin = ctx->chain_err_pin[slot];
    a.donepin = ctx->tag_wait ? ctx->done_pin[slot] : nullptr;
    if (a.donepin != nullptr) {
        ctx->done_counter = (ctx->done_counter == 0x7fffffff) ? 1 : ctx->done_counter + 1;
        a.done_tag = ctx->done_counter;
        ctx->done_seq[slot] = a.done_tag;
    }
    hipError_t e;
#define KH_HOUSE(R) (padded ? launch_house<R, false>(ctx, G, a) : launch_house<R, true>(ctx, G, a))
    switch (r2) {
        case 4: e = KH_HOUSE(4); break;
        case 8: e = KH_HOUSE(8); break;
        case 16: e = KH_HOUSE(16); break;
        case 24: e = KH_HOUSE(24); break;
        case 32: e = KH_HOUSE(32); break;
        default: e = KH_HOUSE(40); break;
    }
#undef KH_HOUSE
    if (e != hipSuccess) {
        // e.g. hipErrorCooperativeLaunchTooLarge: not all workgroups can be co-resident.  A property of this shape on this
        // device: vectors of this length take the per-reflector path from now on
        (void)hipGetLastError();
        ctx->house_refused_n = n;
        return KH_HOUSE_NOT_SERVED;
    }
    if (a.debug == 4) ctx->chain_fault = 0;
    ctx->n_house_chain += 1;
    ctx->chain_epoch += (unsigned)(2 * k + 3);     // at most: k + 1 forward links, the reflector's pair, k + 1 backward links
    ctx->step[slot].kind = 0;                      // (no Gram-Schmidt step is parked in this slot any more)
    chain_blk_touch(ctx, V);
    ctx->wait_tag[slot] = a.donepin != nullptr;
    if (!ctx->wait_tag[slot]) KH_HIP(hipEventRecord(ctx->hev[slot], ctx->stream));
    return 0;
}

int kh_house_step_end(kh_ctx ctx, int slot, int64_t count, double* out) {
    KH_ARG(ctx && out, "kh_house_step_end: NULL");
    KH_ARG(slot >= 0 && slot < KH_NSLOT && count >= 0 && count <= ctx->hcap, "kh_house_step_end: slot %d / count %lld", slot,
           (long long)count);
    KH_ARG(ctx->hev[slot] != nullptr, "kh_house_step_end: no step was begun");
    RoctxScope range_(ctx, "kh_house_step_end slot=%lld count=%lld", (long long)slot, (long long)count);
    KH_TRY(wait_slot(ctx, slot));
    if (*ctx->chain_err_pin[slot] != 0) {
        // a grid-wide sum of the launch timed out (its workgroups were not co-resident: a shared GPU): column k + 1 of both
        // blocks, beta[k + 1] and this H column are garbage, A v_k and everything before are intact
        *ctx->chain_err_pin[slot] = 0;
        KH_HIP(hipStreamSynchronize(ctx->stream));
        KH_HIP(hipMemset(ctx->chain_err, 0, sizeof(int)));
        ctx->n_house_recovered += 1;
        ctx->house_recoveries += 1;
        if (ctx->house_recoveries == KH_CHAIN_MAX_RECOVERIES)
            fprintf(stderr, "krylov_hip: the grid-wide sum of the one-launch Householder step timed out %d times in this context "
                            "(a GPU shared with other work?); it stays off, the per-reflector path takes over\n",
                    KH_CHAIN_MAX_RECOVERIES);
        return KH_HOUSE_TIMED_OUT;
    }
    memcpy(out, ctx->hslot_pin[slot], sizeof(double) * count);
    return 0;
}

}  // extern "C"
