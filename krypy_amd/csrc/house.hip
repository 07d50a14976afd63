// Householder Arnoldi in one launch per step (house.h): the launcher of k_house_chain (real) and k_zhouse_chain (complex
// data: the (re, im) views of c128 blocks) and the entry pairs kh_house_step_begin / _end and kh_zhouse_step_begin / _end.
// A translation unit of its own - the twelve real and ten complex instantiations are compiled here.
//
// Shapes: the rows-per-lane classes of the plain chain family on one GPU, 4 ... 40 double2 rows per lane (complex: 4 ... 32,
// the 40-row complex kernel spills in its streaming loops and is not compiled), each as the
// predicate-free kernel (every block padded to whole workgroup chunks: kh_vec_alloc) and as the MASKED one (short or
// unpadded vectors, a partial last workgroup).  Everything else is declined with KH_HOUSE_NOT_SERVED and the host layer
// applies the reflectors one by one as before: longer vectors (w would need LDS beside the registers), a communicator,
// k + 1 >= N (no reflector is left to make), k + 2 > 1024 (the raw H entries are taken from workgroup 0's first row - complex: its first two rows), more
// workgroups than the XCD-leader form of the sums takes (256), a refused launch (occupancy: remembered for that length).
//
// A timed-out sum (the error word, or the "chain_fault" fake) is reported by kh_house_step_end as KH_HOUSE_TIMED_OUT: the
// kernel has not touched A v_k, so the host re-runs the step on the per-reflector path, which overwrites column k + 1 of both
// blocks and beta[k + 1].  The error word is cleared there and the family is armed again for the next step; the third
// timeout in one context leaves it off (kh_ctx_set "house_chain" 1 starts the count again) - the chain kernels' limit.
// Switch and count are shared by the real and the complex step; the launches are counted apart (n_house_chain,
// n_zhouse_chain), and so is the length whose launch was refused.
#include <hip/hip_runtime.h>
#include <string.h>

#include "krylov_steps.h"
#include "house.h"
#include "kh_launch.h"

namespace kh {

// the resident launcher (kh_launch.h) on the step's kernel
template <int R2, bool MASKED, bool CPLX = false>
static hipError_t launch_house(kh_ctx ctx, int G, const HouseArgs& a) {
    // (if constexpr: a real launcher must not instantiate the complex kernel of its shape - the 40-row one is not shipped)
    if constexpr (CPLX) return launch_resident<k_zhouse_chain<R2, MASKED>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, 0), a);
    else return launch_resident<k_house_chain<R2, MASKED>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, 0), a);
}

}  // namespace kh

using namespace kh;

// Both entries: `cplx` - Hv, V, W are the (re, im) views of complex blocks (one double2 row = one complex row, N = n / 2),
// the kernel is k_zhouse_chain and the H column holds 2 (k + 1) + ZHOUSE_NSCAL doubles.
static int house_begin(kh_ctx ctx, kh_vec Hv, kh_vec Beta, kh_vec V, kh_vec W, int64_t wcol, int64_t k, int slot, bool cplx) {
    const char* who = cplx ? "kh_zhouse_step_begin" : "kh_house_step_begin";
    KH_ARG(ctx && Hv && Beta && V && W, "%s: NULL argument", who);
    KH_ARG(slot >= 0 && slot < KH_NSLOT, "%s: slot %d not in [0,%d)", who, slot, KH_NSLOT);
    KH_ARG(k >= 0 && k + 1 < V->ncols && k + 1 < Hv->ncols,
           "%s: k=%lld needs %lld columns, the basis has %lld, the reflector block %lld", who, (long long)k,
           (long long)(k + 2), (long long)V->ncols, (long long)Hv->ncols);
    KH_ARG(Beta->ncols >= 1 && Beta->n >= k + 2, "%s: the beta array holds %lld entries, step %lld writes entry %lld", who,
           (long long)Beta->n, (long long)k, (long long)(k + 1));
    KH_TRY(check_vec(W, wcol, 1, cplx ? "kh_zhouse_step_begin(W)" : "kh_house_step_begin(W)"));
    KH_ARG(Hv->n == V->n && W->n == V->n, "%s: lengths differ", who);
    KH_ARG(!cplx || (V->n & 1) == 0, "%s: a complex view has an even length, this one %lld", who, (long long)V->n);
    RoctxScope range_(ctx, cplx ? "kh_zhouse_step_begin k=%lld" : "kh_house_step_begin k=%lld", (long long)k);
    const int64_t n = V->n;                  // doubles
    const int64_t rows = cplx ? n / 2 : n;   // rows of the vector: N
    if (!ctx->house_chain || ctx->house_recoveries >= KH_CHAIN_MAX_RECOVERIES || kh_multi(ctx)) return KH_HOUSE_NOT_SERVED;
    int64_t& refused_n = cplx ? ctx->zhouse_refused_n : ctx->house_refused_n;
    if (k + 1 >= rows || k + 2 > 2 * CH_BS || n == refused_n) return KH_HOUSE_NOT_SERVED;
    int r2 = 0, G = 0;
    if (!chain_geometry(ctx, n, &r2, &G) || r2 > 40 || 2 * G > CH_BS) return KH_HOUSE_NOT_SERVED;
    // k_zhouse_chain<40, *> keeps rows of w in scratch: 82 / 116 spilled registers (120 / 224 B per lane) with loads and
    // stores inside the dot and update phases of every link (profiles/zhouse_chain_resource_usage.txt) - not shipped, the
    // 40-row class of complex vectors (N > 32 * 512 * CUs) stays on the per-reflector path
    if (cplx && r2 > ZHOUSE_MAX_R2) return KH_HOUSE_NOT_SERVED;
    // (an odd n is handled as n + 1: row n must exist behind every column)
    if ((n & 1) && (V->ld <= n || Hv->ld <= n || W->ld <= n)) return KH_HOUSE_NOT_SERVED;
    KH_TRY(ensure_hcap(ctx, cplx ? 2 * (k + 1) + ZHOUSE_NSCAL : k + 1 + HOUSE_NSCAL));
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
    if (a.donepin != nullptr) a.done_tag = next_done_tag(ctx, slot);
    hipError_t e;
    if (cplx)        // (40 rows: declined above)
        e = dispatch_int<4, 8, 16, 24, 32>(r2, [&](auto r) {
            return padded ? launch_house<decltype(r)::value, false, true>(ctx, G, a) : launch_house<decltype(r)::value, true, true>(ctx, G, a);
        });
    else
        e = dispatch_int<4, 8, 16, 24, 32, 40>(r2, [&](auto r) {
            return padded ? launch_house<decltype(r)::value, false>(ctx, G, a) : launch_house<decltype(r)::value, true>(ctx, G, a);
        });
    if (e != hipSuccess) {
        // e.g. hipErrorCooperativeLaunchTooLarge: not all workgroups can be co-resident.  A property of this shape on this
        // device: vectors of this length take the per-reflector path from now on
        (void)hipGetLastError();
        refused_n = n;
        return KH_HOUSE_NOT_SERVED;
    }
    if (a.debug == 4) ctx->chain_fault = 0;
    if (cplx) ctx->n_zhouse_chain += 1;
    else ctx->n_house_chain += 1;
    // at most: k + 1 forward links, the reflector's round (complex: a pair and a single), k + 1 backward links
    ctx->chain_epoch += (unsigned)(2 * k + (cplx ? 4 : 3));
    ctx->step[slot].kind = 0;                      // (no Gram-Schmidt step is parked in this slot any more)
    chain_blk_touch(ctx, V);
    ctx->wait_tag[slot] = a.donepin != nullptr;
    if (!ctx->wait_tag[slot]) KH_HIP(hipEventRecord(ctx->hev[slot], ctx->stream));
    return 0;
}

extern "C" {

int kh_house_step_begin(kh_ctx ctx, kh_vec Hv, kh_vec Beta, kh_vec V, kh_vec W, int64_t wcol, int64_t k, int slot) {
    return house_begin(ctx, Hv, Beta, V, W, wcol, k, slot, false);
}

int kh_zhouse_step_begin(kh_ctx ctx, kh_vec Hv, kh_vec Beta, kh_vec V, kh_vec W, int64_t wcol, int64_t k, int slot) {
    return house_begin(ctx, Hv, Beta, V, W, wcol, k, slot, true);
}

// (the slot does not know what kind of step was begun in it: waiting, the error word and the recovery count are the same)
static int house_end(kh_ctx ctx, int slot, int64_t count, double* out, bool cplx) {
    const char* who = cplx ? "kh_zhouse_step_end" : "kh_house_step_end";
    KH_ARG(ctx && out, "%s: NULL", who);
    KH_ARG(slot >= 0 && slot < KH_NSLOT && count >= 0 && count <= ctx->hcap, "%s: slot %d / count %lld", who, slot,
           (long long)count);
    KH_ARG(ctx->hev[slot] != nullptr, "%s: no step was begun", who);
    RoctxScope range_(ctx, cplx ? "kh_zhouse_step_end slot=%lld count=%lld" : "kh_house_step_end slot=%lld count=%lld",
                      (long long)slot, (long long)count);
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

int kh_house_step_end(kh_ctx ctx, int slot, int64_t count, double* out) { return house_end(ctx, slot, count, out, false); }

int kh_zhouse_step_end(kh_ctx ctx, int slot, int64_t count, double* out) { return house_end(ctx, slot, count, out, true); }

}  // extern "C"
