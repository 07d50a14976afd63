// Which register-resident Gram-Schmidt chain kernel takes an Arnoldi / Lanczos step on one GPU, and its launch: the geometry
// of a vector length (chain_geometry, padded_ld), the argument block and the completion tail every chain family shares
// (chain_args_init, chain_launched), and try_chain - four stages in this order, each falling through to the next when its
// kernel does not apply or is refused:
//   1. the Lanczos three-pass kernel (lanczos.h): one link, the banded operator in the prologue
//   2. short vectors without a preconditioner: the blocked kernel (chain_blk.h), else the column ring (k_mgs_chain_small)
//   3. short vectors, all working workgroups on one XCD (chain.h, ONEX)
//   4. the general kernels: plain / LDS parking / PF / long, with one retry on the plain kernel when the LDS form is refused
// The one-GPU instantiations of chain.h, chain_long.h and lanczos.h are compiled here; the launcher itself is kh_launch.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "krylov_steps.h"
#include "chain_long.h"
#include "kh_launch.h"

namespace kh {

// rows-per-workgroup (= template R2) and grid of the chain kernel for vectors of length n
bool chain_geometry(kh_ctx ctx, int64_t n, int* r2_out, int* g_out, bool onex) {
    if (n < 2) return false;
    // an odd n is handled as n+1: the extra element is the (always zero) padding behind the column
    const int64_t n2 = (n + 1) >> 1;
    static const int kR2[] = {4, 8, 16, 24, 32, 40, 48, 56};   // 48 / 56: the last 8 / 16 rows of w live in LDS
    // short vectors: as few workgroups as one XCD has CUs, so that all of them can run there (chain.h, ONEX) - 8 rows
    // per lane on 32 workgroups beat 4 rows on 64 spread over the chip, the sum being the whole link
    if (onex) {
        if (!ctx->chain_onex || ctx->ncu % 8 != 0) return false;
        for (int c : {4, 8}) {
            const int64_t g = (n2 + (int64_t)c * CH_BS - 1) / ((int64_t)c * CH_BS);
            if (g <= ctx->ncu / 8 && g <= 32) {
                *r2_out = c;
                *g_out = (int)g;
                return true;
            }
        }
        return false;
    }
    for (int c : kR2) {
        const int64_t g = (n2 + (int64_t)c * CH_BS - 1) / ((int64_t)c * CH_BS);
        if (g <= ctx->ncu && g <= CH_GMAX) {
            *r2_out = c;
            *g_out = (int)g;
            return true;
        }
    }
    return false;   // w fits neither registers nor registers + LDS (N > 14.68 M on 256 CUs): stream it (k_gs_link)
}

// leading dimension of a block of n-vectors: large vectors are padded to whole chain chunks so
// that the predicate-free kernel applies (<= 0.4 % extra memory at N = 10^7)
int64_t padded_ld(kh_ctx ctx, int64_t n) {
    int64_t ld = ((n + 31) / 32) * 32;
    int r2 = 0, g = 0;
    // (from 4096 rows on: below that a vector is a fraction of one workgroup's chunk)
    if (n >= (1 << 12) && chain_geometry(ctx, n, &r2, &g)) ld = (int64_t)g * r2 * CH_BS * 2;
    if (n >= (1 << 12) && chain_geometry(ctx, n, &r2, &g, true)) ld = std::max(ld, (int64_t)g * r2 * CH_BS * 2);   // (one-XCD shape)
    int cw = 0;
    if (n >= (1 << 12) && chain_blk2_shape(ctx, n, &r2, &g, &cw, ctx->blk2_one >= 1))      // (chain_blk2.h: 4 ... 11 rows, 448 or 512 lanes with rows)
        ld = std::max(ld, (int64_t)g * r2 * (cw ? CH_BS - 64 : CH_BS) * 2);
    return ld == 0 ? 32 : ld;
}

constexpr int KH_BLK_MIN_LINKS = 8;     // Gram-Schmidt links from which the blocked kernel (chain_blk.h) takes a step of short vectors
// true when the step goes to the blocked kernel (which has no operator prologue yet)
static inline bool blk_takes_step(kh_ctx ctx, const ChainArgs& a, int r2) {
    return ctx->chain_blk && r2 == 4 && !a.presub && a.sweeps == 1 && a.col0 == 0 && a.ncol >= KH_BLK_MIN_LINKS &&
           a.ncol + 2 <= KH_BLK_TABCOLS && !kh_multi(ctx);
}

// the epoch counter of the grid-wide sums nears its wrap: everything that carries tags is zeroed, the count starts over
int chain_epoch_check(kh_ctx ctx) {
    if (ctx->chain_epoch <= 0xfff00000u) return 0;
    KH_HIP(hipStreamSynchronize(ctx->stream));
    KH_HIP(hipMemset(ctx->chain_gran, 0, sizeof(unsigned long long) * 4 * CH_GMAX));
    KH_HIP(hipMemset(ctx->chain_xcc, 0, sizeof(unsigned long long) * 128 + sizeof(unsigned) * 16));
    if (ctx->blk_gran != nullptr) {
        // (the blocked kernels' granules only: chain_blk_reset leaves the Gram table of the running Arnoldi sequence
        // alone when the buffer exists - ADVICE r04: a zeroed table behind a still matching (blk_V, blk_next) key
        // silently dropped the corrections.  The key is withdrawn as well: the next blocked step rebuilds its rows.)
        KH_HIP(chain_blk_reset(ctx));
        KH_HIP(hipStreamSynchronize(ctx->stream));
        ctx->blk_next = -1;
    }
    ctx->chain_epoch = 1;
    ctx->n_epoch_wraps += 1;
    return 0;
}

// The argument block of a reference-order step on columns 0 .. k of block V (B == V, one sweep, no operator in the prologue):
// zeroed, then what every chain family fills alike.  try_chain overwrites what its other steps differ in.
void chain_args_init(kh_ctx ctx, ChainArgs& a, kh_vec V, const double* w, int64_t chunk2, int64_t k, double* hdev, int slot,
                     double* hpin, int hcount) {
    memset(&a, 0, sizeof(a));
    a.n2 = (V->n + 1) >> 1;
    a.chunk2 = chunk2;
    a.V = V->d;
    a.B = V->d;
    a.ld = V->ld;
    a.ncol = (int)(k + 1);
    a.sweeps = 1;
    a.w_in = w;
    a.vnext = V->col(k + 1);
    a.hdev = hdev;
    a.hnext = k + 1;
    a.gran = ctx->chain_gran;
    a.xcc_res = ctx->chain_xcc;
    a.xcc_leader = reinterpret_cast<unsigned*>(ctx->chain_xcc + 128);
    a.epoch0 = ctx->chain_epoch;
    a.err = ctx->chain_err;
    a.debug = ctx->chain_fault ? 4 : 0;     // kh_ctx_set("chain_fault", 1): the next launch behaves like a timed-out one
    a.hpin = hpin;
    a.hcount = hcount;
    a.errpin = ctx->chain_err_pin[slot];
    // completion tag (kh_internal.h): whichever chain-family kernel this step ends up launching writes it
    a.donepin = (hpin != nullptr && ctx->tag_wait) ? ctx->done_pin[slot] : nullptr;
    if (a.donepin != nullptr) a.done_tag = next_done_tag(ctx, slot);
    a.n_last = V->n - 1;
#ifdef KH_CHAIN_TRACE
    a.trace = ctx->chain_trace;
#endif
}

// What every successful launch of a chain family leaves behind (nsums: the grid-wide sums it consumed epochs for).  Returns 1.
int chain_launched(kh_ctx ctx, int slot, const ChainArgs& a, int nsums) {
    if (a.debug == 4) ctx->chain_fault = 0;
    ctx->n_chain += 1;
    ctx->chain_epoch += (unsigned)nsums;
    if (a.hpin == nullptr)      // (otherwise workgroup 0 has written the error word to the pinned slot itself)
        KH_HIP(hipMemcpyAsync(ctx->chain_err_pin[slot], ctx->chain_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->wait_tag[slot] = a.donepin != nullptr;
    return 1;
}

// ---- the kernels of chain.h / chain_long.h / lanczos.h on the resident launcher ------------------------------------------
template <int R2, bool MASKED, bool CPLX = false, int FND = 0, int WL = 0>
static hipError_t launch_chain(kh_ctx ctx, int G, const ChainArgs& a) {      // WL: rows of w that live in LDS (long vectors)
    return launch_resident<k_mgs_chain<R2, MASKED, CPLX, FND, WL>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, (size_t)WL * CH_BS * sizeof(double2)), a);
}

// the variant that parks the head of every column in LDS between its dot and its update (B == V)
template <int R2, bool MASKED, bool CPLX = false, int FND = 0>
static hipError_t launch_chain_lds(kh_ctx ctx, int G, const ChainArgs& a) {
    return launch_resident<k_mgs_chain_lds<R2, MASKED, CPLX, FND>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, ChainShapeLds<R2, CPLX>::LDS_BYTES), a);
}

// 48 rows per lane with a third of every column kept on the chip between its two uses (chain_long.h)
template <int FND>
static hipError_t launch_chain_long(kh_ctx ctx, int G, const ChainArgs& a) {
    return launch_resident<k_mgs_chain_long<FND, false>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, ChainShapeLong::LDS_BYTES), a);
}

// the variant that keeps HBM busy through the update phase (chain.h: k_mgs_chain_pf)
template <int R2, bool MASKED, bool CPLX = false, int FND = 0>
static hipError_t launch_chain_pf(kh_ctx ctx, int G, const ChainArgs& a) {
    return launch_resident<k_mgs_chain_pf<R2, MASKED, CPLX, FND>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, ChainShapePf<R2>::LDS_BYTES), a);
}

// short vectors: all working workgroups on one XCD (chain.h, ONEX).  8 G + 8 workgroups are launched; the G that work must
// be co-resident on the 1/8 of the CUs one XCD has.  FND > 0: the banded operator in the prologue.
template <int R2, bool MASKED, bool CPLX, int FND, bool PF>
static hipError_t launch_chain_onex(kh_ctx ctx, int G, const ChainArgs& a) {
    // (both forms of a shape are compiled whichever is asked for, as they always were)
    constexpr auto pf = k_mgs_chain_pf<R2, MASKED, CPLX, FND, true>;
    constexpr auto plain = k_mgs_chain<R2, MASKED, CPLX, FND, 0, true>;
    if constexpr (PF) return launch_resident<pf>(ctx, G, ResidentShape::one_xcd(ctx, CH_BS, G, ChainShapePf<R2>::LDS_BYTES), a);
    else return launch_resident<plain>(ctx, G, ResidentShape::one_xcd(ctx, CH_BS, G, 0), a);
}

// short vectors without a preconditioner: whole columns in a register ring, requested several links ahead
// (chain.h, k_mgs_chain_small); ONEX (+ the communication wave) or spread over the chip
#ifndef KH_SMALL_LA4
#define KH_SMALL_LA4 3
#define KH_SMALL_LA8 2
#endif
template <int R2, bool MASKED, int FND, bool ONEX, bool DMASK = false>
static hipError_t launch_chain_small(kh_ctx ctx, int G, const ChainArgs& a) {
    constexpr int LA = (R2 == 4) ? KH_SMALL_LA4 : KH_SMALL_LA8;          // columns requested ahead
    return launch_resident<k_mgs_chain_small<R2, LA, MASKED, FND, ONEX, DMASK>>(
        ctx, G, ONEX ? ResidentShape::one_xcd(ctx, CH_BS + 64, G, 0) : ResidentShape::chip(ctx, CH_BS, G, 0), a);
}

// one Lanczos step in three passes (lanczos.h)
template <int R2, int FND, bool JAC, bool MR>
static hipError_t launch_lanczos(kh_ctx ctx, int G, const ChainArgs& a, const MinresJob& mr) {
    constexpr size_t lds = (size_t)(LanczosShape<R2>::WL + (JAC ? LanczosShape<R2>::DL : 0)) * CH_BS * sizeof(double2);
    return launch_resident<k_lanczos_fused<R2, FND, JAC, MR>>(ctx, G, ResidentShape::chip(ctx, CH_BS, G, lds), a, mr);
}

// ---- try_chain ------------------------------------------------------------------------------------------------------------
namespace {

// what try_chain has worked out about a step before it picks a kernel
struct ChainPlan {
    int64_t n;
    int r2, G;
    bool want_onex;      // the one-XCD geometry: (r2, G) are that shape's
    bool padded;         // every block involved is padded to G whole chunks: the predicate-free kernels
    bool fused;          // the banded operator in the prologue
    bool use_lds, use_long, use_pf;
    ChainArgs a;
};

// counters of a launch with the operator in its prologue
inline void count_fused(kh_ctx ctx, const ChainPlan& p) {
    ctx->n_chain_fused += p.fused ? 1 : 0;
    ctx->n_dia_mask += (p.fused && p.a.dmask != nullptr) ? 1 : 0;
}

// 1. a step with ONE Gram-Schmidt link (Lanczos / MINRES, the first Arnoldi step): three passes instead of six
int chain_stage_lanczos(kh_ctx ctx, const ChainStep& s, ChainPlan& p) {
    ChainArgs& a = p.a;
    if (!(p.fused && !s.cplx && p.r2 <= 40 && ctx->lanczos_fused && a.ncol == 1 && a.sweeps == 1 && (s.dg == nullptr || s.P != nullptr)))
        return 0;
    if (!s.presub) {                 // no previous column: subtract 0 * (some valid column)
        a.bprev = s.B->col(s.k);
        a.h_km1 = 0.0;
        a.h_km1_dev = nullptr;
    }
    MinresJob job;
    if (s.mr != nullptr) job = *s.mr;
    else {
        job.on = 0;
        job.v = job.w1 = s.w;           // (never dereferenced)
        job.w0 = job.yk = const_cast<double*>(s.w);
        job.r0 = job.r1 = job.y0 = 0.0;
        job.r2 = 1.0;
    }
    const hipError_t e = dispatch_int<4, 8, 16, 24, 32, 40>(p.r2, [&](auto r) {
        return dispatch_nd(a.offs.nd, [&](auto d) {
            return dispatch_bool(s.dg != nullptr, [&](auto jac) {
                return dispatch_bool(job.on != 0, [&](auto mr) {
                    return launch_lanczos<decltype(r)::value, decltype(d)::value, decltype(jac)::value, decltype(mr)::value>(ctx, p.G, a, job);
                });
            });
        });
    });
    if (e == hipSuccess) {
        count_fused(ctx, p);
        ctx->n_lanczos_fused += 1;
        ctx->mr_taken = job.on ? 1 : 0;     // (the MINRES job - if any - went along)
        return chain_launched(ctx, s.slot, a, 2);      // the coefficient's and the norm's grid-wide sums
    }
    (void)hipGetLastError();             // e.g. the dynamic LDS was refused: the general chain kernel below
    if (!s.presub) a.bprev = nullptr;
    return 0;
}

// 2. short vectors, no preconditioner, real data: the column-ring kernel (one read per column, several links of look-ahead),
// and for a long chain its blocked form - one grid-wide sum per FOUR columns (chain_blk.h)
int chain_stage_ring(kh_ctx ctx, const ChainStep& s, ChainPlan& p) {
    ChainArgs& a = p.a;
    const int r2 = p.r2, G = p.G;
    const bool fused = p.fused, padded = p.padded, want_onex = p.want_onex;
    const int64_t k = s.k;
    kh_vec V = s.V;
    const bool blk_debug = (a.debug >= 1 && a.debug <= 3) && !fused && padded && blk_takes_step(ctx, a, r2);   // measurement modes of the blocked kernel
    if (!(ctx->chain_small && r2 <= 8 && s.B == V && s.dg == nullptr && !s.cplx && (a.debug == 0 || a.debug == 4 || blk_debug) &&
          !(fused && ctx->lanczos_fused && a.ncol == 1 && a.sweeps == 1)))
        return 0;
    hipError_t e;
    if (blk_takes_step(ctx, a, r2) && padded && chain_blk_shape_ok(r2, G, a, fused ? a.offs.nd : 0) && ctx->blk_refused_n != p.n) {
        int nsums = 0;
        // the Gram table: valid when this is the next step of the sequence that owns it; otherwise (a sequence's
        // first blocked step, a block grown / recycled / written by another entry point since) its rows are
        // rebuilt from the basis - one panel product per column, once
        if (!(ctx->blk_V == V && ctx->blk_next == k && ctx->blk_kind == 1)) {
            double* gt = chain_blk_table(ctx);
            if (gt == nullptr) return fail(KH_ERR_NOMEM, "chain_blk: no memory for the Gram table");
            for (int64_t j = 1; j <= k; ++j) {
                const int64_t b0 = (j / KH_BLK_BC) * KH_BLK_BC;
                if (b0 >= KH_BLK_BC)      // the block before column j's (the kernel takes its dots one block ahead)
                    KH_TRY(dot_panel_raw(ctx, V, b0 - KH_BLK_BC, KH_BLK_BC, V->col(j), gt + j * KH_BLK_TW));
                if (j > b0) KH_TRY(dot_panel_raw(ctx, V, b0, j - b0, V->col(j), gt + j * KH_BLK_TW + KH_BLK_BC));
            }
            ctx->blk_V = V;
            ctx->blk_next = k;
            ctx->blk_kind = 1;
            ctx->n_blk_rebuild += 1;
        }
        e = chain_blk_launch(ctx, r2, G, want_onex, padded, fused ? a.offs.nd : 0, a, V, &nsums);
        if (e == hipSuccess) {
            ctx->blk_kind = 1;
            ctx->n_chain_small += 1;
            ctx->n_chain_blk += 1;
            ctx->n_chain_onex += want_onex ? 1 : 0;
            count_fused(ctx, p);
            ctx->n_chain_lds += 1;
            return chain_launched(ctx, s.slot, a, nsums);
        }
        (void)hipGetLastError();
        // refused (occupancy: other kernels resident, fewer compute units ...): remembered for vectors of this length, so
        // that the steps to come do not rebuild the table - up to 2 k panel products - just to be refused again
        // (kh_ctx_set("chain_blk", 1) forgets it)
        ctx->blk_refused_n = p.n;
    }
    e = dispatch_int<4, 8>(r2, [&](auto r) {
        return dispatch_bool(want_onex, [&](auto x) {
            constexpr int R = decltype(r)::value;
            constexpr bool X = decltype(x)::value;
            if (fused)
                return dispatch_nd(a.offs.nd, [&](auto d) {
                    return dispatch_bool(a.dmask != nullptr, [&](auto m) {
                        return launch_chain_small<R, false, decltype(d)::value, X, decltype(m)::value>(ctx, G, a);
                    });
                });
            return padded ? launch_chain_small<R, false, 0, X>(ctx, G, a) : launch_chain_small<R, true, 0, X>(ctx, G, a);
        });
    });
    if (e == hipSuccess) {
        ctx->n_chain_small += 1;
        ctx->n_chain_onex += want_onex ? 1 : 0;
        count_fused(ctx, p);
        ctx->n_chain_lds += 1;          // (the column is used twice from the chip: counted with the LDS / ring family)
        return chain_launched(ctx, s.slot, a, a.ncol * a.sweeps + 1);
    }
    (void)hipGetLastError();
    return 0;
}

// 3. short vectors (4 ... 32 workgroups of 4 / 8 rows per lane): a link is its grid-wide sum - all working
// workgroups on ONE XCD, where the sum is an L2 round trip (chain.h, ONEX)
int chain_stage_onex(kh_ctx ctx, const ChainStep& s, ChainPlan& p) {
    ChainArgs& a = p.a;
    if (!p.want_onex) return 0;
    const bool pf_ = (s.B == s.V && s.dg == nullptr && ctx->chain_pf != 0 && ctx->chain_lds != 0);
    const hipError_t e = dispatch_int<4, 8>(p.r2, [&](auto r) {
        return dispatch_bool(pf_, [&](auto pf) {
            constexpr int R = decltype(r)::value;
            constexpr bool PF = decltype(pf)::value;
            if (p.fused)
                return dispatch_nd(a.offs.nd, [&](auto d) { return launch_chain_onex<R, false, false, decltype(d)::value, PF>(ctx, p.G, a); });
            return dispatch_bool(s.cplx, [&](auto z) {
                constexpr bool Z = decltype(z)::value;
                return p.padded ? launch_chain_onex<R, false, Z, 0, PF>(ctx, p.G, a) : launch_chain_onex<R, true, Z, 0, PF>(ctx, p.G, a);
            });
        });
    });
    if (e == hipSuccess) {
        ctx->n_chain_onex += 1;
        count_fused(ctx, p);
        ctx->n_chain_lds += pf_ ? 1 : 0;
        ctx->n_chain_pf += pf_ ? 1 : 0;
        return chain_launched(ctx, s.slot, a, a.ncol * a.sweeps + 1);
    }
    (void)hipGetLastError();
    return 0;
}

// 4. the general kernels, spread over the chip
int chain_stage_general(kh_ctx ctx, const ChainStep& s, ChainPlan& p) {
    ChainArgs& a = p.a;
    const int r2 = p.r2, G = p.G;
    const bool fused = p.fused, padded = p.padded, cplx = s.cplx;
    bool& use_lds = p.use_lds;
    bool& use_long = p.use_long;
    const bool use_pf = p.use_pf;
    hipError_t e = hipSuccess;
    a.onex_G = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        // k_mgs_chain_lds, mask form: x through the prologue's LDS window when a row's band and the block staged beside it
        // fit the parked rows the prologue leaves free (all or nothing per launch; x must start a 16-byte row)
        a.xwin = (fused && !cplx && use_lds && !use_pf && ctx->chain_xwin && a.dmask != nullptr && r2 >= 16 && r2 <= 40 &&
                  (reinterpret_cast<uintptr_t>(a.xk) & 15u) == 0 &&
                  xwin_fits(a.offs, a.offs.nd, r2 == 40 ? ChainShapeLds<40>::XWIN_BLOCKS : ChainShapeLds<32>::XWIN_BLOCKS)) ? 1 : 0;
        if (fused) {
            if (r2 < 16) return 0;       // (4 / 8 rows: only the Lanczos and the one-XCD kernels have the prologue)
            if (cplx) {
                e = dispatch_int<16, 24, 32, 40>(r2, [&](auto r) {
                    return dispatch_nd(a.offs.nd, [&](auto d) {
                        constexpr int R = decltype(r)::value, D = decltype(d)::value;
                        return use_lds ? launch_chain_lds<R, false, true, D>(ctx, G, a) : launch_chain<R, false, true, D>(ctx, G, a);
                    });
                });
            } else if (r2 == 48) {
                e = dispatch_nd(a.offs.nd, [&](auto d) {
                    constexpr int D = decltype(d)::value;
                    if (use_long) {
                        if (launch_chain_long<D>(ctx, G, a) == hipSuccess) return hipSuccess;
                        (void)hipGetLastError();       // (e.g. the 128 KB of dynamic LDS were refused: the kernel with both reads from memory)
                        ctx->chain_long_failed = 1;
                        use_long = false;
                    }
                    return launch_chain<48, false, false, D, 8>(ctx, G, a);
                });
            } else {
                e = dispatch_int<16, 24, 32, 40>(r2, [&](auto r) {
                    return dispatch_nd(a.offs.nd, [&](auto d) {
                        constexpr int R = decltype(r)::value, D = decltype(d)::value;
                        return use_lds ? (use_pf ? launch_chain_pf<R, false, false, D>(ctx, G, a) : launch_chain_lds<R, false, false, D>(ctx, G, a))
                                       : launch_chain<R, false, false, D>(ctx, G, a);
                    });
                });
            }
            if (e != hipSuccess) {       // the caller falls back to SpMV + the ordinary chain
                (void)hipGetLastError();
                return 0;
            }
            break;
        }
        if (r2 <= 40) {
            e = dispatch_int<4, 8, 16, 24, 32, 40>(r2, [&](auto r) {
                return dispatch_bool(cplx, [&](auto z) {
                    return dispatch_bool(!padded, [&](auto m) {
                        constexpr int R = decltype(r)::value;
                        constexpr bool Z = decltype(z)::value, M = decltype(m)::value;
                        return use_lds ? (use_pf ? launch_chain_pf<R, M, Z>(ctx, G, a) : launch_chain_lds<R, M, Z>(ctx, G, a))
                                       : launch_chain<R, M, Z>(ctx, G, a);
                    });
                });
            });
        } else if (r2 == 48 && use_long) {
            e = launch_chain_long<0>(ctx, G, a);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                ctx->chain_long_failed = 1;
                use_long = false;
                e = launch_chain<48, false, false, 0, 8>(ctx, G, a);
            }
        }
        else if (r2 == 48) e = padded ? launch_chain<48, false, false, 0, 8>(ctx, G, a) : launch_chain<48, true, false, 0, 8>(ctx, G, a);
        else e = padded ? launch_chain<56, false, false, 0, 16>(ctx, G, a) : launch_chain<56, true, false, 0, 16>(ctx, G, a);
        if (e == hipSuccess || !use_lds) break;
        (void)hipGetLastError();     // e.g. the 120 KB of dynamic LDS were refused: fall back to the plain kernel
        ctx->chain_lds_failed = 1;
        use_lds = false;
    }
    if (e != hipSuccess) {
        // e.g. hipErrorCooperativeLaunchTooLarge: not all workgroups can be co-resident.  A property of this shape
        // on this device, not of the context: vectors of this length take the per-column kernels from now on
        (void)hipGetLastError();
        ctx->chain_refused_n = p.n;
        return 0;
    }
    ctx->n_chain_lds += (use_lds || use_long) ? 1 : 0;
    ctx->n_chain_long += use_long ? 1 : 0;
    ctx->n_chain_pf += use_pf ? 1 : 0;
    count_fused(ctx, p);
    ctx->n_chain_xwin += a.xwin;
    return chain_launched(ctx, s.slot, a, a.ncol * a.sweeps + 1);   // one grid reduction per link (complex: both parts in it) + the norm
}

}  // namespace

// returns 1 if the chain was launched, 0 if this step is not eligible (caller uses the link
// kernels), negative on error
int try_chain(kh_ctx ctx, const ChainStep& s) {
    kh_vec V = s.V, B = s.B, P = s.P;
    const double* w = s.w;
    const double* dg = s.dg;
    const double* xk = s.xk;
    const int64_t wld = s.wld, k = s.k, start = s.start;
    const int sweeps = s.sweeps;
    const bool presub = s.presub, cplx = s.cplx;
    kh_mat Afuse = s.Afuse;
    if (!ctx->chain_enabled || kh_multi(ctx)) return 0;
    if (cplx && (dg != nullptr || P != nullptr)) return 0;
    const int64_t n = V->n;
    if (n == ctx->chain_refused_n) return 0;
    int r2 = 0, G = 0;
    if (!chain_geometry(ctx, n, &r2, &G)) return 0;
    // short vectors with at least a few links in the launch: as few workgroups as one XCD has CUs, all of them
    // there (chain.h, ONEX) - the sum is the whole link.  (One or two links - Lanczos, the first Arnoldi steps - do
    // not pay for the larger grid: MINRES + Jacobi at N = 10^5 32,400 vs 27,400 it/s.)
    bool want_onex = false;
    if ((k - start + 1) * sweeps >= 3 && (ctx->chain_debug == 0) && ctx->onex_ticket != nullptr) {
        int r2x = 0, Gx = 0;
        // (the column-ring kernel with 8 rows per lane - 1.3e5 < N <= 2.6e5 - is faster spread over the chip with 4:
        // a one-XCD link moves the whole column through one XCD's port; 7,240 vs 6,770 it/s at N = 2.5e5)
        const bool ring_kernel = ctx->chain_small && B == V && dg == nullptr && !cplx;
        // (... and the blocked kernel - four times fewer sums - is bound by the one XCD's memory port from
        // ctx->blk_onex_maxn rows on: it then spreads over the chip as well)
        const bool blk_long = ctx->chain_blk && ring_kernel && !presub && sweeps == 1 && start == 0 &&
                              k + 1 >= KH_BLK_MIN_LINKS && r2 == 4 && n > ctx->blk_onex_maxn;
        if (chain_geometry(ctx, n, &r2x, &Gx, true) && !(ring_kernel && r2x == 8 && r2 == 4) && !blk_long) {
            r2 = r2x;
            G = Gx;
            want_onex = true;
        }
    }
    if (cplx && 4 * G > 2 * CH_GMAX) return 0;      // grid_sum2: four granules per workgroup
    if ((n & 1) && (V->ld <= n || B->ld <= n || wld <= n || (P && P->ld <= n))) return 0;
    // 1.05 M ... 2.5 M rows (8 / 16 rows per lane in the general geometry, 5 ... 11 here), no preconditioner, a long chain: the
    // eight-wave blocked kernel (chain_blk2.h) - one grid-wide sum per four columns, columns read once.  It loads w: with the
    // operator to be fused (Afuse) nothing is launched here, the caller runs the SpMV and comes back without it.
    {
        int r2b = 0, Gb = 0;
        if (ctx->chain_blk2 && ctx->chain_blk && ctx->chain_small && (r2 == 8 || (r2 == 16 && ctx->blk2_one >= 2)) && !want_onex && B == V && dg == nullptr && !cplx && !presub &&
            sweeps == 1 && start == 0 && k + 1 >= KH_BLK_MIN_LINKS && (ctx->chain_debug == 0) && n != ctx->blk2_refused_n &&
            chain_blk2_shape(ctx, n, &r2b, &Gb, nullptr, ctx->blk2_one >= 2) && r2b > 4) {
            if (Afuse != nullptr) return 0;
            const int rc = chain_blk2_step(ctx, V, w, wld, k, s.hdev, s.slot, s.hpin, s.hcount, false);
            if (rc != 0) {
                if (rc == 1) ctx->n_chain_lds += 1;      // (the column is used twice from the chip: counted with that family)
                return rc;
            }
        }
    }
    const int64_t chunk2 = (int64_t)r2 * CH_BS;
    // predicate-free kernel iff every block involved is padded to G whole chunks
    const int64_t need_ld = (int64_t)G * chunk2 * 2;
    const bool padded = V->ld >= need_ld && B->ld >= need_ld && (P == nullptr || P->ld >= need_ld) &&
                        wld >= need_ld;
    KH_TRY(chain_epoch_check(ctx));
    ChainPlan p;
    ChainArgs& a = p.a;
    chain_args_init(ctx, a, V, w, chunk2, k, s.hdev, s.slot, s.hpin, s.hcount);
    a.B = B->d;
    a.col0 = start;
    a.ncol = (int)(k - start + 1);
    a.sweeps = sweeps;
    a.dg = dg;
    a.pnext = P ? P->col(k + 1) : nullptr;
    a.hnext = cplx ? 2 * (k + 1) : k + 1;
    if (!ctx->chain_fault) a.debug = ctx->chain_debug;
    a.presub = presub ? 1 : 0;
    a.h_km1 = s.h_km1;
    a.h_km1_dev = s.h_km1_dev;
    a.bprev = presub ? B->col(k - 1) : nullptr;
    const int lds_env = ctx->chain_lds;
    // (the complex instantiation with 40 rows per lane spills 36 registers with the LDS traffic on top
    // and still beats the plain kernel, 769 vs 677 it/s at N = 5*10^6; 32 rows fit without spills since
    // both parts of the coefficient share one grid reduction)
    // (chain_lds_failed: the LDS variant could not be launched once in this context: plain kernel from then on)
    // (an unpadded block of a long vector - not what kh_vec_alloc produces - takes the plain kernel: the
    // masked LDS instantiations with 32 / 40 rows spill)
    bool use_lds = lds_env && !ctx->chain_lds_failed && B == V && dg == nullptr && (a.debug == 0 || a.debug == 4) &&
                   (padded || r2 <= 24) && r2 <= 40;     // (48 / 56 rows: LDS holds a part of w itself)
    if (r2 > 40 && cplx) return 0;
    // 48 rows per lane, no preconditioner, padded blocks: a third of every column stays on the chip between its two uses
    bool use_long = ctx->chain_long && ctx->chain_lds && !ctx->chain_long_failed && r2 == 48 && B == V && dg == nullptr && !cplx && padded && (a.debug == 0 || a.debug == 4);
    // fused operator: the padded real kernels with 16 ... 40 rows per lane (N > 2.1 M) have that prologue
    bool fused = false;
    if (Afuse != nullptr) {
        // Afuse: compute w = Afuse * xk in the kernel's prologue instead of reading w (banded operators; 0 is returned
        // without launching anything when that variant does not apply - the caller then runs the SpMV and calls again
        // without Afuse)
        // (a step with one Gram-Schmidt link has the three-pass kernel of lanczos.h for every shape up to 40 rows)
        const bool lz_shape = ctx->lanczos_fused && a.ncol == 1 && a.sweeps == 1 && (dg == nullptr || P != nullptr) &&
                              (r2 == 4 || r2 == 8);
        const bool small_shape = ctx->chain_small && r2 <= 8 && B == V && dg == nullptr;
        if (cplx) {
            // complex banded operator (zpath.h: zdia, leading dimension and rows counted in complex entries): the padded
            // chain kernels with 16 ... 40 rows per lane, spread over the chip
            fused = ctx->chain_spmv && padded && ((a.debug & 3) == 0) && r2 >= 16 && r2 <= 40 && !want_onex && xk != nullptr &&
                    Afuse->kind == KH_MAT_ZCSR && Afuse->zdia != nullptr && (Afuse->dia_nd == 5 || Afuse->dia_nd == 7) &&
                    2 * Afuse->n_rows == n && Afuse->nrecv_prev + Afuse->nrecv_next == 0 && 2 * Afuse->zdia_ld >= need_ld;
        } else {
            fused = ctx->chain_spmv && padded && ((a.debug & 3) == 0) && ((r2 >= 16 && r2 <= 48) || want_onex || lz_shape || small_shape) && xk != nullptr &&
                    Afuse->kind == KH_MAT_CSR && kh_banded(Afuse) && (Afuse->dia_nd == 5 || Afuse->dia_nd == 7) &&
                    Afuse->n_rows == n && Afuse->nrecv_prev + Afuse->nrecv_next == 0 && Afuse->dia_ld >= need_ld;
        }
        if (!fused) return 0;
        a.dia = cplx ? Afuse->zdia : Afuse->dia;
        a.dmask = cplx ? nullptr : Afuse->dmask;
        a.dia_ld = cplx ? Afuse->zdia_ld : Afuse->dia_ld;
        a.xk = xk;
        a.n_last = cplx ? Afuse->n_rows - 1 : n - 1;
        a.offs = dia_offs(Afuse);
    }
    p.n = n;
    p.r2 = r2;
    p.G = G;
    p.want_onex = want_onex;
    p.padded = padded;
    p.fused = fused;
    p.use_lds = use_lds;
    p.use_long = use_long;
    // k_mgs_chain_pf wins where the whole column stays on chip (<= 24 rows per lane: 6.9 vs 7.2 us per link at
    // N = 4*10^6); with 32 / 40 rows its prefetches sit in the CU's memory queue in front of the reduction's polls
    // and cost what they save (17.4 vs 16.3 us per link at N = 10^7)
    p.use_pf = use_lds && ctx->chain_pf && (r2 <= 24 || (ctx->chain_pf == 2 && r2 <= 40));   // (2: measurement)
    int rc = chain_stage_lanczos(ctx, s, p);
    if (rc != 0) return rc;
    if (want_onex) {         // the ticket words of a one-XCD launch (rotating: this launch zeroes the word of one far in the future)
        const unsigned slot_ = (unsigned)(ctx->n_chain_onex & 255);
        a.onex_G = G;
        a.onex_target = 0u;
        a.onex_ticket = ctx->onex_ticket + slot_;
        a.onex_clear = ctx->onex_ticket + ((slot_ + 128u) & 255u);
    }
    rc = chain_stage_ring(ctx, s, p);
    if (rc != 0) return rc;
    rc = chain_stage_onex(ctx, s, p);
    if (rc != 0) return rc;
    return chain_stage_general(ctx, s, p);
}

}  // namespace kh
