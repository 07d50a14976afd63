// BiCGStab on the device: the fused vector kernels of the recurrences and the C entry points above them (the header has the
// iteration and the contract).  One iteration on the operator A^ = Ml A Mr, every expression rounded as written:
//
//   k > 0:  p = r + beta * (p - omega * v)                               k_bicg_dir     4 passes  (r, p, v in; p out)
//           v = A^ p ;  sigma = <r~, v>                                  apply_one + the dot kernels (2 passes for the sum)
//           alpha = rho / sigma ;  s = r - alpha * v ;  ss = <s, s>      k_bicg_half    3 passes  (r, v in; s out)
//           t = A^ s ;  theta = <t, s> ;  phi = <t, t>                   apply_one + k_bicg_dots   2 passes  (s, t in)
//           omega = theta / phi ;  y = (y + alpha * p) + omega * s
//           r = s - omega * t ;  rho' = <r~, r> ;  rr = <r, r>           k_bicg_full    7 passes  (r~, p, s, t, y in; y, r out)
//
// 16 vector passes in the four kernels (4 + 3 + 2 + 7), 2 for sigma, and the two operator applications.  sigma, alpha, theta, phi
// and omega stay in device scalars between the launches; a quotient that is not finite is clamped to 0 where it is formed (as
// k_cg_update clamps its step length), so no vector receives inf or nan from finite input.
//
// Partial sums.  k_bicg_dots and k_bicg_full write TWO partials per workgroup.  part_slot(SLOT_NRM) has room for 2 * NB_MAX
// doubles and grid_lin launches up to 2 * ctx->nb workgroups, which k_cg_update fills exactly with ONE sum.  The choice here: all
// kernels of this file that reduce run on a grid of AT MOST ctx->nb (<= NB_MAX) workgroups (bicg_grid), the first sum's partials
// lie in part_slot(SLOT_NRM)[0 .. NB_MAX) and the second's in the NB_MAX doubles behind them; one k_reduce_partials launch with
// pstride = NB_MAX adds both in index order.  No atomics: the same call on the same state returns the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "krylov_steps.h"
#include "bicgstab.h"

using namespace kh;

namespace {

// the largest finite double: !(|x| <= DBL_MAX) is "inf or nan"
constexpr double BICG_DBL_MAX = 1.79769313486231570e308;

// p = r + beta * (p - omega * v).  4 vector passes: r, p, v read, p written.
__global__ __launch_bounds__(BS) void k_bicg_dir(int64_t n, const double* __restrict__ r, double* __restrict__ p,
                                                 const double* __restrict__ v, double beta, double omega) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        const double d = p[i] - omega * v[i];
        st_nt(p + i, r[i] + beta * d);
    }
}

// alpha = rho / sigma (sigma from device memory, clamped to 0 when the quotient is not finite), kept in sc[BICG_ALPHA] for
// k_bicg_full; s = r - alpha * v; one partial of <s, s> per workgroup.  3 vector passes: r, v read, s written.
__global__ __launch_bounds__(BS) void k_bicg_half(int64_t n, double rho, double* __restrict__ sc, const double* __restrict__ r,
                                                  const double* __restrict__ v, double* __restrict__ s,
                                                  double* __restrict__ part_out) {
    __shared__ double sm[8];
    const int64_t stride = (int64_t)gridDim.x * BS;
    double alpha = rho / sc[BICG_SIGMA];      // the same IEEE division the host does afterwards
    if (!(fabs(alpha) <= BICG_DBL_MAX)) alpha = 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc[BICG_ALPHA] = alpha;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        const double sv = r[i] - alpha * v[i];
        st_nt(s + i, sv);
        acc = fma(sv, sv, acc);
    }
    const double sum = block_sum(acc, sm);
    if (threadIdx.x == 0) part_out[blockIdx.x] = sum;
}

// omega = theta / phi (from device memory, clamped as alpha); y = (y + alpha * p) + omega * s; r = s - omega * t; two partials
// per workgroup, <r~, r> in part0 and <r, r> in part1.  7 vector passes: r~, p, s, t, y read, y, r written.
__global__ __launch_bounds__(BS) void k_bicg_full(int64_t n, const double* __restrict__ sc, const double* __restrict__ rt,
                                                  double* __restrict__ r, const double* __restrict__ p,
                                                  const double* __restrict__ s, const double* __restrict__ t,
                                                  double* __restrict__ y, double* __restrict__ part0,
                                                  double* __restrict__ part1) {
    __shared__ double sm0[4], sm1[4];
    const int64_t stride = (int64_t)gridDim.x * BS;
    const double alpha = sc[BICG_ALPHA];
    double omega = sc[BICG_THETA] / sc[BICG_PHI];
    if (!(fabs(omega) <= BICG_DBL_MAX)) omega = 0.0;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        const double sv = s[i];
        const double yv = y[i] + alpha * p[i];
        st_nt(y + i, yv + omega * sv);
        const double rv = sv - omega * t[i];
        st_nt(r + i, rv);
        a0 = fma(rt[i], rv, a0);
        a1 = fma(rv, rv, a1);
    }
    const double r0 = block_sum(a0, sm0);
    const double r1 = block_sum(a1, sm1);
    if (threadIdx.x == 0) {
        part0[blockIdx.x] = r0;
        part1[blockIdx.x] = r1;
    }
}

// the grid of every kernel here: grid_lin's, but never more than ctx->nb workgroups (two sums share SLOT_NRM's 2 * NB_MAX doubles)
int bicg_grid(kh_ctx ctx, int64_t n) { return std::min(grid_lin(ctx, n), ctx->nb); }

inline bool same_col(kh_vec A, int64_t a, kh_vec B, int64_t b) { return A == B && a == b; }

inline double* bicg_scal(kh_ctx ctx) { return ctx->scal + SC_TMP; }

int dir_launch(kh_ctx ctx, int64_t n, const double* r, double* p, const double* v, double beta, double omega) {
    hipLaunchKernelGGL(k_bicg_dir, dim3(bicg_grid(ctx, n)), dim3(BS), 0, ctx->stream, n, r, p, v, beta, omega);
    KH_HIP(hipGetLastError());
    return 0;
}

// sigma = <r~, v> into sc[BICG_SIGMA] (all-reduced), then k_bicg_half and ss into sc[BICG_SS].  fetch: ss is all-reduced and
// (sigma, ss) copied to out2 (one host synchronisation); otherwise ss waits for half2's all-reduce and nothing visits the host.
int half_launch(kh_ctx ctx, kh_vec RT, int64_t rtcol, const double* r, const double* v, double* s, double rho, bool fetch,
                double* out2) {
    const int64_t n = RT->n;
    double* sc = bicg_scal(ctx);
    KH_TRY(dot_panel_raw(ctx, RT, rtcol, 1, v, sc + BICG_SIGMA));
    if (kh_multi(ctx)) KH_TRY(comm_allreduce_dev(ctx, sc + BICG_SIGMA, 1));
    double* part = part_slot(ctx, SLOT_NRM);
    const int grid = bicg_grid(ctx, n);
    hipLaunchKernelGGL(k_bicg_half, dim3(grid), dim3(BS), 0, ctx->stream, n, rho, sc, r, v, s, part);
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(BS), 0, ctx->stream, part, grid, 0, sc + BICG_SS, 0);
    KH_HIP(hipGetLastError());
    if (!fetch) return 0;
    if (kh_multi(ctx)) KH_TRY(comm_allreduce_dev(ctx, sc + BICG_SS, 1));
    return fetch_scalars(ctx, sc + BICG_SIGMA, 2, out2);
}

// theta, phi (k_bicg_dots; theta_known: phi alone, theta lies in sc[BICG_THETA] complete), k_bicg_full, rho', rr.  ss_pending:
// the all-reduce of theta and phi takes the ss before them along (kh_bicgstab_step).  Nothing is fetched here.
int full_launch(kh_ctx ctx, int64_t n, const double* rt, double* r, const double* p, const double* s, const double* t, double* y,
                bool theta_known, bool ss_pending) {
    double* sc = bicg_scal(ctx);
    double* part = part_slot(ctx, SLOT_NRM);
    const int grid = bicg_grid(ctx, n);
    hipLaunchKernelGGL(k_bicg_dots, dim3(grid), dim3(BS), 0, ctx->stream, n, s, t, part, part + NB_MAX);
    if (theta_known)
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(BS), 0, ctx->stream, part + NB_MAX, grid, 0, sc + BICG_PHI, 0);
    else
        hipLaunchKernelGGL(k_reduce_partials, dim3(2), dim3(BS), 0, ctx->stream, part, grid, NB_MAX, sc + BICG_THETA, 0);
    KH_HIP(hipGetLastError());
    if (kh_multi(ctx)) {
        if (ss_pending) KH_TRY(comm_allreduce_dev(ctx, sc + BICG_SS, theta_known ? 1 : 3));       // ss, theta, phi are neighbours
        if (theta_known) KH_TRY(comm_allreduce_dev(ctx, sc + BICG_PHI, 1));
        else if (!ss_pending) KH_TRY(comm_allreduce_dev(ctx, sc + BICG_THETA, 2));
    }
    hipLaunchKernelGGL(k_bicg_full, dim3(grid), dim3(BS), 0, ctx->stream, n, sc, rt, r, p, s, t, y, part, part + NB_MAX);
    hipLaunchKernelGGL(k_reduce_partials, dim3(2), dim3(BS), 0, ctx->stream, part, grid, NB_MAX, sc + BICG_RHO, 0);
    KH_HIP(hipGetLastError());
    if (kh_multi(ctx)) KH_TRY(comm_allreduce_dev(ctx, sc + BICG_RHO, 2));
    return 0;
}

}  // namespace

extern "C" {

int kh_bicgstab_dir(kh_ctx ctx, kh_vec R, int64_t rcol, kh_vec P, int64_t pcol, kh_vec V, int64_t vcol, double beta,
                    double omega) {
    KH_ARG(ctx, "kh_bicgstab_dir: NULL");
    KH_TRY(check_vec(R, rcol, 1, "kh_bicgstab_dir(r)"));
    KH_TRY(check_vec(P, pcol, 1, "kh_bicgstab_dir(p)"));
    KH_TRY(check_vec(V, vcol, 1, "kh_bicgstab_dir(v)"));
    const int64_t n = R->n;
    KH_ARG(P->n == n && V->n == n, "kh_bicgstab_dir: length mismatch");
    KH_ARG(!same_col(P, pcol, R, rcol) && !same_col(P, pcol, V, vcol), "kh_bicgstab_dir: p (written) must be a column of its own");
    return dir_launch(ctx, n, R->col(rcol), P->col(pcol), V->col(vcol), beta, omega);
}

int kh_bicgstab_half(kh_ctx ctx, kh_vec RT, int64_t rtcol, kh_vec R, int64_t rcol, kh_vec V, int64_t vcol, kh_vec S,
                     int64_t scol, double rho, double* out) {
    KH_ARG(ctx && out, "kh_bicgstab_half: NULL");
    KH_TRY(check_vec(RT, rtcol, 1, "kh_bicgstab_half(rt)"));
    KH_TRY(check_vec(R, rcol, 1, "kh_bicgstab_half(r)"));
    KH_TRY(check_vec(V, vcol, 1, "kh_bicgstab_half(v)"));
    KH_TRY(check_vec(S, scol, 1, "kh_bicgstab_half(s)"));
    const int64_t n = R->n;
    KH_ARG(RT->n == n && V->n == n && S->n == n, "kh_bicgstab_half: length mismatch");
    KH_ARG(!same_col(S, scol, RT, rtcol) && !same_col(S, scol, R, rcol) && !same_col(S, scol, V, vcol),
           "kh_bicgstab_half: s (written) must be a column of its own");
    KH_TRY(half_launch(ctx, RT, rtcol, R->col(rcol), V->col(vcol), S->col(scol), rho, true, out));
    out[2] = (double)bicg_sanity_half(rho, out[0]);
    return 0;
}

int kh_bicgstab_full(kh_ctx ctx, kh_vec RT, int64_t rtcol, kh_vec R, int64_t rcol, kh_vec P, int64_t pcol, kh_vec S,
                     int64_t scol, kh_vec T, int64_t tcol, kh_vec YK, int64_t ycol, int theta_known, double* out) {
    KH_ARG(ctx && out, "kh_bicgstab_full: NULL");
    KH_TRY(check_vec(RT, rtcol, 1, "kh_bicgstab_full(rt)"));
    KH_TRY(check_vec(R, rcol, 1, "kh_bicgstab_full(r)"));
    KH_TRY(check_vec(P, pcol, 1, "kh_bicgstab_full(p)"));
    KH_TRY(check_vec(S, scol, 1, "kh_bicgstab_full(s)"));
    KH_TRY(check_vec(T, tcol, 1, "kh_bicgstab_full(t)"));
    KH_TRY(check_vec(YK, ycol, 1, "kh_bicgstab_full(yk)"));
    const int64_t n = R->n;
    KH_ARG(RT->n == n && P->n == n && S->n == n && T->n == n && YK->n == n, "kh_bicgstab_full: length mismatch");
    KH_ARG(!same_col(R, rcol, RT, rtcol) && !same_col(R, rcol, P, pcol) && !same_col(R, rcol, S, scol) &&
               !same_col(R, rcol, T, tcol) && !same_col(R, rcol, YK, ycol),
           "kh_bicgstab_full: r (written) must be a column of its own");
    KH_ARG(!same_col(YK, ycol, RT, rtcol) && !same_col(YK, ycol, P, pcol) && !same_col(YK, ycol, S, scol) &&
               !same_col(YK, ycol, T, tcol),
           "kh_bicgstab_full: yk (written) must be a column of its own");
    KH_TRY(full_launch(ctx, n, RT->col(rtcol), R->col(rcol), P->col(pcol), S->col(scol), T->col(tcol), YK->col(ycol),
                       theta_known != 0, false));
    KH_TRY(fetch_scalars(ctx, bicg_scal(ctx) + BICG_THETA, 4, out));
    out[4] = (double)bicg_sanity_full(out[0], out[1], out[2]);
    return 0;
}

int kh_bicgstab_step(kh_ctx ctx, kh_mat A, kh_vec RT, int64_t rtcol, kh_vec R, int64_t rcol, kh_vec P, int64_t pcol, kh_vec V,
                     int64_t vcol, kh_vec S, int64_t scol, kh_vec T, int64_t tcol, kh_vec YK, int64_t ycol, int first,
                     double beta, double omega_prev, double rho, double* out) {
    KH_ARG(ctx && A && out, "kh_bicgstab_step: NULL");
    RoctxScope range_(ctx, "kh_bicgstab_step");
    kh_vec blk[7] = {RT, R, P, V, S, T, YK};
    const int64_t col[7] = {rtcol, rcol, pcol, vcol, scol, tcol, ycol};
    static const char* const what[7] = {"kh_bicgstab_step(rt)", "kh_bicgstab_step(r)", "kh_bicgstab_step(p)", "kh_bicgstab_step(v)",
                                        "kh_bicgstab_step(s)", "kh_bicgstab_step(t)", "kh_bicgstab_step(yk)"};
    for (int i = 0; i < 7; ++i) KH_TRY(check_vec(blk[i], col[i], 1, what[i]));
    KH_ARG(A->kind <= KH_MAT_DIAG, "kh_bicgstab_step: real operator expected");
    const int64_t n = R->n;
    KH_ARG(A->n_rows == n && A->n_cols == n, "kh_bicgstab_step: length mismatch (operator)");
    for (int i = 0; i < 7; ++i) KH_ARG(blk[i]->n == n, "kh_bicgstab_step: length mismatch");
    // every column but r~ is written at some point of the iteration: the seven are pairwise distinct
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            KH_ARG(!same_col(blk[i], col[i], blk[j], col[j]), "kh_bicgstab_step: %s and %s are the same column", what[i], what[j]);
    double* r = R->col(rcol);
    double* p = P->col(pcol);
    double* v = V->col(vcol);
    double* s = S->col(scol);
    double* t = T->col(tcol);
    if (!first) KH_TRY(dir_launch(ctx, n, r, p, v, beta, omega_prev));
    KH_TRY(apply_one(ctx, A, p, v, EPI_NONE, nullptr, nullptr, 0));
    KH_TRY(half_launch(ctx, RT, rtcol, r, v, s, rho, false, nullptr));
    KH_TRY(apply_one(ctx, A, s, t, EPI_NONE, nullptr, nullptr, 0));
    KH_TRY(full_launch(ctx, n, RT->col(rtcol), r, p, s, t, YK->col(ycol), false, true));
    KH_TRY(fetch_scalars(ctx, bicg_scal(ctx) + BICG_SIGMA, 6, out));      // sigma, ss, theta, phi, rho', rr
    out[6] = (double)(bicg_sanity_half(rho, out[0]) | bicg_sanity_full(out[2], out[3], out[4]));
    out[7] = 0.0;
    ctx->n_bicgstab_steps += 1;
    return 0;
}

}  // extern "C"
