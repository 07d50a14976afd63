// IDR(s) with bi-orthogonalisation on the device: the fused vector kernels of a cycle and the C entry points above them (the
// header has the iteration and the contract, idrs.h the layout of the scalar block).  A cycle of s + 1 positions on A^ = Ml A Mr:
//
//   position k < s:  c from f and M (prologue) ;  v = r - sum c_i g_i ;  u_k = om v + sum c_i u_i    k_idr_dir    2 (s - k) + 2 passes
//                    t = A^ u_k ;  h = P^T t                                     apply_one + dot_panel_raw      s + 1 passes
//                    a, M[k:, k], beta, f[k+1:] from h, M, f (prologue) ;  g_k = t - sum a_i g_i ;
//                    u_k = u_k - sum a_i u_i ;  r = r - beta g_k ;  y = y + beta u_k ;  <r, r>       k_idr_orth   2 k + 8 passes (7 at k = 0)
//   position s:      t = A^ r ;  theta = <t, r> ;  phi = <t, t>                  apply_one + k_bicg_dots        2 passes
//                    om with the kappa correction (prologue) ;  y = y + om r ;  r = r - om t ;  <r, r>   k_idr_omega  5 passes
//                    f = P^T r                                                   dot_panel_raw                  s + 1 passes
//   every position:  rr, the step's record, the counter, the stop word                              k_idr_rr     (one workgroup)
//
// s = 4: 28 + 20 + 43 + 2 + 5 + 5 = 103 vector passes and 5 operator applications per cycle (KERNELS.md 4.28); the host is needed
// once per kh_idrs_run call.
//
// The operator product goes into the scratch column t at EVERY position and k_idr_orth writes g_k itself: the applications of
// a run are not gated by the stop word, and a product written straight into g_k would destroy the previous cycle's g_k, which
// k_idr_dir still reads when a stopped solve is continued.  This way nothing behind a stop changes P, G, U, r, y or a scalar
// that the iteration reads: dot_panel_raw writes sc[IDRS_H] (scratch; at position s k_idr_rr copies it to f), k_bicg_dots
// and k_reduce_partials write theta, phi and sc[IDRS_TMP], which only the launch directly behind them reads.
//
// What a launch stores and another workgroup of the SAME launch reads: nothing.  k_idr_dir stores c and the flags (reads f, M,
// om); k_idr_orth stores a, beta, column k of M from row k down, f[k+1:] and the flags (reads h, f_k, columns < k of M and
// the pivots M_ii, i < k); k_idr_omega stores om and the flags (reads theta, phi, rr); the flags word is read and written by
// thread 0 of workgroup 0 alone.  k_idr_rr is one workgroup and reads the stop word before its barrier, writes it after.
//
// Partial sums as in bicgstab.hip: grids of at most ctx->nb workgroups, partials in part_slot(SLOT_NRM), added in index order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "krylov_steps.h"
#include "bicgstab.h"
#include "idrs.h"

using namespace kh;

namespace {

constexpr double IDR_DBL_MAX = 1.79769313486231570e308;     // !(|x| <= DBL_MAX) is "inf or nan"
constexpr double IDR_KAPPA = 0.7;
constexpr int SM = IDRS_SMAX;

__device__ __forceinline__ bool idr_finite(double x) { return fabs(x) <= IDR_DBL_MAX; }
__device__ __forceinline__ double idr_quot(double a, double b) {
    const double q = a / b;
    return idr_finite(q) ? q : 0.0;
}
__device__ __forceinline__ void idr_raise(double* sc, int bits) { sc[IDRS_FLAGS] = (double)((int)sc[IDRS_FLAGS] | bits); }

// Position k, NC = s - k columns.  c_i = (f_i - sum_{j=k}^{i-1} M_ij c_j) / M_ii in every thread; v = r - sum c_i g_i in
// registers; u_k = om v + sum c_i u_i (i = k reads the old u_k).  g, u: column k of G and of U.
template <int NC>
__global__ __launch_bounds__(BS) void k_idr_dir(int64_t n, int k, double* sc, const double* __restrict__ r,
                                                const double* __restrict__ g, int64_t ldg, double* u, int64_t ldu) {
    if (sc[IDRS_STOP] != 0.0) return;
    const double* M = sc + IDRS_M + k * SM + k;
    double c[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        double acc = sc[IDRS_F + k + i];
#pragma unroll
        for (int j = 0; j < i; ++j) acc = acc - M[i * SM + j] * c[j];
        c[i] = idr_quot(acc, M[i * SM + i]);
    }
    const double om = sc[IDRS_OM];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NC; ++i) sc[IDRS_C + k + i] = c[i];
        if (!idr_finite(M[0]) || M[0] == 0.0) idr_raise(sc, KH_IDRS_PIVOT_ZERO);
    }
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t e = (int64_t)blockIdx.x * BS + threadIdx.x; e < n; e += stride) {
        double v = r[e];
#pragma unroll
        for (int i = 0; i < NC; ++i) v = v - c[i] * g[i * ldg + e];
        double w = om * v;
#pragma unroll
        for (int i = 0; i < NC; ++i) w = w + c[i] * u[i * ldu + e];
        st_nt(u + e, w);
    }
}

// Position K from the product t on.  a_i = (h_i - sum_{j<i} M_ij a_j) / M_ii, M_KK and beta = f_K / M_KK in every thread;
// thread 0 of workgroup 0 stores a, beta, M[K:, K] and f[K+1:].  g_K = t - sum a_i g_i ; u_K = u_K - sum a_i u_i ;
// r = r - beta g_K ; y = y + beta u_K ; one partial of <r, r> per workgroup.  G, U: column 0 of the blocks.
template <int K>
__global__ __launch_bounds__(BS) void k_idr_orth(int64_t n, int s, double* sc, double* __restrict__ r, double* __restrict__ y,
                                                 const double* __restrict__ t, double* G, int64_t ldg, double* U, int64_t ldu,
                                                 double* __restrict__ part_out) {
    __shared__ double sm[8];
    if (sc[IDRS_STOP] != 0.0) return;
    const double* M = sc + IDRS_M;
    const double* h = sc + IDRS_H;
    double a[K > 0 ? K : 1];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double acc = h[i];
#pragma unroll
        for (int j = 0; j < i; ++j) acc = acc - M[i * SM + j] * a[j];
        a[i] = idr_quot(acc, M[i * SM + i]);
    }
    double mkk = h[K];
#pragma unroll
    for (int j = 0; j < K; ++j) mkk = mkk - M[K * SM + j] * a[j];
    const double beta = idr_quot(sc[IDRS_F + K], mkk);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int bits = 0;
        if (!idr_finite(mkk) || mkk == 0.0) bits |= KH_IDRS_PIVOT_ZERO;
        for (int i = 0; i < s; ++i)
            if (!idr_finite(h[i])) bits |= KH_IDRS_NONFINITE;
        if (bits) idr_raise(sc, bits);
#pragma unroll
        for (int i = 0; i < K; ++i) sc[IDRS_A + i] = a[i];
        sc[IDRS_BETA] = beta;
        sc[IDRS_M + K * SM + K] = mkk;
        for (int i = K + 1; i < s; ++i) {
            double mik = h[i];
#pragma unroll
            for (int j = 0; j < K; ++j) mik = mik - M[i * SM + j] * a[j];
            sc[IDRS_M + i * SM + K] = mik;
            sc[IDRS_F + i] = sc[IDRS_F + i] - beta * mik;
        }
    }
    double* gk = G + K * ldg;
    double* uk = U + K * ldu;
    const int64_t stride = (int64_t)gridDim.x * BS;
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * BS + threadIdx.x; e < n; e += stride) {
        double gv = t[e], uv = uk[e];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            gv = gv - a[i] * G[i * ldg + e];
            uv = uv - a[i] * U[i * ldu + e];
        }
        st_nt(gk + e, gv);
        if (K > 0) st_nt(uk + e, uv);
        const double rv = r[e] - beta * gv;
        st_nt(r + e, rv);
        st_nt(y + e, y[e] + beta * uv);
        acc = fma(rv, rv, acc);
    }
    const double sum = block_sum(acc, sm);
    if (threadIdx.x == 0) part_out[blockIdx.x] = sum;
}

// Position s from t = A^ r on.  om = theta / phi, rho = theta / (sqrt(phi) sqrt(rr)), |rho| < kappa: om = (om kappa) / |rho|;
// y = y + om r ; r = r - om t ; one partial of <r, r> per workgroup.  5 vector passes.
__global__ __launch_bounds__(BS) void k_idr_omega(int64_t n, double* sc, double* __restrict__ r, const double* __restrict__ t,
                                                  double* __restrict__ y, double* __restrict__ part_out) {
    __shared__ double sm[8];
    if (sc[IDRS_STOP] != 0.0) return;
    const double theta = sc[IDRS_THETA], phi = sc[IDRS_PHI], rr = sc[IDRS_RR];
    double om = idr_quot(theta, phi);
    const double rho = theta / (sqrt(phi) * sqrt(rr));
    if (fabs(rho) < IDR_KAPPA) om = idr_quot(om * IDR_KAPPA, fabs(rho));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int bits = 0;
        if (!idr_finite(theta) || !idr_finite(phi)) bits |= KH_IDRS_NONFINITE;
        if (phi == 0.0) bits |= KH_IDRS_OMEGA_CLAMPED;
        if (om == 0.0 && rr > 0.0) bits |= KH_IDRS_OMEGA_ZERO;
        if (bits) idr_raise(sc, bits);
        sc[IDRS_OM] = om;
    }
    const int64_t stride = (int64_t)gridDim.x * BS;
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * BS + threadIdx.x; e < n; e += stride) {
        const double rv = r[e];
        st_nt(y + e, y[e] + om * rv);
        const double rn = rv - om * t[e];
        st_nt(r + e, rn);
        acc = fma(rn, rn, acc);
    }
    const double sum = block_sum(acc, sm);
    if (threadIdx.x == 0) part_out[blockIdx.x] = sum;
}

// One workgroup: rr = part[0] + ... + part[nb - 1] exactly as k_reduce_partials adds them; at position s the f that the block
// dot left in sc[IDRS_H] becomes f; the step's record, the counter, and the stop word (sqrt(rr) / bnorm <= tol, or a flag).
__global__ __launch_bounds__(BS) void k_idr_rr(const double* __restrict__ part, int nb, double* sc, int pos, int s, double bnorm,
                                               double tol) {
    __shared__ double sm[8];
    if (sc[IDRS_STOP] != 0.0) return;
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += BS) v += part[i];
    const double rr = block_sum(v, sm);
    if (threadIdx.x != 0) return;
    int bits = (int)sc[IDRS_FLAGS];
    if (!idr_finite(rr)) bits |= KH_IDRS_NONFINITE;
    double x1, x2;
    if (pos < s) {
        x1 = sc[IDRS_M + pos * SM + pos];
        x2 = sc[IDRS_F + pos];
    } else {
        x1 = sc[IDRS_THETA];
        x2 = sc[IDRS_PHI];
        for (int i = 0; i < s; ++i) {
            const double fi = sc[IDRS_H + i];
            if (!idr_finite(fi)) bits |= KH_IDRS_NONFINITE;
            sc[IDRS_F + i] = fi;
        }
    }
    const int idx = (int)sc[IDRS_COUNT];
    bool stop = bits != 0 || sqrt(rr) / bnorm <= tol;
    if (idx < IDRS_RUN_MAX) {
        double* rec = sc + IDRS_REC + 4 * idx;
        rec[0] = rr;
        rec[1] = x1;
        rec[2] = x2;
        rec[3] = (double)bits;
    }
    if (idx + 1 >= IDRS_RUN_MAX) stop = true;       // no room for another record: the caller fetches these first
    sc[IDRS_RR] = rr;
    sc[IDRS_FLAGS] = 0.0;
    sc[IDRS_COUNT] = (double)(idx + 1);
    if (stop) sc[IDRS_STOP] = 1.0;
}

// M = I, om = 1, everything else of the block 0 (f and rr follow from the block dots)
__global__ __launch_bounds__(BS) void k_idr_init(double* sc) {
    for (int i = threadIdx.x; i < IDRS_NSCAL; i += BS) {
        double v = 0.0;
        if (i < IDRS_F && i / SM == i % SM) v = 1.0;
        if (i == IDRS_OM) v = 1.0;
        sc[i] = v;
    }
}

// the grid of every kernel here: as bicg_grid, never more than ctx->nb workgroups
int idr_grid(kh_ctx ctx, int64_t n) { return std::min(grid_lin(ctx, n), ctx->nb); }

struct IdrState {
    int64_t n = 0;
    int s = 0;
    kh_vec P = nullptr;
    int64_t pcol = 0;
    double *G = nullptr, *U = nullptr, *r = nullptr, *y = nullptr, *t = nullptr, *sc = nullptr;
    int64_t ldg = 0, ldu = 0;
};

// lengths, real blocks (every kh_vec of this ABI is a real block; complex data arrives as views the host layer refuses),
// the s range, pairwise distinct columns
int idr_state(const char* who, kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R,
              int64_t rcol, kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, IdrState* st) {
    KH_ARG(ctx && SC, "%s: NULL", who);
    KH_ARG(s >= 1 && s <= IDRS_SMAX, "%s: s = %d is outside 1 .. %d", who, s, IDRS_SMAX);
    kh_vec blk[6] = {P, G, U, R, YK, T};
    const int64_t col[6] = {pcol, gcol, ucol, rcol, ycol, tcol};
    const int64_t cnt[6] = {s, s, s, 1, 1, 1};
    static const char* const what[6] = {"P", "G", "U", "r", "yk", "t"};
    char name[64];
    for (int i = 0; i < 6; ++i) {
        snprintf(name, sizeof(name), "%s(%s)", who, what[i]);
        KH_TRY(check_vec(blk[i], col[i], cnt[i], name));
    }
    const int64_t n = R->n;
    for (int i = 0; i < 6; ++i) KH_ARG(blk[i]->n == n, "%s: length mismatch (%s)", who, what[i]);
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            KH_ARG(blk[i] != blk[j] || col[i] + cnt[i] <= col[j] || col[j] + cnt[j] <= col[i], "%s: %s and %s share a column", who,
                   what[i], what[j]);
    KH_ARG(SC->ncols >= 1 && SC->n >= IDRS_NSCAL, "%s: the scalar block is short (%lld doubles, %d needed)", who,
           (long long)SC->n, (int)IDRS_NSCAL);
    for (int i = 0; i < 6; ++i) KH_ARG(blk[i] != SC, "%s: %s and the scalar block share a column", who, what[i]);
    st->n = n;
    st->s = s;
    st->P = P;
    st->pcol = pcol;
    st->G = G->col(gcol);
    st->ldg = G->ld;
    st->U = U->col(ucol);
    st->ldu = U->ld;
    st->r = R->col(rcol);
    st->y = YK->col(ycol);
    st->t = T->col(tcol);
    st->sc = SC->col(0);
    return 0;
}

int clear_stop(kh_ctx ctx, const IdrState& st) {
    KH_HIP(hipMemsetAsync(st.sc + IDRS_STOP, 0, 2 * sizeof(double), ctx->stream));       // the stop word and the counter
    return 0;
}

template <int NC>
void dir_launch_nc(kh_ctx ctx, const IdrState& st, int k) {
    hipLaunchKernelGGL(k_idr_dir<NC>, dim3(idr_grid(ctx, st.n)), dim3(BS), 0, ctx->stream, st.n, k, st.sc, (const double*)st.r,
                       (const double*)(st.G + k * st.ldg), st.ldg, st.U + k * st.ldu, st.ldu);
}

int dir_launch(kh_ctx ctx, const IdrState& st, int k) {
    switch (st.s - k) {
        case 1: dir_launch_nc<1>(ctx, st, k); break;
        case 2: dir_launch_nc<2>(ctx, st, k); break;
        case 3: dir_launch_nc<3>(ctx, st, k); break;
        case 4: dir_launch_nc<4>(ctx, st, k); break;
        case 5: dir_launch_nc<5>(ctx, st, k); break;
        case 6: dir_launch_nc<6>(ctx, st, k); break;
        case 7: dir_launch_nc<7>(ctx, st, k); break;
        default: dir_launch_nc<8>(ctx, st, k); break;
    }
    KH_HIP(hipGetLastError());
    return 0;
}

// rr from the partials of the step's vector kernel (all-reduced first on a context with a communicator), record, stop word
int rr_launch(kh_ctx ctx, const IdrState& st, int grid, int pos, double bnorm, double tol) {
    const double* part = part_slot(ctx, SLOT_NRM);
    if (kh_multi(ctx)) {
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(BS), 0, ctx->stream, part, grid, 0, st.sc + IDRS_TMP, 0);
        KH_HIP(hipGetLastError());
        KH_TRY(comm_allreduce_dev(ctx, st.sc + IDRS_TMP, 1));
        part = st.sc + IDRS_TMP;
        grid = 1;
    }
    hipLaunchKernelGGL(k_idr_rr, dim3(1), dim3(BS), 0, ctx->stream, part, grid, st.sc, pos, st.s, bnorm, tol);
    KH_HIP(hipGetLastError());
    return 0;
}

template <int K>
void orth_launch_k(kh_ctx ctx, const IdrState& st, int grid) {
    hipLaunchKernelGGL(k_idr_orth<K>, dim3(grid), dim3(BS), 0, ctx->stream, st.n, st.s, st.sc, st.r, st.y, (const double*)st.t,
                       st.G, st.ldg, st.U, st.ldu, part_slot(ctx, SLOT_NRM));
}

// h = P^T t, k_idr_orth, rr
int orth_launch(kh_ctx ctx, const IdrState& st, int k, double bnorm, double tol) {
    KH_TRY(dot_panel_raw(ctx, st.P, st.pcol, st.s, st.t, st.sc + IDRS_H));
    if (kh_multi(ctx)) KH_TRY(comm_allreduce_dev(ctx, st.sc + IDRS_H, st.s));
    const int grid = idr_grid(ctx, st.n);
    switch (k) {
        case 0: orth_launch_k<0>(ctx, st, grid); break;
        case 1: orth_launch_k<1>(ctx, st, grid); break;
        case 2: orth_launch_k<2>(ctx, st, grid); break;
        case 3: orth_launch_k<3>(ctx, st, grid); break;
        case 4: orth_launch_k<4>(ctx, st, grid); break;
        case 5: orth_launch_k<5>(ctx, st, grid); break;
        case 6: orth_launch_k<6>(ctx, st, grid); break;
        default: orth_launch_k<7>(ctx, st, grid); break;
    }
    KH_HIP(hipGetLastError());
    return rr_launch(ctx, st, grid, k, bnorm, tol);
}

// theta, phi (k_bicg_dots), k_idr_omega, f = P^T r into sc[IDRS_H], rr (k_idr_rr takes f over)
int omega_launch(kh_ctx ctx, const IdrState& st, double bnorm, double tol) {
    double* part = part_slot(ctx, SLOT_NRM);
    const int grid = idr_grid(ctx, st.n);
    hipLaunchKernelGGL(k_bicg_dots, dim3(grid), dim3(BS), 0, ctx->stream, st.n, (const double*)st.r, (const double*)st.t, part,
                       part + NB_MAX);
    hipLaunchKernelGGL(k_reduce_partials, dim3(2), dim3(BS), 0, ctx->stream, part, grid, NB_MAX, st.sc + IDRS_THETA, 0);
    KH_HIP(hipGetLastError());
    if (kh_multi(ctx)) KH_TRY(comm_allreduce_dev(ctx, st.sc + IDRS_THETA, 2));
    hipLaunchKernelGGL(k_idr_omega, dim3(grid), dim3(BS), 0, ctx->stream, st.n, st.sc, st.r, (const double*)st.t, st.y, part);
    KH_HIP(hipGetLastError());
    KH_TRY(dot_panel_raw(ctx, st.P, st.pcol, st.s, st.r, st.sc + IDRS_H));
    if (kh_multi(ctx)) KH_TRY(comm_allreduce_dev(ctx, st.sc + IDRS_H, st.s));
    return rr_launch(ctx, st, grid, st.s, bnorm, tol);
}

}  // namespace

extern "C" {

int kh_idrs_init(kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R, int64_t rcol,
                 kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, double* rr_out) {
    IdrState st;
    KH_TRY(idr_state("kh_idrs_init", ctx, P, pcol, G, gcol, U, ucol, R, rcol, YK, ycol, T, tcol, SC, s, &st));
    KH_ARG(rr_out, "kh_idrs_init: NULL");
    hipLaunchKernelGGL(k_idr_init, dim3(1), dim3(BS), 0, ctx->stream, st.sc);
    KH_HIP(hipGetLastError());
    KH_TRY(dot_panel_raw(ctx, P, pcol, s, st.r, st.sc + IDRS_F));
    KH_TRY(dot_panel_raw(ctx, R, rcol, 1, st.r, st.sc + IDRS_RR));
    if (kh_multi(ctx)) {
        KH_TRY(comm_allreduce_dev(ctx, st.sc + IDRS_F, s));
        KH_TRY(comm_allreduce_dev(ctx, st.sc + IDRS_RR, 1));
    }
    return fetch_scalars(ctx, st.sc + IDRS_RR, 1, rr_out);
}

int kh_idrs_dir(kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R, int64_t rcol,
                kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, int k) {
    IdrState st;
    KH_TRY(idr_state("kh_idrs_dir", ctx, P, pcol, G, gcol, U, ucol, R, rcol, YK, ycol, T, tcol, SC, s, &st));
    KH_ARG(k >= 0 && k < s, "kh_idrs_dir: position k = %d is outside 0 .. s - 1 = %d", k, s - 1);
    KH_TRY(clear_stop(ctx, st));
    return dir_launch(ctx, st, k);
}

int kh_idrs_orth(kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R, int64_t rcol,
                 kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, int k, double bnorm, double tol,
                 double* rec) {
    IdrState st;
    KH_TRY(idr_state("kh_idrs_orth", ctx, P, pcol, G, gcol, U, ucol, R, rcol, YK, ycol, T, tcol, SC, s, &st));
    KH_ARG(rec, "kh_idrs_orth: NULL");
    KH_ARG(k >= 0 && k < s, "kh_idrs_orth: position k = %d is outside 0 .. s - 1 = %d", k, s - 1);
    KH_TRY(orth_launch(ctx, st, k, bnorm, tol));
    return fetch_scalars(ctx, st.sc + IDRS_REC, 4, rec);
}

int kh_idrs_omega(kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R, int64_t rcol,
                  kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, double bnorm, double tol, double* rec) {
    IdrState st;
    KH_TRY(idr_state("kh_idrs_omega", ctx, P, pcol, G, gcol, U, ucol, R, rcol, YK, ycol, T, tcol, SC, s, &st));
    KH_ARG(rec, "kh_idrs_omega: NULL");
    KH_TRY(clear_stop(ctx, st));
    KH_TRY(omega_launch(ctx, st, bnorm, tol));
    return fetch_scalars(ctx, st.sc + IDRS_REC, 4, rec);
}

int kh_idrs_run(kh_ctx ctx, kh_mat A, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R,
                int64_t rcol, kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, int pos, int nsteps,
                double bnorm, double tol, double* out) {
    IdrState st;
    KH_TRY(idr_state("kh_idrs_run", ctx, P, pcol, G, gcol, U, ucol, R, rcol, YK, ycol, T, tcol, SC, s, &st));
    KH_ARG(A && out, "kh_idrs_run: NULL");
    RoctxScope range_(ctx, "kh_idrs_run");
    KH_ARG(A->kind <= KH_MAT_DIAG, "kh_idrs_run: real operator expected");
    KH_ARG(A->n_rows == st.n && A->n_cols == st.n, "kh_idrs_run: length mismatch (operator)");
    KH_ARG(pos >= 0 && pos <= s, "kh_idrs_run: position %d is outside 0 .. s = %d", pos, s);
    KH_ARG(nsteps >= 1 && nsteps <= IDRS_RUN_MAX, "kh_idrs_run: nsteps = %d is outside 1 .. %d", nsteps, IDRS_RUN_MAX);
    KH_TRY(clear_stop(ctx, st));
    for (int i = 0; i < nsteps; ++i) {
        const int k = (pos + i) % (s + 1);
        if (k < s) {
            KH_TRY(dir_launch(ctx, st, k));
            KH_TRY(apply_one(ctx, A, st.U + k * st.ldu, st.t, EPI_NONE, nullptr, nullptr, 0));
            KH_TRY(orth_launch(ctx, st, k, bnorm, tol));
        } else {
            KH_TRY(apply_one(ctx, A, st.r, st.t, EPI_NONE, nullptr, nullptr, 0));
            KH_TRY(omega_launch(ctx, st, bnorm, tol));
        }
    }
    KH_TRY(fetch_scalars(ctx, st.sc + IDRS_COUNT, 1 + 4 * nsteps, out));
    ctx->n_idrs_steps += (int64_t)out[0];
    return 0;
}

}  // extern "C"
