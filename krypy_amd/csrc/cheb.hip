// Chebyshev polynomial preconditioner (kh_cheb_*): z = p(A) r as m steps of the Chebyshev iteration for A z = r from z = 0 -
// what a solver applies per iteration through the M, Ml, Mr hooks of krypy/linsys.py (the reference has no counterpart, it
// calls the user's function on host arrays).  Only operator applications and row-local updates: no factorisation, no wait on
// another workgroup, and - composed - the same on a communicator.
//
// Per row, every multiply and add rounded on its own (coefficients (a_k, b_k) from the host, include/krylov_hip.h):
//   step 0:        t = r_i;              [t = t * dinv_i;]  d_i = b_0 * t;                   z_i = d_i
//   step k >= 1:   t = r_i - (A z)_i;    [t = t * dinv_i;]  d_i = (a_k * d_i) + (b_k * t);   z_i = z_i + d_i
//
// Two ways to run a step k >= 1:
//   fused     ONE launch: the SpMV with the step in its epilogue (kernels.h: EPI_CHEB of k_spmv_dia for an operator with a
//             banded form, of k_spmv_stream otherwise; the step's pointers and coefficients wait in a device record that step
//             0's launch wrote, so the SpMV kernels keep their argument lists).  Vector traffic of a constant-coefficient stencil: read z, r, d,
//             write d, z' = 40 N bytes ([+ 8 N for dinv]) against 72 N composed.  Real CSR operators without a halo on a
//             context without a communicator (kh_ctx_set "cheb_fused", default 1).
//   composed  kh_apply's launch into a scratch column, then k_cheb_update.  Everything else: dense and complex operators,
//             shards, a communicator.  The row sums are the same, so both ways give the same bits.
#include <algorithm>

#include "kernels.h"
#include "krylov_steps.h"

using namespace kh;

namespace {

int check_col(kh_vec v, int64_t col, int64_t ncols, int64_t n, const char* fn, const char* what) {
    KH_ARG(v != nullptr, "%s: NULL block (%s)", fn, what);
    KH_ARG(col >= 0 && ncols >= 0 && col + ncols <= v->ncols, "%s(%s): columns [%lld, %lld) out of range (ncols=%lld)", fn, what,
           (long long)col, (long long)(col + ncols), (long long)v->ncols);
    KH_ARG(v->n == n, "%s(%s): block of length %lld, expected %lld", fn, what, (long long)v->n, (long long)n);
    return 0;
}

int check_dinv(kh_mat Dinv, int64_t n, const char* fn) {
    if (Dinv == nullptr) return 0;
    KH_ARG(Dinv->kind == KH_MAT_DIAG, "%s: Dinv is not a real diagonal operator", fn);
    KH_ARG(Dinv->n_rows == n, "%s: Dinv has length %lld, the blocks %lld", fn, (long long)Dinv->n_rows, (long long)n);
    return 0;
}

bool overlap(kh_vec a, int64_t acol, int64_t na, kh_vec b, int64_t bcol, int64_t nb) {
    return a == b && acol < bcol + nb && bcol < acol + na;
}

void launch_update(kh_ctx ctx, int64_t n, const double* az, const double* r, const double* dinv, double* d, const double* zin,
                   double* zout, double a, double b) {
    hipLaunchKernelGGL(k_cheb_update, dim3(grid_lin(ctx, n)), dim3(BS), 0, ctx->stream, n, az, r, dinv, d, zin, zout, a, b);
    ctx->n_cheb_update += 1;
}

// EPI_CHEB finds its record (kernels.h: ChebArgs) in device memory behind `aux`
template <int ITEMS>
void launch_stream_cheb(kh_ctx ctx, kh_mat A, const double* x, double* y, const double* rec) {
    const size_t lds = (size_t)A->tile * sizeof(double);
    if (ctx->spmv_win && A->win_cap > 0 && A->blkwin != nullptr) {
        // tile 4096 + a 4096-entry window is 64 KB: above what a kernel gets without asking (as launch_spmv_items)
        static bool attr_done = false;
        if (!attr_done) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_spmv_stream<EPI_CHEB, ITEMS, true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)((4096 + 4096) * sizeof(double)));
            (void)hipGetLastError();
            attr_done = true;
        }
        hipLaunchKernelGGL((k_spmv_stream<EPI_CHEB, ITEMS, true>), dim3(A->nblk), dim3(BS), lds + (size_t)A->win_cap * sizeof(double),
                           ctx->stream, A->indptr, A->indices, A->data, A->rowblk, A->nblk, A->tile, A->n_cols, x, A->ghost, y,
                           rec, A->part, 0x7fffffff, 0, 0, A->blkwin, A->win_cap);
        ctx->n_spmv_win += 1;
        return;
    }
    hipLaunchKernelGGL((k_spmv_stream<EPI_CHEB, ITEMS>), dim3(A->nblk), dim3(BS), lds, ctx->stream, A->indptr, A->indices,
                       A->data, A->rowblk, A->nblk, A->tile, A->n_cols, x, A->ghost, y, rec, A->part, 0x7fffffff, 0, 0);
}

template <int ND, int RPT>
void launch_dia_cheb_nd(kh_ctx ctx, kh_mat A, const DiaOffs& o, const double* x, double* y, const double* rec) {
    hipLaunchKernelGGL((k_spmv_dia<EPI_CHEB, ND, RPT, false>), dim3(A->dia_nblk), dim3(BS), 0, ctx->stream, o, A->dia, A->dmask,
                       A->dia_ld, A->n_rows, A->dia_nblk, x, A->ghost, 0, 0, y, rec, A->part, 0x7fffffff, 0, 0, XhArgs());
}

template <int RPT>
void launch_dia_cheb(kh_ctx ctx, kh_mat A, const DiaOffs& o, const double* x, double* y, const double* rec) {
    switch (A->dia_nd) {
        case 3: launch_dia_cheb_nd<3, RPT>(ctx, A, o, x, y, rec); break;
        case 5: launch_dia_cheb_nd<5, RPT>(ctx, A, o, x, y, rec); break;
        case 7: launch_dia_cheb_nd<7, RPT>(ctx, A, o, x, y, rec); break;
        case 9: launch_dia_cheb_nd<9, RPT>(ctx, A, o, x, y, rec); break;
        default: launch_dia_cheb_nd<0, RPT>(ctx, A, o, x, y, rec); break;
    }
}

// z_out = z_in + d' in one launch; the same choice between the banded and the CSR-stream kernel as kh_apply makes
void launch_fused(kh_ctx ctx, kh_mat A, const double* zin, double* zout, const ChebArgs* record) {
    const double* rec = reinterpret_cast<const double*>(record);
    if (kh_banded(A) && ctx->spmv_dia && (reinterpret_cast<uintptr_t>(zout) & 15) == 0 && A->dia_nblk > 0) {
        const DiaOffs o = dia_offs(A);
        ctx->n_dia_mask += A->dmask != nullptr ? 1 : 0;
        if (A->dia_rpt == 4) launch_dia_cheb<4>(ctx, A, o, zin, zout, rec);
        else if (A->dia_rpt == 2) launch_dia_cheb<2>(ctx, A, o, zin, zout, rec);
        else launch_dia_cheb<1>(ctx, A, o, zin, zout, rec);
    } else {
        switch (A->tile / BS) {      // as launch_spmv
            case 4: launch_stream_cheb<4>(ctx, A, zin, zout, rec); break;
            case 16: launch_stream_cheb<16>(ctx, A, zin, zout, rec); break;
            default: launch_stream_cheb<8>(ctx, A, zin, zout, rec); break;
        }
    }
    ctx->n_cheb_fused += 1;
}

// the device records of one application's m - 1 fused steps (one table per context: the stream orders its writers and readers)
int ensure_table(kh_ctx ctx, int64_t steps) {
    if (steps <= ctx->cheb_tab_cap) return 0;
    KH_HIP(hipStreamSynchronize(ctx->stream));
    (void)hipFree(ctx->cheb_tab);
    ctx->cheb_tab = nullptr;
    ctx->cheb_tab_cap = 0;
    const int64_t cap = std::max<int64_t>(64, 2 * steps);
    KH_HIP(hipMalloc(&ctx->cheb_tab, sizeof(ChebArgs) * cap));
    ctx->cheb_tab_cap = cap;
    return 0;
}

ChebPlan plan_chunk(const double* r, double* d, const double* dinv, const double* coef, int m, int k0) {
    ChebPlan p;
    p.r = r;
    p.d = d;
    p.dinv = dinv;
    p.k0 = k0;                                          // record k0 + t belongs to step k0 + t + 1
    p.count = std::max(0, std::min(KH_CHEB_PLAN, m - 1 - k0));
    for (int t = 0; t < KH_CHEB_PLAN; ++t) {
        p.ab[2 * t] = t < p.count ? coef[2 * (k0 + t + 1)] : 0.0;
        p.ab[2 * t + 1] = t < p.count ? coef[2 * (k0 + t + 1) + 1] : 0.0;
    }
    return p;
}

bool fused_ok(kh_ctx ctx, kh_mat A) {
    return ctx->cheb_fused && !kh_multi(ctx) && A->kind == KH_MAT_CSR && A->nblk > 0 && A->n_rows == A->n_cols &&
           (A->nrecv_prev + A->nrecv_next + A->nsend_prev + A->nsend_next) == 0;
}

}  // namespace

extern "C" {

int kh_cheb_update(kh_ctx ctx, kh_vec AZ, int64_t azcol, kh_vec R, int64_t rcol, kh_mat Dinv, kh_vec D, int64_t dcol, kh_vec Zin,
                   int64_t zincol, kh_vec Zout, int64_t zoutcol, double a, double b, int first) {
    KH_ARG(ctx != nullptr, "kh_cheb_update: NULL ctx");
    KH_ARG(R != nullptr, "kh_cheb_update: NULL block (r)");
    const int64_t n = R->n;
    KH_TRY(check_col(R, rcol, 1, n, "kh_cheb_update", "r"));
    KH_TRY(check_col(D, dcol, 1, n, "kh_cheb_update", "d"));
    KH_TRY(check_col(Zout, zoutcol, 1, n, "kh_cheb_update", "z_out"));
    KH_TRY(check_dinv(Dinv, n, "kh_cheb_update"));
    KH_ARG(!overlap(R, rcol, 1, D, dcol, 1) && !overlap(R, rcol, 1, Zout, zoutcol, 1) && !overlap(D, dcol, 1, Zout, zoutcol, 1),
           "kh_cheb_update: r, d and z_out must be three different columns");
    if (!first) {
        KH_TRY(check_col(AZ, azcol, 1, n, "kh_cheb_update", "Az"));
        KH_TRY(check_col(Zin, zincol, 1, n, "kh_cheb_update", "z_in"));
        KH_ARG(!overlap(AZ, azcol, 1, D, dcol, 1) && !overlap(AZ, azcol, 1, Zout, zoutcol, 1) && !overlap(Zin, zincol, 1, D, dcol, 1),
               "kh_cheb_update: Az must differ from d and z_out, z_in from d");
    }
    chain_blk_touch(ctx, D);
    chain_blk_touch(ctx, Zout);
    if (n == 0) return 0;
    launch_update(ctx, n, first ? nullptr : AZ->col(azcol), R->col(rcol), Dinv ? Dinv->diag : nullptr, D->col(dcol),
                  first ? nullptr : Zin->col(zincol), Zout->col(zoutcol), a, b);
    KH_HIP(hipGetLastError());
    return 0;
}

int kh_cheb_apply(kh_ctx ctx, kh_mat A, kh_mat Dinv, int m, const double* coef, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol,
                  int64_t ncols, kh_vec S) {
    KH_ARG(ctx != nullptr && A != nullptr && coef != nullptr, "kh_cheb_apply: NULL");
    KH_ARG(A->ctx == ctx, "kh_cheb_apply: the operator belongs to another context");
    KH_ARG(m >= 1, "kh_cheb_apply: degree %d < 1", m);
    KH_ARG(A->kind != KH_MAT_DIAG && A->kind != KH_MAT_ZDIAG, "kh_cheb_apply: A is a diagonal operator");
    const bool cplx = A->kind >= KH_MAT_ZCSR;
    const bool halo = A->kind == KH_MAT_CSR && (A->nrecv_prev + A->nrecv_next) > 0;
    const int64_t cols = halo ? A->n_cols - A->nrecv_prev - A->nrecv_next : A->n_cols;
    KH_ARG(A->n_rows == cols, "kh_cheb_apply: A is %lld x %lld, a square operator expected", (long long)A->n_rows, (long long)cols);
    const int64_t n = cplx ? 2 * A->n_rows : A->n_rows;      // complex blocks are (re, im) views of length 2 N
    KH_TRY(check_col(X, xcol, ncols, n, "kh_cheb_apply", "x"));
    KH_TRY(check_col(Y, ycol, ncols, n, "kh_cheb_apply", "y"));
    KH_TRY(check_dinv(Dinv, n, "kh_cheb_apply"));
    const bool fused = fused_ok(ctx, A);
    const int64_t need = fused ? 2 : 3;
    KH_ARG(S != nullptr, "kh_cheb_apply: NULL block (scratch)");
    KH_ARG(S->n == n, "kh_cheb_apply(scratch): block of length %lld, expected %lld", (long long)S->n, (long long)n);
    KH_ARG(S->ncols >= need, "kh_cheb_apply: the scratch block has %lld columns, %lld needed", (long long)S->ncols, (long long)need);
    KH_ARG(!overlap(X, xcol, ncols, Y, ycol, ncols), "kh_cheb_apply: x and y overlap (r is read in every step)");
    KH_ARG(S != X && S != Y, "kh_cheb_apply: the scratch block overlaps x or y");
    chain_blk_touch(ctx, Y);
    chain_blk_touch(ctx, S);
    if (fused) KH_TRY(ensure_table(ctx, m - 1));
    const double* dinv = Dinv ? Dinv->diag : nullptr;
    double* d = S->col(0);
    for (int64_t c = 0; c < ncols; ++c) {
        ctx->n_cheb_apply += 1;
        if (n == 0) continue;
        const double* r = X->col(xcol + c);
        // z after step k lives in Y when m - 1 - k is even, else in the scratch: the last step lands in Y
        auto in_y = [&](int k) { return ((m - 1 - k) & 1) == 0; };
        auto zbuf = [&](int k) { return in_y(k) ? Y->col(ycol + c) : S->col(1); };
        if (fused) {
            // step 0 writes the records of the fused steps on its way (k_cheb_first); more than KH_CHEB_PLAN of them: k_cheb_plan
            ChebArgs* tab = static_cast<ChebArgs*>(ctx->cheb_tab);
            hipLaunchKernelGGL(k_cheb_first, dim3(grid_lin(ctx, n)), dim3(BS), 0, ctx->stream, n, zbuf(0), coef[1], tab,
                               plan_chunk(r, d, dinv, coef, m, 0));
            ctx->n_cheb_update += 1;
            for (int k0 = KH_CHEB_PLAN; k0 < m - 1; k0 += KH_CHEB_PLAN)
                hipLaunchKernelGGL(k_cheb_plan, dim3(1), dim3(BS), 0, ctx->stream, tab, plan_chunk(r, d, dinv, coef, m, k0));
        } else {
            launch_update(ctx, n, nullptr, r, dinv, d, nullptr, zbuf(0), 0.0, coef[1]);
        }
        for (int k = 1; k < m; ++k) {
            const double* zin = zbuf(k - 1);
            double* zout = zbuf(k);
            if (fused) {
                launch_fused(ctx, A, zin, zout, static_cast<const ChebArgs*>(ctx->cheb_tab) + (k - 1));
            } else {
                KH_TRY(kh_apply(ctx, A, in_y(k - 1) ? Y : S, in_y(k - 1) ? ycol + c : 1, S, 2, 1));
                launch_update(ctx, n, S->col(2), r, dinv, d, zin, zout, coef[2 * k], coef[2 * k + 1]);
            }
        }
        KH_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
