// GMRES polynomial preconditioner (kh_poly_*): y = p(A) x with p(A) ~ A^-1, where the roots of 1 - z p(z) are harmonic Ritz
// values of A that the host computed and ordered (krypy_amd/polyprecond.py) - what a solver applies per iteration through the
// Ml, Mr hooks of krypy/linsys.py (the reference has no counterpart, it calls the user's function on host arrays).  No spectral
// bounds, no symmetry: p is the product form of Loe & Morgan, real roots as linear factors, conjugate pairs as real quadratic
// ones.  Only operator applications and row-local updates: no factorisation, and - composed - the same on a communicator.
//
// The host hands over a table of steps (kind, c, a2, close, cl), ONE operator application each.  Per row, with s = (A in)_i and
// every multiply and add rounded on its own (kernels.h: poly_step):
//   LIN   (in = prod):  y_i = y_i + (c * in_i);                       out_i = in_i - (c * s)
//   QA    (in = prod):  t = (a2 * in_i) - s;   y_i = y_i + (c * t);   out_i = t
//   QB    (in = t):                                                   out_i = prod_i - (c * s)
//   SCALE (alone):      y_i = c * x_i
//   the first step reads x as prod and does not read y;  close: additionally y_i = y_i + (cl * out_i)
// x is never written.  prod ping-pongs between the scratch columns 0 and 1, t lives in column 2; `out` is always another column
// than `in` (the product reads neighbouring rows of `in`) and - in a QB step - than prod.
//
// Two ways to run a step:
//   fused     ONE launch: the SpMV with the step in its epilogue (kernels.h: EPI_POLY of k_spmv_dia for an operator with a
//             banded form, of k_spmv_stream otherwise; the step's record waits in device memory, written by k_poly_plan, so the
//             SpMV kernels keep their argument lists).  Vector traffic of a constant-coefficient stencil: LIN / QA read in, y,
//             write y, out = 32 N bytes; QB reads in, prod, writes out = 24 N.  Real CSR operators without a halo on a context
//             without a communicator (kh_ctx_set "poly_fused", default 1).
//   composed  kh_apply's launch into the column of `out`, then k_poly_update in place (56 N / 40 N).  Everything else: dense
//             operators, shards, a communicator.  The row sums are the same, so both ways give the same bits.
#include <algorithm>
#include <vector>

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

bool overlap(kh_vec a, int64_t acol, int64_t na, kh_vec b, int64_t bcol, int64_t nb) {
    return a == b && acol < bcol + nb && bcol < acol + na;
}

struct Step {
    int kind, close;
    double c, a2, cl;
};

Step step_of(const double* steps, int k) {
    Step s;
    s.kind = (int)steps[5 * k];
    s.c = steps[5 * k + 1];
    s.a2 = steps[5 * k + 2];
    s.close = steps[5 * k + 3] != 0.0 ? 1 : 0;
    s.cl = steps[5 * k + 4];
    return s;
}

int check_table(int nsteps, const double* steps) {
    for (int k = 0; k < nsteps; ++k) {
        const double kd = steps[5 * k];
        KH_ARG(kd == 0.0 || kd == 1.0 || kd == 2.0 || kd == 3.0, "kh_poly_apply: step %d has kind %g, 0 (LIN), 1 (QA), 2 (QB) or 3 (SCALE) expected",
               k, kd);
        const Step s = step_of(steps, k);
        KH_ARG(!(s.kind == POLY_QA && s.close), "kh_poly_apply: step %d closes on a QA step (a real root closes behind LIN or QB)", k);
        KH_ARG(!(s.kind == POLY_SCALE && (nsteps != 1 || s.close)), "kh_poly_apply: step %d is a SCALE step that does not stand alone", k);
        KH_ARG(!(s.kind == POLY_QB && (k == 0 || (int)steps[5 * (k - 1)] != POLY_QA)), "kh_poly_apply: step %d is a QB step not preceded by QA", k);
    }
    return 0;
}

void launch_update(kh_ctx ctx, int64_t n, const double* in, const double* prod, double* y, double* so, const Step& s, int flags) {
    hipLaunchKernelGGL(k_poly_update, dim3(grid_lin(ctx, n)), dim3(BS), 0, ctx->stream, n, in, prod, y, so, s.c, s.a2, s.cl, s.kind, flags);
    ctx->n_poly_update += 1;
}

// EPI_POLY finds its record (kernels.h: PolyArgs) in device memory behind `aux`
template <int ITEMS>
void launch_stream_poly(kh_ctx ctx, kh_mat A, const double* x, double* y, const double* rec) {
    const size_t lds = (size_t)A->tile * sizeof(double);
    if (ctx->spmv_win && A->win_cap > 0 && A->blkwin != nullptr) {
        // tile 4096 + a 4096-entry window is 64 KB: above what a kernel gets without asking (as launch_spmv_items)
        static bool attr_done = false;
        if (!attr_done) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_spmv_stream<EPI_POLY, ITEMS, true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)((4096 + 4096) * sizeof(double)));
            (void)hipGetLastError();
            attr_done = true;
        }
        hipLaunchKernelGGL((k_spmv_stream<EPI_POLY, ITEMS, true>), dim3(A->nblk), dim3(BS), lds + (size_t)A->win_cap * sizeof(double),
                           ctx->stream, A->indptr, A->indices, A->data, A->rowblk, A->nblk, A->tile, A->n_cols, x, A->ghost, y,
                           rec, A->part, 0x7fffffff, 0, 0, A->blkwin, A->win_cap);
        ctx->n_spmv_win += 1;
        return;
    }
    hipLaunchKernelGGL((k_spmv_stream<EPI_POLY, ITEMS>), dim3(A->nblk), dim3(BS), lds, ctx->stream, A->indptr, A->indices,
                       A->data, A->rowblk, A->nblk, A->tile, A->n_cols, x, A->ghost, y, rec, A->part, 0x7fffffff, 0, 0);
}

template <int ND, int RPT>
void launch_dia_poly_nd(kh_ctx ctx, kh_mat A, const DiaOffs& o, const double* x, double* y, const double* rec) {
    hipLaunchKernelGGL((k_spmv_dia<EPI_POLY, ND, RPT, false>), dim3(A->dia_nblk), dim3(BS), 0, ctx->stream, o, A->dia, A->dmask,
                       A->dia_ld, A->n_rows, A->dia_nblk, x, A->ghost, 0, 0, y, rec, A->part, 0x7fffffff, 0, 0, XhArgs());
}

template <int RPT>
void launch_dia_poly(kh_ctx ctx, kh_mat A, const DiaOffs& o, const double* x, double* y, const double* rec) {
    switch (A->dia_nd) {
        case 3: launch_dia_poly_nd<3, RPT>(ctx, A, o, x, y, rec); break;
        case 5: launch_dia_poly_nd<5, RPT>(ctx, A, o, x, y, rec); break;
        case 7: launch_dia_poly_nd<7, RPT>(ctx, A, o, x, y, rec); break;
        case 9: launch_dia_poly_nd<9, RPT>(ctx, A, o, x, y, rec); break;
        default: launch_dia_poly_nd<0, RPT>(ctx, A, o, x, y, rec); break;
    }
}

// out = step(in) in one launch; the same choice between the banded and the CSR-stream kernel as kh_apply makes
void launch_fused(kh_ctx ctx, kh_mat A, const double* in, double* out, const PolyArgs* record) {
    const double* rec = reinterpret_cast<const double*>(record);
    if (kh_banded(A) && ctx->spmv_dia && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && A->dia_nblk > 0) {
        const DiaOffs o = dia_offs(A);
        ctx->n_dia_mask += A->dmask != nullptr ? 1 : 0;
        if (A->dia_rpt == 4) launch_dia_poly<4>(ctx, A, o, in, out, rec);
        else if (A->dia_rpt == 2) launch_dia_poly<2>(ctx, A, o, in, out, rec);
        else launch_dia_poly<1>(ctx, A, o, in, out, rec);
    } else {
        switch (A->tile / BS) {      // as launch_spmv
            case 4: launch_stream_poly<4>(ctx, A, in, out, rec); break;
            case 16: launch_stream_poly<16>(ctx, A, in, out, rec); break;
            default: launch_stream_poly<8>(ctx, A, in, out, rec); break;
        }
    }
    ctx->n_poly_fused += 1;
}

// the device records of one application's fused steps (one table per context: the stream orders its writers and readers)
int ensure_table(kh_ctx ctx, int64_t steps) {
    if (steps <= ctx->poly_tab_cap) return 0;
    KH_HIP(hipStreamSynchronize(ctx->stream));
    (void)hipFree(ctx->poly_tab);
    ctx->poly_tab = nullptr;
    ctx->poly_tab_cap = 0;
    const int64_t cap = std::max<int64_t>(64, 2 * steps);
    KH_HIP(hipMalloc(&ctx->poly_tab, sizeof(PolyArgs) * cap));
    ctx->poly_tab_cap = cap;
    return 0;
}

bool fused_ok(kh_ctx ctx, kh_mat A) {
    return ctx->poly_fused && !kh_multi(ctx) && A->kind == KH_MAT_CSR && A->nblk > 0 && A->n_rows == A->n_cols &&
           (A->nrecv_prev + A->nrecv_next + A->nsend_prev + A->nsend_next) == 0;
}

// Where step k reads and writes: prod sits in scratch column p (x itself before the first step), t in column 2.
struct Route {
    int in;        // -1: x, else a scratch column
    int prod;      // QB: the column of prod (-1 otherwise)
    int out;       // the scratch column of s and of out
    int flags;
};

}  // namespace

extern "C" {

int kh_poly_update(kh_ctx ctx, kh_vec In, int64_t incol, kh_vec P, int64_t pcol, kh_vec Y, int64_t ycol, kh_vec SO, int64_t socol,
                   int kind, double c, double a2, double cl, int first, int close) {
    KH_ARG(ctx != nullptr, "kh_poly_update: NULL ctx");
    KH_ARG(In != nullptr, "kh_poly_update: NULL block (in)");
    KH_ARG(kind >= POLY_LIN && kind <= POLY_SCALE, "kh_poly_update: kind %d, 0 (LIN), 1 (QA), 2 (QB) or 3 (SCALE) expected", kind);
    KH_ARG(!(kind == POLY_QA && close), "kh_poly_update: close on a QA step");
    KH_ARG(!(kind == POLY_QB && first), "kh_poly_update: a QB step cannot be the first");
    KH_ARG(!(kind == POLY_SCALE && close), "kh_poly_update: close on a SCALE step");
    const int64_t n = In->n;
    KH_TRY(check_col(In, incol, 1, n, "kh_poly_update", "in"));
    KH_TRY(check_col(Y, ycol, 1, n, "kh_poly_update", "y"));
    KH_ARG(!overlap(In, incol, 1, Y, ycol, 1), "kh_poly_update: in, prod, y and s/out must be different columns");
    if (kind != POLY_SCALE) {
        KH_TRY(check_col(SO, socol, 1, n, "kh_poly_update", "s/out"));
        KH_ARG(!overlap(SO, socol, 1, Y, ycol, 1) && !overlap(SO, socol, 1, In, incol, 1),
               "kh_poly_update: in, prod, y and s/out must be different columns");
    }
    if (kind == POLY_QB) {
        KH_TRY(check_col(P, pcol, 1, n, "kh_poly_update", "prod"));
        KH_ARG(!overlap(P, pcol, 1, Y, ycol, 1) && !overlap(P, pcol, 1, SO, socol, 1) && !overlap(P, pcol, 1, In, incol, 1),
               "kh_poly_update: in, prod, y and s/out must be different columns");
    }
    chain_blk_touch(ctx, Y);
    if (kind != POLY_SCALE) chain_blk_touch(ctx, SO);
    if (n == 0) return 0;
    Step s;
    s.kind = kind;
    s.close = close ? 1 : 0;
    s.c = c;
    s.a2 = a2;
    s.cl = cl;
    launch_update(ctx, n, In->col(incol), kind == POLY_QB ? P->col(pcol) : nullptr, Y->col(ycol),
                  kind != POLY_SCALE ? SO->col(socol) : nullptr, s, (first ? POLY_FIRST : 0) | (close ? POLY_CLOSE : 0));
    KH_HIP(hipGetLastError());
    return 0;
}

int kh_poly_apply(kh_ctx ctx, kh_mat A, int nsteps, const double* steps, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol,
                  int64_t ncols, kh_vec S) {
    KH_ARG(nsteps >= 1, "kh_poly_apply: %d steps, at least 1 expected", nsteps);
    KH_ARG(ctx != nullptr && A != nullptr && steps != nullptr, "kh_poly_apply: NULL");
    KH_ARG(A->ctx == ctx, "kh_poly_apply: the operator belongs to another context");
    KH_ARG(A->kind != KH_MAT_DIAG && A->kind != KH_MAT_ZDIAG, "kh_poly_apply: A is a diagonal operator");
    KH_ARG(A->kind < KH_MAT_ZCSR, "kh_poly_apply: A is a complex operator (real operators on real blocks only)");
    const bool halo = A->kind == KH_MAT_CSR && (A->nrecv_prev + A->nrecv_next) > 0;
    const int64_t cols = halo ? A->n_cols - A->nrecv_prev - A->nrecv_next : A->n_cols;
    KH_ARG(A->n_rows == cols, "kh_poly_apply: A is %lld x %lld, a square operator expected", (long long)A->n_rows, (long long)cols);
    const int64_t n = A->n_rows;
    KH_TRY(check_col(X, xcol, ncols, n, "kh_poly_apply", "x"));
    KH_TRY(check_col(Y, ycol, ncols, n, "kh_poly_apply", "y"));
    KH_ARG(S != nullptr, "kh_poly_apply: NULL block (scratch)");
    KH_ARG(S->n == n, "kh_poly_apply(scratch): block of length %lld, expected %lld", (long long)S->n, (long long)n);
    KH_ARG(S->ncols >= 3, "kh_poly_apply: the scratch block has %lld columns, 3 needed", (long long)S->ncols);
    KH_ARG(!overlap(X, xcol, ncols, Y, ycol, ncols), "kh_poly_apply: x and y overlap (x is read after y is first written)");
    KH_ARG(S != X && S != Y, "kh_poly_apply: the scratch block overlaps x or y");
    KH_TRY(check_table(nsteps, steps));
    chain_blk_touch(ctx, Y);
    chain_blk_touch(ctx, S);
    const bool scale = (int)steps[0] == POLY_SCALE;
    const bool fused = !scale && fused_ok(ctx, A);
    if (fused) KH_TRY(ensure_table(ctx, nsteps));
    // the route through the scratch columns is the same for every column of x, fused or composed
    std::vector<Route> route((size_t)nsteps);
    {
        int p = -1;                    // where prod is: -1 x, else scratch column 0 / 1
        for (int k = 0; k < nsteps; ++k) {
            const Step s = step_of(steps, k);
            Route& r = route[(size_t)k];
            r.flags = (k == 0 ? POLY_FIRST : 0) | (s.close ? POLY_CLOSE : 0);
            r.prod = -1;
            const int other = p == 0 ? 1 : 0;
            if (s.kind == POLY_LIN) {
                r.in = p;
                r.out = other;
                p = other;
            } else if (s.kind == POLY_QA) {
                r.in = p;
                r.out = 2;
            } else if (s.kind == POLY_QB) {
                r.in = 2;
                r.prod = p;
                r.out = other;
                p = other;
            } else {
                r.in = -1;
                r.out = -1;
            }
        }
        // (a QB step whose prod is still x - the first pair - reads x row-locally as prod)
    }
    for (int64_t c = 0; c < ncols; ++c) {
        ctx->n_poly_apply += 1;
        if (n == 0) continue;
        const double* x = X->col(xcol + c);
        double* y = Y->col(ycol + c);
        auto src = [&](int col) -> const double* { return col < 0 ? x : S->col(col); };
        if (scale) {
            launch_update(ctx, n, x, nullptr, y, nullptr, step_of(steps, 0), POLY_FIRST);
            KH_HIP(hipGetLastError());
            continue;
        }
        if (fused) {
            PolyArgs* tab = static_cast<PolyArgs*>(ctx->poly_tab);
            for (int k0 = 0; k0 < nsteps; k0 += KH_POLY_PLAN) {
                PolyPlan plan;
                plan.k0 = k0;
                plan.count = std::min(KH_POLY_PLAN, nsteps - k0);
                for (int t = 0; t < KH_POLY_PLAN; ++t) {
                    PolyArgs& rec = plan.rec[t];
                    rec = PolyArgs();
                    if (t >= plan.count) continue;
                    const Step s = step_of(steps, k0 + t);
                    const Route& r = route[(size_t)(k0 + t)];
                    rec.y = y;
                    rec.prod = s.kind == POLY_QB ? src(r.prod) : nullptr;
                    rec.c = s.c;
                    rec.a2 = s.a2;
                    rec.cl = s.cl;
                    rec.kind = s.kind;
                    rec.flags = r.flags;
                }
                hipLaunchKernelGGL(k_poly_plan, dim3(1), dim3(BS), 0, ctx->stream, tab, plan);
            }
        }
        for (int k = 0; k < nsteps; ++k) {
            const Step s = step_of(steps, k);
            const Route& r = route[(size_t)k];
            if (fused) {
                launch_fused(ctx, A, src(r.in), S->col(r.out), static_cast<const PolyArgs*>(ctx->poly_tab) + k);
            } else {
                KH_TRY(kh_apply(ctx, A, r.in < 0 ? X : S, r.in < 0 ? xcol + c : r.in, S, r.out, 1));
                launch_update(ctx, n, src(r.in), s.kind == POLY_QB ? src(r.prod) : nullptr, y, S->col(r.out), s, r.flags);
            }
        }
        KH_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
