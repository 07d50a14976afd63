// Device kernels of libkrylov_hip: CDNA4 (gfx950, wave64) only.
//
// Every kernel on this path is HBM-bandwidth bound: the design rules are
//  * 16-byte (double2) coalesced loads/stores of column-contiguous vectors,
//  * a fixed streaming grid (ctx->nb workgroups of 256 threads = 4 wave64) with grid-stride
//    loops, so every reduction has a fixed, timing-independent summation order,
//  * reductions = per-thread serial sum -> wave64 shuffle tree -> 4 wave sums through LDS ->
//    one partial per workgroup; the consumer kernel re-sums the partials in a fixed order in its
//    prologue (no float atomics, no extra launch on the dependent MGS chain),
//  * compiled with -ffp-contract=off: `w - alpha*p` rounds twice exactly like NumPy's
//    `Av -= alpha * V[:, [j]]`; fused multiply-adds are used only where written as fma().
#pragma once
#include <type_traits>

#include "kh_internal.h"
#include "xr_dev.h"

namespace kh {

// ------------------------------------------------------------------------------------------
// deterministic workgroup reductions (256 threads = 4 wave64)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// result valid in thread 0 only; sm must hold >= 4 doubles; ends with no barrier pending
__device__ __forceinline__ double block_sum(double v, double* sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) sm[wid] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    return r;
}

// every thread of the workgroup gets the fixed-order sum of part[0..nb)
__device__ __forceinline__ double bcast_sum_partials(const double* __restrict__ part, int nb,
                                                     double* sm) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += BS) v += part[i];
    double r = block_sum(v, sm);
    if (threadIdx.x == 0) sm[4] = r;
    __syncthreads();
    r = sm[4];
    __syncthreads();
    return r;
}

// 16-byte non-temporal load (streams that are used once: keep them out of the way of what is reused)
typedef double v2f64_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ld_nt2(const double2* p) {
    const v2f64_t v = __builtin_nontemporal_load(reinterpret_cast<const v2f64_t*>(p));
    double2 r;
    r.x = v.x;
    r.y = v.y;
    return r;
}

// Non-temporal stores for streams nobody reads before the kernel ends (the next basis vector, the updated iterate, the
// product of an SpMV): with plain stores the lines sit in the XCD's L2 until its write-back policy gets to them, in the
// way of the streams still being read; MINRES + Jacobi at N = 10^7 3820 -> 4040 it/s on one box from the four stores
// of the Lanczos kernel's last pass alone.
__device__ __forceinline__ void st_nt2(double2* p, double2 v) {
    v2f64_t t;
    t.x = v.x;
    t.y = v.y;
    __builtin_nontemporal_store(t, reinterpret_cast<v2f64_t*>(p));
}
__device__ __forceinline__ void st_nt(double* p, double v) { __builtin_nontemporal_store(v, p); }

// where a kernel takes the coefficient of its axpy from
enum { A_NONE = 0, A_PART = 1, A_SCAL = 2, A_ARG = 3 };
// what a kernel reduces after the axpy
enum { T_NONE = 0, T_DOT = 1, T_NRM = 2, T_NRM_DIAG = 3 };

// ------------------------------------------------------------------------------------------
// The Gram-Schmidt link kernel.  One launch = `w -= alpha * p` fused with the NEXT reduction:
//   T_DOT      partial <vnext, w>            (the next MGS coefficient)
//   T_NRM      partial <w, w>                (H[k+1,k] after the last coefficient)
//   T_NRM_DIAG mw = d.*w stored, partial <w, mw>   (Jacobi-preconditioned Arnoldi/Lanczos)
// alpha is the fixed-order sum of the previous launch's partials (A_PART), a device scalar
// (A_SCAL, multi-GPU after the all-reduce / after the SpMV-fused dot) or an argument (A_ARG,
// the Lanczos `H[k,k-1]` term).  Workgroup 0 accumulates alpha into *hslot (H[j,k] += alpha).
// Reference: utils.py:1012-1034.
// ------------------------------------------------------------------------------------------
template <int ASRC, int TAIL>
__global__ __launch_bounds__(BS) void k_gs_link(int64_t n, const double* __restrict__ p,
                                                const double* __restrict__ vnext,
                                                double* __restrict__ w,
                                                const double* __restrict__ dg,
                                                double* __restrict__ mw,
                                                const double* __restrict__ part_in, int nb_in,
                                                const double* __restrict__ scal_in,
                                                double alpha_arg, double* __restrict__ part_out,
                                                double* __restrict__ hslot) {
    __shared__ double sm[8];
    double alpha = 0.0;
    if (ASRC == A_PART) alpha = bcast_sum_partials(part_in, nb_in, sm);
    if (ASRC == A_SCAL) alpha = scal_in[0];
    if (ASRC == A_ARG) alpha = alpha_arg;
    if (ASRC != A_NONE && hslot != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
        *hslot += alpha;

    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * BS;
    const double2* __restrict__ p2 = reinterpret_cast<const double2*>(p);
    const double2* __restrict__ v2 = reinterpret_cast<const double2*>(vnext);
    const double2* __restrict__ d2 = reinterpret_cast<const double2*>(dg);
    double2* __restrict__ w2 = reinterpret_cast<double2*>(w);
    double2* __restrict__ mw2 = reinterpret_cast<double2*>(mw);
    double acc = 0.0;
#pragma unroll 2
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n2; i += stride) {
        double2 wv = w2[i];
        if (ASRC != A_NONE) {
            const double2 pv = p2[i];
            wv.x = wv.x - alpha * pv.x;
            wv.y = wv.y - alpha * pv.y;
            st_nt2(w2 + i, wv);
        }
        if (TAIL == T_DOT) {
            const double2 vv = v2[i];
            acc = fma(vv.x, wv.x, acc);
            acc = fma(vv.y, wv.y, acc);
        } else if (TAIL == T_NRM) {
            acc = fma(wv.x, wv.x, acc);
            acc = fma(wv.y, wv.y, acc);
        } else if (TAIL == T_NRM_DIAG) {
            const double2 dv = d2[i];
            double2 m;
            m.x = dv.x * wv.x;
            m.y = dv.y * wv.y;
            st_nt2(mw2 + i, m);
            acc = fma(wv.x, m.x, acc);
            acc = fma(wv.y, m.y, acc);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd tail element
        const int64_t i = n - 1;
        double wv = w[i];
        if (ASRC != A_NONE) {
            wv = wv - alpha * p[i];
            w[i] = wv;
        }
        if (TAIL == T_DOT) acc = fma(vnext[i], wv, acc);
        if (TAIL == T_NRM) acc = fma(wv, wv, acc);
        if (TAIL == T_NRM_DIAG) {
            const double m = dg[i] * wv;
            mw[i] = m;
            acc = fma(wv, m, acc);
        }
    }
    if (TAIL != T_NONE) {
        const double r = block_sum(acc, sm);
        if (threadIdx.x == 0) part_out[blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------------------------------
// Normalise-and-store: h = sqrt(|sum of partials|) (or a device scalar), then
//   vnext = (mw | w) / h,  pnext = w / h      (true division, utils.py:1041-1045)
// ------------------------------------------------------------------------------------------
template <int HSRC>
__global__ __launch_bounds__(BS) void k_scale_store(int64_t n, const double* __restrict__ w,
                                                    const double* __restrict__ mw,
                                                    double* __restrict__ vnext,
                                                    double* __restrict__ pnext,
                                                    const double* __restrict__ part_in, int nb_in,
                                                    const double* __restrict__ scal_in,
                                                    double* __restrict__ hslot,
                                                    const double* hcol = nullptr, int hcount = 0,
                                                    double* hpin = nullptr) {
    __shared__ double sm[8];
    double h2 = (HSRC == A_PART) ? bcast_sum_partials(part_in, nb_in, sm) : scal_in[0];
    const double h = sqrt(fabs(h2));
    if (hslot != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *hslot = h;
    if (hpin != nullptr && blockIdx.x == 0) {
        // last kernel of an Arnoldi step: workgroup 0 puts the finished H column (hcount doubles,
        // *hslot among them) straight into pinned host memory - no device-to-host copy behind it
        __syncthreads();
        for (int i = threadIdx.x; i < hcount; i += BS)
            hpin[i] = __hip_atomic_load(hcol + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * BS;
    const double2* __restrict__ w2 = reinterpret_cast<const double2*>(w);
    const double2* __restrict__ m2 = reinterpret_cast<const double2*>(mw);
    double2* __restrict__ v2 = reinterpret_cast<double2*>(vnext);
    double2* __restrict__ p2 = reinterpret_cast<double2*>(pnext);
#pragma unroll 2
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n2; i += stride) {
        const double2 wv = w2[i];
        double2 o;
        o.x = wv.x / h;
        o.y = wv.y / h;
        if (mw != nullptr) {
            st_nt2(p2 + i, o);
            const double2 mv = m2[i];
            o.x = mv.x / h;
            o.y = mv.y / h;
        }
        st_nt2(v2 + i, o);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        if (mw != nullptr) {
            pnext[i] = w[i] / h;
            vnext[i] = mw[i] / h;
        } else {
            vnext[i] = w[i] / h;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Panel kernels (tall-skinny V^T w and w -= V h), C columns per launch.
// ------------------------------------------------------------------------------------------
struct ColPtrs {
    const double* c[MAXC];
};

// part_out[c * pstride + workgroup] = partial <V_c, w>
template <int C>
__global__ __launch_bounds__(BS) void k_multidot(int64_t n, ColPtrs cols,
                                                 const double* __restrict__ w,
                                                 double* __restrict__ part_out, int pstride) {
    __shared__ double sm[8];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * BS;
    const double2* __restrict__ w2 = reinterpret_cast<const double2*>(w);
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n2; i += stride) {
        const double2 wv = w2[i];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double2 vv = ld_nt2(reinterpret_cast<const double2*>(cols.c[c]) + i);   // column: used once
            acc[c] = fma(vv.x, wv.x, acc[c]);
            acc[c] = fma(vv.y, wv.y, acc[c]);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double wv = w[n - 1];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = fma(cols.c[c][n - 1], wv, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double r = block_sum(acc[c], sm);
        if (threadIdx.x == 0) part_out[(int64_t)c * pstride + blockIdx.x] = r;
        __syncthreads();
    }
}

// out[c] (op)= fixed-order sum of part[c*pstride + 0..nb); one workgroup per column.
// mode 0: out = s, 1: out += s, 2: out = sqrt(|s|)
static __global__ __launch_bounds__(BS) void k_reduce_partials(const double* __restrict__ part, int nb,
                                                        int pstride, double* __restrict__ out,
                                                        int mode) {
    __shared__ double sm[8];
    const double* p = part + (int64_t)blockIdx.x * pstride;
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += BS) v += p[i];
    const double r = block_sum(v, sm);
    if (threadIdx.x == 0) {
        if (mode == 0) out[blockIdx.x] = r;
        if (mode == 1) out[blockIdx.x] += r;
        if (mode == 2) out[blockIdx.x] = sqrt(fabs(r));
    }
}

// w = beta*w - sum_c coef[c] * V_c  applied left to right (multiply, then subtract), optionally
// followed by the partial <w,w> (TAIL == T_NRM) or the Jacobi variant (T_NRM_DIAG).
// BETA: 1 -> keep w, 0 -> start from zero (w is not read), 2 -> runtime beta.
template <int C, int TAIL, int BETA>
__global__ __launch_bounds__(BS) void k_multiaxpy(int64_t n, ColPtrs cols,
                                                  const double* __restrict__ coef, double sign,
                                                  double beta, double* __restrict__ w,
                                                  const double* __restrict__ dg,
                                                  double* __restrict__ mw,
                                                  double* __restrict__ part_out) {
    __shared__ double sm[8];
    double h[C];
#pragma unroll
    for (int c = 0; c < C; ++c) h[c] = sign * coef[c];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * BS;
    double2* __restrict__ w2 = reinterpret_cast<double2*>(w);
    const double2* __restrict__ d2 = reinterpret_cast<const double2*>(dg);
    double2* __restrict__ mw2 = reinterpret_cast<double2*>(mw);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n2; i += stride) {
        double2 wv;
        if (BETA == 0) {
            wv.x = 0.0;
            wv.y = 0.0;
        } else {
            wv = w2[i];
            if (BETA == 2) {
                wv.x = beta * wv.x;
                wv.y = beta * wv.y;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double2 vv = ld_nt2(reinterpret_cast<const double2*>(cols.c[c]) + i);   // column: used once
            wv.x = wv.x - h[c] * vv.x;
            wv.y = wv.y - h[c] * vv.y;
        }
        st_nt2(w2 + i, wv);
        if (TAIL == T_NRM) {
            acc = fma(wv.x, wv.x, acc);
            acc = fma(wv.y, wv.y, acc);
        } else if (TAIL == T_NRM_DIAG) {
            const double2 dv = d2[i];
            double2 m;
            m.x = dv.x * wv.x;
            m.y = dv.y * wv.y;
            st_nt2(mw2 + i, m);
            acc = fma(wv.x, m.x, acc);
            acc = fma(wv.y, m.y, acc);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        double wv = (BETA == 0) ? 0.0 : (BETA == 2 ? beta * w[i] : w[i]);
#pragma unroll
        for (int c = 0; c < C; ++c) wv = wv - h[c] * cols.c[c][i];
        w[i] = wv;
        if (TAIL == T_NRM) acc = fma(wv, wv, acc);
        if (TAIL == T_NRM_DIAG) {
            const double m = dg[i] * wv;
            mw[i] = m;
            acc = fma(wv, m, acc);
        }
    }
    if (TAIL != T_NONE) {
        const double r = block_sum(acc, sm);
        if (threadIdx.x == 0) part_out[blockIdx.x] = r;
    }
}

// z = alpha*x + beta*y  (numpy order: (alpha*x) + (beta*y); alpha==1 / beta==1 skip the multiply)
static __global__ __launch_bounds__(BS) void k_waxpby(int64_t n, double* z, double alpha,
                                               const double* x, double beta,
                                               const double* y) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        const double a = (alpha == 1.0) ? x[i] : alpha * x[i];
        if (beta == 0.0) {
            st_nt(z + i, a);
        } else {
            const double b = (beta == 1.0) ? y[i] : beta * y[i];
            st_nt(z + i, a + b);
        }
    }
}

// z and x may be the same column (utils.py divides a reflector, a basis column and the columns of a QR factor in place): no
// __restrict__ here.  Element i is read once and written once by the same lane (tests/test_gpu_panel.py holds the in-place form).
static __global__ __launch_bounds__(BS) void k_vdiv(int64_t n, double* z, const double* x, double s) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) st_nt(z + i, x[i] / s);
}

static __global__ __launch_bounds__(BS) void k_diag_apply(int64_t n, const double* __restrict__ d,
                                                   const double* __restrict__ x,
                                                   double* __restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) st_nt(y + i, d[i] * x[i]);
}

// ------------------------------------------------------------------------------------------
// MINRES vector recurrences (linsys.py:844-846), one pass:
//   z = (v - r0*w0 - r1*w1)/r2 ;  w0 <- z (the slot that held W0 becomes the new W1) ; yk += y0*z
// ------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(BS) void k_minres_update(int64_t n, const double* __restrict__ v,
                                                      double* __restrict__ w0,
                                                      const double* __restrict__ w1, double r0,
                                                      double r1, double r2, double y0,
                                                      double* __restrict__ yk) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        const double z = ((v[i] - r0 * w0[i]) - r1 * w1[i]) / r2;
        st_nt(w0 + i, z);
        st_nt(yk + i, yk[i] + y0 * z);
    }
}

// ------------------------------------------------------------------------------------------
// CG vector recurrences (linsys.py:655-665), one pass:
//   yk += alpha*p ; r -= alpha*Ap ; z = d.*r (or r) ; partial <r, z>
// ------------------------------------------------------------------------------------------
template <bool DIAG>
__global__ __launch_bounds__(BS) void k_cg_update(int64_t n, double alpha,
                                                  const double* __restrict__ p,
                                                  const double* __restrict__ ap,
                                                  double* __restrict__ yk, double* __restrict__ r,
                                                  const double* __restrict__ dg,
                                                  double* __restrict__ z,
                                                  double* __restrict__ part_out,
                                                  const double* __restrict__ pap = nullptr) {
    __shared__ double sm[8];
    const int64_t stride = (int64_t)gridDim.x * BS;
    // kh_cg_step: `alpha` carries rho and the step length is rho / <p, Ap> with the inner product
    // still on the device (same IEEE division the host would do)
    if (pap != nullptr) {
        alpha = alpha / pap[0];
        if (!(fabs(alpha) <= 1.79769313486231570e308)) alpha = 0.0;   // not finite: leave yk and r as they are, the caller's sanity word tells the host (kh_cg_step)
    }
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        st_nt(yk + i, yk[i] + alpha * p[i]);
        const double rv = r[i] - alpha * ap[i];
        st_nt(r + i, rv);
        double zv = rv;
        if (DIAG) {
            zv = dg[i] * rv;
            st_nt(z + i, zv);
        }
        acc = fma(rv, zv, acc);
    }
    const double s = block_sum(acc, sm);
    if (threadIdx.x == 0) part_out[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------
// CSR SpMV, "CSR-stream": a workgroup owns a run of consecutive rows whose nnz fit the LDS
// tile.  It streams `data`/`indices` fully coalesced, gathers x (stencil locality -> L2), parks
// the products a_ij*x_j in LDS, then one lane per row adds that row's products left to right.
// Separate multiply and add in storage order == scipy's csr_matvec bit for bit.
// A row longer than the tile gets a workgroup of its own (tree reduction, not bit-ordered).
// Epilogues: EPI_DOT  partial <v0, y>  (first MGS coefficient, saves one pass over w)
//            EPI_RES  y = b - A x and partial <y, y>  (explicit residual)
// blockIdx -> row-block mapping is XCD-aware: XCD x (workgroups b with b%8==x, each with a
// private 4 MiB L2) walks a contiguous range of row blocks, so the x[i +- nx] neighbours of a
// stencil row are L2 hits instead of cross-XCD refetches.
// ------------------------------------------------------------------------------------------
//            EPI_CHEB one step k >= 1 of the Chebyshev iteration (cheb.hip), row-local behind the row sum s = (A z)_i:
//                     t = r_i - s; [t = t * dinv_i;] d_i = (a * d_i) + (b * t); y_i = z_i + d_i   (x = z, every operation
//                     rounded on its own).  No reduction (part_out is not touched), no halo.
//            EPI_POLY one step of the GMRES polynomial preconditioner (poly.hip), row-local behind the row sum s = (A in)_i
//                     (x = in, y = out; the formulas stand at PolyArgs).  No reduction, no halo.
enum { EPI_NONE = 0, EPI_DOT = 1, EPI_RES = 2, EPI_CHEB = 3, EPI_POLY = 4 };

// What EPI_CHEB needs beyond the SpMV's own arguments (x = z_in, y = z_out).  The record lives in DEVICE memory and the kernel
// finds it behind `aux` (one uniform 40-byte load): the argument lists of k_spmv_stream / k_spmv_dia - and with them every
// instantiation of the other epilogues - stay what they were.  k_cheb_first / k_cheb_plan write one record per step.
struct ChebArgs {
    const double* r;      // the right-hand side of the iteration (read in every step)
    double* d;            // the direction, updated in place (row-local)
    const double* dinv;   // optional diagonal scaling (nullptr: none)
    double a, b;          // this step's pair of coefficients
};

__device__ __forceinline__ ChebArgs cheb_args(const double* aux) { return *reinterpret_cast<const ChebArgs*>(aux); }

// one row of the step: returns z_out_i, stores d_i (read by the next launch, not by this one: non-temporal)
__device__ __forceinline__ double cheb_row(const ChebArgs& ch, int64_t i, double zin, double s) {
    double t = ch.r[i] - s;
    if (ch.dinv != nullptr) t = t * ch.dinv[i];
    const double d = (ch.a * ch.d[i]) + (ch.b * t);
    st_nt(ch.d + i, d);
    return zin + d;
}

// ... and an aligned pair of neighbouring rows with 16-byte accesses
__device__ __forceinline__ double2 cheb_row2(const ChebArgs& ch, int64_t i, double2 zin, double2 s) {
    const double2 rv = ld_nt2(reinterpret_cast<const double2*>(ch.r + i));
    const double2 dv = ld_nt2(reinterpret_cast<const double2*>(ch.d + i));
    double t0 = rv.x - s.x, t1 = rv.y - s.y;
    if (ch.dinv != nullptr) {
        const double2 sv = ld_nt2(reinterpret_cast<const double2*>(ch.dinv + i));
        t0 = t0 * sv.x;
        t1 = t1 * sv.y;
    }
    const double2 d = make_double2((ch.a * dv.x) + (ch.b * t0), (ch.a * dv.y) + (ch.b * t1));
    st_nt2(reinterpret_cast<double2*>(ch.d + i), d);
    return make_double2(zin.x + d.x, zin.y + d.y);
}

// One step of the Chebyshev iteration for A z = r (cheb.hip), the row-local part alone:
//   az == nullptr (step 0):  t = r_i;          [t = t * dinv_i;]  d_i = b * t;                   z_out_i = d_i
//   otherwise:               t = r_i - az_i;   [t = t * dinv_i;]  d_i = (a * d_i) + (b * t);     z_out_i = z_in_i + d_i
// every multiply and add rounded on its own.  Step 0 reads neither d nor z_in.  z_in may be z_out (row-local).
__device__ __forceinline__ void cheb_update_rows(int64_t n, const double* __restrict__ az, const double* __restrict__ r,
                                                 const double* __restrict__ dinv, double* __restrict__ d, const double* z_in,
                                                 double* z_out, double a, double b) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        if (az == nullptr) {
            double t = r[i];
            if (dinv != nullptr) t = t * dinv[i];
            const double dv = b * t;
            st_nt(d + i, dv);
            st_nt(z_out + i, dv);
        } else {
            double t = r[i] - az[i];
            if (dinv != nullptr) t = t * dinv[i];
            const double dv = (a * d[i]) + (b * t);
            const double zv = z_in[i] + dv;
            st_nt(d + i, dv);
            st_nt(z_out + i, zv);
        }
    }
}

static __global__ __launch_bounds__(BS) void k_cheb_update(int64_t n, const double* __restrict__ az,
                                                    const double* __restrict__ r,
                                                    const double* __restrict__ dinv, double* __restrict__ d,
                                                    const double* z_in, double* z_out, double a, double b) {
    cheb_update_rows(n, az, r, dinv, d, z_in, z_out, a, b);
}

// The records of the fused steps (EPI_CHEB reads them from device memory): tab[k0 + t] = (r, d, dinv, ab[2 t], ab[2 t + 1]).
constexpr int KH_CHEB_PLAN = 16;      // records one launch writes
struct ChebPlan {
    const double* r;
    double* d;
    const double* dinv;
    int k0, count;
    double ab[2 * KH_CHEB_PLAN];
};

__device__ __forceinline__ void cheb_plan_write(ChebArgs* __restrict__ tab, const ChebPlan& p) {
    if (blockIdx.x == 0 && (int)threadIdx.x < p.count) {
        ChebArgs rec;
        rec.r = p.r;
        rec.d = p.d;
        rec.dinv = p.dinv;
        rec.a = p.ab[2 * threadIdx.x];
        rec.b = p.ab[2 * threadIdx.x + 1];
        tab[p.k0 + threadIdx.x] = rec;
    }
}

// step 0 of a fused application, and the records of its first KH_CHEB_PLAN fused steps on the way (b0: step 0's coefficient)
static __global__ __launch_bounds__(BS) void k_cheb_first(int64_t n, double* __restrict__ z_out, double b0,
                                                   ChebArgs* __restrict__ tab, ChebPlan p) {
    cheb_plan_write(tab, p);
    cheb_update_rows(n, nullptr, p.r, p.dinv, p.d, nullptr, z_out, 0.0, b0);
}

// ... further records (more than KH_CHEB_PLAN + 1 steps)
static __global__ __launch_bounds__(BS) void k_cheb_plan(ChebArgs* __restrict__ tab, ChebPlan p) { cheb_plan_write(tab, p); }

// ------------------------------------------------------------------------------------------
// GMRES polynomial preconditioner (poly.hip): y = p(A) x as a product of linear and quadratic factors, one operator
// application per step.  One step, per row, with s = (A in)_i and every multiply and add rounded on its own:
//   LIN   (in = prod):  y_i = y_i + (c * in_i);                         out_i = in_i - (c * s)
//   QA    (in = prod):  t = (a2 * in_i) - s;   y_i = y_i + (c * t);     out_i = t
//   QB    (in = t):                                                     out_i = prod_i - (c * s)
//   SCALE (no product): y_i = c * in_i
//   first:  y_i = (c * ...) without reading y;   close:  additionally y_i = y_i + (cl * out_i)
// What EPI_POLY needs beyond the SpMV's own arguments (x = in, y = out): a record in DEVICE memory behind `aux`, as ChebArgs.
// ------------------------------------------------------------------------------------------
enum { POLY_LIN = 0, POLY_QA = 1, POLY_QB = 2, POLY_SCALE = 3 };
enum { POLY_FIRST = 1, POLY_CLOSE = 2 };
struct PolyArgs {
    double* y;             // the result, accumulated over the steps
    const double* prod;    // QB: the running product (another column than in and out)
    double c, a2, cl;
    int kind, flags;
};

__device__ __forceinline__ PolyArgs poly_args(const double* aux) { return *reinterpret_cast<const PolyArgs*>(aux); }

// the arithmetic of one row: returns out_i; yv is y_i on entry (unused when first) and on exit, *ywrite whether it changed
__device__ __forceinline__ double poly_step(int kind, int flags, double c, double a2, double cl, double in, double pv, double s,
                                            double& yv, bool& ywrite) {
    const bool first = (flags & POLY_FIRST) != 0;
    double out;
    ywrite = true;
    if (kind == POLY_LIN) {
        const double u = c * in;
        yv = first ? u : yv + u;
        out = in - (c * s);
    } else if (kind == POLY_QA) {
        const double t = (a2 * in) - s;
        const double u = c * t;
        yv = first ? u : yv + u;
        out = t;
    } else {
        out = pv - (c * s);
        ywrite = false;
    }
    if (flags & POLY_CLOSE) {
        yv = yv + (cl * out);
        ywrite = true;
    }
    return out;
}

// one row of the step: returns out_i, stores y_i (read by the next launch, not by this one: non-temporal)
__device__ __forceinline__ double poly_row(const PolyArgs& pa, int64_t i, double in, double s) {
    const bool ready = pa.kind == POLY_QB ? (pa.flags & POLY_CLOSE) != 0 : (pa.flags & POLY_FIRST) == 0;
    double yv = ready ? pa.y[i] : 0.0;
    const double pv = pa.kind == POLY_QB ? pa.prod[i] : 0.0;
    bool yw;
    const double out = poly_step(pa.kind, pa.flags, pa.c, pa.a2, pa.cl, in, pv, s, yv, yw);
    if (yw) st_nt(pa.y + i, yv);
    return out;
}

// ... and an aligned pair of neighbouring rows with 16-byte accesses
__device__ __forceinline__ double2 poly_row2(const PolyArgs& pa, int64_t i, double2 in, double2 s) {
    const bool ready = pa.kind == POLY_QB ? (pa.flags & POLY_CLOSE) != 0 : (pa.flags & POLY_FIRST) == 0;
    double2 yv = make_double2(0.0, 0.0), pv = make_double2(0.0, 0.0);
    if (ready) yv = ld_nt2(reinterpret_cast<const double2*>(pa.y + i));
    if (pa.kind == POLY_QB) pv = ld_nt2(reinterpret_cast<const double2*>(pa.prod + i));
    bool yw;
    double2 out;
    out.x = poly_step(pa.kind, pa.flags, pa.c, pa.a2, pa.cl, in.x, pv.x, s.x, yv.x, yw);
    out.y = poly_step(pa.kind, pa.flags, pa.c, pa.a2, pa.cl, in.y, pv.y, s.y, yv.y, yw);
    if (yw) st_nt2(reinterpret_cast<double2*>(pa.y + i), yv);
    return out;
}

// The composed step: so[i] holds s = (A in)_i on entry and out_i on exit (row-local, in place); SCALE reads no s.
static __global__ __launch_bounds__(BS) void k_poly_update(int64_t n, const double* __restrict__ in,
                                                    const double* __restrict__ prod, double* __restrict__ y, double* so,
                                                    double c, double a2, double cl, int kind, int flags) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        if (kind == POLY_SCALE) {
            st_nt(y + i, c * in[i]);
            continue;
        }
        const bool ready = kind == POLY_QB ? (flags & POLY_CLOSE) != 0 : (flags & POLY_FIRST) == 0;
        double yv = ready ? y[i] : 0.0;
        const double pv = kind == POLY_QB ? prod[i] : 0.0;
        bool yw;
        const double out = poly_step(kind, flags, c, a2, cl, in[i], pv, so[i], yv, yw);
        if (yw) st_nt(y + i, yv);
        st_nt(so + i, out);
    }
}

// The records of the fused steps, written by ONE workgroup: tab[k0 + t] = rec[t], t < count.
constexpr int KH_POLY_PLAN = 16;      // records one launch writes
struct PolyPlan {
    PolyArgs rec[KH_POLY_PLAN];
    int k0, count;
};

static __global__ __launch_bounds__(BS) void k_poly_plan(PolyArgs* __restrict__ tab, PolyPlan p) {
    if (blockIdx.x == 0 && (int)threadIdx.x < p.count) tab[p.k0 + threadIdx.x] = p.rec[threadIdx.x];
}

__device__ __forceinline__ int xcd_remap(int b, int nblk) {
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = b & 7, idx = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// the block number that xcd_remap sends to logical block lb
__device__ __forceinline__ int xcd_unmap(int lb, int nblk) {
    const int q = nblk >> 3, r = nblk & 7;
    const int head = r * (q + 1);
    const int xcd = lb < head ? lb / (q + 1) : r + (lb - head) / (q > 0 ? q : 1);
    const int idx = lb < head ? lb % (q + 1) : (lb - head) % (q > 0 ? q : 1);
    return idx * 8 + xcd;
}

// WIN: the x entries a row block touches lie within `span` columns from `cmin` (blkwin, found at upload); where the span fits
// the LDS window the workgroup loads x[cmin .. cmin + span) ONCE, coalesced, and gathers from LDS.  A gather from global memory
// fills a 128-byte line for 8 bytes of x - on a matrix with entries at random places of a band that is ten times the bytes of
// the matrix itself between L2 and the compute units (273 us as is, 95 us without the gather).  Same products in
// the same order: the same bits.
// (Round 6 tried three things on this kernel - ONE table of (first row, first entry) pairs instead of rowblk[bid] -> indptr[r0],
// indptr[r1]; every lane's indptr[r], indptr[r + 1] requested with the stream loads instead of behind the barrier; the index /
// value streams in aligned runs of four entries per lane - all bit-identical, all SLOWER on the stencil matrix: 146 us against
// 137-138 for this form on the same boxes (EXPERIMENTS.md).  This is round 5's kernel.)
template <int EPI, int ITEMS, bool WIN = false>
__global__ __launch_bounds__(BS) void k_spmv_stream(const int32_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ indices,
                                                    const double* __restrict__ data,
                                                    const int32_t* __restrict__ rowblk, int nblk,
                                                    int tile, int64_t nloc,
                                                    const double* __restrict__ x,
                                                    const double* __restrict__ ghost,
                                                    double* __restrict__ y,
                                                    const double* __restrict__ aux,
                                                    double* __restrict__ part_out,
                                                    int blk_lo = 0x7fffffff, int blk_skip = 0, int part_off = 0,
                                                    const int32_t* __restrict__ blkwin = nullptr, int wcap = 0) {
    extern __shared__ __attribute__((aligned(16))) double prod[];   // tile == ITEMS * BS products (WIN: + wcap entries of x)
    __shared__ double sm[8];
    // a launch over a subset of the row blocks (interior / boundary rows of a shard, krylov_hip.hip): the
    // launch's blocks 0 .. blk_lo-1 are themselves, the others lie blk_skip further on
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    bid = bid < blk_lo ? bid : bid + blk_skip;
    const int r0 = rowblk[bid], r1 = rowblk[bid + 1];
    const int nz0 = indptr[r0], nz1 = indptr[r1];
    const int cnt = nz1 - nz0;
    double acc = 0.0;
    if (cnt <= tile) {
        if (cnt > 0) {
            // all index/value loads first, then all gathers: ITEMS independent loads in flight per
            // lane (clamped addresses instead of predicated loads, which would serialise)
            int c[ITEMS];
            double a[ITEMS];
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const int t = threadIdx.x + i * BS;
                const int tc = t < cnt ? t : cnt - 1;
                // read-once streams: non-temporal, so that they do not push the x lines that the
                // gathers below (and the neighbouring row blocks) need out of L2
                c[i] = __builtin_nontemporal_load(indices + nz0 + tc);
                a[i] = __builtin_nontemporal_load(data + nz0 + tc);
            }
            bool direct = true;
            if constexpr (WIN) {
                const int cmin = blkwin[2 * bid], span = blkwin[2 * bid + 1];
                if (span <= wcap) {                                  // (the same for the whole workgroup)
                    double* __restrict__ xw = prod + tile;
                    for (int j = threadIdx.x; j < span; j += BS) xw[j] = x[cmin + j];
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < ITEMS; ++i) a[i] = a[i] * xw[c[i] - cmin];
                    direct = false;
                }
            }
            if (direct) {
#pragma unroll
                for (int i = 0; i < ITEMS; ++i) {
                    const double xv = (c[i] < nloc) ? x[c[i]] : ghost[c[i] - nloc];
                    a[i] = a[i] * xv;
                }
            }
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const int t = threadIdx.x + i * BS;
                if (t < cnt) prod[t] = a[i];
            }
        }
        __syncthreads();
        for (int r = r0 + threadIdx.x; r < r1; r += BS) {
            const int p0 = indptr[r] - nz0, p1 = indptr[r + 1] - nz0;
            double s = 0.0;
            for (int p = p0; p < p1; ++p) s += prod[p];
            if (EPI == EPI_RES) {
                s = aux[r] - s;
                acc = fma(s, s, acc);
            }
            if constexpr (EPI == EPI_CHEB) s = cheb_row(cheb_args(aux), r, x[r], s);
            if constexpr (EPI == EPI_POLY) s = poly_row(poly_args(aux), r, x[r], s);
            st_nt(y + r, s);
            if (EPI == EPI_DOT) acc = fma(aux[r], s, acc);
        }
    } else {  // one long row
        double s = 0.0;
        for (int t = threadIdx.x; t < cnt; t += BS) {
            const int c = indices[nz0 + t];
            const double xv = (c < nloc) ? x[c] : ghost[c - nloc];
            s += data[nz0 + t] * xv;
        }
        s = block_sum(s, sm);
        __syncthreads();
        if (threadIdx.x == 0) {
            if (EPI == EPI_RES) {
                s = aux[r0] - s;
                acc = s * s;
            }
            if constexpr (EPI == EPI_CHEB) s = cheb_row(cheb_args(aux), r0, x[r0], s);
            if constexpr (EPI == EPI_POLY) s = poly_row(poly_args(aux), r0, x[r0], s);
            y[r0] = s;
            if (EPI == EPI_DOT) acc = aux[r0] * s;
        }
    }
    if (EPI != EPI_NONE && EPI != EPI_CHEB && EPI != EPI_POLY) {
        const double r = block_sum(acc, sm);
        if (threadIdx.x == 0) part_out[part_off + blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------------------------------
// CSR SpMM, Y[:, 0:ncols] = A X[:, 0:ncols] (utils.py:1593-1594 with a block argument: A U of the deflation
// set-up deflation.py:47, the explicit Ritz residuals deflation.py:849-855).  Same row blocks and the
// same LDS staging as k_spmv_stream, but the matrix is read ONCE: a lane keeps its ITEMS (index, value)
// pairs in registers and walks the columns of X in chunks of DC - gather, multiply, park DC product
// tiles in LDS, one lane per row adds each column's products left to right.  Per column that is the
// order of scipy's csr_matvecs (y[i, v] += a_ij * x[j, v], separate multiply and add): bit-identical
// to A.dot(X).
// ------------------------------------------------------------------------------------------
template <int ITEMS, int DC>
__global__ __launch_bounds__(BS) void k_spmm_stream(const int32_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ indices,
                                                    const double* __restrict__ data,
                                                    const int32_t* __restrict__ rowblk, int nblk, int tile,
                                                    const double* __restrict__ X, int64_t ldx,
                                                    double* __restrict__ Y, int64_t ldy, int ncols,
                                                    int64_t nloc = (int64_t)1 << 62,
                                                    const double* __restrict__ ghost = nullptr, int64_t ldg = 0) {
    // (a block-row shard: column ids >= nloc address the ghost entries the halo exchange delivered, one run of
    // ldg doubles per column of X)
    extern __shared__ __attribute__((aligned(16))) double prod[];   // [DC][tile]
    __shared__ double sm[8];
    const int bid = xcd_remap(blockIdx.x, nblk);
    const int r0 = rowblk[bid], r1 = rowblk[bid + 1];
    const int nz0 = indptr[r0], nz1 = indptr[r1];
    const int cnt = nz1 - nz0;
    if (cnt <= tile) {
        int c[ITEMS];
        double a[ITEMS];
        if (cnt > 0) {
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const int t = threadIdx.x + i * BS;
                const int tc = t < cnt ? t : cnt - 1;
                c[i] = __builtin_nontemporal_load(indices + nz0 + tc);
                a[i] = __builtin_nontemporal_load(data + nz0 + tc);
            }
        }
        for (int j0 = 0; j0 < ncols; j0 += DC) {
            const int nc = (ncols - j0 < DC) ? ncols - j0 : DC;
            if (cnt > 0) {
#pragma unroll
                for (int dc = 0; dc < DC; ++dc) {
                    if (dc < nc) {
                        const double* __restrict__ x = X + (int64_t)(j0 + dc) * ldx;
                        const double* __restrict__ gx = ghost + (int64_t)(j0 + dc) * ldg;
                        double pv[ITEMS];
#pragma unroll
                        for (int i = 0; i < ITEMS; ++i) pv[i] = a[i] * ((c[i] < nloc) ? x[c[i]] : gx[c[i] - nloc]);
#pragma unroll
                        for (int i = 0; i < ITEMS; ++i) {
                            const int t = threadIdx.x + i * BS;
                            if (t < cnt) prod[dc * tile + t] = pv[i];
                        }
                    }
                }
            }
            __syncthreads();
            for (int r = r0 + threadIdx.x; r < r1; r += BS) {
                const int p0 = indptr[r] - nz0, p1 = indptr[r + 1] - nz0;
                for (int dc = 0; dc < nc; ++dc) {
                    const double* __restrict__ pr = prod + dc * tile;
                    double s = 0.0;
                    for (int p = p0; p < p1; ++p) s += pr[p];
                    st_nt(Y + (int64_t)(j0 + dc) * ldy + r, s);
                }
            }
            __syncthreads();
        }
    } else {  // one long row: tree reduction per column (not bit-ordered, like k_spmv_stream)
        for (int j = 0; j < ncols; ++j) {
            const double* __restrict__ x = X + (int64_t)j * ldx;
            const double* __restrict__ gx = ghost + (int64_t)j * ldg;
            double s = 0.0;
            for (int t = threadIdx.x; t < cnt; t += BS) {
                const int cc = indices[nz0 + t];
                s += data[nz0 + t] * ((cc < nloc) ? x[cc] : gx[cc - nloc]);
            }
            s = block_sum(s, sm);
            if (threadIdx.x == 0) Y[(int64_t)j * ldy + r0] = s;
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------
// Banded ("DIA") SpMV for CSR operators whose entries sit on a few diagonals (finite-difference /
// stencil matrices: configs 2, 3, 5).  kh_csr_upload detects the structure and k_dia_fill builds
// the diagonal-major copy on the device: dia[d * ld + i] = A[i, i + off[d]] (0.0 where the row has
// no entry there; operators that store explicit zeros keep the CSR kernel, so "a == 0" <=> "no
// entry").  Per row 8 B per diagonal instead of 12 B per entry + indptr, no index stream, no LDS
// stage, and the x gather becomes nd coalesced streams.  A lane owns RPT pairs of neighbouring
// rows (16-byte value loads); the diagonals are visited in ascending offset = the storage order of
// a CSR row with sorted columns, separate multiply and add: the same bits as scipy's csr_matvec
// and as k_spmv_stream.  Same epilogues and the same XCD-aware block order as the CSR kernel.
//
// Constant coefficients (every stored value of a diagonal bitwise equal, at most KH_DIA_CMAX diagonals: the Laplacians
// of configs 2, 3 and 5) have a second form without the value copy: one presence mask per row pair (uint16_t: bit d of
// the low / high byte = row 2 i2 / 2 i2 + 1 has an entry on diagonal d; 1 B per row instead of 8 nd) and the nd values
// in DiaOffs::cst.  dia_slot gives the slot values of either form, and since a slot is non-zero exactly where an entry
// exists, the arithmetic behind it - and its bits - are the same.
// ------------------------------------------------------------------------------------------
constexpr int KH_DIA_MAX = 32;
constexpr int KH_DIA_CMAX = 8;      // diagonals of the mask form: a row's presence bits fit one byte
struct DiaOffs {
    int nd;
    int off[KH_DIA_MAX];
    double cst[KH_DIA_CMAX];        // mask form: the value of diagonal d (unused otherwise)
};

// Slot values of diagonal d at row pair i2 (rows 2 i2, 2 i2 + 1): from the value copy dia[d * ld + 2 i2 ...], or - MASK -
// from the row pair's presence bits m (loaded once per row pair) and the diagonal's value c: bit ? c : 0.0.  The form is
// a template parameter: a kernel branches once, wave-uniformly, around two straight-line copies of its row loop.
template <bool MASK>
__device__ __forceinline__ double2 dia_slot(const double* __restrict__ dia, int64_t ld, int d, int64_t i2, unsigned m,
                                            double c) {
    if constexpr (MASK) {
        return make_double2(((m >> d) & 1u) ? c : 0.0, ((m >> (d + 8)) & 1u) ? c : 0.0);
    } else {
        return ld_nt2(reinterpret_cast<const double2*>(dia + (int64_t)d * ld) + i2);
    }
}

// the presence mask of row pair i2 (streamed once, like the value copy)
__device__ __forceinline__ unsigned dia_mask_load(const uint16_t* __restrict__ mask, int64_t i2) {
    return (unsigned)__builtin_nontemporal_load(mask + i2);
}

// Column of a block-row shard on the axis of its own rows: local columns stay, the ghost columns
// (CSR ids nloc .. nloc+nprev+nnext, krypy_amd/dist.py) are the rows just before / after the slab:
// -nprev .. -1 and nloc .. nloc+nnext-1.  With it a sharded stencil matrix is banded again.
__host__ __device__ __forceinline__ int dia_virtual_col(int c, int nloc, int nprev) {
    return c < nloc ? c : (c < nloc + nprev ? c - nloc - nprev : c - nprev);
}

static __global__ __launch_bounds__(BS) void k_dia_fill(const int32_t* __restrict__ indptr,
                                                 const int32_t* __restrict__ indices,
                                                 const double* __restrict__ data, int64_t n_rows,
                                                 int nprev, DiaOffs o, double* __restrict__ dia,
                                                 int64_t ld) {
    const int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (r >= n_rows) return;
    for (int p = indptr[r]; p < indptr[r + 1]; ++p) {
        const int off = dia_virtual_col(indices[p], (int)n_rows, nprev) - (int)r;
        int d = 0;
        while (d < o.nd - 1 && o.off[d] != off) ++d;
        dia[(int64_t)d * ld + r] = data[p];
    }
}

// The mask form of the same operator: thread i2 writes the mask of row pair i2 - every one of the npair = ld / 2 entries,
// so the padding rows come out empty (w = 0 there, as with the zeros of the value copy).
static __global__ __launch_bounds__(BS) void k_dia_mask_fill(const int32_t* __restrict__ indptr,
                                                      const int32_t* __restrict__ indices, int64_t n_rows,
                                                      int nprev, DiaOffs o, uint16_t* __restrict__ mask,
                                                      int64_t npair) {
    const int64_t i2 = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (i2 >= npair) return;
    unsigned m = 0;
    for (int h = 0; h < 2; ++h) {
        const int64_t r = 2 * i2 + h;
        if (r >= n_rows) break;
        for (int p = indptr[r]; p < indptr[r + 1]; ++p) {
            const int off = dia_virtual_col(indices[p], (int)n_rows, nprev) - (int)r;
            int d = 0;
            while (d < o.nd - 1 && o.off[d] != off) ++d;
            m |= 1u << (d + 8 * h);
        }
    }
    mask[i2] = (uint16_t)m;
}

// XH (with HALO): the halo travels through IPC-mapped granules (xr_dev.h) inside THIS launch - every lane first stores the rows
// of x it owns among the slab's first nsend_prev / last nsend_next into the neighbours' ghost granules (system scope: xGMI
// writes), and a ghost entry is read by polling the own granules for this exchange's epoch.  Same arithmetic, same order.
// dmask != nullptr: the operator's mask form (dia unused; DiaOffs::cst holds the values).
template <int EPI, int ND, int RPT, bool HALO, bool XH = false>
__global__ __launch_bounds__(BS) void k_spmv_dia(DiaOffs o, const double* __restrict__ dia,
                                                 const uint16_t* __restrict__ dmask,
                                                 int64_t ld, int64_t n, int nblk,
                                                 const double* __restrict__ x,
                                                 const double* __restrict__ ghost, int nprev,
                                                 int nnext, double* __restrict__ y,
                                                 const double* __restrict__ aux,
                                                 double* __restrict__ part_out,
                                                 int blk_lo = 0x7fffffff, int blk_skip = 0, int part_off = 0,
                                                 XhArgs xh = XhArgs()) {
    static_assert(EPI != EPI_CHEB || (!HALO && !XH), "EPI_CHEB has no halo form");
    static_assert(EPI != EPI_POLY || (!HALO && !XH), "EPI_POLY has no halo form");
    __shared__ double sm[8];
    int lb, pslot = blockIdx.x;
    if constexpr (XH) {
        // Who stores and who polls, in dispatch order.  x is complete when this launch starts, so ANY workgroup can send the
        // slab's first / last rows: the first workgroups dispatched do (one entry per lane).  The workgroups whose rows read
        // ghost entries are mapped to the LAST block numbers: by the time they start, the neighbours' first workgroups - which
        // started with ours, the ranks run in step through the sums of the orthogonalisation - have long stored, and a poll is
        // one read.  (The owners of the boundary rows stored them and polled at once before: 33 us per product of the N/8 shard
        // against 18 without a halo - a polling workgroup then waits for a neighbour's LAST workgroups to be dispatched.)
        const int64_t nsend = (int64_t)xh.nsend_prev + xh.nsend_next;
        for (int64_t j = (int64_t)blockIdx.x * BS + threadIdx.x; j < nsend; j += (int64_t)gridDim.x * BS) {
            if (j < xh.nsend_prev) {
                xh_put(xh.prev, xh.prev_ng, xh.prev_off + j, xh.epoch, x[j]);
            } else {
                const int64_t jj = j - xh.nsend_prev;
                xh_put(xh.next, xh.next_ng, jj, xh.epoch, x[n - xh.nsend_next + jj]);
            }
        }
        const int gi = xh.ihi - xh.ilo;                      // interior blocks [ilo, ihi): no ghost entry in their rows
        const int b = blockIdx.x;
        if (b < gi) {
            lb = xh.ilo + xcd_remap(b, gi);
        } else {
            const int j = b - gi;
            lb = j < xh.ilo ? j : j + gi;
        }
        pslot = xcd_unmap(lb, gridDim.x);                    // the partial sums in the plain launch's order: the same bits
    } else {
        lb = xcd_remap(blockIdx.x, gridDim.x);       // (subset launches: see k_spmv_stream)
        lb = lb < blk_lo ? lb : lb + blk_skip;
    }
    const int64_t base = (int64_t)lb * (2 * BS * RPT);
    const int64_t last = n - 1;
    const bool xal = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    double s0[RPT], s1[RPT];
#pragma unroll
    for (int u = 0; u < RPT; ++u) s0[u] = s1[u] = 0.0;
    unsigned msk[RPT];                 // mask form: the presence bits of this lane's row pairs
    auto diagonal = [&](int d, auto form) {
        constexpr bool MF = decltype(form)::value;
        const int64_t off = o.off[d];
        const bool even = ((off & 1) == 0) && xal;
        const double c = MF ? o.cst[d] : 0.0;
        double2 a[RPT];
        double x0[RPT], x1[RPT];
        long long gix[XH ? 2 * RPT : 1];       // XH: the ghost entries this lane needs from this diagonal (-1: none)
        bool gany = false;
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const int64_t r = base + 2 * (threadIdx.x + u * BS);   // ld covers the whole grid
            a[u] = dia_slot<MF>(dia, ld, d, r >> 1, MF ? msk[u] : 0u, c);
            int64_t c0 = r + off, c1 = r + 1 + off;
            if (even && c0 >= 0 && c1 <= last) {            // aligned pair of x: one 16-byte load
                const double2 xv = *reinterpret_cast<const double2*>(x + c0);
                x0[u] = xv.x;
                x1[u] = xv.y;
                if constexpr (XH) gix[2 * u] = gix[2 * u + 1] = -1;
            } else if (HALO) {                              // rows of the neighbouring slabs: ghost[]
                const int64_t lo = -(int64_t)nprev, hi = last + nnext;
                c0 = c0 < lo ? lo : (c0 > hi ? hi : c0);
                c1 = c1 < lo ? lo : (c1 > hi ? hi : c1);
                if constexpr (XH) {
                    // own rows now, ghost entries after the loop: all of a lane's polls in flight together (one after the
                    // other - eight round trips to the uncached granules per diagonal - they were 12 us of this kernel)
                    const long long g0 = c0 < 0 ? c0 + nprev : (c0 > last ? nprev + (c0 - n) : -1);
                    const long long g1 = c1 < 0 ? c1 + nprev : (c1 > last ? nprev + (c1 - n) : -1);
                    gix[2 * u] = g0;
                    gix[2 * u + 1] = g1;
                    gany = gany || g0 >= 0 || g1 >= 0;
                    x0[u] = x[g0 >= 0 ? 0 : c0];
                    x1[u] = x[g1 >= 0 ? 0 : c1];
                } else {
                    x0[u] = c0 < 0 ? ghost[c0 + nprev] : (c0 > last ? ghost[nprev + (c0 - n)] : x[c0]);
                    x1[u] = c1 < 0 ? ghost[c1 + nprev] : (c1 > last ? ghost[nprev + (c1 - n)] : x[c1]);
                }
            } else {
                c0 = c0 < 0 ? 0 : (c0 > last ? last : c0);
                c1 = c1 < 0 ? 0 : (c1 > last ? last : c1);
                x0[u] = x[c0];
                x1[u] = x[c1];
            }
        }
        if constexpr (XH) {
            if (gany) {
                double gv[2 * RPT];
                xh_take_n<2 * RPT>(xh, gix, gv);
#pragma unroll
                for (int u = 0; u < RPT; ++u) {
                    x0[u] = gix[2 * u] >= 0 ? gv[2 * u] : x0[u];
                    x1[u] = gix[2 * u + 1] >= 0 ? gv[2 * u + 1] : x1[u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const double p0 = a[u].x * x0[u], p1 = a[u].y * x1[u];
            s0[u] = (a[u].x != 0.0) ? s0[u] + p0 : s0[u];
            s1[u] = (a[u].y != 0.0) ? s1[u] + p1 : s1[u];
        }
    };
    auto diagonals = [&](auto form) {
        if constexpr (ND > 0) {
#pragma unroll
            for (int d = 0; d < ND; ++d) diagonal(d, form);
        } else {
            for (int d = 0; d < o.nd; ++d) diagonal(d, form);
        }
    };
    bool masked = false;
    if constexpr (ND <= KH_DIA_CMAX) masked = dmask != nullptr;     // (wave-uniform: a kernel argument)
    if (masked) {
        if constexpr (ND <= KH_DIA_CMAX) {
#pragma unroll
            for (int u = 0; u < RPT; ++u) msk[u] = dia_mask_load(dmask, (base >> 1) + threadIdx.x + u * BS);
            diagonals(std::true_type());
        }
    } else {
        diagonals(std::false_type());
    }
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        const int64_t r = base + 2 * (threadIdx.x + u * BS);
        double v0 = s0[u], v1 = s1[u];
        if (r + 1 < n) {
            if (EPI == EPI_RES) {
                v0 = aux[r] - v0;
                v1 = aux[r + 1] - v1;
                acc = fma(v0, v0, acc);
                acc = fma(v1, v1, acc);
            }
            if (EPI == EPI_DOT) {
                acc = fma(aux[r], v0, acc);
                acc = fma(aux[r + 1], v1, acc);
            }
            if constexpr (EPI == EPI_CHEB) {
                const ChebArgs ch = cheb_args(aux);
                // r, d, dinv and x allow 16-byte accesses to a row pair (y does: the launcher)
                const bool chal = xal && ((reinterpret_cast<uintptr_t>(ch.r) | reinterpret_cast<uintptr_t>(ch.d) |
                                           reinterpret_cast<uintptr_t>(ch.dinv)) & 15) == 0;
                if (chal) {
                    const double2 z2 = cheb_row2(ch, r, *reinterpret_cast<const double2*>(x + r), make_double2(v0, v1));
                    v0 = z2.x;
                    v1 = z2.y;
                } else {
                    v0 = cheb_row(ch, r, x[r], v0);
                    v1 = cheb_row(ch, r + 1, x[r + 1], v1);
                }
            }
            if constexpr (EPI == EPI_POLY) {
                const PolyArgs pa = poly_args(aux);
                // y, prod and x allow 16-byte accesses to a row pair (out does: the launcher)
                const bool pal = xal && ((reinterpret_cast<uintptr_t>(pa.y) | reinterpret_cast<uintptr_t>(pa.prod)) & 15) == 0;
                if (pal) {
                    const double2 o2 = poly_row2(pa, r, *reinterpret_cast<const double2*>(x + r), make_double2(v0, v1));
                    v0 = o2.x;
                    v1 = o2.y;
                } else {
                    v0 = poly_row(pa, r, x[r], v0);
                    v1 = poly_row(pa, r + 1, x[r + 1], v1);
                }
            }
            st_nt2(reinterpret_cast<double2*>(y + r), make_double2(v0, v1));
        } else if (r < n) {
            if (EPI == EPI_RES) {
                v0 = aux[r] - v0;
                acc = fma(v0, v0, acc);
            }
            if (EPI == EPI_DOT) acc = fma(aux[r], v0, acc);
            if constexpr (EPI == EPI_CHEB) v0 = cheb_row(cheb_args(aux), r, x[r], v0);
            if constexpr (EPI == EPI_POLY) v0 = poly_row(poly_args(aux), r, x[r], v0);
            y[r] = v0;
        }
    }
    if (EPI != EPI_NONE && EPI != EPI_CHEB && EPI != EPI_POLY) {
        const double r = block_sum(acc, sm);
        if (threadIdx.x == 0) part_out[part_off + pslot] = r;
    }
}

// Banded SpMM: the operator (either form) streamed once for DC columns of X (k_spmv_dia's order per column:
// ascending offsets, separate multiply and add, empty slots skipped - the same bits).  A lane owns one pair
// of neighbouring rows and DC accumulator pairs.
template <int DC>
__global__ __launch_bounds__(BS) void k_spmm_dia(DiaOffs o, const double* __restrict__ dia,
                                                 const uint16_t* __restrict__ dmask, int64_t ld,
                                                 int64_t n, const double* __restrict__ X, int64_t ldx,
                                                 double* __restrict__ Y, int64_t ldy, int nc) {
    const int64_t r = ((int64_t)blockIdx.x * BS + threadIdx.x) * 2;
    if (r >= n) return;
    const int64_t last = n - 1;
    double s0[DC], s1[DC];
#pragma unroll
    for (int j = 0; j < DC; ++j) s0[j] = s1[j] = 0.0;
    auto diagonal = [&](int d, unsigned m, auto form) {
        constexpr bool MF = decltype(form)::value;
        const int64_t off = o.off[d];
        const double2 a = dia_slot<MF>(dia, ld, d, r >> 1, m, MF ? o.cst[d] : 0.0);
        int64_t c0 = r + off, c1 = r + 1 + off;
        c0 = c0 < 0 ? 0 : (c0 > last ? last : c0);
        c1 = c1 < 0 ? 0 : (c1 > last ? last : c1);
        double x0[DC], x1[DC];
#pragma unroll
        for (int j = 0; j < DC; ++j) {
            const double* __restrict__ x = X + (int64_t)(j < nc ? j : 0) * ldx;
            x0[j] = x[c0];
            x1[j] = x[c1];
        }
#pragma unroll
        for (int j = 0; j < DC; ++j) {
            const double p0 = a.x * x0[j], p1 = a.y * x1[j];
            s0[j] = (a.x != 0.0) ? s0[j] + p0 : s0[j];
            s1[j] = (a.y != 0.0) ? s1[j] + p1 : s1[j];
        }
    };
    if (dmask != nullptr) {           // (wave-uniform)
        const unsigned m = dia_mask_load(dmask, r >> 1);
        for (int d = 0; d < o.nd; ++d) diagonal(d, m, std::true_type());
    } else {
        for (int d = 0; d < o.nd; ++d) diagonal(d, 0u, std::false_type());
    }
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        if (j < nc) {
            double* __restrict__ y = Y + (int64_t)j * ldy;
            if (r + 1 < n) st_nt2(reinterpret_cast<double2*>(y + r), make_double2(s0[j], s1[j]));
            else y[r] = s0[j];
        }
    }
}

// ------------------------------------------------------------------------------------------
// Dense row-major GEMV (config 4: A 32768^2 fp64 = 8.6 GB streamed once per CG step).
// One wave64 per row: lanes stride the row with double2 loads, x stays in L2 (256 KB).
// HBM-bound (0.25 flop/B); MFMA cannot help a single right-hand side.
// ------------------------------------------------------------------------------------------
// ROWS rows per wave: the rows share every load of x (x is read from L2 once per ROWS rows instead of once per row - at one row
// per wave the L2 delivers as many bytes of x as HBM delivers of A) and ROWS x 4 row loads are in flight per lane.  Every row
// keeps its own four accumulators and their order: the same bits as with one row per wave.
template <int ROWS>
static __global__ __launch_bounds__(BS) void k_gemv_dense(int64_t n_rows, int64_t n_cols,
                                                   const double* __restrict__ a, int64_t lda,
                                                   const double* __restrict__ x,
                                                   double* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6)) * ROWS;
    if (row0 >= n_rows) return;
    const double* ar[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) ar[r] = a + (row0 + r < n_rows ? row0 + r : n_rows - 1) * lda;     // (a row past the end: the last one again, not stored)
    double acc[ROWS][4];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.0;
    if (((lda & 1) == 0) && ((reinterpret_cast<uintptr_t>(a) & 15) == 0)) {
        const double2* __restrict__ x2 = reinterpret_cast<const double2*>(x);
        const int64_t n2 = n_cols >> 1;
        int64_t i = lane;
        // four independent 16-byte loads per row in flight per lane (1 KB per wave instruction)
        for (; i + 192 < n2; i += 256) {
            // the matrix is streamed once: non-temporal, x stays in L2
            double2 av[ROWS][4];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const double2* __restrict__ a2 = reinterpret_cast<const double2*>(ar[r]);
#pragma unroll
                for (int q = 0; q < 4; ++q) av[r][q] = ld_nt2(a2 + i + 64 * q);
            }
            double2 xv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) xv[q] = x2[i + 64 * q];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[r][q] = fma(av[r][q].x, xv[q].x, acc[r][q]);
                    acc[r][q] = fma(av[r][q].y, xv[q].y, acc[r][q]);
                }
            }
        }
        for (; i < n2; i += 64) {
            const double2 xv = x2[i];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const double2 av = reinterpret_cast<const double2*>(ar[r])[i];
                acc[r][0] = fma(av.x, xv.x, acc[r][0]);
                acc[r][0] = fma(av.y, xv.y, acc[r][0]);
            }
        }
        if ((n_cols & 1) && lane == 0) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[r][0] = fma(ar[r][n_cols - 1], x[n_cols - 1], acc[r][0]);
        }
    } else {
        for (int64_t i = lane; i < n_cols; i += 64) {
            const double xv = x[i];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[r][0] = fma(ar[r][i], xv, acc[r][0]);
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const double s = wave_sum((acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3]));
        if (lane == 0 && row0 + r < n_rows) y[row0 + r] = s;
    }
}

// ------------------------------------------------------------------------------------------
// Dense A times a PANEL of up to 16 vectors on the FP64 matrix cores (v_mfma_f64_16x16x4_f64):
// Y[:, 0:nc] = A X[:, 0:nc].  The one GEMM-shaped operation of the path (A U of the deflation set-up,
// multi-column LinearOperator.dot, Ritz residuals with a dense operator): A is streamed once for
// all columns instead of once per column.  A wave owns RT tiles of 16 rows; per 64-column chunk
// every lane loads 8 double2 of its row (lane = (row r, quarter q): columns c0 + 8i + 2q, +1 - the
// four lanes of a row read 64 contiguous bytes per instruction) and the matching 8 double2 of its
// X column; the k index of an MFMA only has to agree between the A and the B operand, so this
// interleaved order needs no shuffles.  MFMA f64 layouts: A[l&15][l>>4], B[l>>4][l&15],
// D: col = l&15, row = (l>>4) + 4*reg.
// ------------------------------------------------------------------------------------------
typedef double v4f64 __attribute__((ext_vector_type(4)));

template <int RT>
__global__ __launch_bounds__(BS) void k_gemm_dense_mfma(int64_t n_rows, int64_t n_cols,
                                                        const double* __restrict__ a, int64_t lda,
                                                        const double* __restrict__ X, int64_t ldx, int nc,
                                                        double* __restrict__ Y, int64_t ldy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int64_t row_base = ((int64_t)blockIdx.x * (BS / 64) + wave) * (16 * RT);
    if (row_base >= n_rows) return;
    v4f64 acc[RT];
    const double* __restrict__ arow[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
        int64_t row = row_base + 16 * t + r;
        row = row < n_rows ? row : n_rows - 1;          // tail tiles re-read the last row (never stored)
        arow[t] = a + row * lda;
    }
    const bool colok = r < nc;
    const double* __restrict__ xcol = X + (int64_t)(colok ? r : 0) * ldx;
    const int64_t full = n_cols & ~(int64_t)63;
    for (int64_t c0 = 0; c0 < full; c0 += 64) {
        double2 bv[8], av[RT][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) bv[i] = *reinterpret_cast<const double2*>(xcol + c0 + 8 * i + 2 * q);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int i = 0; i < 8; ++i) av[t][i] = *reinterpret_cast<const double2*>(arow[t] + c0 + 8 * i + 2 * q);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double bx = colok ? bv[i].x : 0.0, by = colok ? bv[i].y : 0.0;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t][i].x, bx, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t][i].y, by, acc[t], 0, 0, 0);
            }
        }
    }
    if (full < n_cols) {   // last, partial chunk: guarded scalar loads
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t kk = full + 8 * i + 2 * q + h;
                const bool ok = kk < n_cols;
                const double bx = (ok && colok) ? xcol[kk] : 0.0;
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const double ax = ok ? arow[t][kk] : 0.0;
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bx, acc[t], 0, 0, 0);
                }
            }
        }
    }
    if (colok) {
        double* __restrict__ ycol = Y + (int64_t)r * ldy;
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t row = row_base + 16 * t + q + 4 * i;
                if (row < n_rows) ycol[row] = acc[t][i];
            }
    }
}

// ------------------------------------------------------------------------------------------
// X^T Y for two tall blocks of up to 16 columns each on the FP64 matrix cores: utils.inner with a block on both sides
// (utils.py:160-193 - <W, V> of Projection.__init__, <U, AU>, <V, AU> of the Ritz set-up).  The per-column form
// (k_multidot, one launch and one host round trip per column of Y) reads X once PER COLUMN of Y: 272 column reads for a
// 16 x 16 product; here both blocks are read once (32).  A wave takes chunks of 64 rows; lane (c, q) loads the rows
// r0 + 8 i + 2 q, + 1 (i = 0 .. 7) of column c of X and of Y - the four lanes of a column read 64 contiguous bytes per
// instruction - and feeds them to 16 MFMAs whose k index only has to agree between the two operands (the layouts of
// k_gemm_dense_mfma above).  Per workgroup the four waves' tiles are added in wave order and stored to
// part[e * pstride + blockIdx.x], e = 16 i + j; k_reduce_partials adds the workgroups in index order: the same bits from run to
// run, another summation order than k_multidot's (parity with the oracle at 1e-10 like every other sum, tests/test_gpu_gram.py).
// ------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(BS) void k_gram_mfma(int64_t n, const double* __restrict__ X, int64_t ldx, int nx,
                                                         const double* __restrict__ Y, int64_t ldy, int ny,
                                                         double* __restrict__ part, int pstride) {
    __shared__ double sm[BS / 64][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const bool xok = c < nx, yok = c < ny;
    const double* __restrict__ xc = X + (int64_t)(xok ? c : 0) * ldx;
    const double* __restrict__ yc = Y + (int64_t)(yok ? c : 0) * ldy;
    v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
    const int64_t nchunk = n >> 6;
    const int64_t nw = (int64_t)gridDim.x * (BS / 64);
    const int64_t me = (int64_t)blockIdx.x * (BS / 64) + wave;
    for (int64_t ch = me; ch < nchunk; ch += nw) {
        const int64_t r0 = (ch << 6) + 2 * q;
        double2 xv[8], yv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) xv[i] = ld_nt2(reinterpret_cast<const double2*>(xc + r0 + 8 * i));
#pragma unroll
        for (int i = 0; i < 8; ++i) yv[i] = ld_nt2(reinterpret_cast<const double2*>(yc + r0 + 8 * i));
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xok ? xv[i].x : 0.0, yok ? yv[i].x : 0.0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xok ? xv[i].y : 0.0, yok ? yv[i].y : 0.0, acc, 0, 0, 0);
        }
    }
    if ((n & 63) != 0 && me == nchunk % nw) {      // the last, partial chunk: guarded scalar loads, one wave
        const int64_t r0 = nchunk << 6;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t row = r0 + 8 * i + 2 * q + h;
                const bool ok = row < n;
                const double ax = (ok && xok) ? xc[row] : 0.0;
                const double bx = (ok && yok) ? yc[row] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bx, acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sm[wave][(q + 4 * r) * 16 + c] = acc[r];      // D: row = q + 4 reg, column = c
    __syncthreads();
    double s = sm[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < BS / 64; ++w) s += sm[w][threadIdx.x];
    part[(int64_t)threadIdx.x * pstride + blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------
// A tall block times a small matrix on the FP64 matrix cores: Y[:, 0:nc] = beta Y + X[:, 0:k] C, nc = 2 ... 16 - the Ritz
// vectors [V_n, U] @ coeffs (deflation.py:840-847), utils.py:1618's V @ Ur.  The per-column form (k_multiaxpy, one pass over all
// of X per OUTPUT column) read the basis nc times; here it is read once.  Another summation order than k_multiaxpy's left-to-right
// fold (1e-13 against it, tests/test_gpu_gram.py); one output column (the x update of every solver) keeps k_multiaxpy and its bits.
// Y[:, 0:nc] = beta * Y[:, 0:nc] + X[:, 0:k] C   (C: k x 16 in LDS order, rows beyond nc zero) on the FP64 matrix cores.
// A wave takes tiles of 32 rows: lane (r, q) loads the row PAIR (2 r, 2 r + 1) of basis column i0 + q as one 16-byte load (the
// sixteen lanes of a column read 256 contiguous bytes) - .x feeds the MFMA of the even rows, .y the one of the odd rows; the B
// operand is C[i0 + q][c] from LDS.  D: column c = l & 15, row t = (l >> 4) + 4 reg of the even / odd half: stored as the pair
// (even, odd) = rows 2 t, 2 t + 1 of output column c, 16 bytes per lane.
template <int RT, int BETA>      // RT tiles of 32 rows per wave and pass; BETA 0: Y not read, 1: Y += , 2: runtime beta
__global__ __launch_bounds__(BS) void k_panel_gemm_mfma(int64_t n, const double* __restrict__ X, int64_t ldx, int k,
                                                         const double* __restrict__ Cdev, int nc, double beta,
                                                         double* __restrict__ Y, int64_t ldy) {
    extern __shared__ double csm[];              // [kpad][16]
    const int kpad = (k + 3) & ~3;
    for (int i = threadIdx.x; i < kpad * 16; i += BS) {
        const int row = i >> 4, c = i & 15;
        csm[i] = (row < k && c < nc) ? Cdev[row * nc + c] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int64_t ntile = (n + 31) >> 5;
    const int64_t nw = (int64_t)gridDim.x * (BS / 64);
    const int64_t n2 = (n + 1) >> 1;             // row pairs (the padding behind n is zero and stays zero: 0 * C)
    for (int64_t t0 = ((int64_t)blockIdx.x * (BS / 64) + wave) * RT; t0 < ntile; t0 += nw * RT) {
        v4f64 ae[RT], ao[RT];
        const double2* __restrict__ xp[RT];
        bool ok[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            ae[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
            ao[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
            const int64_t pair = ((t0 + t) << 4) + r;          // row pair of this lane
            ok[t] = pair < n2;
            xp[t] = reinterpret_cast<const double2*>(X + (int64_t)q * ldx) + (ok[t] ? pair : 0);
        }
        const int64_t cstep = 2 * ldx;                          // four columns on, in double2 units
        for (int i0 = 0; i0 < kpad; i0 += 8) {
            double2 xa[RT], xb[RT];
            const bool two = i0 + 4 < kpad;
            const bool va = i0 + q < k, vb = two && (i0 + 4 + q < k);
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                xa[t] = (ok[t] && va) ? ld_nt2(xp[t]) : make_double2(0.0, 0.0);
                xb[t] = (ok[t] && vb) ? ld_nt2(xp[t] + cstep) : make_double2(0.0, 0.0);
                xp[t] += 2 * cstep;
            }
            const double ba = csm[(i0 + q) * 16 + r];
            const double bb = two ? csm[(i0 + 4 + q) * 16 + r] : 0.0;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                ae[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[t].x, ba, ae[t], 0, 0, 0);
                ao[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[t].y, ba, ao[t], 0, 0, 0);
                ae[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[t].x, bb, ae[t], 0, 0, 0);
                ao[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[t].y, bb, ao[t], 0, 0, 0);
            }
        }
        if (r < nc) {
            double2* __restrict__ yc = reinterpret_cast<double2*>(Y + (int64_t)r * ldy);
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int64_t pair = ((t0 + t) << 4) + q + 4 * g;
                    if (pair < n2) {
                        double2 v = make_double2(ae[t][g], ao[t][g]);
                        if (BETA != 0) {
                            const double2 y = yc[pair];
                            const double b = BETA == 1 ? 1.0 : beta;
                            v.x += b * y.x;
                            v.y += b * y.y;
                        }
                        yc[pair] = v;
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Attainable-bandwidth probes for bench.py ("measure the attainable ceiling on the box with
// a device triad/copy kernel"): plain 16-byte grid-stride streams, non-temporal loads, no reuse.
// ------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(BS) void k_stream_copy(int64_t n2, const double2* __restrict__ src,
                                                    double2* __restrict__ dst) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    for (; i + 3 * stride < n2; i += 4 * stride) {
        const double2 a = ld_nt2(src + i), b = ld_nt2(src + i + stride), c = ld_nt2(src + i + 2 * stride),
                      d = ld_nt2(src + i + 3 * stride);
        dst[i] = a;
        dst[i + stride] = b;
        dst[i + 2 * stride] = c;
        dst[i + 3 * stride] = d;
    }
    for (; i < n2; i += stride) dst[i] = ld_nt2(src + i);
}

static __global__ __launch_bounds__(BS) void k_stream_triad(int64_t n2, const double2* __restrict__ b,
                                                     const double2* __restrict__ c, double s,
                                                     double2* __restrict__ a) {
    const int64_t stride = (int64_t)gridDim.x * BS;
    int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    for (; i + stride < n2; i += 2 * stride) {
        const double2 b0 = ld_nt2(b + i), b1 = ld_nt2(b + i + stride), c0 = ld_nt2(c + i), c1 = ld_nt2(c + i + stride);
        a[i] = make_double2(b0.x + s * c0.x, b0.y + s * c0.y);
        a[i + stride] = make_double2(b1.x + s * c1.x, b1.y + s * c1.y);
    }
    for (; i < n2; i += stride) {
        const double2 b0 = ld_nt2(b + i), c0 = ld_nt2(c + i);
        a[i] = make_double2(b0.x + s * c0.x, b0.y + s * c0.y);
    }
}

static __global__ __launch_bounds__(BS) void k_stream_read(int64_t n2, const double2* __restrict__ src,
                                                    double* __restrict__ part_out) {
    __shared__ double sm[8];
    const int64_t stride = (int64_t)gridDim.x * BS;
    int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (; i + 3 * stride < n2; i += 4 * stride) {
        const double2 a = ld_nt2(src + i), b = ld_nt2(src + i + stride), c = ld_nt2(src + i + 2 * stride),
                      d = ld_nt2(src + i + 3 * stride);
        s0 += a.x + a.y;
        s1 += b.x + b.y;
        s2 += c.x + c.y;
        s3 += d.x + d.y;
    }
    for (; i < n2; i += stride) {
        const double2 a = ld_nt2(src + i);
        s0 += a.x + a.y;
    }
    const double r = block_sum((s0 + s1) + (s2 + s3), sm);
    if (threadIdx.x == 0) part_out[blockIdx.x] = r;
}

// tile-based probes (no grid-stride loop): a workgroup owns U*BS consecutive double2, every lane U of them
template <int U, bool NTS>
__global__ __launch_bounds__(BS) void k_probe_copy(int64_t n2, const double2* __restrict__ src,
                                                   double2* __restrict__ dst) {
    const int64_t base = (int64_t)blockIdx.x * (U * BS) + threadIdx.x;
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = (base + u * BS < n2) ? ld_nt2(src + base + u * BS) : make_double2(0.0, 0.0);
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (base + u * BS < n2) {
            if (NTS) {
                v2f64_t t;
                t.x = v[u].x;
                t.y = v[u].y;
                __builtin_nontemporal_store(t, reinterpret_cast<v2f64_t*>(dst + base + u * BS));
            } else {
                dst[base + u * BS] = v[u];
            }
        }
}

template <int U>
__global__ __launch_bounds__(BS) void k_probe_read(int64_t n2, const double2* __restrict__ src,
                                                   double* __restrict__ sink) {
    const int64_t base = (int64_t)blockIdx.x * (U * BS) + threadIdx.x;
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = (base + u * BS < n2) ? ld_nt2(src + base + u * BS) : make_double2(0.0, 0.0);
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) s += v[u].x + v[u].y;
    if (s == 1.2345e300) sink[0] = s;       // never true: keeps the loads alive
}

// y = M x for a tiny dense row-major M (d x d, d <= 1024) held on the device: the projector's
// R^{-1} Q^H and WR^H factors.  One workgroup, one row per thread, sequential sums (deterministic).
static __global__ __launch_bounds__(BS) void k_small_matvec(int d, const double* __restrict__ M,
                                                     const double* __restrict__ x,
                                                     double* __restrict__ y) {
    for (int i = threadIdx.x; i < d; i += BS) {
        double s = 0.0;
        if (M == nullptr) {
            s = x[i];
        } else {
            for (int j = 0; j < d; ++j) s += M[(int64_t)i * d + j] * x[j];
        }
        y[i] = s;
    }
}

}  // namespace kh
