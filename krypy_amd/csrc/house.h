// Householder Arnoldi (utils.py:970-994, House at 332-402) in ONE launch per step.
//
// The reference applies the k + 1 reflectors H_j = I - beta_j u_j u_j^T to w = A v_k one after the other, makes reflector
// k + 1 from what is left below row k, and builds v_{k+1} = alpha_{k+1} H_0 ... H_{k+1} e_{k+1} with a second, descending pass
// over the same reflectors.  A reflector link has the shape of a Gram-Schmidt link - d = <u_j, w>, w -= (beta_j d) u_j - so the
// step runs like k_mgs_chain (chain.h): the vector stays in registers, every dot is a grid-wide fixed-order sum inside the
// launch (grid_role / grid_sum / grid_sum2, unchanged), every column is streamed through the same two-deep register ring.
//
//   load w = A v_k (the caller applied the operator)                                         8 N bytes
//   forward, j = 0 .. k:      d = <u_j, w>,  w -= (beta_j d) u_j          (beta_j == 0: skipped)   16 N per link
//   rows 0 .. k of w are the raw H entries: workgroup 0 stores them to the pinned H column
//   one grid_sum2:  sigma2 = sum_{i > k+1} w_i^2,  gamma = w[k+1] (its owner contributes it, everybody else 0)
//   every thread: (v0, xnorm, alpha, beta) of _house_scalars (utils.py:349-377) from (gamma, sigma)
//   u_{k+1} = [0 .. 0, v0, w_{k+2}, ...] * s,  s = 1 / sqrt(v0^2 + sigma^2),  written from the registers   8 N
//   x = e_{k+1} - (beta u_{k+1}[k+1]) u_{k+1}   in the same registers: <u_{k+1}, e_{k+1}> is the entry the thread
//       has just made - link k + 1 of the descending pass needs neither a sum nor a read
//   backward, j = k .. 0:     d = <u_j, x>,  x -= (beta_j d) u_j                              16 N per link
//   V[:, k+1] = alpha_{k+1} x                                                                 8 N
//
// 2 k + 3 grid-wide sums at most per launch.  Two rearrangements against the reference's order of operations make the
// single launch possible, neither changes a result beyond rounding:
//   (1) the factors Av[j] *= conj(alpha_j) touch row j only, and no later reflector (zero above its own row) reads row j:
//       the host applies them to the k + 1 downloaded entries;
//   (2) H[k+1, k] = |alpha| xnorm = xnorm analytically - the reference applies the new reflector to w and takes abs().
// beta_j lives in a device array next to the reflector block (entry k + 1 is written here; the host sets entries made by the
// per-reflector path).  The skip of a link with beta_j == 0 is uniform over the grid: every workgroup reads the same word.
//
// Storage contracts as in chain.h: columns are read in whole CH_BS-strided rows (zero padding or, MASKED, a select on the
// register), nothing but rows [0, n) of the two new columns is stored - with an odd n row n goes along with row n - 1 and is
// 0 * s = 0 in the reflector and alpha * (0 - c * 0) = 0 in the basis column (s is finite: the root is >= 1 when sigma == 0,
// so no 0 / 0 anywhere).
// A thread never reads what this launch wrote: no hand-off between workgroups except through the sums.
#pragma once
#include "chain.h"

namespace kh {

struct HouseArgs {
    int64_t n2;        // vector length in double2
    int64_t chunk2;    // double2 per workgroup (R2 * CH_BS)
    const double* U;   // reflector block: u_j = U + j * ldu
    int64_t ldu;
    double* unext;     // U[:, k+1]
    double* beta;      // beta[0 .. k] read, beta[k+1] written
    const double* w_in;
    double* vnext;     // V[:, k+1]
    int k;
    unsigned long long* gran;
    unsigned* xcc_leader;
    unsigned long long* xcc_res;
    unsigned epoch0;
    int* err;
    int debug;         // tests: 4 = fake a timed-out sum (the error word is set, garbage is left behind)
    // pinned H column of the slot: [0 .. k] raw entries of w, then gamma, sigma2, xnorm, alpha_{k+1}, beta_{k+1}
    double* hpin;
    int* errpin;
    int* donepin;      // completion tag behind the column (CH_SIGNAL_DONE), or nullptr: the host waits for an event
    int done_tag;
};

constexpr int HOUSE_NSCAL = 5;         // scalars behind the raw H entries

// One reflector link on the register-resident vector: d = <u, w> (grid-wide), w -= (beta d) u.  The column is streamed twice
// through the two-deep ring of k_mgs_chain; ring[0] holds its first batch on entry and the first batch of `vn` on exit.
template <int R2, bool MASKED>
__device__ __forceinline__ void house_link(double2 (&w)[R2], double2 (&ring)[2][ChainShape<R2>::PB], const double2* __restrict__ v2,
                                           const double2* __restrict__ vn, const double bj, const int rem, unsigned& epoch,
                                           const HouseArgs& a, const int G, double* smd, unsigned* smu, const GridRole role) {
    constexpr int PB = ChainShape<R2>::PB;
    constexpr int NB = ChainShape<R2>::NB;
#define CH_OK(r) (!MASKED || (r) * CH_BS < rem)
    // ---- dot phase: <u_j, w> ----
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        // issue the next batch: rows of batch b+1, or the first rows again for the update
        const double2* __restrict__ nx = (b + 1 < NB) ? v2 + (int64_t)(b + 1) * PB * CH_BS : v2;
#pragma unroll
        for (int i = 0; i < PB; ++i) ring[(b + 1) & 1][i] = nx[(int64_t)i * CH_BS];
        CH_ISSUE_FENCE();
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            double2 v = ring[b & 1][i];
            if (MASKED && !CH_OK(b * PB + i)) v = make_double2(0.0, 0.0);   // beyond the vector: whatever the block holds there
            acc0 = fma(v.x, w[b * PB + i].x, acc0);
            acc1 = fma(v.y, w[b * PB + i].y, acc1);
        }
    }
    double d = grid_sum(acc0 + acc1, epoch++, a.gran, G, a.err, smd, smu, role, a.xcc_res);
    if (a.debug == 4) d *= 0.5;          // ... that leaves garbage behind
    const double c = bj * d;
    // ---- update phase: w -= (beta_j d) u_j ----
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const double2* __restrict__ nx = (b + 1 < NB) ? v2 + (int64_t)(b + 1) * PB * CH_BS : vn;
#pragma unroll
        for (int i = 0; i < PB; ++i) ring[(b + 1) & 1][i] = nx[(int64_t)i * CH_BS];
        CH_ISSUE_FENCE();
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const double2 p = ring[b & 1][i];
            const int r = b * PB + i;
            w[r].x = CH_OK(r) ? w[r].x - c * p.x : 0.0;
            w[r].y = CH_OK(r) ? w[r].y - c * p.y : 0.0;
        }
    }
#undef CH_OK
}

template <int R2, bool MASKED>
__global__ __launch_bounds__(CH_BS) void k_house_chain(HouseArgs a) {
    constexpr int PB = ChainShape<R2>::PB;
    __shared__ double smd[4 * (CH_BS / 64)];
    __shared__ unsigned smu[2 * CH_GMAX];
    __shared__ int slead;
    __shared__ double sbeta[2 * CH_BS];      // beta[0 .. k] (k + 2 <= 2 CH_BS): read at every item, never from memory again
    const int tid = threadIdx.x;
    const int G = gridDim.x;
    const int bid = blockIdx.x;
    const int k = a.k;
    for (int i = tid; i <= k; i += CH_BS) sbeta[i] = a.beta[i];      // (the barrier inside grid_role publishes them)
    const GridRole role = grid_role(a.xcc_leader, a.epoch0, &slead);
    // chunk2 == R2 * CH_BS: thread `tid` owns double2 rows first + r*CH_BS, r < R2
    const int64_t first = (int64_t)bid * a.chunk2 + tid;
    const int64_t left = a.n2 - first;
    const int rem = (int)(left < 0 ? 0 : (left > a.chunk2 ? a.chunk2 : left));
#define CH_OK(r) (!MASKED || (r) * CH_BS < rem)
    double2 w[R2];
    double2 ring[2][PB];
    {
        const double2* __restrict__ win2 = reinterpret_cast<const double2*>(a.w_in) + first;
#pragma unroll
        for (int r = 0; r < R2; ++r) {
            const double2 v = win2[(int64_t)r * CH_BS];
            w[r].x = CH_OK(r) ? v.x : 0.0;
            w[r].y = CH_OK(r) ? v.y : 0.0;
            if ((r + 1) % 8 == 0) CH_ISSUE_FENCE();
        }
    }
    unsigned epoch = a.epoch0;
    if (a.debug == 4 && tid == 0) __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // tests: a faked timeout
    // links whose beta is zero are left out (uniform over the grid); the forward pass walks the others upwards, the
    // backward pass downwards, and the first batch of the column that comes next is loaded ahead of it (across the
    // new reflector: the first backward column)
    auto up = [&](int j) {
        while (j <= k && sbeta[j] == 0.0) ++j;
        return j;                                    // k + 1: none left
    };
    auto down = [&](int j) {
        while (j >= 0 && sbeta[j] == 0.0) --j;
        return j;                                    // -1: none left
    };
    auto col2 = [&](int j) { return reinterpret_cast<const double2*>(a.U + (int64_t)j * a.ldu) + first; };
    const bool e_odd = ((k + 1) & 1) != 0;           // row k + 1 is the .y (odd) or the .x (even) half of double2 row (k + 1) / 2
    const int jtop = down(k);                        // the first backward link
    int j = up(0);
    {
        const double2* __restrict__ v2 = col2(jtop < 0 ? 0 : j);      // (no link at all: column 0, valid memory, never used)
#pragma unroll
        for (int i = 0; i < PB; ++i) ring[0][i] = v2[(int64_t)i * CH_BS];
        CH_ISSUE_FENCE();
    }
    while (j <= k) {
        const int jn = up(j + 1);
        house_link<R2, MASKED>(w, ring, col2(j), col2(jn <= k ? jn : jtop), sbeta[j], rem, epoch, a, G, smd, smu, role);
        j = jn;
    }
    // ---- the new reflector (ring[0] keeps the first batch of the first backward column) ----
    if (bid == 0) {          // rows 0 .. k: row 0 of workgroup 0 (k + 2 <= 2 CH_BS: the launcher)
        if (2 * tid <= k) a.hpin[2 * tid] = w[0].x;
        if (2 * tid + 1 <= k) a.hpin[2 * tid + 1] = w[0].y;
    }
    // this thread's row r holds row k + 1 iff de == r * CH_BS, rows behind it iff de < r * CH_BS
    const int de = (int)((int64_t)((k + 1) >> 1) - first);
    double s2 = 0.0, gm = 0.0;
#pragma unroll
    for (int r = 0; r < R2; ++r) {
        const bool at = de == r * CH_BS, behind = de < r * CH_BS;
        const double qx = behind ? w[r].x : 0.0;
        const double qy = (behind || (at && !e_odd)) ? w[r].y : 0.0;
        s2 = fma(qx, qx, s2);
        s2 = fma(qy, qy, s2);
        gm = at ? (e_odd ? w[r].y : w[r].x) : gm;
    }
    __syncthreads();         // (grid_sum2 begins with stores to the LDS words a slow wave of an XCD leader may still be reading
                             // as the last step of the forward pass's final grid_sum)
    grid_sum2(s2, gm, epoch++, a.gran, G, a.err, smd, smu, role, a.xcc_res);
    // the scalar part, every thread for itself (utils.py:349-377)
    const double sigma = sqrt(s2);
    double v0, xnorm, beta, alpha_new;
    if (sigma == 0.0) {
        v0 = 1.0;
        xnorm = fabs(gm);
        alpha_new = (gm == 0.0) ? 1.0 : gm / xnorm;
        beta = 0.0;
    } else {
        xnorm = sqrt(gm * gm + sigma * sigma);
        if (gm == 0.0) {
            v0 = -sigma;
            alpha_new = 1.0;
        } else {
            const double sg = gm / fabs(gm);
            v0 = gm + sg * xnorm;
            alpha_new = -sg;
        }
        beta = 2.0;
    }
    // (one division: 2 R2 of them in the loop below cost the kernel its register allocation)
    const double sc = 1.0 / sqrt(v0 * v0 + sigma * sigma);       // the root is >= 1 when sigma == 0, > 0 otherwise
    // link k + 1 of the descending pass on x = e_{k+1}: <u_{k+1}, x> is the entry u_{k+1}[k+1] itself
    double du = v0 * sc;
    if (a.debug == 4) du *= 0.5;          // ... that leaves garbage behind
    const double c = beta * du;
    double2* __restrict__ un2 = reinterpret_cast<double2*>(a.unext) + first;
#pragma unroll
    for (int r = 0; r < R2; ++r) {
        const bool at = de == r * CH_BS, behind = de < r * CH_BS;
        double2 u;
        u.x = (behind ? w[r].x : ((at && !e_odd) ? v0 : 0.0)) * sc;
        u.y = (behind || (at && !e_odd) ? w[r].y : (at ? v0 : 0.0)) * sc;
        if (r * CH_BS < rem) st_nt2(un2 + (int64_t)r * CH_BS, u);
        w[r].x = ((at && !e_odd) ? 1.0 : 0.0) - c * u.x;
        w[r].y = ((at && e_odd) ? 1.0 : 0.0) - c * u.y;
    }
    if (bid == 0 && tid == 0) {
        a.beta[k + 1] = beta;
        a.hpin[k + 1] = gm;
        a.hpin[k + 2] = s2;
        a.hpin[k + 3] = xnorm;
        a.hpin[k + 4] = alpha_new;
        a.hpin[k + 5] = beta;
    }
    j = jtop;
    while (j >= 0) {
        const int jn = down(j - 1);
        house_link<R2, MASKED>(w, ring, col2(j), col2(jn >= 0 ? jn : 0), sbeta[j], rem, epoch, a, G, smd, smu, role);
        j = jn;
    }
    // V[:, k+1] = alpha_{k+1} x
    double2* __restrict__ vn2 = reinterpret_cast<double2*>(a.vnext) + first;
#pragma unroll
    for (int r = 0; r < R2; ++r) {
        if (r * CH_BS < rem) {
            double2 o;
            o.x = alpha_new * w[r].x;
            o.y = alpha_new * w[r].y;
            st_nt2(vn2 + (int64_t)r * CH_BS, o);
        }
    }
    if (bid == 0) {
        if (tid == 0) *a.errpin = __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        CH_SIGNAL_DONE(a);
    }
#undef CH_OK
}

// ------------------------------------------------------------------------------------------
// The same step for complex (c128) vectors: k_zhouse_chain.
//
// A complex N-vector is the real block of 2 N interleaved doubles (zpath.h), so ONE double2 register row is ONE complex
// row: geometry, ring, padding and the MASKED form are those of the real kernel with n2 = N, and complex row i is row
// i - first of its owner (no odd / even halves).  What differs:
//   link          d = conj(u_j) . w, both parts in ONE grid_sum2 round (as k_mgs_chain<..., CPLX>);
//                 w -= (beta_j d) u_j with NumPy's product (ar br - ai bi, ar bi + ai br), separate roundings
//                 (-ffp-contract=off).  beta_j stays real (LDS), a link with beta_j == 0 is skipped.
//   raw H rows    complex rows 0 .. k sit in the first TWO register rows of workgroup 0 (512 each): k + 2 <= 1024 as in
//                 the real kernel.  The pinned column holds 2 (k + 1) doubles of them, then
//                 Re gamma, Im gamma, sigma2, xnorm, Re alpha, Im alpha, beta   (ZHOUSE_NSCAL = 7).
//   new reflector gamma = w[k+1] (its owner contributes it) in one grid_sum2, sigma2 = sum_{i > k+1} |w_i|^2 in one
//                 grid_sum: 2 k + 4 grid-wide rounds at most per launch ((k + 1) + 2 + (k + 1)).
//                 Scalars (utils.py:349-377 with a complex gamma): |gamma| = hypot(re, im), xnorm = sqrt(|gamma|^2 + sigma^2),
//                 v0 = gamma + gamma / |gamma| xnorm, alpha = -gamma / |gamma|, beta = 2; gamma == 0: v0 = -sigma, alpha = 1;
//                 sigma == 0: v0 = 1, xnorm = |gamma|, alpha = gamma / |gamma| (or 1), beta = 0.
//   backward      x = e_{k+1} - (beta conj(u_{k+1}[k+1])) u_{k+1}: the coefficient is v^* e_{k+1}, the CONJUGATE of the
//                 entry just made; V[:, k+1] = alpha_{k+1} x is a complex product.
// (The sum of a grid_sum ends with reads of LDS words that a grid_sum2 begins by writing: one barrier behind the
// reflector's grid_sum, like the one in front of the real kernel's grid_sum2.)
// Storage contracts, error word and completion tag exactly as above.
// ------------------------------------------------------------------------------------------
constexpr int ZHOUSE_NSCAL = 7;
constexpr int ZHOUSE_MAX_R2 = 32;      // rows per lane served (house.hip: the 40-row instantiations spill in the streaming loops)

template <int R2, bool MASKED>
__device__ __forceinline__ void zhouse_link(double2 (&w)[R2], double2 (&ring)[2][ChainShape<R2>::PB], const double2* __restrict__ v2,
                                            const double2* __restrict__ vn, const double bj, const int rem, unsigned& epoch,
                                            const HouseArgs& a, const int G, double* smd, unsigned* smu, const GridRole role) {
    constexpr int PB = ChainShape<R2>::PB;
    constexpr int NB = ChainShape<R2>::NB;
#define CH_OK(r) (!MASKED || (r) * CH_BS < rem)
    // ---- dot phase: conj(u_j) . w  (acc0 = re, acc1 = im) ----
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const double2* __restrict__ nx = (b + 1 < NB) ? v2 + (int64_t)(b + 1) * PB * CH_BS : v2;
#pragma unroll
        for (int i = 0; i < PB; ++i) ring[(b + 1) & 1][i] = nx[(int64_t)i * CH_BS];
        CH_ISSUE_FENCE();
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            double2 v = ring[b & 1][i];
            if (MASKED && !CH_OK(b * PB + i)) v = make_double2(0.0, 0.0);   // beyond the vector: whatever the block holds there
            const double2 wr = w[b * PB + i];
            acc0 = fma(v.x, wr.x, acc0);
            acc0 = fma(v.y, wr.y, acc0);
            acc1 = fma(v.x, wr.y, acc1);
            acc1 = fma(-v.y, wr.x, acc1);
        }
    }
    grid_sum2(acc0, acc1, epoch++, a.gran, G, a.err, smd, smu, role, a.xcc_res);
    if (a.debug == 4) acc0 *= 0.5;          // ... that leaves garbage behind
    const double cr = bj * acc0, ci = bj * acc1;
    // ---- update phase: w -= (beta_j d) u_j ----
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const double2* __restrict__ nx = (b + 1 < NB) ? v2 + (int64_t)(b + 1) * PB * CH_BS : vn;
#pragma unroll
        for (int i = 0; i < PB; ++i) ring[(b + 1) & 1][i] = nx[(int64_t)i * CH_BS];
        CH_ISSUE_FENCE();
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const double2 p = ring[b & 1][i];
            const int r = b * PB + i;
            const double tr = cr * p.x - ci * p.y;
            const double ti = cr * p.y + ci * p.x;
            w[r].x = CH_OK(r) ? w[r].x - tr : 0.0;
            w[r].y = CH_OK(r) ? w[r].y - ti : 0.0;
        }
    }
#undef CH_OK
}

template <int R2, bool MASKED>
__global__ __launch_bounds__(CH_BS) void k_zhouse_chain(HouseArgs a) {
    static_assert(R2 >= 2, "complex rows 0 .. 1023 are taken from the first two register rows");
    constexpr int PB = ChainShape<R2>::PB;
    __shared__ double smd[4 * (CH_BS / 64)];
    __shared__ unsigned smu[2 * CH_GMAX];
    __shared__ int slead;
    __shared__ double sbeta[2 * CH_BS];      // beta[0 .. k] (k + 2 <= 2 CH_BS)
    const int tid = threadIdx.x;
    const int G = gridDim.x;
    const int bid = blockIdx.x;
    const int k = a.k;
    for (int i = tid; i <= k; i += CH_BS) sbeta[i] = a.beta[i];      // (the barrier inside grid_role publishes them)
    const GridRole role = grid_role(a.xcc_leader, a.epoch0, &slead);
    // chunk2 == R2 * CH_BS: thread `tid` owns complex rows first + r*CH_BS, r < R2
    const int64_t first = (int64_t)bid * a.chunk2 + tid;
    const int64_t left = a.n2 - first;
    const int rem = (int)(left < 0 ? 0 : (left > a.chunk2 ? a.chunk2 : left));
#define CH_OK(r) (!MASKED || (r) * CH_BS < rem)
    double2 w[R2];
    double2 ring[2][PB];
    {
        const double2* __restrict__ win2 = reinterpret_cast<const double2*>(a.w_in) + first;
#pragma unroll
        for (int r = 0; r < R2; ++r) {
            const double2 v = win2[(int64_t)r * CH_BS];
            w[r].x = CH_OK(r) ? v.x : 0.0;
            w[r].y = CH_OK(r) ? v.y : 0.0;
            if ((r + 1) % 8 == 0) CH_ISSUE_FENCE();
        }
    }
    unsigned epoch = a.epoch0;
    if (a.debug == 4 && tid == 0) __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // tests: a faked timeout
    auto up = [&](int j) {
        while (j <= k && sbeta[j] == 0.0) ++j;
        return j;                                    // k + 1: none left
    };
    auto down = [&](int j) {
        while (j >= 0 && sbeta[j] == 0.0) --j;
        return j;                                    // -1: none left
    };
    auto col2 = [&](int j) { return reinterpret_cast<const double2*>(a.U + (int64_t)j * a.ldu) + first; };
    const int jtop = down(k);                        // the first backward link
    int j = up(0);
    {
        const double2* __restrict__ v2 = col2(jtop < 0 ? 0 : j);      // (no link at all: column 0, valid memory, never used)
#pragma unroll
        for (int i = 0; i < PB; ++i) ring[0][i] = v2[(int64_t)i * CH_BS];
        CH_ISSUE_FENCE();
    }
    while (j <= k) {
        const int jn = up(j + 1);
        zhouse_link<R2, MASKED>(w, ring, col2(j), col2(jn <= k ? jn : jtop), sbeta[j], rem, epoch, a, G, smd, smu, role);
        j = jn;
    }
    // ---- the new reflector (ring[0] keeps the first batch of the first backward column) ----
    if (bid == 0) {          // complex rows 0 .. k: rows 0 and 1 of workgroup 0 (k + 2 <= 2 CH_BS: the launcher)
        if (tid <= k) {
            a.hpin[2 * tid] = w[0].x;
            a.hpin[2 * tid + 1] = w[0].y;
        }
        if (tid + CH_BS <= k) {
            a.hpin[2 * (tid + CH_BS)] = w[1].x;
            a.hpin[2 * (tid + CH_BS) + 1] = w[1].y;
        }
    }
    // this thread's row r holds complex row k + 1 iff de == r * CH_BS, rows behind it iff de < r * CH_BS
    const int64_t de64 = (int64_t)(k + 1) - first;
    const int de = (int)(de64 < -1 ? -1 : de64);     // (every row is behind: the exact distance does not matter)
    double s2 = 0.0, gr = 0.0, gi = 0.0;
#pragma unroll
    for (int r = 0; r < R2; ++r) {
        const bool at = de == r * CH_BS, behind = de < r * CH_BS;
        const double qx = behind ? w[r].x : 0.0;
        const double qy = behind ? w[r].y : 0.0;
        s2 = fma(qx, qx, s2);
        s2 = fma(qy, qy, s2);
        gr = at ? w[r].x : gr;
        gi = at ? w[r].y : gi;
    }
    grid_sum2(gr, gi, epoch++, a.gran, G, a.err, smd, smu, role, a.xcc_res);
    s2 = grid_sum(s2, epoch++, a.gran, G, a.err, smd, smu, role, a.xcc_res);
    __syncthreads();         // (the next grid_sum2 begins with stores to the LDS words a slow wave of an XCD leader may still
                             // be reading as the last step of this grid_sum)
    // the scalar part, every thread for itself (utils.py:349-377, complex gamma)
    const double sigma = sqrt(s2);
    const double ag = hypot(gr, gi);                 // |gamma| (exactly |re| or |im| when the other part is zero)
    double v0r, v0i, xnorm, beta, alr, ali;
    if (sigma == 0.0) {
        v0r = 1.0;
        v0i = 0.0;
        xnorm = ag;
        alr = (ag == 0.0) ? 1.0 : gr / xnorm;
        ali = (ag == 0.0) ? 0.0 : gi / xnorm;
        beta = 0.0;
    } else {
        xnorm = sqrt(ag * ag + sigma * sigma);
        if (ag == 0.0) {
            v0r = -sigma;
            v0i = 0.0;
            alr = 1.0;
            ali = 0.0;
        } else {
            const double sgr = gr / ag, sgi = gi / ag;
            v0r = gr + sgr * xnorm;
            v0i = gi + sgi * xnorm;
            alr = -sgr;
            ali = -sgi;
        }
        beta = 2.0;
    }
    // (one division, as in the real kernel)
    const double sc = 1.0 / sqrt((v0r * v0r + v0i * v0i) + sigma * sigma);       // the root is >= 1 when sigma == 0, > 0 otherwise
    // link k + 1 of the descending pass on x = e_{k+1}: v^* e_{k+1} is the conjugate of the entry u_{k+1}[k+1] itself
    const double u0r = v0r * sc, u0i = v0i * sc;
    double dur = u0r, dui = -u0i;
    if (a.debug == 4) dur *= 0.5;          // ... that leaves garbage behind
    const double cr = beta * dur, ci = beta * dui;
    double2* __restrict__ un2 = reinterpret_cast<double2*>(a.unext) + first;
#pragma unroll
    for (int r = 0; r < R2; ++r) {
        const bool at = de == r * CH_BS, behind = de < r * CH_BS;
        double2 u;
        u.x = behind ? w[r].x * sc : (at ? u0r : 0.0);
        u.y = behind ? w[r].y * sc : (at ? u0i : 0.0);
        if (r * CH_BS < rem) st_nt2(un2 + (int64_t)r * CH_BS, u);
        const double tr = cr * u.x - ci * u.y;
        const double ti = cr * u.y + ci * u.x;
        w[r].x = (at ? 1.0 : 0.0) - tr;
        w[r].y = 0.0 - ti;
    }
    if (bid == 0 && tid == 0) {
        a.beta[k + 1] = beta;
        double* __restrict__ sc_out = a.hpin + 2 * (k + 1);
        sc_out[0] = gr;
        sc_out[1] = gi;
        sc_out[2] = s2;
        sc_out[3] = xnorm;
        sc_out[4] = alr;
        sc_out[5] = ali;
        sc_out[6] = beta;
    }
    j = jtop;
    while (j >= 0) {
        const int jn = down(j - 1);
        zhouse_link<R2, MASKED>(w, ring, col2(j), col2(jn >= 0 ? jn : 0), sbeta[j], rem, epoch, a, G, smd, smu, role);
        j = jn;
    }
    // V[:, k+1] = alpha_{k+1} x
    double2* __restrict__ vn2 = reinterpret_cast<double2*>(a.vnext) + first;
#pragma unroll
    for (int r = 0; r < R2; ++r) {
        if (r * CH_BS < rem) {
            double2 o;
            o.x = alr * w[r].x - ali * w[r].y;
            o.y = alr * w[r].y + ali * w[r].x;
            st_nt2(vn2 + (int64_t)r * CH_BS, o);
        }
    }
    if (bid == 0) {
        if (tid == 0) *a.errpin = __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        CH_SIGNAL_DONE(a);
    }
#undef CH_OK
}

}  // namespace kh
