/*
 * krylov_hip.h - C ABI of libkrylov_hip.so, the MI355X (gfx950) Krylov solver core.
 *
 * The reference (andrenarchy/krypy, pure Python) has no FFI: every flop of its
 * Arnoldi/Lanczos hot path is a NumPy/SciPy/OpenBLAS call.  This header is the
 * boundary the device core exposes in place of those calls; each entry point
 * names the reference call site it replaces (file:line under /root/reference).
 * The only caller is krypy_amd/_hip.py (ctypes); see INTEGRATION.md for the
 * binding a KryPy maintainer would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no C++/torch types cross the boundary.
 *  - every function returns 0 on success, a negative kh_status on failure and
 *    stores a message retrievable with kh_last_error() (thread-local).
 *  - handles are opaque; host pointers are caller-owned; device buffers are
 *    library-owned and released by kh_*_free / kh_ctx_destroy.
 *  - one HIP stream per context; a context is single-threaded by contract (like
 *    the reference).  Calls that return host scalars synchronise the stream
 *    before returning; all others are asynchronous on the context's stream.
 *  - all storage is fp64.  A kh_vec is a block of `ncols` column vectors of
 *    length n, each column contiguous and 256-byte aligned (leading dimension
 *    rounded up to 32 doubles): the reference's (N, k) ndarrays, stored
 *    column-major so that basis vectors stream at full HBM width.  A COMPLEX
 *    (c128) N-vector block is a kh_vec of length 2N (re, im interleaved) handed
 *    to the kh_z* entry points, which take complex coefficients as (re, im) pairs.
 *  - reductions are deterministic: fixed grid, fixed-order tree, no float atomics.
 */
#ifndef KRYLOV_HIP_H
#define KRYLOV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kh_ctx_s* kh_ctx;
typedef struct kh_mat_s* kh_mat;
typedef struct kh_vec_s* kh_vec;
typedef struct kh_proj_s* kh_proj;
typedef struct kh_tri_s* kh_tri;
typedef struct kh_ilu0_s* kh_ilu0;
typedef struct kh_bjac_s* kh_bjac;

typedef enum {
    KH_OK = 0,
    KH_ERR_HIP = -1,      /* a HIP runtime call failed (message has hipGetErrorString) */
    KH_ERR_ARG = -2,      /* invalid argument (shape mismatch, bad index, NULL handle) */
    KH_ERR_NOMEM = -3,    /* device or pinned-host allocation failed */
    KH_ERR_COMM = -4,     /* RCCL call failed */
    KH_ERR_UNSUPPORTED = -5
} kh_status;

/* Gram-Schmidt variants of kh_arnoldi_step */
typedef enum {
    KH_GS_MGS = 0,   /* reference order: for j: alpha=<v_j,w>; w-=alpha*b_j  (utils.py:1012-1029) */
    KH_GS_CGS = 1    /* panel form: h=V^T w; w-=B h  (one reduction per sweep)                     */
} kh_gs_mode;

/* ---- library / context ------------------------------------------------------------ */
const char* kh_last_error(void);
int kh_version(void);
int kh_device_count(int* count);
/* create a context on HIP device `device` (one stream, scratch for reductions).  One context = one device = one
 * process: N GPUs are N processes that join with kh_comm_init (the blueprint sketched (ndev, devs) here; with one
 * process per GPU a context never spans devices). */
int kh_ctx_create(int device, kh_ctx* out);
int kh_ctx_destroy(kh_ctx ctx);
int kh_ctx_sync(kh_ctx ctx);
/* info[0]=compute units, info[1]=total device memory (bytes), info[2]=free bytes, info[3]=reduction grid */
int kh_ctx_info(kh_ctx ctx, int64_t info[4]);
/* which Gram-Schmidt kernels ran so far on this context: [0] chain launches (k_mgs_chain*), [1] of
 * those with the column head parked in LDS, [2] of those with the operator fused into the prologue,
 * [3] register-resident panel sweeps (k_cgs_dots + k_cgs_update) */
int kh_ctx_counters(kh_ctx ctx, int64_t out[4]);
/* tuning knobs (0 keeps the default): reduction grid size, SpMV LDS tile (nnz) */
int kh_ctx_tune(kh_ctx ctx, int reduce_blocks, int spmv_tile);
/* named switches of a context (1 = on, the default; the environment variables of INTEGRATION.md set the
 * initial values): "spmv_dia" banded SpMV for stencil CSR operators, "chain" register-resident MGS chain,
 * "chain_lds" column head parked in LDS, "chain_spmv" operator fused into the chain prologue ("chain_xwin": its
 * mask form reads x through an LDS window; kh_ctx_get("n_chain_xwin") counts those launches), "chain_onex" short vectors
 * on one XCD, "chain_small" the column-ring kernel for them, "lanczos_fused" the three-pass Lanczos kernel, "tag_wait"
 * completion tags in pinned memory instead of an event per Arnoldi step, "house_chain" the one-launch Householder step
 * (kh_house_step_begin; 0: the caller's per-reflector path).  bench.py
 * uses it to time the CSR-stream and the banded SpMV kernel on the same operator.  Test-only switches (0 by
 * default): "chain_fault" the next chain launch fakes a timeout, "halo_loopback" a 1-rank communicator exchanges
 * the halo of a sharded operator with ITSELF (grouped ncclSend / ncclRecv to its own rank: the slab of an operator
 * that is periodic across the slab boundary) - the real exchange on one GPU. */
int kh_ctx_set(kh_ctx ctx, const char* key, int64_t value);
/* read a switch back, or a counter: "n_spmm" panel applications of a CSR operator that streamed the matrix
 * once (k_spmm_stream / k_spmm_dia), "n_chain_recovered" Arnoldi steps re-run on the per-column kernels after
 * a timeout of the chain kernel's grid-wide reduction, "n_spmv_split" sharded SpMVs run as interior / boundary
 * launches around the halo exchange, "n_halo_exchange" grouped ncclSend / ncclRecv exchanges issued */
int kh_ctx_get(kh_ctx ctx, const char* key, int64_t* value);
/* event timing on the context's stream (for bench.py's per-kernel roofline numbers) */
int kh_timer_start(kh_ctx ctx);
int kh_timer_stop(kh_ctx ctx, double* elapsed_ms);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI) ------------------------------- */
/* 128-byte ncclUniqueId; rank 0 creates it, the launcher broadcasts it to all ranks */
int kh_comm_unique_id(unsigned char id[128]);
int kh_comm_init(kh_ctx ctx, int rank, int nranks, const unsigned char id[128]);
int kh_comm_destroy(kh_ctx ctx);
/* in-place sum all-reduce of `count` host doubles through a device staging buffer (setup paths) */
int kh_comm_allreduce_host(kh_ctx ctx, double* vals, int64_t count);
/* xr - sums across the ranks of ONE node without a library call (csrc/xr.hip; replaces the ncclAllReduce of the inner
 * products of /root/reference/krypy/utils.py:182-183 on N ranks).  kh_xr_export allocates this rank's mailbox in
 * fine-grained device memory and returns its 64-byte hipIpcMemHandle_t; the launcher gathers the handles of all ranks
 * (rank order) and hands the 64 * nranks bytes to kh_xr_attach, which maps every peer's mailbox.  After EVERY rank has
 * attached successfully the launcher sets kh_ctx_set(ctx, "xr", 1) on all of them (the choice must be the same on every
 * rank): all-reduces of panels then run as one kernel of tagged 8-byte system-scope stores into the peers' mailboxes and
 * a rank-ordered sum (the same bits on every rank).  Works with or without an RCCL communicator (without one: sums
 * cross the ranks, halos do not).  A peer that does not arrive within KRYPY_AMD_XR_TIMEOUT_S (60) seconds is reported as
 * KH_ERR_COMM by the next call that synchronises with the host. */
int kh_xr_export(kh_ctx ctx, unsigned char handle[64]);
int kh_xr_attach(kh_ctx ctx, int rank, int nranks, const unsigned char* handles);
int kh_xr_detach(kh_ctx ctx);
/* xh - the halo of a block-row shard through the same kind of mailboxes: after kh_mat_set_halo, kh_mat_xh_export allocates this
 * shard's ghost GRANULES in fine-grained device memory and returns their 64-byte IPC handle; the launcher hands every rank its two
 * neighbours' handles (kh_mat_xh_attach: `prev_ng` / `next_ng` = the ghost entries nrecv_prev + nrecv_next of THEIR boxes, `prev_off`
 * = the previous rank's nrecv_prev; NULL = no such neighbour; self_loop = 1: the slab of an operator that is periodic across the slab
 * boundary, the rank is its own neighbour) and, after EVERY rank has attached, switches it on everywhere (kh_mat_xh_enable).  The
 * banded SpMV of the shard (the operator of /root/reference/krypy/utils.py:1593-1594 on this rank's rows) then stores its boundary
 * rows into the neighbours' granules and polls its own INSIDE its one launch: no ncclSend / ncclRecv kernel, no second stream. */
int kh_mat_xh_export(kh_ctx ctx, kh_mat A, unsigned char handle[64]);
int kh_mat_xh_attach(kh_ctx ctx, kh_mat A, const unsigned char* prev, int64_t prev_ng, int64_t prev_off, const unsigned char* next,
                     int64_t next_ng, int self_loop);
int kh_mat_xh_enable(kh_ctx ctx, kh_mat A, int on);
/* unmap the neighbours' granules again (every rank, when the collective decision about the in-launch halo is "off" after
 * some ranks had attached): a later kh_mat_xh_attach starts from scratch.  New component. */
int kh_mat_xh_detach(kh_ctx ctx, kh_mat A);
/* describe the halo of a block-row-sharded matrix: this rank sends `nsend_*` of its first/last
 * local rows to the previous/next rank and receives as many ghost entries from them.  After
 * this call kh_apply() on `A` exchanges halos (ncclSend/ncclRecv) before the local SpMV; the
 * matrix' column indices must address [local rows | ghosts from prev | ghosts from next]. */
int kh_mat_set_halo(kh_ctx ctx, kh_mat A, int64_t nsend_prev, int64_t nsend_next,
                    int64_t nrecv_prev, int64_t nrecv_next);
/* The LONGEST slab of the run this shard belongs to (every rank passes the same number).  Kernel choices of an Arnoldi step that
 * change the PATTERN of sums across the ranks - the one-reduction form, the blocked and the chain kernels with the sums inside
 * their launch - are made for it, so that every rank decides alike whatever the length of its own slab; keyed on the operator
 * (steps without an operator: kh_ctx_set "lowsync_rows" by local length).  New component: the reference is
 * single-process. */
int kh_mat_set_rows_max(kh_mat A, int64_t rows_max);
/* diagnostic: write the nrecv_prev + nrecv_next ghost entries directly (what the halo exchange would
 * deliver); lets a single process check a shard's SpMV against the global operator */
int kh_mat_set_ghost(kh_mat A, const double* values, int64_t count);
/* diagnostic: read the ghost entries back (what the last halo exchange delivered) */
int kh_mat_get_ghost(kh_mat A, double* values, int64_t count);

/* ---- vectors ---------------------------------------------------------------------- */
int kh_vec_alloc(kh_ctx ctx, int64_t n, int64_t ncols, kh_vec* out);   /* zero-filled */
int kh_vec_free(kh_vec v);
int kh_vec_shape(kh_vec v, int64_t* n, int64_t* ncols, int64_t* ld);
/* host <-> device; `host` is column-major with leading dimension host_ld (>= n) */
int kh_vec_upload(kh_vec v, int64_t col0, int64_t ncols, const double* host, int64_t host_ld);
int kh_vec_download(kh_vec v, int64_t col0, int64_t ncols, double* host, int64_t host_ld);
int kh_vec_zero(kh_vec v, int64_t col0, int64_t ncols);
int kh_vec_copy(kh_vec dst, int64_t dcol, kh_vec src, int64_t scol, int64_t ncols);
/* a few consecutive entries of one column (Householder Arnoldi reads/writes single elements:
 * utils.py:349-375, 973-983); synchronous */
int kh_vec_get(kh_vec v, int64_t col, int64_t i0, int64_t count, double* out);
int kh_vec_set(kh_vec v, int64_t col, int64_t i0, int64_t count, const double* in);
/* zero entries [i0, i0+count) of one column */
int kh_vec_zero_range(kh_vec v, int64_t col, int64_t i0, int64_t count);
/* diagnostic: *count = how many doubles of the block's padding - rows [n, ld) of every column and the slack the
 * allocation keeps behind the last column - are not +-0.0 (a NaN counts).  The kernels that run without a row
 * predicate rely on that padding being zero, and nothing else in this interface can read it (kh_vec_get and
 * kh_vec_download stop at row n).  Synchronous: waits for the stream, copies the padding strips to the host and counts
 * there. */
int kh_vec_padding_nonzero(kh_vec v, int64_t* count);

/* ---- operators (replace MatrixLinearOperator._dot -> A.dot(X), utils.py:1593-1594) --- */
/* CSR as SciPy holds it: int32 indptr[n_rows+1], int32 indices[nnz] (sorted or not), fp64 data.
 * n_cols may exceed n_rows for a sharded matrix with ghost columns. */
int kh_csr_upload(kh_ctx ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* indptr,
                  const int32_t* indices, const double* data, kh_mat* out);
/* dense row-major (C-ordered ndarray), leading dimension lda */
int kh_dense_upload(kh_ctx ctx, int64_t n_rows, int64_t n_cols, const double* a, int64_t lda,
                    kh_mat* out);
/* dense operator from a block already on the device: A = alpha X[:, col0 : col0 + n_rows]^T + beta I (row i of the
 * operator = column col0 + i of X).  With Y = G G^T formed by kh_apply's panel path the columns of the symmetric Y are
 * the rows of the row-major operator: BASELINE config 4's A = G G^T / n + I without a trip over the host
 * ("build on device or in blocks"; the reference gets its ndarray through get_linearoperator,
 * utils.py:241-259).  Synchronous. */
int kh_dense_from_block(kh_ctx ctx, kh_vec X, int64_t col0, int64_t n_rows, double alpha, double beta,
                        kh_mat* out);
/* diagonal operator (Jacobi M / Minv given as scipy.sparse.diags) */
int kh_diag_upload(kh_ctx ctx, int64_t n, const double* d, kh_mat* out);
int kh_mat_free(kh_mat A);
/* number of diagonals of the banded copy kh_csr_upload built for this operator (square, sorted
 * columns, no stored zeros, <= 32 diagonals at least 70 % full; KRYPY_AMD_SPMV_DIA=0 disables it),
 * 0 when the CSR kernel serves.  Same results bit for bit either way. */
int kh_mat_diagonals(kh_mat A);
/* Y[:, ycol:ycol+nc] = A * X[:, xcol:xcol+nc].  CSR rows are summed left to right in storage
 * order with separate multiply and add, i.e. bit-identical to scipy's csr_matvec(s) - for every row that fits the
 * kernel's LDS tile (2048 entries; kh_ctx_tune).  A longer row gets a workgroup of its own that adds its products as a
 * fixed tree: the same sum to rounding (tested at 1e-12), not the same bits. */
int kh_apply(kh_ctx ctx, kh_mat A, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol, int64_t ncols);

/* ---- inner products, norms, updates (utils.inner/norm utils.py:160-238) ------------- */
/* out[j] = <V[:, j0+j], W[:, wcol]>, j < ncols   (numpy.dot(X.T.conj(), Y), utils.py:183) */
int kh_dot_panel(kh_ctx ctx, kh_vec V, int64_t j0, int64_t ncols, kh_vec W, int64_t wcol,
                 double* out);
/* out (row-major nx*ny) = X[:, x0:x0+nx]^T Y[:, y0:y0+ny]   (utils.inner with a block on both sides, utils.py:160-193).
 * ny >= 2: 16 x 16 tiles on the FP64 matrix cores, both blocks read once per tile (k_gram_mfma; kh_ctx_set "gram_mfma" 0 /
 * KRYPY_AMD_GRAM_MFMA=0: one kh_dot_panel per column of Y).  Either way a fixed summation order: the same bits from run to run. */
int kh_gemm_tn(kh_ctx ctx, kh_vec X, int64_t x0, int64_t nx, kh_vec Y, int64_t y0, int64_t ny,
               double* out);
/* W[:, wcol] -= sum_j h[j] * V[:, j0+j], applied left to right, multiply then subtract
 * (the `Av -= alpha * V[:, [j]]` of utils.py:1027-1029) */
int kh_axpy_panel(kh_ctx ctx, kh_vec V, int64_t j0, int64_t ncols, const double* h, kh_vec W,
                  int64_t wcol);
/* Y[:, y0:y0+nc] = beta*Y[:, ...] + alpha * X[:, x0:x0+k] @ C  with C (k x nc) row-major.
 * (V[:, :k].dot(yy) linsys.py:947;  V.dot(c) utils.py:549;  Ritz.get_vectors deflation.py:845)
 * nc = 1: one k_multiaxpy pass, additions left to right.  nc = 2 ... 16: the block is read ONCE for all output columns on the FP64
 * matrix cores (k_panel_gemm_mfma, passes of 64 columns; kh_ctx_set "gram_mfma" 0: one pass over the block per output column). */
int kh_gemm_nn(kh_ctx ctx, kh_vec X, int64_t x0, int64_t k, const double* C, int64_t nc,
               double alpha, double beta, kh_vec Y, int64_t y0);
/* out = ||W[:, wcol]||_2   (numpy.linalg.norm(x, 2), utils.py:226) */
int kh_nrm2(kh_ctx ctx, kh_vec W, int64_t wcol, double* out);
/* Z[:, zcol] = alpha*X[:, xcol] + beta*Y[:, ycol]   (Z may alias X or Y) */
int kh_waxpby(kh_ctx ctx, kh_vec Z, int64_t zcol, double alpha, kh_vec X, int64_t xcol,
              double beta, kh_vec Y, int64_t ycol);
/* Z[:, zcol] = X[:, xcol] / s   (true division, as `V[:, [k+1]] = Av / H[k+1, k]` utils.py:1045) */
int kh_vdiv(kh_ctx ctx, kh_vec Z, int64_t zcol, kh_vec X, int64_t xcol, double s);

/* ---- fused hot path ------------------------------------------------------------------ */
/* One Arnoldi.advance() (utils.py:954-1048, mgs/dmgs/lanczos branches) entirely on the device:
 *   w = A V[:,k]           (skipped when A == NULL: W[:, wcol] already holds the operator result)
 *   lanczos (start==k>0):  w -= h_km1 * B[:,k-1]                      (utils.py:1000-1009)
 *   `sweeps` times, j=start..k:  alpha=<V_j,w>; hcol[j]+=alpha; w -= alpha*B_j   (1012-1029)
 *   hcol[k+1] = ||w||  or sqrt(<w, Md w>) when Md != NULL             (1030-1034)
 *   V[:,k+1] = (Md w | w)/hcol[k+1],  P[:,k+1] = w/hcol[k+1]          (1041-1045)
 * with B = P when P != NULL (preconditioned: V = M P) else V.  Md is a diagonal kh_mat or NULL.
 * hcol_out receives k+2 doubles (entries below `start` are zero).  The invariance test and the
 * Hessenberg/Givens algebra stay on the host (O(k)).  MW is an optional work column for Md*w.
 */
int kh_arnoldi_step(kh_ctx ctx, kh_mat A, kh_mat Md, kh_vec V, kh_vec P, kh_vec W, int64_t wcol,
                    int64_t k, int64_t start, int sweeps, int gs_mode, double h_km1,
                    double* hcol_out);
/* ---- deflation projector (utils.Projection._apply / apply_complement, utils.py:522-627) ------- */
/* Device image of a Projection with orthonormalised bases: W, V are (N, d) blocks, T = R^{-1} Q^H
 * and WRH = WR^H are d x d row-major host matrices (NULL = identity), copied to the device.  One
 * application z = a - P a is, per sweep, c = W^T z (panel product, all-reduced), c' = T c (tiny
 * device kernel), z -= V c' (panel update); <Y,a> = WRH c of the FIRST sweep is what the reference
 * returns as Ya.  Nothing goes through the host. */
int kh_proj_create(kh_ctx ctx, kh_vec W, kh_vec V, int64_t d, const double* T, const double* WRH,
                   int iterations, kh_proj* out);
int kh_proj_free(kh_proj p);
/* Z[:, zcol] = complement projection of A[:, acol]  (Z may be the same column: in place);
 * ya_out (d doubles, may be NULL) receives <Y, a>; synchronises only when ya_out != NULL */
int kh_proj_apply_complement(kh_ctx ctx, kh_proj p, kh_vec A, int64_t acol, kh_vec Z, int64_t zcol,
                             double* ya_out);

/* The same step split in two so that the host can process step k's Hessenberg column while the
 * device already runs step k+1 (whose kernels depend on device data only): _begin enqueues the
 * whole step plus an asynchronous copy of the H column into pinned slot `slot` (0..3) and records
 * an event; _end waits for that event only and returns `count` (= k+2) doubles.  With a
 * projector `proj` (deflated solvers: operator = (I - P) A, deflation.py:127-143) the projection is
 * applied to A v_k on the device and its d values <U, A v_k> (the new column of C) follow the H
 * column: count = k+2+d.  Steps begun in
 * order on one context execute in order.  A speculative step past convergence/invariance only
 * writes V[:,k+1] (P[:,k+1]) and the work vector; the caller discards it. */
int kh_arnoldi_step_begin(kh_ctx ctx, kh_mat A, kh_proj proj, kh_mat Md, kh_vec V, kh_vec P,
                          kh_vec W, int64_t wcol, int64_t k, int64_t start, int sweeps, int gs_mode,
                          double h_km1, int slot);
int kh_arnoldi_step_end(kh_ctx ctx, int slot, int64_t count, double* hcol_out);

/* One step of Householder Arnoldi (ortho='house': utils.py:970-994, House at utils.py:332-402) in ONE launch (k_house_chain,
 * krypy_amd/csrc/house.h).  W[:, wcol] holds A v_k (the caller applied the operator; it is not written).  Hv is the
 * reflector block: column j holds reflector j, zero above row j and normalised (what the reference keeps as House.v);
 * Beta is a one-column block of at least k + 2 rows that belongs to Hv's owner: Beta[j] = beta_j of reflector j (0 or 2;
 * the host sets entries of reflectors made elsewhere with kh_vec_set).  The launch applies reflectors 0 .. k to w in
 * ascending order (beta_j == 0: skipped), makes reflector k + 1 from rows k+1 .. N-1 of the result (written to Hv[:, k+1]
 * and Beta[k+1]), and stores V[:, k+1] = alpha_{k+1} H_0 ... H_{k+1} e_{k+1}.  _end returns count = k + 6 doubles:
 *   out[0 .. k]   rows 0 .. k of the reflected w, WITHOUT the factors conj(alpha_j) of utils.py:976 (the caller multiplies:
 *                 H[j, k] = out[j] * conj(alpha_j); no later reflector reads row j)
 *   out[k+1 ..]   gamma = w[k+1], sigma^2 = ||w[k+2:]||^2, xnorm (= H[k+1, k]), alpha_{k+1}, beta_{k+1}
 * Return values beside 0 and the negative kh_status codes: _begin returns KH_HOUSE_NOT_SERVED when this step is not served
 * by the kernel (kh_ctx_set "house_chain" 0, a communicator, more than 40 double2 rows per lane, k + 1 >= N, k + 2 > 1024, a
 * refused launch) - real data only: a kh_vec does not know whether it backs a complex block, the caller keeps
 * complex bases away from this entry (krypy_amd/_hip.py: Context.house_step checks the dtypes) -: nothing was enqueued, the caller applies the reflectors one by one.  _end returns KH_HOUSE_TIMED_OUT
 * when a grid-wide sum of the launch timed out (or the test switch "chain_fault" faked that): out is not written, column
 * k + 1 of Hv and V and Beta[k+1] hold garbage, W is intact - the caller re-runs the step on the per-reflector path, which
 * overwrites all three.  Counters (kh_ctx_get): "n_house_chain" launches, "n_house_recovered" timed-out steps. */
#define KH_HOUSE_NOT_SERVED 1
#define KH_HOUSE_TIMED_OUT 2
int kh_house_step_begin(kh_ctx ctx, kh_vec Hv, kh_vec Beta, kh_vec V, kh_vec W, int64_t wcol, int64_t k, int slot);
int kh_house_step_end(kh_ctx ctx, int slot, int64_t count, double* out);

/* The same step for complex (c128) data (utils.py:970-994 with a complex basis; House at utils.py:332-402, the scalar
 * branches at 349-377 with a complex gamma) in ONE launch (k_zhouse_chain, krypy_amd/csrc/house.h).  Hv, V and W are the
 * (re, im) views of complex blocks (length 2 N), Beta is a plain f64 vector as above: the factors are real.  The links are
 * d = conj(u_j) . w, w -= (beta_j d) u_j; reflector k + 1 has v0 = gamma + gamma / |gamma| xnorm, alpha = -gamma / |gamma|.
 * _end returns count = 2 (k + 1) + 7 doubles:
 *   out[0 .. 2k+1]   rows 0 .. k of the reflected w as (re, im) pairs, WITHOUT the factors conj(alpha_j)
 *   out[2k+2 ..]     Re gamma, Im gamma, sigma^2, xnorm (= H[k+1, k]), Re alpha_{k+1}, Im alpha_{k+1}, beta_{k+1}
 * KH_HOUSE_NOT_SERVED from _begin: kh_ctx_set "house_chain" 0, a spent recovery budget (three timed-out launches, shared
 * with the real step), a communicator, more than 32 double2 rows per lane (N > 32 * 512 * compute units complex rows:
 * 4,194,304 on 256 CUs - the 40-row class of the real step is not served here), k + 1 >= N, k + 2 > 1024, a refused launch.  KH_HOUSE_TIMED_OUT from _end as above.  Counter: "n_zhouse_chain" launches
 * ("n_house_chain" counts the real step only); "n_house_recovered" is shared. */
int kh_zhouse_step_begin(kh_ctx ctx, kh_vec Hv, kh_vec Beta, kh_vec V, kh_vec W, int64_t wcol, int64_t k, int slot);
int kh_zhouse_step_end(kh_ctx ctx, int slot, int64_t count, double* out);

/* A run of GMRES iterations in ONE call (krypy/linsys.py:951-997; SURVEY 8b "fused cycle"): Arnoldi steps
 * k0 .. k_stop-1 with look-ahead on the device (kh_arnoldi_step_begin / _end, slots k mod 4), and on the host - in C,
 * not in the caller's interpreter - what the reference does between two steps: the new Hessenberg column through the
 * previous Givens rotations and its own (BLAS drotg convention), R, the rotated right-hand side y and the residual
 * recurrence |y[k+1]|.  H and R are (ldh = ldr >= k_stop) row-major like the reference's arrays; cs holds (c, s) per
 * step; *h2_io the running squared Frobenius norm of H; *enq_io the number of steps begun on the device (in: steps the
 * caller has already begun, out: k_done + what is still in flight - at most step k_last is ever begun).
 * Stops  KH_CYCLE_TOL    after the step whose |y[k+1]| / bnorm <= tol (that step IS recorded),
 *        KH_CYCLE_CHECK  at a step whose H[k+1,k] / ||H||_F is not > 1e-14: maybe an invariant subspace - the step is
 *                        NOT recorded (its column stays in its slot for kh_arnoldi_step_end), the caller decides,
 *        KH_CYCLE_LIMIT  at k_stop.
 * *k_done = number of recorded steps (counted from 0). */
#define KH_CYCLE_LIMIT 0
#define KH_CYCLE_TOL 1
#define KH_CYCLE_CHECK 2
int kh_gmres_cycle(kh_ctx ctx, kh_mat A, kh_mat Md, kh_vec V, kh_vec P, kh_vec W, int64_t k0, int64_t k_stop,
                   int64_t k_last, int sweeps, int gs_mode, int64_t* enq_io, double tol, double bnorm, double* H, int64_t ldh,
                   double* R, int64_t ldr, double* cs, double* y, double* h2_io, double* resn, int64_t* k_done,
                   int* reason);

/* The Givens rotation the C host loops (kh_gmres_cycle, kh_minres_cycle) generate: by default the reference BLAS formula;
 * a caller whose own per-step loop uses its BLAS library's drotg (krypy/utils.py:426-427 through scipy.linalg.blas)
 * hands that function over - Fortran convention drotg(a, b, c, s), a and b overwritten - and gets the same bits from
 * both loops.  NULL restores the built-in formula. */
int kh_ctx_set_rotg(kh_ctx ctx, void (*drotg)(double* a, double* b, double* c, double* s));

/* A run of MINRES iterations in ONE call (krypy/linsys.py:791-853): Lanczos steps k0 .. k_stop-1 with look-ahead on the
 * device (kh_arnoldi_step_begin / _end, slots k mod 4; the basis may be a sliding WINDOW whose column 0 is logical
 * column `base`), and on the host in C what the reference does between two steps: the symmetric fill H[k-1,k] = H[k,k-1],
 * the new column through the two remembered Givens rotations and its own, the rotated right-hand side, and the vector
 * recurrences z = (v_k - R0 W0 - R1 W1)/R2; W <- [W1, z]; yk += y0 z as a DEFERRED update (kh_minres_update_deferred:
 * the next Lanczos launch carries it; call kh_minres_flush before yk is read).  H is (ldh >= k_stop) row-major like the
 * reference's array and receives the three entries of each recorded column.  st[0..3] = the two remembered rotations
 * (c, s) older first, st[4] = how many of them exist (0, 1, 2), st[5..6] = the rotated right-hand side (y[0], y[1]);
 * *wslot_io = the column of Wm that holds W0; *h2_io the running squared Frobenius norm of H; *enq_io as for
 * kh_gmres_cycle.  resn[k] = |y[k+1]| of every recorded step.  Stop reasons and *k_done as for kh_gmres_cycle. */
int kh_minres_cycle(kh_ctx ctx, kh_mat A, kh_mat Md, kh_vec V, kh_vec P, kh_vec W, int64_t k0, int64_t k_stop,
                    int64_t k_last, int64_t base, int64_t* enq_io, double tol, double bnorm, double* H, int64_t ldh,
                    kh_vec Wm, int* wslot_io, kh_vec YK, int64_t ycol, double* st, double* h2_io, double* resn,
                    int64_t* k_done, int* reason);

/* r = b - A x fused with its squared norm: R[:, rcol] = B[:, bcol] - A X[:, xcol]; *nrm = ||r||_2
 * (LinearSystem.get_residual linsys.py:156-160 for M = Ml = identity) */
int kh_residual(kh_ctx ctx, kh_mat A, kh_vec B, int64_t bcol, kh_vec X, int64_t xcol, kh_vec R,
                int64_t rcol, double* nrm);

/* One MINRES vector update (linsys.py:844-846):
 *   z = (V[:,k] - r0*W0 - r1*W1)/r2;   W0 <- W1;  W1 <- z;   yk += y0*z
 * Wk holds the two columns W0|W1 addressed through `slot` (the column that is W0 now and
 * receives z): no copies. */
int kh_minres_update(kh_ctx ctx, kh_vec V, int64_t k, kh_vec Wk, int slot, double r0, double r1,
                     double r2, double y0, kh_vec YK, int64_t ycol);
/* The same update, DEFERRED: it is carried by the next Lanczos step launch (kh_arnoldi_step_begin with a banded
 * operator: krypy_amd/csrc/lanczos.h - six independent streams in the shadow of that launch's last pass) or, failing
 * that, run by kh_minres_flush / the next kh_minres_update[_deferred] call.  Updates take effect in the order given.
 * Nothing but these entries reads W or yk in between: call kh_minres_flush before yk is used (krypy/linsys.py:844-847:
 * yk is needed only when an iterate is formed). */
int kh_minres_update_deferred(kh_ctx ctx, kh_vec V, int64_t k, kh_vec W, int slot, double r0, double r1, double r2,
                              double y0, kh_vec YK, int64_t ycol);
int kh_minres_flush(kh_ctx ctx);

/* One CG step after Ap is known (linsys.py:655-665), fused:
 *   yk += alpha*p;  r -= alpha*Ap;  z = Md r (or r);  *rho_new = <r, z>
 *   and, when beta_valid, nothing else; the direction update p = z + (rho_new/rho_old) p is
 *   kh_waxpby. */
int kh_cg_update(kh_ctx ctx, double alpha, kh_vec Pd, int64_t pcol, kh_vec AP, int64_t apcol,
                 kh_vec YK, int64_t ycol, kh_vec R, int64_t rcol, kh_mat Md, kh_vec Z, int64_t zcol,
                 double* rho_new);

/* One whole CG iteration (linsys.py:622-665) in one call, one host synchronisation:
 *   p = z + omega*p (skipped when `first`);  Ap = A p;  pAp = <p, Ap>;  alpha = rho / pAp (on the
 *   device);  yk += alpha p;  r -= alpha Ap;  z = Md r (z is r when Md == NULL);  rho_new = <r, z>
 * out[0] = <p, Ap>, out[1] = rho_new, out[2] = sanity word (KH_CG_* bits, 0 = fine): the step length is formed
 * on the device, so a divisor that is not a positive finite number is reported with the scalars; with a step length
 * that is not finite yk and r are left untouched.  omega = rho/rho_prev and rho are the host's values (the host
 * may have replaced rho by an explicit residual, linsys.py:667-669). */
#define KH_CG_NONFINITE_PAP 1     /* <p, Ap> (or the divisor formed from it) is inf / nan */
#define KH_CG_NONPOSITIVE_PAP 2   /* Re <p, Ap> <= 0: not a positive definite operator in this inner product */
#define KH_CG_NONFINITE_RHO 4     /* <r, z> is inf / nan */
#define KH_CG_NEGATIVE_RHO 8      /* <r, z> < 0: the preconditioner is not positive definite */
#define KH_CG_STEP_CLAMPED 16     /* rho / <p, Ap> is not finite although both are (a zero divisor): the device took NO step */
int kh_cg_step(kh_ctx ctx, kh_mat A, kh_mat Md, kh_vec Pd, int64_t pcol, kh_vec AP, int64_t apcol,
               kh_vec YK, int64_t ycol, kh_vec R, int64_t rcol, kh_vec Z, int64_t zcol, int first,
               double omega, double rho, double* out);

/* A run of CG iterations in ONE call (krypy/linsys.py:622-690): iterations k0 .. k_stop-1 of kh_cg_step with what the
 * reference does between two of them on the host in C - omega = rho_k / rho_{k-1}, rho_{k+1} = (sqrt |<r, z>|)^2 as the
 * caller forms it, the convergence test.  rhos[i] = rho after i iterations (in: rhos[k0] and, for k0 > 0, rhos[k0 - 1];
 * out: rhos[k0 + 1 ..]); trace receives six doubles per iteration: rho, d, <p, Ap>, <r, z>, the KH_CG_* sanity word,
 * sqrt(|<r, z>|).  (rho_{k+1} is libm's pow(sqrt |<r, z>|, 2.0), which is what `norm ** 2` on a NumPy scalar evaluates.)
 * Stops  KH_CYCLE_TOL    after the iteration whose sqrt(|<r, z>|) / bnorm <= tol (recorded; the caller finalises it),
 *        KH_CYCLE_CHECK  at an iteration that returned non-finite scalars from finite input (NOT recorded; yk and r are
 *                        as before it, the caller raises with the trace),
 *        KH_CYCLE_LIMIT  at k_stop.        *k_done = iterations recorded (counted from 0). */
int kh_cg_cycle(kh_ctx ctx, kh_mat A, kh_mat Md, kh_vec Pd, int64_t pcol, kh_vec AP, int64_t apcol, kh_vec YK, int64_t ycol,
                kh_vec R, int64_t rcol, kh_vec Z, int64_t zcol, int64_t k0, int64_t k_stop, double tol, double bnorm,
                double* rhos, double* trace, int64_t* k_done, int* reason);

/* ---- BiCGStab (real fp64; krypy_amd/csrc/bicgstab.hip) ------------------------------------ */
/* One iteration on the operator A^ = Ml A Mr, every elementwise expression rounded as written (r~ fixed for the solve):
 *   k > 0:  p = r + beta * (p - omega * v)
 *           v = A^ p ;  sigma = <r~, v> ;  alpha = rho / sigma          (formed on the device)
 *           s = r - alpha * v ;  ss = <s, s>
 *           t = A^ s ;  theta = <t, s> ;  phi = <t, t> ;  omega = theta / phi   (on the device)
 *           y = (y + alpha * p) + omega * s ;  r = s - omega * t ;  rho' = <r~, r> ;  rr = <r, r>
 * An alpha or omega that is not finite is clamped to 0 on the device: no vector receives inf / nan from finite input.  The
 * sums have a fixed order (no atomics) and are all-reduced over the ranks where they are formed.  All vectors are columns of
 * real device blocks of one length; a column that is written must differ from every column read (KH_ERR_ARG otherwise).
 * Sanity word beside the sums (0 = fine): */
#define KH_BICG_NONFINITE_SIGMA 1  /* <r~, v> is inf / nan */
#define KH_BICG_ALPHA_CLAMPED 2    /* rho and <r~, v> are finite but rho / <r~, v> is not (a zero divisor): the device took alpha = 0 */
#define KH_BICG_OMEGA_CLAMPED 4    /* <t, s> / <t, t> is not finite (t = 0 when s = 0: the regular early end): the device took omega = 0 */
#define KH_BICG_RHO_ZERO 8         /* <r~, r> of the new residual is 0 or not finite: the next beta cannot be formed */
/* p = r + beta * (p - omega * v) */
int kh_bicgstab_dir(kh_ctx ctx, kh_vec R, int64_t rcol, kh_vec P, int64_t pcol, kh_vec V, int64_t vcol, double beta,
                    double omega);
/* sigma = <r~, v>; alpha = rho / sigma (kept on the device for kh_bicgstab_full); s = r - alpha v.
 * out[0] = sigma, out[1] = <s, s>, out[2] = sanity word (NONFINITE_SIGMA, ALPHA_CLAMPED).  One host synchronisation. */
int kh_bicgstab_half(kh_ctx ctx, kh_vec RT, int64_t rtcol, kh_vec R, int64_t rcol, kh_vec V, int64_t vcol, kh_vec S,
                     int64_t scol, double rho, double* out);
/* theta = <t, s>, phi = <t, t>; omega = theta / phi; y = (y + alpha p) + omega s; r = s - omega t, with the alpha of the
 * kh_bicgstab_half call before it.  theta_known = 1: <t, s> already lies, complete, in the context's scratch scalar for it
 * (left there by an SpMV epilogue) and only phi is summed.  out[0] = theta, out[1] = phi, out[2] = rho', out[3] = rr,
 * out[4] = sanity word (OMEGA_CLAMPED, RHO_ZERO).  One host synchronisation. */
int kh_bicgstab_full(kh_ctx ctx, kh_vec RT, int64_t rtcol, kh_vec R, int64_t rcol, kh_vec P, int64_t pcol, kh_vec S,
                     int64_t scol, kh_vec T, int64_t tcol, kh_vec YK, int64_t ycol, int theta_known, double* out);
/* The whole iteration in one call and ONE host synchronisation (A real: CSR, dense or diagonal): the direction update
 * (skipped when `first`; beta, omega_prev are the host's), both applications of A, the two halves above.  rho = <r~, r>.
 * out[0..5] = sigma, ss, theta, phi, rho', rr; out[6] = sanity word; out[7] = 0 (reserved).  The same bits as
 * kh_bicgstab_dir, kh_apply, kh_bicgstab_half, kh_apply, kh_bicgstab_full(theta_known = 0) in a row. */
int kh_bicgstab_step(kh_ctx ctx, kh_mat A, kh_vec RT, int64_t rtcol, kh_vec R, int64_t rcol, kh_vec P, int64_t pcol, kh_vec V,
                     int64_t vcol, kh_vec S, int64_t scol, kh_vec T, int64_t tcol, kh_vec YK, int64_t ycol, int first,
                     double beta, double omega_prev, double rho, double* out);

/* ---- IDR(s) with bi-orthogonalisation (real fp64; krypy_amd/csrc/idrs.hip) ----------------- */
/* van Gijzen & Sonneveld 2011 with ONE block inner product per step (Collignon & van Gijzen 2011) on A^ = Ml A Mr.  Vectors:
 * the shadow space P, G and U (s columns each, 1 <= s <= KH_IDRS_SMAX; G = U = 0 at the start), r, y, and a scratch column t
 * that takes every operator product.  One ITERATION is one operator application; a cycle has the positions 0 .. s.  Every
 * elementwise expression is rounded as written, sums over j and i run in rising order, one term at a time:
 *   position k < s:  c_i = (f_i - sum_{j=k}^{i-1} M_ij c_j) / M_ii                                   i = k .. s-1
 *                    v = r ; v = v - c_i g_i ; u_k = om v ; u_k = u_k + c_i u_i  (i = k reads the old u_k)   i = k .. s-1
 *                    t = A^ u_k ;  h_i = <p_i, t>                                                     i = 0 .. s-1
 *                    a_i = (h_i - sum_{j<i} M_ij a_j) / M_ii                                          i = 0 .. k-1
 *                    g_k = t - a_i g_i ;  u_k = u_k - a_i u_i                                         i = 0 .. k-1
 *                    M_ik = h_i - sum_{j<k} M_ij a_j                                                  i = k .. s-1
 *                    beta = f_k / M_kk ;  r = r - beta g_k ;  y = y + beta u_k ;  rr = <r, r>
 *                    f_i = f_i - beta M_ik                                                            i = k+1 .. s-1
 *   position s:      t = A^ r ;  theta = <t, r> ;  phi = <t, t> ;  om = theta / phi
 *                    rho = theta / (sqrt(phi) sqrt(rr)) ;  if |rho| < 0.7:  om = (om 0.7) / |rho|
 *                    y = y + om r ;  r = r - om t ;  rr = <r, r> ;  f_i = <p_i, r>
 * Every scalar of this lives in the caller's scalar block SC: one zero-initialised column of at least KH_IDRS_NSCAL doubles
 * (layout: krypy_amd/csrc/idrs.h), and is formed on the device; the host gets one RECORD per step:
 * (rr, M_kk or theta, f_k or phi, flags).  A quotient that is not finite is clamped to 0 where it is formed: no vector
 * receives inf / nan from finite input.  After a step with sqrt(rr) / bnorm <= tol, or with a flag, a stop word in SC makes
 * every IDR kernel queued behind it return at once: P, G, U, r, y and the scalars stand where that step left them (operator
 * products queued behind it write t only).  Sums have a fixed order (no atomics) and are all-reduced over the ranks where
 * they are formed.  All columns are pairwise distinct columns of real device blocks of one length (KH_ERR_ARG otherwise). */
#define KH_IDRS_SMAX 8
#define KH_IDRS_RUN_MAX 64          /* positions of one kh_idrs_run call at most */
#define KH_IDRS_NSCAL 361
#define KH_IDRS_PIVOT_ZERO 1        /* M_kk is zero or not finite where beta or c_k divides by it */
#define KH_IDRS_OMEGA_CLAMPED 2     /* <t, t> = 0: theta / phi is not finite, the device took 0 */
#define KH_IDRS_OMEGA_ZERO 4        /* om = 0 after the correction while rr > 0: the next cycle could not move */
#define KH_IDRS_NONFINITE 8         /* a sum (h, theta, phi, f, rr) is inf / nan */
/* M = I, om = 1, f = P^T r, rr = <r, r>, stop word, counter and pending flags cleared; *rr_out = rr.  One host
 * synchronisation.  (G, U and y are the caller's to zero.) */
int kh_idrs_init(kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R, int64_t rcol,
                 kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, double* rr_out);
/* position k < s up to the operator: c, then u_k.  Clears the stop word and the counter.  The caller then forms t = A^ u_k
 * (column ucol + k of U into column tcol of T).  Nothing visits the host. */
int kh_idrs_dir(kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R, int64_t rcol,
                kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, int k);
/* position k < s from the operator product t on: h, a, g_k, u_k, M[k:, k], beta, r, y, rr, f.  rec[0..3] = the step's record.
 * One host synchronisation. */
int kh_idrs_orth(kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R, int64_t rcol,
                 kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, int k, double bnorm, double tol,
                 double* rec);
/* position s from t = A^ r on (the caller's product).  Clears the stop word and the counter first.  rec[0..3] = the record.
 * One host synchronisation. */
int kh_idrs_omega(kh_ctx ctx, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R, int64_t rcol,
                  kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, double bnorm, double tol, double* rec);
/* nsteps <= KH_IDRS_RUN_MAX consecutive positions from `pos` on (0 <= pos <= s, wrapping from s to 0) for a real kh_mat
 * (CSR, dense, diagonal), the operator applied in between, and ONE copy to the host at the end: out[0] = the number of steps
 * done (fewer than nsteps after a stop), out[1 + 4 i ..] = the record of step i.  out holds 1 + 4 * nsteps doubles.  The
 * stop word is cleared on entry: a caller who does not accept a stop calls again from the position after the last step
 * done.  The same bits as the pieces above with kh_apply in between. */
int kh_idrs_run(kh_ctx ctx, kh_mat A, kh_vec P, int64_t pcol, kh_vec G, int64_t gcol, kh_vec U, int64_t ucol, kh_vec R,
                int64_t rcol, kh_vec YK, int64_t ycol, kh_vec T, int64_t tcol, kh_vec SC, int s, int pos, int nsteps,
                double bnorm, double tol, double* out);

/* ---- complex (c128) twin of the hot path ------------------------------------------------- */
/* KryPy's kernels are dtype-generic NumPy (H/V are allocated with the common dtype of A, v, M:
 * utils.py:893-905, complex inner products are X^H Y: utils.py:183).  A complex N-vector block is
 * a REAL kh_vec of length 2N (interleaved re, im), allocated / copied / zeroed / normed / scaled
 * by a real with the entry points above; the entry points below are what is genuinely complex.
 * Complex scalars cross the ABI as (re, im) pairs of doubles. */
/* complex operators; kh_apply dispatches on the handle (X, Y are 2N-real views).  A square complex CSR operator whose
 * entries sit on 5 or 7 well-filled diagonals (a shifted stencil matrix) also gets a diagonal-major copy of (re, im) pairs:
 * the complex Arnoldi / Lanczos step then forms w = A v_k inside its Gram-Schmidt kernel - same bits as the SpMV launch. */
int kh_zcsr_upload(kh_ctx ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* indptr,
                   const int32_t* indices, const double* data_re_im, kh_mat* out);
int kh_zdense_upload(kh_ctx ctx, int64_t n_rows, int64_t n_cols, const double* a_re_im, int64_t lda,
                     kh_mat* out);
int kh_zdiag_upload(kh_ctx ctx, int64_t n, const double* d_re_im, kh_mat* out);
/* Z[:, zcol..] (complex view) = X[:, xcol..] (real) + 0i: NumPy's upcast of a real operand */
int kh_zfrom_real(kh_ctx ctx, kh_vec X, int64_t xcol, kh_vec Z, int64_t zcol, int64_t ncols);
/* out[2j], out[2j+1] = <V[:, j0+j], W[:, wcol]> = conj(v)^T w   (utils.py:183, ncols <= 512) */
int kh_zdot_panel(kh_ctx ctx, kh_vec V, int64_t j0, int64_t ncols, kh_vec W, int64_t wcol, double* out);
/* W[:, wcol] -= sum_j h[j] V[:, j0+j], complex h, left to right (utils.py:1029) */
int kh_zaxpy_panel(kh_ctx ctx, kh_vec V, int64_t j0, int64_t ncols, const double* h, kh_vec W,
                   int64_t wcol);
/* Y[:, y0..y0+nc) = beta*Y + X[:, x0..x0+k) C, C complex k x nc row-major (linsys.py:947) */
int kh_zgemm_nn(kh_ctx ctx, kh_vec X, int64_t x0, int64_t k, const double* C, int64_t nc, double beta,
                kh_vec Y, int64_t y0);
/* z = alpha*x + beta*y with complex alpha, beta */
int kh_zwaxpby(kh_ctx ctx, kh_vec Z, int64_t zcol, const double alpha[2], kh_vec X, int64_t xcol,
               const double beta[2], kh_vec Y, int64_t ycol);
/* Arnoldi.advance for complex data (utils.py:954-1048; mgs / dmgs / lanczos / panel CGS, Euclidean
 * inner product, no preconditioner): hcol_out receives k+2 complex numbers, the last (H[k+1,k], 0). */
int kh_zarnoldi_step(kh_ctx ctx, kh_mat A, kh_vec V, kh_vec W, int64_t wcol, int64_t k, int64_t start,
                     int sweeps, int gs_mode, const double h_km1[2], double* hcol_out);
/* ... and split for look-ahead like kh_arnoldi_step_begin: collect the column with
 * kh_arnoldi_step_end(ctx, slot, 2*(k+2), out).  h_km1[0] = NaN takes the Lanczos coefficient from
 * the previous slot's device-side column. */
int kh_zarnoldi_step_begin(kh_ctx ctx, kh_mat A, kh_vec V, kh_vec W, int64_t wcol, int64_t k,
                           int64_t start, int sweeps, int gs_mode, const double h_km1[2], int slot);
/* the complex twins of kh_proj_create / kh_proj_apply_complement (utils.py:604-627 with complex data) and the
 * complex step with the deflation projector inside it (deflation.py:127-143): T = R^{-1} Q^H and WRH = WR^H are
 * d x d row-major arrays of (re, im) pairs (NULL: identity); the step returns <U, A v_k> (d complex numbers) behind
 * the H column, like the real one */
int kh_zproj_create(kh_ctx ctx, kh_vec W, kh_vec V, int64_t d, const double* T, const double* WRH, int iterations,
                    kh_proj* out);
int kh_zproj_apply_complement(kh_ctx ctx, kh_proj p, kh_vec A, int64_t acol, kh_vec Z, int64_t zcol, double* ya_out);
int kh_zarnoldi_step_begin_proj(kh_ctx ctx, kh_mat A, kh_proj proj, kh_vec V, kh_vec W, int64_t wcol, int64_t k,
                                int64_t start, int sweeps, int gs_mode, const double h_km1[2], int slot);
/* The general complex step: Md = the Jacobi preconditioner as a complex diagonal (kh_zdiag_upload) with its second
 * block P (V = Md P, krypy/utils.py:1026-1045), W with two columns then; Md = P = NULL: as above. */
int kh_zarnoldi_step_begin_md(kh_ctx ctx, kh_mat A, kh_proj proj, kh_mat Md, kh_vec V, kh_vec P, kh_vec W, int64_t wcol,
                              int64_t k, int64_t start, int sweeps, int gs_mode, const double h_km1[2], int slot);
/* Complex kh_minres_update (krypy/linsys.py:844-846): z = (v_k - r0 W0 - r1 W1)/r2; W <- [W1, z]; yk += y0 z with
 * complex coefficients ((re, im) pairs), one pass. */
int kh_zminres_update(kh_ctx ctx, kh_vec V, int64_t k, kh_vec Wk, int slot, const double r0[2], const double r1[2],
                      const double r2[2], const double y0[2], kh_vec YK, int64_t ycol);
/* Complex kh_cg_step (krypy/linsys.py:622-665), one host synchronisation per iteration.  A complex; the vectors are
 * complex blocks (real kh_vec of length 2N); Md NULL or a REAL diagonal of length 2N (each Jacobi entry twice).
 * out[0] = d with step length alpha = rho / d = Re(rho / <p, Ap>), out[1] = <r, z>, out[2..3] = <p, Ap>,
 * out[4] = sanity word (KH_CG_* bits as for kh_cg_step). */
int kh_zcg_step(kh_ctx ctx, kh_mat A, kh_mat Md, kh_vec Pd, int64_t pcol, kh_vec AP, int64_t apcol, kh_vec YK,
                int64_t ycol, kh_vec R, int64_t rcol, kh_vec Z, int64_t zcol, int first, double omega, double rho,
                double* out);

/* ---- sparse triangular solves (incomplete-factorisation / Gauss-Seidel preconditioners) ------------------------------ */
/* All five entry points serve the M, Ml, Mr hooks of krypy/linsys.py (and ip_B): the factors of an ILU / IC / SSOR
 * preconditioner applied on the device.  No reference counterpart - the reference calls the user's function on host arrays.
 * The operator is T^{-1} for a sparse triangular T, by level scheduling (krypy_amd/csrc/tri.h, tri.hip): one thread per row,
 * s = b_i; s -= t_ij x_j in ascending column order (multiply and subtract rounded separately); x_i = s / t_ii - the bits of the
 * sequential row-by-row substitution.  A handle type of its own: a kh_tri is not a kh_mat and kh_apply never sees one. */
/* M / Ml / Mr hooks, no reference counterpart.  T as CSR with SORTED, duplicate-free int32 indices; lower != 0: lower triangle;
 * unit_diag != 0: the diagonal is 1 and a stored diagonal entry is ignored, else every row needs a non-zero diagonal entry.
 * The level analysis runs on the host here, O(nnz).  kh_ctx_set "tri_narrow_rows" (default 1024; read HERE): consecutive levels
 * of at most that many rows share one launch of one workgroup, every other level is one launch of its own.  KH_ERR_ARG: an
 * entry on the wrong side of the diagonal, a missing / zero diagonal, unsorted or duplicate indices; KH_ERR_NOMEM: an
 * allocation failed; KH_ERR_UNSUPPORTED: the context has a communicator (sharded triangular solves do not exist). */
int kh_tri_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data,
                  int lower, int unit_diag, kh_tri* out);
/* M / Ml / Mr hooks with complex data, no reference counterpart: the same with (re, im) pairs; NumPy's complex product and
 * quotient (Smith's formula), as kh_zcg_step. */
int kh_ztri_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                   int lower, int unit_diag, kh_tri* out);
/* M / Ml / Mr hooks, no reference counterpart: releases the device copy (waits for the stream first). */
int kh_tri_free(kh_tri t);
/* M / Ml / Mr hooks, no reference counterpart.  Y[:, ycol + c] = T^{-1} X[:, xcol + c], c < ncols (one column after the other).
 * X and Y may be the same columns (in place); ranges of one block that overlap without being identical are KH_ERR_ARG (a
 * column would overwrite a later right-hand side).  Rows [n, ld) of Y are not written.  Blocks of a complex handle are the (re, im) views of
 * length 2 n.  KH_ERR_ARG when the length of the blocks does not match (also: a real handle on complex blocks or the reverse).
 * Counters (kh_ctx_get): "n_tri_solve" columns solved, "n_tri_wide" / "n_tri_narrow" launches of the two kinds. */
int kh_tri_solve(kh_ctx ctx, kh_tri t, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol, int64_t ncols);
/* M / Ml / Mr hooks, no reference counterpart (diagnostics of the plan): out = n, nnz, levels, wide launches per solve, narrow
 * launches per solve, stored off-diagonal slots including padding, rows of the widest level, off-diagonal entries of the
 * longest row. */
int kh_tri_info(kh_tri t, int64_t out[8]);

/* ---- ILU(0) factorisation and the multicolour ordering ------------------------------------------------------------------- */
/* All three entry points serve the M, Ml, Mr hooks of krypy/linsys.py: they build, from A alone, the factors kh_tri_create
 * takes.  No reference counterpart - the reference calls the user's function on host arrays.  ILU(0) keeps the pattern of A
 * (krypy_amd/csrc/ilu0.h, ilu0.hip), in place on a copy a of the values, one thread per row, rows scheduled by the levels of
 * tril(A, -1):  for the entries p of row i with k = col[p] < i, ascending:  a[p] = a[p] / a[diagonal of row k];  for the entries
 * q of row i behind p whose column row k also holds (entry r):  a[q] = a[q] - a[p] * a[r]  (multiply and subtract rounded
 * separately) - the bits of the sequential row-by-row loop. */
/* M / Ml / Mr hooks, no reference counterpart.  A as CSR with SORTED, duplicate-free int32 indices and a structural diagonal
 * entry in every row (stored zeros belong to the pattern).  Uploads pattern, values and plan, factors on the device, downloads
 * the factored values into lu_out (the CSR positions of data: L strictly below the diagonal, its unit diagonal implied; U on and
 * above it) and frees everything.  info = n, nnz, levels, wide launches, narrow launches, rows of the widest level, entries of
 * the longest row, first row that broke down or -1.  A breakdown (a finished pivot that is zero or not finite) is NOT an error:
 * the call returns 0, info[7] is the smallest such row and lu_out holds what the sequential loop holds when it goes on.
 * kh_ctx_set "tri_narrow_rows" decides the two kinds of launch as for kh_tri_create.  KH_ERR_ARG (the row named): n or nnz out of
 * int32 range, unsorted or duplicate indices, a column out of range, a row without a diagonal entry; KH_ERR_NOMEM: an allocation
 * failed; KH_ERR_UNSUPPORTED: the context has a communicator (sharded factorisations do not exist).  Nothing stays allocated on
 * any way out.  Counters (kh_ctx_get): "n_ilu0_factor" calls, "n_ilu0_wide" / "n_ilu0_narrow" launches of the two kinds,
 * "ilu0_device_us" the device time of the last call's launches (HIP events around them). */
int kh_ilu0_factor(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data,
                   double* lu_out, int64_t info[8]);
/* M / Ml / Mr hooks with complex data, no reference counterpart: the same with (re, im) pairs; NumPy's complex product and
 * quotient (Smith's formula), as kh_ztri_create.  A pivot is zero when both parts are. */
int kh_zilu0_factor(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                    double* lu_out_re_im, int64_t info[8]);
/* M / Ml / Mr hooks, no reference counterpart (host only, no context): greedy colouring of the graph given as a CSR pattern - the
 * caller passes the pattern of A + A^T, a diagonal entry is ignored.  Rows in ascending order, each takes the smallest colour
 * that no already-coloured neighbour holds; color_out[i] in [0, *ncolors).  The multicolour ordering is the stable sort of the
 * rows by colour: rows of one colour do not depend on each other, so ILU(0) of the reordered matrix has at most *ncolors levels
 * per factor.  KH_ERR_ARG: n or nnz out of int32 range, a column out of range. */
int kh_multicolor(int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, int32_t* color_out, int64_t* ncolors);

/* ---- Persistent ILU(0) preconditioner: refactor and solve on the device ----------------------------------------------------- */
/* All six entry points serve the M, Ml, Mr hooks of krypy/linsys.py over a SEQUENCE of systems with one pattern (time steps,
 * Newton iterations): the analysis runs once, new values of A cost one upload and a few launches, the factors stay on the
 * device and the ordering is folded into the solves.  No reference counterpart - the reference calls the user's function on
 * host arrays.  With Ap = A[perm][:, perm] (perm NULL: Ap = A) the handle holds the ILU(0) factors L (unit lower) and U of Ap,
 * the bits of kh_ilu0_factor on Ap, as the two sliced-ELL images kh_tri_create would build for them (krypy_amd/csrc/ilu0p.h,
 * ilu0p.hip).  A handle type of its own: a kh_ilu0 is not a kh_mat and kh_apply never sees one. */
/* M / Ml / Mr hooks, no reference counterpart.  The PATTERN of A as CSR with SORTED, duplicate-free int32 indices and a structural
 * diagonal entry in every row; perm: new row r = old row perm[r], or NULL for the natural order; cplx != 0: values and blocks are
 * (re, im) pairs.  Everything that does not depend on values runs here, once, on the host: the pattern of Ap and the position
 * src[q] in the caller's value array of its entry q, the factorisation's plan (that of kh_ilu0_factor on Ap), the plans of L and
 * U (those of kh_tri_create) and the maps from Ap's value array into the two images.  kh_ctx_set "tri_narrow_rows" is read
 * HERE.  KH_ERR_ARG (the row named, in the caller's numbering): n or nnz out of int32 range, unsorted or duplicate indices, a
 * column out of range, a row without a diagonal entry, perm not a permutation of 0 .. n-1; KH_ERR_NOMEM: an allocation failed
 * (nothing half-built stays behind); KH_ERR_UNSUPPORTED: the context has a communicator.  Counter: "n_ilu0p_create". */
int kh_ilu0_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const int32_t* perm, int cplx,
                   kh_ilu0* out);
/* M / Ml / Mr hooks, no reference counterpart.  Factors the values data (the caller's CSR positions; (re, im) pairs for a complex
 * handle): ONE host-to-device copy of nnz values, then on the context's stream a gather a[q] = data[src[q]], the launches of
 * kh_ilu0_factor's contract on Ap (arithmetic and plan), and one kernel that writes the off-diagonal slots of both images and U's
 * diagonal through the maps.  The 4 bytes of the breakdown word are the only traffic back; no host analysis, no allocation, no
 * sort.  info as kh_ilu0_factor's: n, nnz, levels, wide launches, narrow launches, rows of the widest level, entries of the
 * longest row, first row that broke down IN THE NUMBERING OF Ap or -1.  A breakdown is NOT an error of the call, but the handle
 * is then not factored until a later refactorisation succeeds.  Counters (kh_ctx_get): "n_ilu0p_refactor" calls,
 * "ilu0p_h2d_bytes" / "ilu0p_d2h_bytes" / "ilu0p_refactor_us" of the last call (HIP events around gather, factorisation and
 * fill), "n_ilu0p_wide" / "n_ilu0p_narrow" launches of the two kinds (shared with kh_ilu0_solve). */
int kh_ilu0_refactor(kh_ctx ctx, kh_ilu0 h, const double* data, int64_t info[8]);
/* M / Ml / Mr hooks, no reference counterpart.  Y[perm[i], ycol + c] = (U^{-1} L^{-1} b')_i with b'_i = X[perm[i], xcol + c],
 * c < ncols (one column after the other) - the permutation inside the triangular kernels, compiled out for perm == NULL.  Per
 * row the arithmetic of kh_tri_solve, to the bit.  All launches of the L stage precede those of the U stage, so X and Y may be
 * the same columns; ranges of one block that overlap without being identical are KH_ERR_ARG.  Rows [n, ld) of Y are not
 * written.  KH_ERR_ARG: the handle is not factored (never refactored, or the last refactorisation broke down); another
 * context's handle; the length of the blocks does not match (also: a real handle on complex blocks or the reverse).  Counters:
 * "n_ilu0p_solve" columns, "n_ilu0p_wide" / "n_ilu0p_narrow" launches. */
int kh_ilu0_solve(kh_ctx ctx, kh_ilu0 h, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol, int64_t ncols);
/* M / Ml / Mr hooks, no reference counterpart (diagnostics and tests): downloads the factored values to the positions of the
 * caller's value array, lu_out[src[q]] = a[q] - L strictly below the diagonal of Ap, U on and above it.  KH_ERR_ARG on a handle
 * that is not factored. */
int kh_ilu0_values(kh_ilu0 h, double* lu_out);
/* M / Ml / Mr hooks, no reference counterpart (diagnostics of the plan): out = n, nnz, levels of the factorisation, wide launches
 * per refactorisation, narrow launches per refactorisation, levels of L, levels of U, wide launches per solve, narrow launches
 * per solve, stored slots of L including padding, stored slots of U, permuted (0 / 1), factored (0 / 1), device bytes held,
 * 0, 0 (reserved). */
int kh_ilu0_info(kh_ilu0 h, int64_t out[16]);
/* M / Ml / Mr hooks, no reference counterpart: releases everything the handle holds on the device (waits for the stream first). */
int kh_ilu0_free(kh_ilu0 h);

/* ---- Sparse approximate inverse on a fixed pattern ------------------------------------------------------------------------ */
/* M / Ml / Mr hooks, no reference counterpart: the preconditioner as a MATRIX, which kh_apply and the fused Arnoldi step take
 * like any other.  Row i of M minimises || e_i^T - m^T A[J, :] ||_2 over the values m at the pattern columns J of row i (at most 32;
 * so M minimises || I - M A ||_F on the pattern): normal equations by a root-free Cholesky factorisation, every multiply, add and
 * divide rounded on its own - the contract is in krypy_amd/csrc/spai.h, the result does not depend on how the device splits a row.
 * A (n, nnz, indptr, indices, data) and the pattern (pnnz, pindptr, pindices; n rows) as CSR with SORTED, duplicate-free int32
 * indices.  Uploads, launches ONCE (one group of lanes per row, the small matrices in LDS), downloads the values into m_out (the
 * CSR positions of the pattern; a row without pattern entries writes nothing) and frees everything.  info = n, pnnz, entries of
 * the longest pattern row, lanes per row, workgroups, LDS bytes per workgroup, reserved (0), first row that broke down or -1.
 * A breakdown (the rows of A a pattern row selects are linearly dependent: a pivot d_j that is not > 0 or not finite) is NOT an
 * error: the call returns 0, info[7] is the smallest such row and m_out holds what IEEE arithmetic makes of it.  KH_ERR_ARG (the
 * row named): n, nnz or pnnz out of int32 range, unsorted or duplicate indices in A or in the pattern, a column out of range, a
 * pattern row with more than 32 entries; KH_ERR_NOMEM: an allocation failed; KH_ERR_UNSUPPORTED: the context has a communicator
 * (sharded construction does not exist).  Nothing stays allocated on any way out.  Counters (kh_ctx_get): "n_spai_build" calls,
 * "spai_device_us" the device time of the last call's launch (HIP events around it). */
int kh_spai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t pnnz,
                  const int32_t* pindptr, const int32_t* pindices, double* m_out, int64_t info[8]);
/* M / Ml / Mr hooks with complex data, no reference counterpart: the same with (re, im) pairs; G = conj(A[J, :]) A[J, :]^T is
 * Hermitian, the product is (ac - bd, ad + bc), a complex value times or over a real pivot is taken part by part. */
int kh_zspai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                   int64_t pnnz, const int32_t* pindptr, const int32_t* pindices, double* m_out_re_im, int64_t info[8]);

/* ---- Factorized sparse approximate inverse on a fixed lower-triangular pattern --------------------------------------------- */
/* M / Ml / Mr hooks, no reference counterpart: for a Hermitian positive definite A = L L^H the sparse lower-triangular G ~ L^-1 on
 * a given pattern, so that M = G^H G is Hermitian positive definite BY CONSTRUCTION - the M of CG and MINRES, or Ml = G, Mr = G^H
 * of GMRES - and is applied as sparse products, which kh_apply and the fused steps take like any other matrix.  Every pattern row
 * i ends in column i; with its columns J (at most 32) the call computes u and d_i with A[J, J] = L D L^H (root-free Cholesky),
 * L^T u = e_last, d_i the last pivot; row i of G is u / sqrt(d_i), which is the CALLER's step (no square root on the device), and
 * G A G^H then has a unit diagonal.  Every multiply, add and divide is rounded on its own - the contract is in
 * krypy_amd/csrc/fsai.h, the result does not depend on how the device splits a row.  Only the LOWER triangle of A is read.
 * A (n, nnz, indptr, indices, data) and the pattern (pnnz, pindptr, pindices; n rows) as CSR with SORTED, duplicate-free int32
 * indices.  Uploads, launches ONCE (one group of lanes per row, the small matrices in LDS), downloads u into u_out (the CSR
 * positions of the pattern) and the n values d_i into d_out, and frees everything.  info = n, pnnz, entries of the longest pattern
 * row, lanes per row, workgroups, LDS bytes per workgroup, reserved (0), first row that broke down or -1.  A breakdown (A[J, J]
 * is not positive definite: a pivot d_j that is not > 0 or not finite) is NOT an error: the call returns 0, info[7] is the
 * smallest such row and the outputs hold what IEEE arithmetic makes of it (a NaN as 0x7ff8000000000000).  KH_ERR_ARG (the row
 * named): n, nnz or pnnz out of int32 range, unsorted or duplicate indices in A or in the pattern, a column out of range, an empty
 * pattern row, a pattern row that does not end in its diagonal, a pattern row with more than 32 entries; KH_ERR_NOMEM: an
 * allocation failed; KH_ERR_UNSUPPORTED: the context has a communicator (sharded construction does not exist).  Nothing stays
 * allocated on any way out.  Counters (kh_ctx_get): "n_fsai_build" calls, "fsai_device_us" the device time of the last call's
 * launch (HIP events around it). */
int kh_fsai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t pnnz,
                  const int32_t* pindptr, const int32_t* pindices, double* u_out, double* d_out, int64_t info[8]);
/* M / Ml / Mr hooks with complex data, no reference counterpart: the same with (re, im) pairs in data and u_out; d_out stays real
 * (n doubles).  The product is (ac - bd, ad + bc), a complex value times or over a real pivot is taken part by part; the back
 * substitution takes L unconjugated. */
int kh_zfsai_build(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                   int64_t pnnz, const int32_t* pindptr, const int32_t* pindices, double* u_out_re_im, double* d_out, int64_t info[8]);

/* ---- Block-Jacobi preconditioner: blocks inverted and applied on the device ------------------------------------------------- */
/* All entry points serve the M, Ml, Mr hooks of krypy/linsys.py; no reference counterpart (the reference calls the user's
 * function on host arrays).  For a partition of 0 .. n into nblk consecutive ranges blkptr[0 .. nblk] (blkptr[0] = 0,
 * blkptr[nblk] = n, strictly increasing, every block of 1 .. 32 rows) the handle holds the inverses of the diagonal blocks
 * A[blkptr[g] : blkptr[g+1], blkptr[g] : blkptr[g+1]] on the device, in the layout its apply kernel reads.  A handle type of its
 * own: a kh_bjac is not a kh_mat and kh_apply never sees one.  Contract (the order of every operation), layout and kernels:
 * krypy_amd/csrc/bjac.h, bjac.hip. */
/* M / Ml / Mr hooks, no reference counterpart.  A (n, nnz, indptr, indices, data) as CSR with SORTED, duplicate-free int32
 * indices; stored zeros are kept, entries a block's rows do not store are 0.  Validates, uploads, and inverts ALL blocks in ONE
 * launch: one block per group of W lanes (W the smallest of 1, 2, 4, 8, 16, 32 that holds the largest block), Gauss-Jordan
 * elimination with row pivoting (pivot: the largest |re| + |im| of the column at or below the diagonal, the smallest row among
 * equals, a NaN counting as the largest), every multiply, add and divide rounded on its own, complex products as
 * (ac - bd, ad + bc), 1 / pivot by Smith's formula.  info = n, nnz, nblk, rows of the largest block, W, workgroups of the build
 * launch, device bytes held, smallest block that is BROKEN or -1.  A block is broken when a pivot is 0 or not finite; that is
 * NOT an error of the call: it returns 0 and the inverse holds what IEEE arithmetic makes of it.  KH_ERR_ARG (the row or the
 * block named): n, nnz or nblk out of int32 range, unsorted or duplicate indices, a column out of range, a blkptr that does not
 * start at 0, does not end at n, is not strictly increasing or has a block above 32 rows; KH_ERR_NOMEM: an allocation failed
 * (nothing stays allocated on any way out); KH_ERR_UNSUPPORTED: the context has a communicator.  Counters (kh_ctx_get):
 * "n_bjac_build" build launches, "bjac_device_us" the device time of the last one (HIP events around it). */
int kh_bjac_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data, int64_t nblk,
                   const int32_t* blkptr, kh_bjac* out, int64_t info[8]);
/* M / Ml / Mr hooks with complex data, no reference counterpart: the same with (re, im) pairs; the handle is then complex. */
int kh_zbjac_create(kh_ctx ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices, const double* data_re_im,
                    int64_t nblk, const int32_t* blkptr, kh_bjac* out, int64_t info[8]);
/* M / Ml / Mr hooks, no reference counterpart.  New values at the SAME CSR positions ((re, im) pairs for a complex handle): one
 * upload, the build launch again, nothing re-analysed or allocated; kh_bjac_info then gives the refreshed info. */
int kh_bjac_update(kh_bjac h, const double* data);
/* M / Ml / Mr hooks, no reference counterpart: the info block of kh_bjac_create as of the last build. */
int kh_bjac_info(kh_bjac h, int64_t info[8]);
/* M / Ml / Mr hooks, no reference counterpart.  Y[:, ycol + c] = D^-1 X[:, xcol + c], c < ncols, one launch per column:
 * y_i = ((0 + b[i][0] x_0) + b[i][1] x_1) + ... over the columns of row i's block in rising order, separate multiply and add -
 * the bits of kh_apply with the block-diagonal CSR matrix that stores every entry of every inverse.  Complex handles take the
 * (re, im) views of length 2 n.  Rows [n, ld) of Y are not written.  KH_ERR_ARG: another context's handle; the length of the
 * blocks does not match (also: a real handle on complex blocks or the reverse); X and Y the same block with overlapping column
 * ranges (the kernel does not work in place).  A handle with a broken block is applied as it is.  Counter: "n_bjac_apply"
 * columns. */
int kh_bjac_apply(kh_ctx ctx, kh_bjac h, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol, int64_t ncols);
/* M / Ml / Mr hooks, no reference counterpart (diagnostics, tests, the matrix form): downloads the inverses as dense row-major
 * m_g x m_g arrays, one after another in block order (sum of m_g^2 values, (re, im) pairs for a complex handle), whatever the
 * device layout is. */
int kh_bjac_values(kh_bjac h, double* out);
/* M / Ml / Mr hooks, no reference counterpart: releases everything the handle holds on the device (waits for the stream first). */
int kh_bjac_free(kh_bjac h);

/* ---- Chebyshev polynomial preconditioner -------------------------------------------------------------------------------- */
/* Both entry points serve the M, Ml, Mr hooks of krypy/linsys.py: z = p(A) r as m steps of the Chebyshev iteration for A z = r
 * from z = 0, for a Hermitian positive definite A with spectrum in [lmin, lmax] (of Dinv A when scaled).  No reference
 * counterpart - the reference calls the user's function on host arrays.  The caller computes the m pairs (a_k, b_k) on the host:
 *   theta = (lmax + lmin) / 2; delta = (lmax - lmin) / 2; sigma = theta / delta; rho_0 = 1 / sigma; (a_0, b_0) = (0, 1 / theta);
 *   rho_k = 1 / (2 sigma - rho_{k-1}); (a_k, b_k) = (rho_k rho_{k-1}, 2 rho_k / delta).
 * Per row, every multiply and add rounded on its own (krypy_amd/csrc/cheb.hip):
 *   step 0:      t = r_i;            [t = t * dinv_i;]  d_i = b_0 * t;                  z_i = d_i
 *   step k >= 1: t = r_i - (A z)_i;  [t = t * dinv_i;]  d_i = (a_k * d_i) + (b_k * t);  z_i = z_i + d_i
 * Complex blocks are their (re, im) views of length 2 N; the scalars and dinv (length 2 N, every entry twice) are real. */
/* M / Ml / Mr hooks, no reference counterpart: one composed step on single columns.  first != 0: step 0 (AZ, Zin, a unused,
 * may be NULL; d and z_out are only written); else AZ[:, azcol] holds A z_in.  Dinv: a real diagonal kh_mat of the blocks'
 * length, or NULL.  z_in may be z_out; r, d, z_out (and Az) are different columns.  Rows [n, ld) are not written.  KH_ERR_ARG:
 * lengths differ, Dinv is no diagonal of that length, columns coincide.  Counter: "n_cheb_update". */
int kh_cheb_update(kh_ctx ctx, kh_vec AZ, int64_t azcol, kh_vec R, int64_t rcol, kh_mat Dinv, kh_vec D, int64_t dcol, kh_vec Zin,
                   int64_t zincol, kh_vec Zout, int64_t zoutcol, double a, double b, int first);
/* M / Ml / Mr hooks, no reference counterpart.  Y[:, ycol + c] = p(A) X[:, xcol + c], c < ncols (one column after the other): all
 * m steps for a kh_mat operator in one call, m - 1 operator applications per column.  coef: m pairs (a_k, b_k).  S: a
 * caller-owned scratch block of the same length with at least 2 columns (d and the other half of the z ping-pong; the last
 * step lands in Y), 3 on the composed path (A z); its contents on entry do not matter.  Steps k >= 1 are ONE launch each - the
 * SpMV with the step in its epilogue - when A is a real CSR handle without halo, the context has no communicator, and
 * kh_ctx_set "cheb_fused" (default 1) is on; otherwise kh_apply + the update kernel: the same bits.  KH_ERR_ARG: m < 1; A not
 * square; lengths differ (also: a real handle on complex blocks or the reverse); Dinv is no real diagonal of the blocks'
 * length; S has too few columns; X and Y overlap (r is read in every step); S is X or Y.
 * Counters (kh_ctx_get): "n_cheb_apply" columns applied, "n_cheb_fused" fused launches, "n_cheb_update" update launches. */
int kh_cheb_apply(kh_ctx ctx, kh_mat A, kh_mat Dinv, int m, const double* coef, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol,
                  int64_t ncols, kh_vec S);

/* ---- GMRES polynomial preconditioner ------------------------------------------------------------------------------------ */
/* Both entry points serve the Ml, Mr hooks of krypy/linsys.py: y = p(A) x with p(A) ~ A^-1 in the product form of Loe & Morgan
 * (the roots of 1 - z p(z) are harmonic Ritz values of A, real ones as linear factors, conjugate pairs as real quadratic ones).
 * No reference counterpart - the reference calls the user's function on host arrays.  The caller computes and orders the roots
 * on the host and hands over a table of steps, five doubles (kind, c, a2, close, cl) each, ONE operator application per step.
 * Per row, with s = (A in)_i, every multiply and add rounded on its own (krypy_amd/csrc/poly.hip):
 *   kind 0 LIN   (in = prod):  y_i = y_i + (c * in_i);                      out_i = in_i - (c * s)      c = 1 / theta
 *   kind 1 QA    (in = prod):  t = (a2 * in_i) - s;  y_i = y_i + (c * t);   out_i = t                   a2 = 2 Re theta, c = 1 / |theta|^2
 *   kind 2 QB    (in = t):                                                  out_i = prod_i - (c * s)
 *   kind 3 SCALE (alone):      y_i = c * x_i
 *   the first step takes x as prod and does not read y;  close != 0 (LIN, QB): additionally y_i = y_i + (cl * out_i).
 * Real operators on real blocks only. */
/* Ml / Mr hooks, no reference counterpart: one composed step on single columns.  SO[:, socol] holds A in on entry and out on
 * exit (unused by SCALE, may be NULL); P[:, pcol] is prod of a QB step (NULL otherwise); first != 0: y is only written.  in,
 * prod, y and s/out are different columns.  Rows [n, ld) are not written.  KH_ERR_ARG: a kind outside 0 - 3; close on QA or
 * SCALE; QB as the first step; lengths differ; columns coincide.  Counter: "n_poly_update". */
int kh_poly_update(kh_ctx ctx, kh_vec In, int64_t incol, kh_vec P, int64_t pcol, kh_vec Y, int64_t ycol, kh_vec SO, int64_t socol,
                   int kind, double c, double a2, double cl, int first, int close);
/* Ml / Mr hooks, no reference counterpart.  Y[:, ycol + c] = p(A) X[:, xcol + c], c < ncols (one column after the other): all
 * nsteps steps for a kh_mat operator in one call.  steps: nsteps x 5 doubles, row-major.  S: a caller-owned scratch block of the
 * same length with at least 3 columns (prod ping-pongs between 0 and 1, t lives in 2); its contents on entry do not matter, and
 * neither do Y's.  X is never written.  Every step is ONE launch - the SpMV with the step in its epilogue - when A is a real CSR
 * handle without halo, the context has no communicator, and kh_ctx_set "poly_fused" (default 1) is on; otherwise kh_apply + the
 * update kernel: the same bits.  KH_ERR_ARG: nsteps < 1; A diagonal, complex or not square; lengths differ; S has fewer than 3
 * columns; X and Y overlap; S is X or Y; a kind outside 0 - 3; close on a QA step; a SCALE step that does not stand alone; a QB
 * step not preceded by QA.
 * Counters (kh_ctx_get): "n_poly_apply" columns applied, "n_poly_fused" fused launches, "n_poly_update" update launches. */
int kh_poly_apply(kh_ctx ctx, kh_mat A, int nsteps, const double* steps, kh_vec X, int64_t xcol, kh_vec Y, int64_t ycol,
                  int64_t ncols, kh_vec S);

/* ---- measurement ----------------------------------------------------------------------- */
/* bench.py's roofline numbers: average duration (ms) of `reps` back-to-back launches of one hot
 * kernel, HIP events on the context's stream.  which: 0 Gram-Schmidt link (axpy+dot),
 * 1 multidot<16>, 2 multiaxpy<16>, 3 link with norm tail, 4 scale-and-store, 5 register-resident
 * MGS chain (16 columns x 4 sweeps = 64 links per launch; 6/7: without the grid reduction / the
 * reduction alone), 8 register-resident panel GS over 16 columns (k_cgs_dots + k_reduce_partials +
 * k_cgs_update).  V needs >= 17 columns, W 2 columns. */
int kh_bench_kernel(kh_ctx ctx, int which, kh_vec V, kh_vec W, int reps, double* avg_ms);
/* The solver's own launch sequence (what Gmres._solve / kh_gmres_cycle enqueue, utils.py:954-1048 once per k):
 * `reps` times the Arnoldi steps k = 0 .. m-1 on V (>= m+1 columns, column 0 a unit vector), one step of look-ahead,
 * columns fetched in order.  avg_step_ms = HIP-event time / (reps * m).  With a banded operator and vectors that
 * fit the register file each step is ONE launch of the fused chain kernel: its average duration over k+1 = 1 .. m
 * Gram-Schmidt links is the `roofline.avg_launch_ms` of bench.py. */
int kh_bench_arnoldi(kh_ctx ctx, kh_mat A, kh_vec V, kh_vec W, int64_t m, int gs_mode, int reps,
                     double* avg_step_ms);

#ifdef __cplusplus
}
#endif
#endif /* KRYLOV_HIP_H */
