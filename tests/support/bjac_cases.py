"""Cases of the block-Jacobi tests, shared by tests/test_bjac_host.py (NumPy double) and tests/test_gpu_bjac.py (device) - TEST
INFRASTRUCTURE ONLY.  Every case is a CSR matrix with sorted, duplicate-free indices and a partition; the expectation is always
tests/support/bjac_ref.py on the same inputs."""
import numpy as np
import scipy.sparse as sp

from tests.support.bjac_ref import group_width

UNIFORM_SIZES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32]      # every group width at its full size and one above the width below


def canonical(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def uniform_ptr(n, bs):
    return np.concatenate([np.arange(0, n, bs), [n]]).astype(np.int32)


def uniform_counts(bs):
    """Numbers of blocks around a wave's 64 / W and a workgroup's 256 / W."""
    W = group_width(bs)
    return sorted({c for c in (1, 64 // W - 1, 64 // W, 64 // W + 1, 256 // W + 1) if c > 0})


def random_block(rng, m, cplx):
    """The generator's block: standard normal entries and a diagonal shift of 2, which keeps most blocks comfortably regular
    without making the pivots trivial (many steps still swap)."""
    B = rng.standard_normal((m, m))
    if cplx:
        B = B + 1j * rng.standard_normal((m, m))
    return B + 2.0 * np.eye(m)


def block_system(blkptr, seed, cplx, off=2):
    """Dense random diagonal blocks on the partition plus ``off`` random entries per row anywhere (those that fall into a
    diagonal block add to it)."""
    rng = np.random.RandomState(seed)
    n = int(blkptr[-1])
    rows, cols, vals = [], [], []
    for g in range(len(blkptr) - 1):
        b0, b1 = int(blkptr[g]), int(blkptr[g + 1])
        B = random_block(rng, b1 - b0, cplx)
        i, j = np.meshgrid(np.arange(b0, b1), np.arange(b0, b1), indexing="ij")
        rows.append(i.ravel())
        cols.append(j.ravel())
        vals.append(B.ravel())
    if off and n > 1:
        r = np.repeat(np.arange(n), off)
        rows.append(r)
        cols.append(rng.randint(0, n, r.size))
        v = 0.25 * rng.standard_normal(r.size)
        vals.append(v + 0.25j * rng.standard_normal(r.size) if cplx else v)
    dt = np.complex128 if cplx else np.float64
    A = sp.csr_matrix((np.concatenate(vals).astype(dt), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return canonical(A)


def uniform_case(bs, nblk, cplx):
    """``nblk`` blocks of ``bs`` rows, ``n`` one short of the multiple: the last block is shorter (not for bs = 1)."""
    n = nblk * bs - 1 if bs > 1 and nblk * bs > 1 else nblk * bs
    ptr = uniform_ptr(n, bs)
    return block_system(ptr, 1000 * bs + nblk, cplx), ptr


def cycle_ptr(nblk=70):
    """Sizes 1, 2, ..., 32, 1, 2, ..."""
    return np.concatenate([[0], np.cumsum([1 + g % 32 for g in range(nblk)])]).astype(np.int32)


def lone_32_ptr():
    """One block of 32 between blocks of 1."""
    return np.concatenate([[0], np.cumsum([1] * 5 + [32] + [1] * 5)]).astype(np.int32)


def from_blocks(blocks, cplx, between=0.0):
    """The block-diagonal matrix of the given dense blocks (zeros inside a block are NOT stored) and its partition;
    ``between`` != 0 adds that value at (i, i + m) and (i + m, i) style couplings outside the blocks."""
    dt = np.complex128 if cplx else np.float64
    A = sp.block_diag([sp.csr_matrix(np.asarray(B, dtype=dt)) for B in blocks], format="lil", dtype=dt)
    n = A.shape[0]
    if between:
        for i in range(n):
            A[i, (i + 37) % n] = A[i, (i + 37) % n] + between
    ptr = np.concatenate([[0], np.cumsum([np.shape(B)[0] for B in blocks])]).astype(np.int32)
    return canonical(A.tocsr()), ptr


def _z(B, cplx, rng):
    """a complex companion of a real block with the same magnitudes |re| + |im|: the entry split between the two parts"""
    B = np.asarray(B, dtype=float)
    if not cplx:
        return B
    t = rng.choice([0.0, 0.25, 0.5, 1.0], B.shape)          # (exact splits: equal magnitudes stay exactly equal)
    return B * t + 1j * B * (1.0 - t) * rng.choice([-1.0, 1.0], B.shape)


def pivot_cases(cplx):
    """name -> (A, blkptr).  antidiagonal: a swap at every step; ties: equal magnitudes in a column (the smallest row must
    win); tiny: a diagonal entry of 1e-300 beside entries of order 1 (without the swap the inverse is garbage)."""
    rng = np.random.RandomState(11)
    anti = [np.fliplr(np.diag(rng.uniform(1.0, 2.0, m))) for m in (2, 3, 5, 8, 13, 32)]
    H4 = np.array([[1.0, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]])
    ties = [H4, np.kron(H4, H4[:2, :2]), np.array([[2.0, 1], [-2, 1]]), np.array([[1.0, 3, 0], [-1, 1, 2], [1, 0, 5]])]
    tiny = [np.array([[1e-300, 1.0], [1.0, 1.0]]), np.array([[1e-300, 2.0, 1.0], [1.0, 1e-300, 3.0], [2.0, 1.0, 1e-300]]),
            np.array([[1.0, 2.0], [3.0, 1e-300]])]
    out = {}
    for name, blocks in (("antidiagonal", anti), ("ties", ties), ("tiny", tiny)):
        out[name] = from_blocks([_z(B, cplx, rng) for B in blocks], cplx, between=0.5)
    return out


def extraction_case(cplx):
    """One matrix with blocks of 5: block 0 tridiagonal (in-block entries missing), block 1 dense with 40 entries left and
    right of it in every row, block 2 with a row that has entries outside the block only (broken), block 3 dense, block 4 with
    an empty row (broken), block 5 diagonal, block 6 dense with a NaN (broken), block 7 dense.  Returns (A, blkptr, broken
    blocks)."""
    rng = np.random.RandomState(5)
    m, nblk = 5, 20
    n = m * nblk
    dt = np.complex128 if cplx else np.float64
    A = sp.lil_matrix((n, n), dtype=dt)

    def val(shape=None):
        v = rng.standard_normal(shape)
        return v + 1j * rng.standard_normal(shape) if cplx else v

    def put(g, B):
        A[g * m:(g + 1) * m, g * m:(g + 1) * m] = B

    put(0, np.diag(val(m) + 3) + np.diag(val(m - 1), 1) + np.diag(val(m - 1), -1))
    put(1, val((m, m)) + 2 * np.eye(m))
    for i in range(m, 2 * m):
        for c in list(range(0, 5)) + list(range(2 * m, 2 * m + 75)):
            A[i, c] = val()
    B2 = val((m, m)) + 2 * np.eye(m)
    put(2, B2)
    A[2 * m + 3, 2 * m:3 * m] = 0
    A[2 * m + 3, 0] = 1.0
    A[2 * m + 3, n - 1] = 2.0
    put(3, val((m, m)) + 2 * np.eye(m))
    put(4, val((m, m)) + 2 * np.eye(m))
    A[4 * m + 1, :] = 0
    put(5, np.diag(val(m) + 3))
    B6 = val((m, m)) + 2 * np.eye(m)
    B6[2, 1] = np.nan
    put(6, B6)
    for g in range(7, nblk):
        put(g, val((m, m)) + 2 * np.eye(m))
    A = A.tocsr()
    A.eliminate_zeros()          # the zeroed rows really are absent; NaN is not zero and stays
    return canonical(A), uniform_ptr(n, m), [2, 4, 6]


def stride_ptr(W):
    """2 * 3 * 256 / W + 1 blocks of W rows: with reduce_blocks = 3 every workgroup strides twice and one starts a third
    round."""
    nblk = 2 * 3 * 256 // W + 1
    return uniform_ptr(nblk * W, W)


def rhs(n, ncols, cplx, seed):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, ncols))
    return x + 1j * rng.standard_normal((n, ncols)) if cplx else x
