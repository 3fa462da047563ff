"""Generators for the pivot edge cases of the LDL^T factors (zero pivots,
pivots that cancel to zero, zero diagonal entries that fill in, non-finite
entries), shared by test_gpu_pivot_edges.py (GPU) and
test_oracle_pivot_cases.py (CPU only: the generators' conditions against the
oracle).  numpy only: importable without a GPU."""
import numpy as np

# (N, (nbo, nbi)): the configurations the oracle factors in test time ...
ORACLE_CONFIGS = [(200, (0, 64)), (300, (128, 64)), (700, (0, 64)), (300, (256, 128)), (700, (256, 128))]
# ... and the ones only the exact test runs (its expected factor is known in closed form)
EXACT_ONLY_CONFIGS = [(2560, (0, 64)), (4100, (0, 64))]


def resolve_blocking(N, blocking):
    """(nbo, nbi) an order-N factor uses: ipmz_ctx_set_blocking's rule for nbo = 0
    with nbi = 64 (include/ipmz.h).  The GPU tests check it against the context."""
    nbo, nbi = blocking
    if nbo == 0:
        nbo = 512 if N > 4096 else 384 if N >= 2048 else 256
    return nbo, nbi


def positions(N, nbo, nbi):
    """Pivot positions at every edge of the blocking: the first pivot, a
    16-tile edge, the inner-block edges (64 and 128), the outer-panel edge, one
    index inside the last (ragged) inner block and the last pivot."""
    last0 = (N - 1) // nbi * nbi
    pos = {0, 15, 16, 63, 64, 127, 128, nbo - 1, nbo, (last0 + N - 1) // 2, N - 1}
    return sorted(p for p in pos if 0 <= p < N)


def pair_positions(N, nbo):
    """First indices j of the pairs (j, j + 1) that straddle a boundary."""
    pos = sorted({15, 63, 127, nbo - 1, N - 2})
    pos = [j for j in pos if 0 <= j and j + 1 < N]
    assert all(b - a >= 2 for a, b in zip(pos, pos[1:]))  # the pairs do not overlap
    return pos


def qd(N, seed):
    """The quasi-definite matrix of test_gpu_parity.py (_qd), restated here so
    that the CPU-only tests need no GPU module."""
    rng = np.random.default_rng(seed)
    n1 = (3 * N + 3) // 4
    K = rng.uniform(-1, 1, (N, N))
    K[:n1, :n1] /= n1
    K[n1:, :n1] /= np.sqrt(n1)
    K[n1:, n1:] = 0
    K = np.tril(K) + np.tril(K, -1).T  # symmetric
    d = rng.uniform(0.5, 1.5, N)
    K[np.arange(n1), np.arange(n1)] = 1 + d[:n1]
    K[np.arange(n1, N), np.arange(n1, N)] = -d[n1:]
    return K


def aug(n, mp, seed):
    """The augmented matrix [[H, B^T], [B, -E]] of test_gpu_normal.py (_aug, H SPD)."""
    rng = np.random.default_rng(seed)
    H = rng.uniform(-1, 1, (n, n)) / n
    H = np.tril(H) + np.tril(H, -1).T
    H[np.arange(n), np.arange(n)] = rng.uniform(1, 2, n)
    B = rng.uniform(-1, 1, (mp, n)) / np.sqrt(n)
    E = rng.uniform(0.5, 1.5, mp)
    K = np.zeros((n + mp, n + mp))
    K[:n, :n] = H
    K[n:, :n] = B
    K[:n, n:] = B.T
    K[n:, n:] = -np.diag(E)
    return K


# ---------------------------------------------------------------------------
# case 1: exact integer factor
def int_factor(N, seed, zero_at=()):
    """K = (L0 D0) L0^T with L0 unit lower triangular, at most 4 entries of
    {-1, +1} per row left of the diagonal (two among the 8 columns next to it,
    two anywhere), D0 from {1, 2, -1, -2} and D0[j] = 0 for j in zero_at.
    Returns (K, L0, D0, L_exp, D_exp): the factor every elimination order
    must produce exactly -- a zero pivot becomes 1e-8 and the column below it
    0 * (1 / 1e-8) = 0."""
    rng = np.random.default_rng(seed)
    L0 = np.zeros((N, N))
    for i in range(1, N):
        near = rng.integers(max(0, i - 8), i, 2)
        far = rng.integers(0, i, 2)
        L0[i, np.concatenate([far, near])] = rng.choice([-1.0, 1.0], 4)
    L0[np.arange(N), np.arange(N)] = 1.0
    D0 = rng.choice([1.0, 2.0, -1.0, -2.0], N)
    zero_at = np.asarray(sorted(zero_at), dtype=np.int64)
    D0[zero_at] = 0.0
    # K row by row from the <= 5 entries of each row of L0 (all integers: exact)
    L0T = np.ascontiguousarray(L0.T)
    K = np.zeros((N, N))
    cols = np.argpartition(-np.abs(L0), 5, axis=1)[:, :5] if N > 5 else np.tile(np.arange(N), (N, 1))
    for a in range(cols.shape[1]):
        c = cols[:, a]
        K += (L0[np.arange(N), c] * D0[c])[:, None] * L0T[c, :]
    L_exp = np.tril(L0, -1)
    L_exp[:, zero_at] = 0.0
    D_exp = D0.copy()
    D_exp[zero_at] = 1e-8
    return K, L0, D0, L_exp, D_exp


def exactness_product(L0, D0):
    """A * B * 128 of the exactness condition (must stay below 2^53):
    A = max |inverse of a diagonal block of L0| over the 64- and 128-blocks (the
    factors the blocked elimination multiplies a row strip by), B = the max
    row sum of |L0| |D0| |L0|^T (a bound on every partial sum of every Schur
    complement entry), 128 = the longest inner product of one block step."""
    N = L0.shape[0]
    A = 0.0
    for nb in (64, 128):
        for k0 in range(0, N, nb):
            blk = L0[k0:k0 + nb, k0:k0 + nb]
            A = max(A, np.abs(np.rint(np.linalg.inv(blk))).max())
    aL = np.abs(L0)
    B = (aL @ (np.abs(D0) * aL.sum(axis=0))).max()
    return A, B, A * B * 128


# ---------------------------------------------------------------------------
# case 2: decoupled zero rows and columns; case 3: a 1e8 multiplier
def zero_rows(K, pos):
    K = K.copy()
    K[pos, :] = 0.0
    K[:, pos] = 0.0
    return K


def embed_pairs(K, pairs):
    """Rows and columns j, j + 1 cleared and [[0, 1], [1, 2]] embedded there:
    D[j] = 1e-8, L[j+1, j] = 1e8, D[j+1] = 2 - 1e8."""
    K = K.copy()
    for j in pairs:
        K[[j, j + 1], :] = 0.0
        K[:, [j, j + 1]] = 0.0
        K[j + 1, j] = K[j, j + 1] = 1.0
        K[j + 1, j + 1] = 2.0
    return K


# ---------------------------------------------------------------------------
# case 4: zero (2,2) block that fills in
def saddle(n, mp, seed):
    K = aug(n, mp, seed)
    K[n:, n:] = 0.0
    return K


# ---------------------------------------------------------------------------
# case 5: one non-finite entry per factor
def contaminations(N, nbo, limit=None):
    """[(label, row, col, value)]: K[row, col] = K[col, row] = value makes pivot
    `row` the first non-finite one.  limit: keep the entries inside the
    leading limit x limit block (the H block of the normal equations)."""
    M = N if limit is None else limit
    out = [("+inf diag 0", 0, 0, np.inf), ("-inf diag 70", 70, 70, -np.inf), ("+inf diag last", M - 1, M - 1, np.inf)]
    j = 3
    rows = [("same 16-tile", 9), ("next 64-block", 69), ("next outer panel", nbo + 7),
            ("last panel", (N - 1) // nbo * nbo + 3), ("last row", M - 1)]
    seen = set()
    for label, i in rows:
        if j < i < M and i not in seen:
            seen.add(i)
            out.append((f"nan ({i}, {j}) {label}", i, j, np.nan))
    return out


def contaminate(K, row, col, value):
    K = K.copy()
    K[row, col] = K[col, row] = value
    return K
