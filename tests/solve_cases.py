"""EXACT inputs for the real solves (ldiv!(F, B) and ldiv!(F', B)): LU factors, interchanges and right-hand sides for which every
correct blocked substitution returns the same bits, whatever its summation order and whatever its precision.

For n, nrhs and a seed:
  * x_true: n x nrhs, integers in [-4, 4];
  * L: unit lower triangular; l[i+1, i] in {-1, 0, 1}; every row of block row r >= 1 (blocks of NB = 64 rows) has three more entries of
    +-1 at random columns left of its own 64 x 64 diagonal block;
  * U: diagonal in {+-1, +-2}; u[i-1, i] in {0, +-u[i, i]}; every column beyond the first block has three more entries from
    {+-1, +-2} at random rows above its own diagonal block;
  * ipiv: 1-based, k + 1 <= ipiv[k] <= n, and every entry but the last one moves a row;
  * B = P^T L U x_true (forward) and B = U^T L^T P x_true (transposed), in int64 through scipy.sparse: O(n) work per column.

Why a solve of these is exact.  Inside a diagonal block both triangles are bidiagonal, and along a chain of off-diagonal entries every
u[i-1, i] cancels against the diagonal entry u[i, i] up to a sign (in U and in U^T alike; L has a unit diagonal), so the inverse of a
diagonal block has entries in {0, +-1, +-1/2}; the right-hand sides are small integers; hence every intermediate of
a blocked substitution -- b - T x, inv(D) (...), (inv(D) T) x -- is a small multiple of 1/2, far inside the 24 bits of Float32, and no
sum is ever rounded.  tests/test_solve_cases.py proves that on the host for the generator as committed.

What they do NOT exercise: rounding.  A reciprocal that is a few ulps off is still exact on a power of two, a Float32 product where
Float64 was meant returns the same bits.  tests/test_gpu_solve_exact.py part (e) (LAPACK factors of uniform matrices, componentwise
backward error in extended precision) covers that side.

No dense n x n array is made unless `dense_factors` is asked for: the factors are lists of (row, column, value), and `device_factors`
scatters them into a zeroed torch tensor by index, so n = 49217 costs no host memory of order n^2.
"""
import numpy as np
import scipy.sparse as sp

NB = 64   # rows of a block of the solve (rflu_internal.hpp)


def _dedupe(n, rows, cols, vals):
    """One value per (row, column): the LAST one given wins."""
    key = rows.astype(np.int64) * n + cols
    _, first_in_reversed = np.unique(key[::-1], return_index=True)
    keep = np.sort(key.size - 1 - first_in_reversed)
    return rows[keep], cols[keep], vals[keep]


def _far_entries(n, rng, choices):
    """Three entries per index i >= NB at random positions in [0, NB * (i // NB)), i.e. outside i's own diagonal block."""
    idx = np.repeat(np.arange(NB, n, dtype=np.int64), 3)
    if idx.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    other = (rng.random(idx.size) * (NB * (idx // NB))).astype(np.int64)
    return idx, other, rng.choice(np.asarray(choices, dtype=np.int64), size=idx.size)


class SolveCase:
    """The factors as coordinate lists (`lower`: strict lower triangle of L, `upper`: U with its diagonal), `ipiv`, `x_true`."""

    def __init__(self, n, nrhs, seed=0):
        assert n >= 1 and nrhs >= 1
        rng = np.random.default_rng([int(seed), int(n)])
        self.n, self.nrhs, self.seed = int(n), int(nrhs), int(seed)
        i = np.arange(n, dtype=np.int64)
        # ---- L (strictly lower part): far entries first, the subdiagonal last so that it wins a collision at a block's first row
        fr, fc, fv = _far_entries(n, rng, (-1, 1))
        sub = rng.integers(-1, 2, size=max(n - 1, 0)).astype(np.int64)
        rows = np.concatenate([fr, i[1:]]); cols = np.concatenate([fc, i[:-1]]); vals = np.concatenate([fv, sub])
        rows, cols, vals = _dedupe(n, rows, cols, vals)
        nz = vals != 0
        self.lower = (rows[nz], cols[nz], vals[nz])
        # ---- U: diagonal, superdiagonal in {0, +-u[i, i]}, far entries by column
        diag = rng.choice(np.asarray((-2, -1, 1, 2), dtype=np.int64), size=n)
        sup = rng.integers(-1, 2, size=max(n - 1, 0)).astype(np.int64) * diag[1:]
        fcol, frow, fv = _far_entries(n, rng, (-2, -1, 1, 2))
        rows = np.concatenate([frow, i[:-1], i]); cols = np.concatenate([fcol, i[1:], i]); vals = np.concatenate([fv, sup, diag])
        rows, cols, vals = _dedupe(n, rows, cols, vals)
        nz = vals != 0
        self.upper = (rows[nz], cols[nz], vals[nz])
        # ---- interchanges: row k with a row strictly below it, for every k but the last
        ipiv = np.empty(n, dtype=np.int64)
        ipiv[:-1] = i[:-1] + 2 + (rng.random(n - 1) * (n - 1 - i[:-1])).astype(np.int64)
        ipiv[-1] = n
        self.ipiv = ipiv
        self.x_true = rng.integers(-4, 5, size=(n, nrhs)).astype(np.int64)
        self._perm = None

    # ---- the factors as sparse int64 matrices
    def L(self):
        r, c, v = self.lower
        d = np.arange(self.n)
        return sp.csr_matrix((np.concatenate([v, np.ones(self.n, np.int64)]), (np.concatenate([r, d]), np.concatenate([c, d]))),
                             shape=(self.n, self.n), dtype=np.int64)

    def U(self):
        r, c, v = self.upper
        return sp.csr_matrix((v, (r, c)), shape=(self.n, self.n), dtype=np.int64)

    def packed(self):
        """(rows, columns, values) of the packed L\\U, every position once."""
        return tuple(np.concatenate([a, b]) for a, b in zip(self.lower, self.upper))

    # ---- the interchanges as one permutation: (P X)[i] = X[perm[i]] (LAPACK laswp, first to last)
    def perm(self):
        if self._perm is None:
            p = list(range(self.n))
            for k, t in enumerate(self.ipiv.tolist()):
                j = t - 1
                if j != k:
                    p[k], p[j] = p[j], p[k]
            self._perm = np.asarray(p, dtype=np.int64)
        return self._perm

    def apply_p(self, X):
        return X[self.perm()]

    def apply_pt(self, Y):
        out = np.empty_like(Y)
        out[self.perm()] = Y
        return out

    # ---- right-hand sides, exact in int64 (columns [0, nrhs) of the case)
    def b_forward(self):
        """A x_true for A = P^T L U: what ldiv!(F, B) must turn back into x_true."""
        return self.apply_pt(self.L() @ (self.U() @ self.x_true))

    def b_transposed(self):
        """A^T x_true = U^T L^T P x_true: what ldiv!(F', B) must turn back into x_true."""
        return self.U().T.tocsr() @ (self.L().T.tocsr() @ self.apply_p(self.x_true))

    def dense_factors(self, dtype=np.float64):
        """Packed L\\U as a dense column-major array (small n only)."""
        F = np.zeros((self.n, self.n), dtype=dtype, order="F")
        r, c, v = self.packed()
        F[r, c] = v
        return F

    def device_factors(self, dtype, row_major, ld, device="cuda:0", pad=0.0):
        """Packed L\\U scattered into a torch tensor of n * ld elements on `device`: element (i, j) at [i * ld + j] (row_major) or at
        [i + j * ld] (column-major, ld >= n).  Zeros inside the matrix, `pad` in the ld - n elements behind every row / column.
        Returns the tensor shaped (n, ld): row i (row_major) or column j (column-major) per tensor row."""
        import torch

        assert ld >= self.n
        t = torch.zeros((self.n, ld), dtype=dtype, device=device)
        if ld > self.n and pad != 0.0:
            t[:, self.n:] = pad
        r, c, v = self.packed()
        flat = (r * ld + c) if row_major else (c * ld + r)
        t.view(-1).index_put_((torch.from_numpy(flat).to(device),), torch.from_numpy(v).to(device=device, dtype=dtype))
        return t


_CACHE = {}


def solve_case(n, nrhs, seed=0):
    """The case for (n, nrhs, seed), generated once per process; treat it as read-only."""
    key = (n, nrhs, seed)
    if key not in _CACHE:
        _CACHE[key] = SolveCase(n, nrhs, seed)
    return _CACHE[key]
