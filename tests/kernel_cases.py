"""EXACT inputs, references and dispatch predictions for the C ABI building blocks (rflu_gemm_rm_{f64,f32,cf64,cf32}_dev, rflu_trsm_rm_*,
rflu_laswp_rm_*).  No GPU and no torch here: tests/test_kernel_cases.py proves the claims below on the host, and
tests/test_gpu_kernels_exact.py runs the grids on the device and compares whole buffers by value.

Exactness rule: every input is a small integer held in the floating type.
  * real GEMM  C <- C - A B: A, B in [-3, 3], C in [-8, 8].  Every partial sum of c - sum a b, over any subset of the products and in any
    order, is an integer of magnitude <= 9 K + 8;
  * complex GEMM: Gaussian integers, parts in [-3, 3] (A, B) and [-8, 8] (C); every partial sum of a part is an integer <= 18 K + 8;
  * K <= 512, so both stay below 2^14, far inside the 24 bits of Float32: no product and no sum is ever rounded, on the matrix cores or
    anywhere else, and every correct kernel returns the same values in both precisions;
  * TRSM: L = solve_case(n, 400, seed=n).L() of tests/solve_cases.py (unit lower, subdiagonal in {-1, 0, 1}, three far +-1 per row; the
    inverses of its 64 x 64 diagonal blocks have entries in {0, +-1}), B = L x_true in int64 with x_true in [-4, 4];
  * interchanges: element (i, j) of the m x ld buffer holds i * ld + j (< 2^24), so a misplaced element names where it came from.
References are float64 BLAS products of the integer valued arrays (exact below 2^53) or int64; nothing loops over K in Python.

What these inputs do NOT exercise: rounding.  A product taken in the wrong precision, a reciprocal a few ulps off or a lost guard digit
returns the same integers.  The uniform random cases of tests/test_gpu_kernels.py and tests/test_gpu_complex.py (and, for the TRSM, the
sizes around the fused / recursive boundary added there) stay responsible for that side.
Out of scope, and untested: the experiments-only variants (RFLU_GEMM_CFIRST_BELOW, RFLU_LASWP_LPR, RFLU_SKINNY_WIDE, RFLU_GEMM_FLAGS: read
by an RFLU_EXPERIMENTS build only) and the two-region "first columns first" order of gemm_sub_kernel, which no C ABI entry can reach.

Operands are views into one larger flat buffer per operand (`Operand`: buffer, offset of the view's first element, leading dimension);
the elements around a view belong to what is checked.  Offsets are counted in REAL elements from the start of the buffer, which the
device tests place on a 16-byte boundary, so `offset * itemsize % 16` is the alignment the launcher sees.

The `*_class` functions restate the launchers' dispatch rules.  They predict which code a case runs (for the failure messages and for the
coverage floor of tests/test_kernel_cases.py); they are never used to decide what to expect of a result.
"""
import functools
import itertools

import numpy as np

from solve_cases import solve_case

NB = 64                      # rows of a pivot chunk / of a TRSM block (rflu_internal.hpp)
SENTINEL = 3.0e30            # finite in both precisions: what a kernel must neither read into a result nor overwrite
REAL_DTYPES = (np.float64, np.float32)


def _round_up(x, q):
    return (x + q - 1) // q * q


class Operand:
    """A row-major rows x cols view (complex: cols complex elements = 2 * cols reals per row) inside the flat real array `buf`: element
    (i, j) at buf[off + i * step + j] with step = ld (real) or at buf[off + 2 * (i * ld + j)] (+ 1: imaginary part)."""

    def __init__(self, buf, off, ld, rows, cols, cplx=False):
        self.buf, self.off, self.ld, self.rows, self.cols, self.cplx = buf, int(off), int(ld), int(rows), int(cols), bool(cplx)

    def view(self, rows=None, cols=None, buf=None):
        """Strided numpy view of the top left rows x cols part (real: 2-D; complex: 3-D with a last axis (re, im))."""
        b = self.buf if buf is None else buf
        rows = self.rows if rows is None else rows
        cols = self.cols if cols is None else cols
        it = b.itemsize
        if self.cplx:
            return np.lib.stride_tricks.as_strided(b[self.off:], shape=(rows, cols, 2), strides=(2 * self.ld * it, 2 * it, it))
        return np.lib.stride_tricks.as_strided(b[self.off:], shape=(rows, cols), strides=(self.ld * it, it))

    def values(self, rows=None, cols=None, buf=None):
        """The view's values as float64 / complex128 (a copy)."""
        v = self.view(rows, cols, buf).astype(np.float64)
        return v[..., 0] + 1j * v[..., 1] if self.cplx else v


def _embed(rng, lo, hi, rows, cols, ld, shift, dtype, cplx):
    """A flat buffer of integers in [lo, hi] everywhere, and the view that starts 4 rows and 16 elements (complex: 8) plus `shift` reals in."""
    w = 2 if cplx else 1
    off = 4 * w * ld + 16 + shift
    size = off + w * ld * (rows + 4)
    assert off + w * ld * (rows - 1) + w * cols <= size and w * cols + 16 + shift <= w * ld
    buf = rng.integers(lo, hi + 1, size=size).astype(dtype)
    return Operand(buf, off, ld, rows, cols, cplx)


# ============================================================================================================== real GEMM
GEMM_M = (1, 63, 64, 65, 127, 128, 129, 257)
GEMM_N = (1, 63, 64, 65, 127, 128, 129, 130, 257)
GEMM_K = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128, 129, 256)
GEMM_REDUCED_MN = (65, 128, 257)
GEMM_REDUCED_K = (16, 17, 64, 128, 129)
# P0 only: >= 2 groups of 8 tile rows with a partial last group and nwg % 8 != 0 (in an interior launch at K = 96 / 32 / 512, with a K tail at
# K = 100, next to the skinny bound at (2100, 130, 64): N = 130 > 2 K keeps that one on the tiled kernel) and skinny launches with an N and
# an M tail: (1100, 129, 128) with 18 tile rows and (2100, 127, 64) with 33
GEMM_LARGE = ((1100, 300, 96), (1100, 300, 100), (2049, 129, 32), (1025, 385, 512), (2100, 130, 64), (1100, 129, 128), (2100, 127, 64))
# placement -> shifts of the three pointers in elements, odd lda / ldb, odd ldc
REAL_PLACEMENTS = {
    "P0": dict(a=0, b=0, c=0, odd_ab=False, odd_c=False),   # every pointer 16-byte aligned, leading dimensions multiples of 16 elements
    "P1": dict(a=0, b=0, c=1, odd_ab=False, odd_c=True),    # C one element off and ldc odd: vec_ok (A, B, lda, ldb only) stays true
    "P2": dict(a=1, b=0, c=0, odd_ab=False, odd_c=False),   # A one element off
    "P3": dict(a=0, b=1, c=0, odd_ab=False, odd_c=False),   # B one element off
    "P4": dict(a=0, b=0, c=0, odd_ab=True, odd_c=False),    # aligned pointers, odd lda and ldb
    "P5": dict(a=2, b=2, c=0, odd_ab=False, odd_c=False),   # Float32 only: A and B 8-byte but not 16-byte aligned
}


def real_placements(dtype):
    return [p for p in REAL_PLACEMENTS if p != "P5" or np.dtype(dtype) == np.float32]


def real_gemm_grid(placement):
    """The (M, N, K) of a placement, the large cases (P0) last."""
    if placement in ("P0", "P1"):
        grid = list(itertools.product(GEMM_M, GEMM_N, GEMM_K))
    else:
        grid = list(itertools.product(GEMM_REDUCED_MN, GEMM_REDUCED_MN, GEMM_REDUCED_K))
    return grid


class GemmOperands:
    """A (Mmax x Kmax), B (Kmax x Nmax), C (Mmax x Nmax) of one placement; the case (M, N, K) uses their top left parts, so one product per K
    serves every (M, N).  Real: `cplx=False`, placements REAL_PLACEMENTS; complex: `cplx=True`, placements COMPLEX_PLACEMENTS."""

    def __init__(self, dtype, placement, Mmax, Nmax, Kmax, cplx=False):
        self.dtype, self.placement, self.cplx = np.dtype(dtype), placement, cplx
        self.Mmax, self.Nmax, self.Kmax = Mmax, Nmax, Kmax
        if cplx:
            pl = COMPLEX_PLACEMENTS[placement]
            per = 8 // self.dtype.itemsize                    # reals per 8 bytes
            sa, sb, sc = (pl[k] * per for k in ("a8", "b8", "c8"))
        else:
            pl = REAL_PLACEMENTS[placement]
            sa, sb, sc = pl["a"], pl["b"], pl["c"]
        odd_ab, odd_c = int(pl["odd_ab"]), int(pl["odd_c"])
        rng = np.random.default_rng([17, Mmax, Nmax, Kmax, sorted(REAL_PLACEMENTS | COMPLEX_PLACEMENTS).index(placement), int(cplx)])
        self.A = _embed(rng, -3, 3, Mmax, Kmax, _round_up(Kmax, 16) + 32 + odd_ab, sa, self.dtype, cplx)
        self.B = _embed(rng, -3, 3, Kmax, Nmax, _round_up(Nmax, 16) + 32 + odd_ab, sb, self.dtype, cplx)
        self.C = _embed(rng, -8, 8, Mmax, Nmax, _round_up(Nmax, 16) + 32 + odd_c, sc, self.dtype, cplx)
        for op in (self.A, self.B, self.C):
            op.buf.setflags(write=False)

    def product(self, K):
        """C - A[:, :K] B[:K, :] over the whole Mmax x Nmax window, in float64 / complex128 BLAS (exact: integers below 2^53)."""
        return self.C.values() - self.A.values(cols=K) @ self.B.values(rows=K)

    def expected_full(self, K):
        """The C buffer with the WHOLE Mmax x Nmax window replaced by `product(K)`, in the element type."""
        out = self.C.buf.copy()
        p = self.product(K)
        v = self.C.view(buf=out)
        if self.cplx:
            v[..., 0], v[..., 1] = p.real, p.imag
        else:
            v[...] = p
        return out

    def expected(self, M, N, K, full=None):
        """The C buffer after the call (M, N, K): the M x N window from expected_full(K), every other element as it was."""
        full = self.expected_full(K) if full is None else full
        out = self.C.buf.copy()
        self.C.view(M, N, buf=out)[...] = self.C.view(M, N, buf=full)
        return out

    def bound(self, M, N, K):
        """max|c| + K max|a| max|b| (complex: 2 K, on the parts) of the case's actual operands: what every partial sum stays below."""
        a, b, c = (np.abs(op.view(r, s)).max() for op, r, s in ((self.A, M, K), (self.B, K, N), (self.C, M, N)))
        return float(c + (2 if self.cplx else 1) * K * a * b)

    def classify(self, M, N, K):
        if self.cplx:
            return complex_gemm_class(M, N, K, self.A.off, self.B.off, self.C.off, self.A.ld, self.B.ld, self.dtype)
        return real_gemm_class(M, N, K, self.A.off, self.B.off, self.A.ld, self.B.ld, self.dtype)


@functools.lru_cache(maxsize=None)
def real_gemm_operands(dtype, placement, dims=None):
    """The shared operands of a placement's grid (dims None) or of one large case (dims = (M, N, K)); read-only."""
    M, N, K = dims if dims else (max(GEMM_M), max(GEMM_N), max(GEMM_K))
    return GemmOperands(dtype, placement, M, N, K)


# ---- gemm.hip: launch_gemm (vec_ok, the skinny test, tiles) and gemm_sub_kernel / gemm_tile.hpp (full_mn, INTERIOR, the remap) ----------
G_BM = G_BN = 128
G_BK = 16
G_GROUP_M = 8
S_BM = S_BN = S_KC = 64
SKINNY_MAX_K = 128           # Tune::skinny_max_k (rflu_internal.hpp); skinny_wide = 0 in the shipped library


def real_vec_ok(a_off, b_off, lda, ldb, dtype):
    """launch_gemm: `g.vec_ok = (A | B) % 16 == 0 && lda % VW == 0 && ldb % VW == 0`; C and ldc play no part."""
    vw = 16 // np.dtype(dtype).itemsize
    return a_off % vw == 0 and b_off % vw == 0 and lda % vw == 0 and ldb % vw == 0


def real_gemm_class(M, N, K, a_off, b_off, lda, ldb, dtype):
    """(class, flags) of a launch.  class: 'skinny1' / 'skinny2' (gemm_skinny_kernel<T, 1 / 2>: vec_ok, K = 64 / 128, N <= 2 K), else by
    the tiles of gemm_sub_kernel: 'scalar' (vec_ok false: guarded scalar loads everywhere), 'interior' (a full 128 x 128 tile exists, K % 16 == 0
    and K >= 32: gemm_tile<.., true>), 'full_vec_ktail' (a full tile exists, K % 16 != 0 or K < 32: 16-byte loads for whole slabs, guarded
    scalar loads for the last one), 'edge_vec' (vec_ok but no full tile).  flags: 'm_tail' / 'n_tail' = a partial tile row / column exists
    (tiles of 64 for the skinny kernel, of 128 otherwise)."""
    vec = real_vec_ok(a_off, b_off, lda, ldb, dtype)
    if vec and K in (S_KC, 2 * S_KC) and K <= SKINNY_MAX_K and N <= 2 * K:
        cls, bm, bn = ("skinny1" if K == S_KC else "skinny2"), S_BM, S_BN
    else:
        bm, bn = G_BM, G_BN
        if not vec:
            cls = "scalar"
        elif M >= G_BM and N >= G_BN:
            cls = "interior" if (K % G_BK == 0 and K >= 2 * G_BK) else "full_vec_ktail"
        else:
            cls = "edge_vec"
    flags = frozenset(f for f, on in (("m_tail", M % bm != 0), ("n_tail", N % bn != 0)) if on)
    return cls, flags


def gemm_remap_facts(M, N):
    """gemm_sub_kernel's tile order: (tiles_m, tiles_n, nwg % 8, groups of G_GROUP_M tile rows, tile rows of the last group)."""
    tiles_m, tiles_n = -(-M // G_BM), -(-N // G_BN)
    groups = -(-tiles_m // G_GROUP_M)
    return tiles_m, tiles_n, (tiles_m * tiles_n) % 8, groups, tiles_m - (groups - 1) * G_GROUP_M


def gemm_remap_tiles(M, N):
    """The (tile_m, tile_n) of every workgroup 0 .. nwg-1, restated from gemm_sub_kernel (one region: na_tiles_n = 0)."""
    tiles_m, tiles_n = -(-M // G_BM), -(-N // G_BN)
    nwg = tiles_m * tiles_n
    q, r = nwg >> 3, nwg & 7
    out = []
    for bid in range(nwg):
        xcd, loc = bid & 7, bid >> 3
        wg = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + loc
        per_group = G_GROUP_M * tiles_n
        group = wg // per_group
        first_m = group * G_GROUP_M
        gsz = min(tiles_m - first_m, G_GROUP_M)
        in_group = wg - group * per_group
        out.append((first_m + in_group % gsz, in_group // gsz))
    return out


# ============================================================================================================ complex GEMM
CGEMM_M = (1, 31, 32, 33, 63, 64, 65, 129)
CGEMM_N = (1, 31, 32, 33, 63, 64, 65, 130)
CGEMM_K = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 65, 129)
CGEMM_REDUCED_MN = (33, 64, 129)
CGEMM_REDUCED_K = (16, 17, 65)
# placement -> shifts of the three pointers in units of 8 bytes (half a ComplexF64, one ComplexF32), odd lda / ldb
COMPLEX_PLACEMENTS = {
    "Q0": dict(a8=0, b8=0, c8=0, odd_ab=False, odd_c=False),   # all pointers 16-byte aligned, even strides
    "Q1": dict(a8=1, b8=1, c8=1, odd_ab=False, odd_c=False),   # every buffer 8 bytes off
    "Q2": dict(a8=0, b8=0, c8=0, odd_ab=True, odd_c=False),    # cf32: aligned pointers, odd lda and ldb
    "Q3": dict(a8=1, b8=0, c8=0, odd_ab=False, odd_c=False),   # cf32: A one complex element off
    "Q4": dict(a8=0, b8=0, c8=1, odd_ab=False, odd_c=False),   # cf32: C alone one complex element off
}


def complex_placements(dtype):
    """`dtype` is the REAL type of the parts: float64 for cf64, float32 for cf32."""
    return ["Q0", "Q1"] + (["Q2", "Q3", "Q4"] if np.dtype(dtype) == np.float32 else [])


def complex_gemm_grid(placement):
    if placement == "Q0":
        return list(itertools.product(CGEMM_M, CGEMM_N, CGEMM_K))
    return list(itertools.product(CGEMM_REDUCED_MN, CGEMM_REDUCED_MN, CGEMM_REDUCED_K))


@functools.lru_cache(maxsize=None)
def complex_gemm_operands(dtype, placement):
    return GemmOperands(dtype, placement, max(CGEMM_M), max(CGEMM_N), max(CGEMM_K), cplx=True)


# ---- complex_gemm.hip: launch_cgemm (al16 of all three pointers, strides_ok) and cgemm_sub_kernel / cgemm_tile (INTERIOR, the K tail) ----
CG_BM = CG_BN = 64
CG_BK = 16


def complex_vec_ok(a_off, b_off, c_off, lda, ldb, dtype):
    """launch_cgemm: `al16(A) && al16(B) && al16(C) && (sizeof(R) == 8 || (lda % 2 == 0 && ldb % 2 == 0))`; offsets in reals, strides in
    complex elements."""
    it = np.dtype(dtype).itemsize
    aligned = all((o * it) % 16 == 0 for o in (a_off, b_off, c_off))
    return aligned and (it == 8 or (lda % 2 == 0 and ldb % 2 == 0))


def complex_gemm_class(M, N, K, a_off, b_off, c_off, lda, ldb, dtype):
    """(class, flags): 'scalar' (vec_ok false: element by element everywhere), 'interior' (a full 64 x 64 tile exists and K % 16 == 0: 16-byte
    loads only), 'interior_ktail' (a full tile exists, K % 16 != 0: the last slab element by element), 'edge' (vec_ok but no full tile)."""
    if not complex_vec_ok(a_off, b_off, c_off, lda, ldb, dtype):
        cls = "scalar"
    elif M >= CG_BM and N >= CG_BN:
        cls = "interior" if K % CG_BK == 0 else "interior_ktail"
    else:
        cls = "edge"
    flags = frozenset(f for f, on in (("m_tail", M % CG_BM != 0), ("n_tail", N % CG_BN != 0)) if on)
    return cls, flags


# ==================================================================================================================== TRSM
TRSM_N = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 513, 1000)
TRSM_NRHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 400)
TRSM_LDL = ("plus3", "round16")          # ldl = n + 3, and n rounded up to a multiple of 16
TRSM_PAD = 3                             # sentinel columns behind the right-hand sides
TRSM_FUSED_MAX = 256                     # driver.cpp


def trsm_ldl(n, kind):
    return n + 3 if kind == "plus3" else _round_up(n, 16)


def trsm_class(n):
    """driver.cpp: trsm_public always has the block inverses, so trsm_rec takes the fused strip kernel up to 256 rows and splits beyond."""
    if n <= TRSM_FUSED_MAX:
        return "fused" if n <= 3 * NB else "fused_slot_reuse"   # 193 .. 256: the fourth block is staged in block 0's LDS slot
    return "recursive"


@functools.lru_cache(maxsize=None)
def trsm_case(n):
    """(L dense int64 with its unit diagonal, x_true n x 400 int64, B = L x_true int64); read-only."""
    case = solve_case(n, max(TRSM_NRHS), seed=n)
    Ls = case.L()
    B = Ls @ case.x_true
    L = Ls.toarray()
    for a in (L, B):
        a.setflags(write=False)
    return L, case.x_true, B


def trsm_l_buffer(n, kind, dtype):
    """The n x ldl row-major L operand: strict lower triangle of L, SENTINEL on the diagonal, above it and in the padding columns (the ABI's
    contract: the unit diagonal is implied and nothing but the strict lower triangle is read)."""
    L, _, _ = trsm_case(n)
    ldl = trsm_ldl(n, kind)
    buf = np.full((n, ldl), SENTINEL, dtype=dtype)
    i, j = np.tril_indices(n, -1)
    buf[i, j] = L[i, j]
    return buf, ldl


def trsm_b_buffer(n, nrhs, dtype, solved=False):
    """The n x (nrhs + 3) right-hand sides (`solved`: x_true in their place), SENTINEL in the three padding columns."""
    _, x_true, B = trsm_case(n)
    buf = np.full((n, nrhs + TRSM_PAD), SENTINEL, dtype=dtype)
    buf[:, :nrhs] = (x_true if solved else B)[:, :nrhs]
    return buf


# ============================================================================================================ interchanges
LASWP_M = 700
LASWP_LD = (1040, 1041)
LASWP_RANGES = ((0, 1), (0, 63), (0, 64), (64, 129), (64, 214), (128, 328))
LASWP_PATTERNS = ("identity", "distinct_far", "same_far", "shift", "next_chunk", "random")
LASWP_SCALAR_C0 = 17
LASWP_SCALAR_NCOLS = (1, 7, 8, 9, 31, 32, 33, 333)
LASWP_VEC_C0 = 16


def laswp_vec_ncols(dtype):
    vwf = 16 // np.dtype(dtype).itemsize
    return (vwf, 8 * vwf - vwf, 8 * vwf, 8 * vwf + vwf, 32 * vwf, 32 * vwf + vwf, 1000)


def laswp_columns(dtype):
    """Every (c0, ncols) of the grid: the ranges made for the 16-byte kernel (which an odd ld sends to the scalar one) and for the scalar one."""
    return [(LASWP_VEC_C0, n) for n in laswp_vec_ncols(dtype)] + [(LASWP_SCALAR_C0, n) for n in LASWP_SCALAR_NCOLS]


def laswp_class(ptr_off, ld, c0, ncols, dtype):
    """laswp.hip: launch_laswp3 -- 16-byte accesses ('vec': laswp_kernel<T, VWF, 8>) when R is 16-byte aligned, ld % VWF == 0 and the column
    range starts and ends on a 16-byte boundary; else one element per lane ('scalar': laswp_kernel<T, 1, 8>)."""
    it = np.dtype(dtype).itemsize
    vwf = 16 // it
    return "vec" if ((ptr_off * it) % 16 == 0 and ld % vwf == 0 and c0 % vwf == 0 and ncols % vwf == 0) else "scalar"


def laswp_matrix(ld, dtype, m=LASWP_M):
    """m x ld, element (i, j) = i * ld + j: exact in Float32 (< 2^24)."""
    assert m * ld < 2 ** 24
    return (np.arange(m, dtype=np.int64)[:, None] * ld + np.arange(ld, dtype=np.int64)[None, :]).astype(dtype)


@functools.lru_cache(maxsize=None)
def laswp_ipiv(pattern, k0, k1, m=LASWP_M):
    """A valid 1-based ipiv of length m (k + 1 <= ipiv[k] <= m).  Entries outside [k0, k1) name row m: a kernel that applies one of them
    moves a row it must not."""
    k = np.arange(m, dtype=np.int64)
    ipiv = np.full(m, m, dtype=np.int64)
    rng = np.random.default_rng([3, k0, k1])
    r = np.arange(k0, k1)
    if pattern == "identity":                       # (a) no moves
        ipiv[r] = r + 1
    elif pattern == "distinct_far":                 # (b) every pivot to a row of its own beyond k1: 2 moves per pivot, 128 per full chunk
        ipiv[r] = rng.permutation(np.arange(k1, m))[:r.size] + 1
    elif pattern == "same_far":                     # (c) every pivot of a chunk to the same row beyond k1
        ipiv[r] = k1 + 5 + r // NB + 1
    elif pattern == "shift":                        # (d) ipiv[k] = k + 2: row k + 1, a shift inside the chunk
        ipiv[r] = r + 2
    elif pattern == "next_chunk":                   # (e) ipiv[k] = k + 65: a row of the next chunk, which moves it again
        ipiv[r] = r + NB + 1
    elif pattern == "random":                       # (f) the mix of test_laswp_matches_sequential_interchanges
        for q in r:
            t = rng.integers(0, 10)
            ipiv[q] = (q if t == 0 else (k0 + 5 if (t == 1 and q < k0 + 5) else rng.integers(q, m))) + 1
        if k1 - k0 > 7:
            ipiv[k0 + 7] = max(ipiv[k0 + 3], k0 + 8)   # a repeated target
    else:
        raise ValueError(pattern)
    assert (ipiv >= k + 1).all() and (ipiv <= m).all()
    ipiv.setflags(write=False)
    return ipiv


def laswp_reference(A, c0, ncols, ipiv, k0, k1):
    """apply_permutation!: the interchanges k0 .. k1-1 one after the other on columns [c0, c0 + ncols) of a copy of A."""
    out = A.copy()
    for q in range(k0, k1):
        p = int(ipiv[q]) - 1
        if p != q:
            out[[q, p], c0:c0 + ncols] = out[[p, q], c0:c0 + ncols]
    return out


@functools.lru_cache(maxsize=None)
def laswp_perm(pattern, k0, k1, m=LASWP_M):
    """The same interchanges on the row numbers alone: new row i = old row perm[i]."""
    ipiv = laswp_ipiv(pattern, k0, k1, m)
    perm = np.arange(m, dtype=np.int64)
    for q in range(k0, k1):
        p = int(ipiv[q]) - 1
        if p != q:
            perm[[q, p]] = perm[[p, q]]
    perm.setflags(write=False)
    return perm


def laswp_chunk_moves(ipiv, chunk, k1):
    """The move list of a chunk as the header of laswp.hip defines it: the pivots [64 chunk, min(64 chunk + 64, k1)) folded into independent
    row moves new[dst] = old[src]; returns (dst, src), every row whose content changes exactly once."""
    content = {}
    for q in range(chunk * NB, min(chunk * NB + NB, k1)):
        p = int(ipiv[q]) - 1
        if p != q:
            cq, cp = content.get(q, q), content.get(p, p)
            content[q], content[p] = cp, cq
    moves = sorted((d, s) for d, s in content.items() if d != s)
    return [d for d, _ in moves], [s for _, s in moves]
