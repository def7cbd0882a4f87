// complex_gemm.hip -- C <- C - A*B for ComplexF64 / ComplexF32 on the MFMA matrix cores of gfx950 (the schur_complement! of the complex
// recursion, /root/reference/src/lu.jl:265-284 with complex T).  Row-major operands, interleaved (re, im), any M, N, K and strides.
//
// One workgroup (256 threads = 4 waves in 2 x 2) computes a 64 x 64 complex tile of C; a wave owns 32 x 32 of it as 2 x 2 MFMA tiles,
// each with a real and an imaginary accumulator.  K runs in slabs of 16 complex: the slab of A (64 x 16) and of B (16 x 64) goes to LDS
// INTERLEAVED, exactly as it came from memory, and one LDS read per fragment (8 / 16 bytes) hands a lane the real and the imaginary
// fragment of its element.  A 4-deep K step is then four real MFMA products per pair of fragments:
//     Cr -= Ar*Br    Cr += Ai*Bi    Ci -= Ar*Bi    Ci -= Ai*Br
//   Float64: the signs ride on the negate bit of v_mfma_f64_16x16x4_f64 (Mfma<double>::run_neg), the accumulators hold C itself;
//   Float32: that MFMA has no negate bits, so the slab of A is NEGATED ONCE on its way into LDS (the fragments read are -Ar, -Ai) and the
//            one positive product takes +Ai = -(-Ai), one VALU operation per fragment and K step, none per product.
// The accumulators start as the C tile, so the result is the k-ordered chain c - a0*b0 - a1*b1 ... per part, one rounding per product.
//
// LDS: A image [64][16 + 1] complex, B image [16][64 + 4] complex = 2176 complex per stage = 34816 B (Float64) / 17408 B (Float32), one
// stage: the next slab waits in registers while the current one is multiplied (16 MFMAs of >= 32 cycles per K step and wave against four
// LDS reads: the matrix pipe, not LDS or the two barriers per slab, sets the pace).  A fragment read has its 16 lanes of one k on 16
// rows, 17 * 16 B = 68 dwords apart -> banks 4r .. 4r+3 (Float64, 64 banks per 16-byte read): no conflict inside a k; B fragment reads
// are 16 consecutive elements of one row.
// Interior tiles (whole tile inside C, every pointer 16-byte aligned, Float32: even lda / ldb) use 16-byte global loads and carry no
// bounds test; every other tile, and the last partial K slab, goes element by element with tests -- the same arithmetic.
#include "complex.hpp"
#include "gemm_tile.hpp"

namespace rflu {

constexpr int CG_BM = 64, CG_BN = 64, CG_BK = 16;
constexpr int CG_SA = CG_BK + 1;   // complex elements per row of the A image
constexpr int CG_SB = CG_BN + 4;   // ... of the B image
constexpr int CG_STAGE = CG_BM * CG_SA + CG_BK * CG_SB;   // complex elements

template <typename R>
struct CGemmArgs {
    int64_t M, N, K;
    const R* A;
    int64_t lda;
    const R* B;
    int64_t ldb;
    R* C;
    int64_t ldc;
    int tiles_n;
    int vec_ok;
};

template <typename R, bool INTERIOR>
__device__ __forceinline__ void cgemm_tile(const CGemmArgs<R>& g, R* smem, const int64_t m0, const int64_t n0)
{
    typedef typename Mfma<R>::acc_t acc_t;
    typedef R cx_t __attribute__((ext_vector_type(2)));   // one complex element
    constexpr int VR = 16 / (int)sizeof(R);               // reals per 16-byte vector
    typedef R vec_t __attribute__((ext_vector_type(VR)));
    constexpr bool NEG = Mfma<R>::HAS_NEG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    cx_t* As = reinterpret_cast<cx_t*>(smem);
    cx_t* Bs = As + CG_BM * CG_SA;

    // staging map: A slab 64 x 16 (4 consecutive k per thread), B slab 16 x 64 (4 consecutive columns per thread)
    const int a_row = tid >> 2, a_kb = (tid & 3) * 4;
    const int b_k = tid >> 4, b_jb = (tid & 15) * 4;
    const R* Ap = g.A + 2 * ((m0 + a_row) * g.lda + a_kb);
    const R* Bp = g.B + 2 * ((int64_t)b_k * g.ldb + n0 + b_jb);
    const bool a_row_ok = (m0 + a_row) < g.M;
    R ra[8], rb[8];

    auto gload = [&](int64_t k0) {
        if (INTERIOR && k0 + CG_BK <= g.K) {
#pragma unroll
            for (int v = 0; v < 8 / VR; ++v) {
                const vec_t x = *reinterpret_cast<const vec_t*>(Ap + 2 * k0 + v * VR);
                const vec_t y = *reinterpret_cast<const vec_t*>(Bp + 2 * k0 * g.ldb + v * VR);
#pragma unroll
                for (int e = 0; e < VR; ++e) {
                    ra[v * VR + e] = x[e];
                    rb[v * VR + e] = y[e];
                }
            }
        } else {
            const bool bk_ok = (k0 + b_k) < g.K;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool oka = a_row_ok && (k0 + a_kb + e) < g.K;
                const bool okb = bk_ok && (n0 + b_jb + e) < g.N;
                ra[2 * e] = oka ? Ap[2 * (k0 + e)] : R(0);
                ra[2 * e + 1] = oka ? Ap[2 * (k0 + e) + 1] : R(0);
                rb[2 * e] = okb ? Bp[2 * (k0 * g.ldb + e)] : R(0);
                rb[2 * e + 1] = okb ? Bp[2 * (k0 * g.ldb + e) + 1] : R(0);
            }
        }
    };
    auto sstore = [&]() {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            cx_t a, b;
            a.x = NEG ? ra[2 * e] : -ra[2 * e];   // Float32: the slab of A enters LDS negated (see the header)
            a.y = NEG ? ra[2 * e + 1] : -ra[2 * e + 1];
            b.x = rb[2 * e];
            b.y = rb[2 * e + 1];
            As[a_row * CG_SA + a_kb + e] = a;
            Bs[b_k * CG_SB + b_jb + e] = b;
        }
    };

    gload(0);
    // the C tile: for a fixed (i, j, r) sixteen lanes cover 16 consecutive complex elements of one row
    acc_t cr[2][2], ci[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + wr * 32 + i * 16 + Mfma<R>::crow(lane, r);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t col = n0 + wc * 32 + j * 16 + (lane & 15);
                const R* cp = g.C + 2 * (row * g.ldc + col);
                if (INTERIOR) {
                    const cx_t c = *reinterpret_cast<const cx_t*>(cp);
                    cr[i][j][r] = c.x;
                    ci[i][j][r] = c.y;
                } else {
                    const bool ok = row < g.M && col < g.N;
                    cr[i][j][r] = ok ? cp[0] : R(0);
                    ci[i][j][r] = ok ? cp[1] : R(0);
                }
            }
        }

    const int a_frag = (wr * 32 + (lane & 15)) * CG_SA + (lane >> 4);
    const int b_frag = (lane >> 4) * CG_SB + wc * 32 + (lane & 15);
    const int64_t nk = (g.K + CG_BK - 1) / CG_BK;
    for (int64_t kt = 0; kt < nk; ++kt) {
        sstore();
        __syncthreads();
        if (kt + 1 < nk) gload((kt + 1) * CG_BK);
#pragma unroll
        for (int kk = 0; kk < CG_BK / 4; ++kk) {
            cx_t a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = As[a_frag + t * 16 * CG_SA + kk * 4];
                b[t] = Bs[b_frag + kk * 4 * CG_SB + t * 16];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const R pai = -a[i].y;   // Float32 only: +Ai from the negated image
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (NEG) {
                        cr[i][j] = Mfma<R>::run_neg(a[i].x, b[j].x, cr[i][j]);
                        cr[i][j] = Mfma<R>::run(a[i].y, b[j].y, cr[i][j]);
                        ci[i][j] = Mfma<R>::run_neg(a[i].x, b[j].y, ci[i][j]);
                        ci[i][j] = Mfma<R>::run_neg(a[i].y, b[j].x, ci[i][j]);
                    } else {
                        cr[i][j] = Mfma<R>::run(a[i].x, b[j].x, cr[i][j]);
                        cr[i][j] = Mfma<R>::run(pai, b[j].y, cr[i][j]);
                        ci[i][j] = Mfma<R>::run(a[i].x, b[j].y, ci[i][j]);
                        ci[i][j] = Mfma<R>::run(a[i].y, b[j].x, ci[i][j]);
                    }
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + wr * 32 + i * 16 + Mfma<R>::crow(lane, r);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t col = n0 + wc * 32 + j * 16 + (lane & 15);
                R* cp = g.C + 2 * (row * g.ldc + col);
                if (INTERIOR) {
                    cx_t c;
                    c.x = cr[i][j][r];
                    c.y = ci[i][j][r];
                    *reinterpret_cast<cx_t*>(cp) = c;
                } else if (row < g.M && col < g.N) {
                    cp[0] = cr[i][j][r];
                    cp[1] = ci[i][j][r];
                }
            }
        }
}

template <typename R>
__global__ void __launch_bounds__(256) cgemm_sub_kernel(const CGemmArgs<R> g)
{
    __shared__ __attribute__((aligned(16))) R smem[2 * CG_STAGE];
    const int64_t m0 = (int64_t)(blockIdx.x / g.tiles_n) * CG_BM, n0 = (int64_t)(blockIdx.x % g.tiles_n) * CG_BN;
    if (g.vec_ok && m0 + CG_BM <= g.M && n0 + CG_BN <= g.N) cgemm_tile<R, true>(g, smem, m0, n0);   // (uniform over the workgroup)
    else cgemm_tile<R, false>(g, smem, m0, n0);
}

template <typename R>
int launch_cgemm(Handle* h, int64_t M, int64_t N, int64_t K, const R* A, int64_t lda, const R* B, int64_t ldb, R* C, int64_t ldc)
{
    if (M <= 0 || N <= 0 || K <= 0) return RFLU_OK;
    const int64_t tiles_m = (M + CG_BM - 1) / CG_BM, tiles_n = (N + CG_BN - 1) / CG_BN;
    if (tiles_n > INT32_MAX || tiles_m * tiles_n > INT32_MAX) { set_error("complex gemm: %lld x %lld is beyond one launch", (long long)M, (long long)N); return RFLU_ERR_ARG; }
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    // 16-byte loads of the operands (Float32: two elements, so even strides) and element-aligned vector accesses to C
    const bool strides_ok = sizeof(R) == 8 || (lda % 2 == 0 && ldb % 2 == 0);
    CGemmArgs<R> g{M, N, K, A, lda, B, ldb, C, ldc, (int)tiles_n, (al16(A) && al16(B) && al16(C) && strides_ok) ? 1 : 0};
    ProfScope ps(h, RFLU_K_GEMM, 8.0 * (double)M * (double)N * (double)K,
                 2.0 * sizeof(R) * ((double)M * K + (double)K * N + 2.0 * (double)M * N));
    hipLaunchKernelGGL(cgemm_sub_kernel<R>, dim3((unsigned)(tiles_m * tiles_n)), dim3(256), 0, h->stream, g);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

template int launch_cgemm<double>(Handle*, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*, int64_t);
template int launch_cgemm<float>(Handle*, int64_t, int64_t, int64_t, const float*, int64_t, const float*, int64_t, float*, int64_t);

}  // namespace rflu
