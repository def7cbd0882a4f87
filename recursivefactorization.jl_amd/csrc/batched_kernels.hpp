// batched_kernels.hpp -- what the batched kernels of batched.hip (Float64, Float32) and batched_complex.hip (ComplexF64, ComplexF32)
// share without a change to their code: the thread and LDS geometry of a group, the 64-bit-key wave maximum of
// the pivot search, and the launch.  The kernel bodies, the composition of the interchanges among them, stay in the two files:
// stated once as templates on the element they compiled to the same loops at other addresses, and that cost up to 2.5 %
// (profiles/batched_unified_ab.txt).
//
// Shape: a GROUP of 64 / 128 / 256 threads (max(m, n) <= 32 / 64 / 128) owns one matrix; a 256-thread workgroup holds 4 / 2 / 1 groups.
// The matrix is read from HBM once into LDS (column-major, odd leading dimension: a column AND a row are bank-conflict free), worked on
// there, and written once.  The matrices never talk to each other: no global-memory hand-off, no cooperative launch, nothing a
// workgroup could wait for -- one workgroup barrier per pivot column is all the synchronisation there is.
#pragma once
#include <algorithm>

#include "rflu_internal.hpp"

namespace rflu {
namespace batched {   // the short names below stay out of the project's namespace

typedef unsigned long long bu64;
constexpr int BT = 256;                   // threads per workgroup
constexpr int BNR = 8;                    // right-hand sides per pass of the solve
constexpr unsigned BPOS_NONE = 0x7fffffffu;

struct BGeo {
    int tpm;        // threads per matrix (64 | 128 | 256)
    int tpm_log;
    int rt_log;     // log2 of RT = rows of the (row, column-slice) thread grid: the smallest power of two >= m
    int ct_log;     // log2 of the same for the columns (row-major loads and stores: lanes along a row)
    int ld;         // LDS leading dimension in elements (odd)
    unsigned group_bytes;
    unsigned off_x;          // byte offsets inside a group's LDS: the right-hand sides (solve), then the sections after them in order:
    unsigned off_a, off_b;   // real elements: off_a = the integer arrays; complex: off_a = reciprocals of the diagonal, off_b = the integer arrays
};

inline int blog2_ceil(int64_t v)
{
    int l = 0;
    for (; ((int64_t)1 << l) < v; ++l) {}
    return l;
}

// esize: bytes of an element; recip_diag: the solve keeps n reciprocals of the diagonal in a section of its own (complex elements)
inline BGeo batched_geo(int64_t m, int64_t n, size_t esize, bool solve, bool recip_diag)
{
    BGeo g;
    const int64_t mx = std::max(m, n);
    g.tpm_log = mx <= 32 ? 6 : (mx <= 64 ? 7 : 8);
    g.tpm = 1 << g.tpm_log;
    g.rt_log = blog2_ceil(m);
    g.ct_log = blog2_ceil(n);
    g.ld = (int)(m | 1);
    size_t off = ((size_t)g.ld * (size_t)n * esize + 15) & ~(size_t)15;   // the base is 16-byte aligned: so is every section
    g.off_x = (unsigned)off;
    if (solve) off += ((size_t)g.ld * BNR * esize + 15) & ~(size_t)15;
    g.off_a = g.off_b = (unsigned)off;
    if (solve && recip_diag) off += ((size_t)n * esize + 15) & ~(size_t)15;
    if (recip_diag) g.off_b = (unsigned)off;
    off += ((size_t)(m + std::min(m, n)) * sizeof(int) + 15) & ~(size_t)15;
    g.group_bytes = (unsigned)off;
    return g;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ bu64 bdpp_max(bu64 v)
{
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    const bu64 o = ((bu64)(unsigned)ohi << 32) | (bu64)(unsigned)olo;
    return o > v ? o : v;
}
// maximum over the 64 lanes of a wave (all of them active), wave-uniform: the DPP ladder of panel_single.hip on 64-bit keys
__device__ __forceinline__ bu64 bwave_max(bu64 v)
{
    v = bdpp_max<0xB1, 0xf>(v);    // quad_perm:[1,0,3,2]
    v = bdpp_max<0x4E, 0xf>(v);    // quad_perm:[2,3,0,1]
    v = bdpp_max<0x141, 0xf>(v);   // row_half_mirror
    v = bdpp_max<0x140, 0xf>(v);   // row_mirror
    v = bdpp_max<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v = bdpp_max<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3: lane 63 holds the maximum
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((bu64)hi << 32) | (bu64)lo;
}

// the launch of one batched kernel.  `which`: 0 = getrf, 1 = getrs, 2 = getri; slot: 0 = f64, 1 = f32, 2 = cf64, 3 = cf32 (row and
// column of Handle::batched_attr_set).  work, bytes: what the profile counts for the call.
template <typename Args>
int launch_batched(Handle* h, int which, int slot, void (*kernel)(Args), const Args& a, int64_t batch, int kind, double work, double bytes)
{
    const int groups = BT / a.g.tpm;
    const size_t lds = (size_t)groups * a.g.group_bytes;
    bool* done = &h->batched_attr_set[which][slot];
    if (lds > 64 * 1024 && !*done) {   // above the default limit a kernel has to ask once (160 KiB per CU on gfx950)
        RFLU_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        *done = true;
    }
    const int64_t wgs = (batch + groups - 1) / groups;
    ProfScope ps(h, kind, work, bytes);
    hipLaunchKernelGGL(kernel, dim3((unsigned)wgs), dim3(BT), lds, h->stream, a);
    RFLU_HIP(hipGetLastError());
    return RFLU_OK;
}

}  // namespace batched
}  // namespace rflu
