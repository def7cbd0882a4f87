// mixed_dev.hpp -- what the real (mixed.hip) and the complex (complex_mixed.hip) mixed-precision kernels share: the NaN-keeping maximum
// and the second stage of ||A||_inf.
#pragma once
#include "rflu_internal.hpp"

namespace rflu {

// max that keeps a NaN once it has seen one (fmax drops it): a NaN or Inf anywhere must reach the host's convergence test
__device__ __forceinline__ double nanmax(double m, double v) { return (v > m || v != v) ? v : m; }

// all 256 threads of the workgroup call it; thread 0 holds the result (fixed tree: the same order every run)
__device__ __forceinline__ double block_nanmax(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = nanmax(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    return sh[0];
}

// mixed.hip: *out (device) <- the largest over rows i < n of part[0 * n + i] + part[1 * n + i] + ... (ntj terms, in that order);
// blockmax: ceil(n / 256) doubles of workspace (rowsum_max_kernel, final_max_kernel)
int launch_rowsum_max(Handle* h, int64_t n, int64_t ntj, const double* part, double* blockmax, double* out);

}  // namespace rflu
