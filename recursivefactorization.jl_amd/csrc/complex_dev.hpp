// complex_dev.hpp -- the complex element and its arithmetic on the device, shared by the complex kernel sources
#pragma once
#include "complex.hpp"

namespace rflu {

template <typename R>
struct Cx {   // 2-word POD, the layout of Julia's Complex{R}
    R re, im;
};
template <typename R>
__device__ __forceinline__ Cx<R> cmul(Cx<R> a, Cx<R> b) { return Cx<R>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename R>
__device__ __forceinline__ Cx<R> csub(Cx<R> a, Cx<R> b) { return Cx<R>{a.re - b.re, a.im - b.im}; }
// acc + v * x as four fused multiply-adds in a fixed order (spelled out so that no two call sites can be contracted differently)
template <typename R>
__device__ __forceinline__ Cx<R> cfma(Cx<R> v, Cx<R> x, Cx<R> acc)
{
    return Cx<R>{fma(-v.im, x.im, fma(v.re, x.re, acc.re)), fma(v.im, x.re, fma(v.re, x.im, acc.im))};
}
__device__ __forceinline__ double cmodulus(Cx<double> z) { return hypot(z.re, z.im); }
__device__ __forceinline__ float cmodulus(Cx<float> z) { return hypotf(z.re, z.im); }
// a / b by Smith's formula (one reciprocal, no overflow of |b|^2); b == 0 gives Inf / NaN like the real division
template <typename R>
__device__ __forceinline__ Cx<R> cdiv(Cx<R> a, Cx<R> b)
{
    if (fabs(b.re) >= fabs(b.im)) {
        if (b.re == R(0) && b.im == R(0)) return Cx<R>{a.re / fabs(b.re), a.im / fabs(b.im)};
        const R rat = b.im / b.re, scl = R(1) / (b.re + b.im * rat);
        return Cx<R>{(a.re + a.im * rat) * scl, (a.im - a.re * rat) * scl};
    }
    const R rat = b.re / b.im, scl = R(1) / (b.re * rat + b.im);
    return Cx<R>{(a.re * rat + a.im) * scl, (a.im * rat - a.re) * scl};
}

}  // namespace rflu
