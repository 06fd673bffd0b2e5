// gspl_resample.h — one axis of F.interpolate(mode="bilinear", align_corners=False), shared by spotless.hip and segany.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace gspl {

struct SlsAxis {
    int i0, i1;
    float l, h;      // weights of i1 and i0
};

// output index o of an axis resampled from I to O entries; scale = (float)I / (float)O
__device__ __forceinline__ SlsAxis sls_axis(float scale, int o, int I) {
#pragma clang fp contract(off)
    const float centre = (float)o + 0.5f;
    float src = fmaf(scale, centre, -0.5f);      // ONE rounding: torch's kernels, CPU and GPU, are compiled with this product and sum fused
    src = src < 0.f ? 0.f : src;
    SlsAxis a;
    a.i0 = min((int)src, I - 1);
    a.i1 = min(a.i0 + 1, I - 1);
    a.l = fminf(fmaxf(src - (float)a.i0, 0.f), 1.f);
    a.h = 1.f - a.l;
    return a;
}

}  // namespace gspl
