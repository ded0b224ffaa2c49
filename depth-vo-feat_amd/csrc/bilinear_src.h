// Source index rule of F.interpolate(mode='bilinear', align_corners=False), shared by the bilinear resize kernels
// (elementwise.hip) and the integer-factor upsampling pair (upsample.hip).
#pragma once
#include <hip/hip_runtime.h>

// aten area_pixel_compute_source_index(scale, dst, align_corners=False, cubic=False)
__device__ __forceinline__ void up_src(int dst, float scale, int in_size, int &i0, int &i1, float &lam) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;                       // floor: src >= 0
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
    lam = src - (float)i0;
    if (lam < 0.f) lam = 0.f;
    if (lam > 1.f) lam = 1.f;
}
