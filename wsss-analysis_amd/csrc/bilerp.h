// bilerp.h -- the bilinear sampler every kernel that resizes a float map shares (cam_tail.hip, cue_seeds.hip).
// Arithmetic of torch's CPU kernel for align_corners=False:
//   scale = in/out (fp32); src = scale*(dst+0.5)-0.5, clamped at 0; i0=(int)src;
//   i1 = i0 + (i0 < in-1); l1 = src - i0; l0 = 1 - l1;
//   out = lh0*(lw0*a + lw1*b) + lh1*(lw0*c + lw1*d)
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void src_index(int dst, float scale, int in, int &i0, int &i1, float &l0, float &l1) {
    float s = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    l0 = 1.f - l1;
}

__device__ __forceinline__ float bilerp(const float *src, int w, int y0, int y1, float ly0, float ly1, int x0, int x1,
                                        float lx0, float lx1) {
    // the fused multiply-adds are spelled out (not left to -ffp-contract): every kernel that samples a map --
    // cam_tail_kernel, cam_max_kernel, cam_unary_kernel, bilinear_kernel, cue_maps_kernel -- then computes the same bits
    const float top = __builtin_fmaf(lx0, src[y0 * w + x0], lx1 * src[y0 * w + x1]);
    const float bot = __builtin_fmaf(lx0, src[y1 * w + x0], lx1 * src[y1 * w + x1]);
    return __builtin_fmaf(ly0, top, ly1 * bot);
}

// bilerp on four taps already loaded (a strided or gated source): a = (y0, x0), b = (y0, x1), c = (y1, x0), d = (y1, x1)
__device__ __forceinline__ float bilerp4(float a, float b, float c, float d, float ly0, float ly1, float lx0, float lx1) {
    const float t[4] = {a, b, c, d};
    return bilerp(t, 2, 0, 1, ly0, ly1, 0, 1, lx0, lx1);
}
