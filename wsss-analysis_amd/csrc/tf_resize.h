// tf_resize.h -- the sampler of TensorFlow 1.x tf.image.resize_bilinear(align_corners=False), the legacy one WITHOUT the half-pixel
// offset (seg_chain.hip; deeplab.hip's resize_bilinear_tf_kernel takes tf_lerp and keeps tf_tap's lines written out for two axes):
//   scale = in / out (float32); src = dst * scale; i0 = floor(src), i1 = min(i0 + 1, in - 1), t = src - i0
//   top = tl + (tr - tl) tx, bottom = bl + (br - bl) tx, out = top + (bottom - top) ty
// The lerps are the products and sums written here, each rounded on its own: a file that includes this header MUST be compiled
// with -ffp-contract=off (EXTRA_FLAGS of the build), or the compiler fuses them into FMAs and the bits are no longer TF's.
#pragma once
#include <hip/hip_runtime.h>

// taps and weight of one output coordinate
__device__ __forceinline__ void tf_tap(int dst, float scale, int in, int &i0, int &i1, float &t) {
    const float f = (float)dst * scale;
    i0 = min((int)floorf(f), in - 1); // (floor(src) <= in - 1 but for rounding of the product)
    i1 = min(i0 + 1, in - 1);
    t = f - (float)i0;
}

__device__ __forceinline__ float tf_lerp(float tl, float tr, float bl, float br, float tx, float ty) {
    const float top = tl + (tr - tl) * tx;
    const float bottom = bl + (br - bl) * tx;
    return top + (bottom - top) * ty;
}
