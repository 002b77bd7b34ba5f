// pil_nearest.h -- the index table of PIL's Image.resize(NEAREST), shared by irn_batch.hip and cls_batch.hip.
#pragma once

#include <stdint.h>

#include <vector>

// ImagingScaleAffine's (Geometry.c) source index of every output index of an axis in -> out: a = in / out, v = a / 2, per index
// idx = (int)v, v += a -- the running sum in double, not i * a.  Appended to tab; -> the int32 index of the section.
inline int pil_add_nearest(std::vector<int32_t> &tab, int in, int out) {
    const size_t off = tab.size();
    tab.resize(off + out);
    const double a = (double)in / (double)out;
    double v = a * 0.5;
    for (int i = 0; i < out; ++i) {
        int idx = (int)v;
        tab[off + i] = idx < in ? idx : in - 1; // (PIL leaves such a pixel unwritten; it does not occur below 2^31 / in outputs)
        v += a;
    }
    return (int)off;
}
