// dropout_rng.h -- the counter-based keep-masks of every dropout site of the project (the contract: include/wsscam.h, DESIGN.md
// section 7): THE definition of the counter layout.  seg_dropout.hip (the SEC / DSRG sites) and cls_grad.hip (the 01_train sites
// behind a BatchNorm, forward and backward) include it; nothing else forms a counter.
//
//   element i of a site's [B][h][w][C] tensor (its linear NHWC index) draws Philox4x32-10 with key = (seed low, seed high) and
//   counter = (low(i >> 2), high(i >> 2), step, site) and takes output word i & 3; u = float(word >> 8) 2^-24 (exact); keep iff
//   u >= drop_prob in fp32; d = fmul_rn(y, scale) where kept, +0.0 where dropped, scale = 1.0f / (1.0f - drop_prob).
// A mask depends on (seed, step, site, i) alone.  Every product is spelled (__fmul_rn): the functions give the same bits under
// any -ffp-contract setting.
#pragma once
#include <cstdint>

struct DropRng {
    uint32_t k0, k1;   // the seed
    uint32_t step, site;
    float drop_prob, scale;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the four words of counter block `blk` (= element index >> 2)
__device__ __forceinline__ void drop_words(const DropRng &g, unsigned long long blk, uint32_t out[4]) {
    philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), g.step, g.site, g.k0, g.k1, out);
}
__device__ __forceinline__ bool drop_keeps(const DropRng &g, uint32_t word) { return (float)(word >> 8) * 0x1p-24f >= g.drop_prob; }
__device__ __forceinline__ float drop_value(const DropRng &g, float y, bool keep) { return keep ? __fmul_rn(y, g.scale) : 0.f; }

inline DropRng drop_rng(float drop_prob, unsigned long long seed, unsigned step, unsigned site) {
    DropRng g;
    g.k0 = (uint32_t)seed; g.k1 = (uint32_t)(seed >> 32);
    g.step = step; g.site = site;
    g.drop_prob = drop_prob;
    g.scale = 1.0f / (1.0f - drop_prob);
    return g;
}
