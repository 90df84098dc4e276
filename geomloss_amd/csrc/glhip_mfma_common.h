// glhip_mfma_common.h — what the matrix-core kernels share: the bf16 x 3 split of fp32 operands, the constants of the lazy running
// max, and the row tiling of the 16x16x32 weighted-sum kernels (glhip_wsum_mfma.h).
//
// bf16 x 3.  Every fp32 number is the exact sum of three bf16 numbers (8 + 8 + 8 significand bits, obtained by truncation), so
//     a * y = (a1 + a2 + a3)(y1 + y2 + y3) = a1y1 + a1y2 + a2y1 + a1y3 + a3y1 + a2y2 + a2y3 + a3y2   (+ a3y3 ~ 2^-32)
// — 8 exact bf16 products per coordinate, accumulated in fp32 by a bf16 MFMA (K = 32 slots on v_mfma_f32_16x16x32_bf16, 16 on
// v_mfma_f32_32x32x16_bf16) at fp32 accuracy.  Per coordinate, the row side holds [a1,a1,a2,a1,a3,a2,a2,a3] (pack_a) and the
// column side [y1,y2,y1,y3,y1,y2,y3,y2] (pack_y); a scalar H_j enters as [H1,H2,H3,0,...] against [1,1,1,0,...] (pack_h).
//
// Lazy running max (the soft-min kernels).  The first column group of a row initialises its max m exactly.  After that a whole
// LDS tile is accumulated speculatively with -m folded into the exponents and NO per-pair max / compare at all; only at the end of
// the tile are the tile sums checked: if one passed kSumThr = 2^100 (a term ~2^80 above m arrived, or overflowed to +inf / NaN) the
// tile is redone from the untouched old sums with exact per-group maxima.  m <= true max always, nothing can overflow unnoticed,
// and the hot loop is branch-free so the compiler can pipeline across column groups.
#pragma once

#include "glhip_mapreduce.h"
#include "glhip_softmin_ops.h"

namespace glhip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kMfmaRT = 4;                            // 16-row tiles per wavefront (weighted-sum kernels)
constexpr int kMfmaRowsPerWave = kMfmaRT * 16;        // 64
constexpr int kMfmaRowsPerBlock = 4 * kMfmaRowsPerWave;   // 256
constexpr float kSumThr = 1.2676506e30f;            // 2^100: refresh the lazy max when a row sum passes it
constexpr float kMinusHuge = -3.0e38f;
constexpr int kTileX = 512;                 // columns per LDS tile: 32 groups x 64 lanes x 16 B = 32 KiB

__device__ __forceinline__ f32x4 exp2v(f32x4 v) {
    return f32x4{fast_exp2(v.x), fast_exp2(v.y), fast_exp2(v.z), fast_exp2(v.w)};
}

union Pack16 { uint4 u; bf16x8 v; };

// three bf16 numbers (as the high halves of fp32 bit patterns) whose sum is v, by truncation
__device__ __forceinline__ void split3(float v, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
    const uint32_t b1 = __float_as_uint(v) & 0xFFFF0000u;
    const float f1 = __uint_as_float(b1);
    float r = v - f1;                                  // exact
    if ((b1 & 0x7F800000u) == 0x7F800000u) r = 0.f;    // inf / nan stay in the first piece only
    const uint32_t b2 = __float_as_uint(r) & 0xFFFF0000u;
    const float r2 = r - __uint_as_float(b2);          // exact
    p1 = b1 >> 16;
    p2 = b2 >> 16;
    p3 = __float_as_uint(r2) >> 16;
}

__device__ __forceinline__ uint4 pack_a(float a) {     // [a1,a1,a2,a1,a3,a2,a2,a3]
    uint32_t p1, p2, p3;
    split3(a, p1, p2, p3);
    return uint4{p1 | (p1 << 16), p2 | (p1 << 16), p3 | (p2 << 16), p2 | (p3 << 16)};
}
__device__ __forceinline__ uint4 pack_y(float y) {     // [y1,y2,y1,y3,y1,y2,y3,y2]
    uint32_t p1, p2, p3;
    split3(y, p1, p2, p3);
    return uint4{p1 | (p2 << 16), p1 | (p3 << 16), p1 | (p2 << 16), p3 | (p2 << 16)};
}
__device__ __forceinline__ uint4 pack_h(float h) {     // [H1,H2,H3,0,0,0,0,0]
    uint32_t p1, p2, p3;
    split3(h, p1, p2, p3);
    return uint4{p1 | (p2 << 16), p3, 0u, 0u};
}

__device__ __forceinline__ f32x4 mfma_x(const uint4& a, const uint4& b, f32x4 c) {
    Pack16 pa, pb;
    pa.u = a;
    pb.u = b;
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa.v, pb.v, c, 0, 0, 0);
}

}  // namespace glhip
