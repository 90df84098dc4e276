// glhip_gauss_grad_xk.h — the gradient of a gaussian kernel product with respect to the row points on the matrix cores, 17 <= D <= 4095:
//
//     k_ij = exp(-|x_i - y_j|^2 / 2 blur^2),   U_i = sum_j k_ij v_j,   S_i = sum_j k_ij v_j (y_j - c),   c = first row of the row block
//     dU_i/dx_i = (1 / blur^2) [ S_i - (x_i - c) U_i ]            glhip_kernel_conv_fwd_grad: grad_unit (and out = U)
//     grad_x[i] = g_i dU_i/dx_i                                   glhip_kernel_conv_bwd_x
//
// A plan application without the normalisation: xk_plan_kernel (glhip_plan_apply_xk.h) instantiated on XkGaussGradParams, its third
// instantiation (`if constexpr (GAUSS)` there).  The exponent half, the weights relative to the running row maximum times 2^kWqShift in
// two f16 pieces, the features in two f16 pieces under a power-of-two scale per column and tile, six MFMAs per chunk and the meeting of
// the two column halves are that kernel's.  What differs:
//
//   exponents  those of the gaussian product (xk_fwd_kernel, XD_GAUSS): eps = blur^2, H_j = -s/2 |yt_j|^2, C_i = -s/2 |xt_i|^2, no dual
//              and no saved forward value.  u_ij <= 0 up to rounding, so 2^m never overflows.
//   features   v_j (to_f32(y[j][v0 + c]) - to_f32(centre[v0 + c])), read in the cloud's dtype; padded columns contribute 0.
//   mass       the SIGNED sum W = sum_j w_ij v_j, on the VALU from the unsplit fp32 weights; lds.xk.v carries v_j of the tile (0 for padded
//              columns: with their zero features they weigh exactly 0 in both layouts).  The running maximum m is taken over the
//              exponents only.
//   epilogue   nothing is row-normalised: gx = g_i / blur^2 2^m (S - xc W), xc = x_i - centre; fwd_grad (g == NULL) leaves g_i out and
//              writes out_i = 2^m W on the pass with v0 == 0.
//   empty rows W can be exactly 0 while S is not (two columns of weights +v and -v at equal distance), so a row is empty only when no
//              column reached it: 2^m == 0 (m still at its initial value, or the power underflowed).  Such a row writes 0, never NaN.
//   splits     partials (S[nv], W, m) per split as the soft-min gradient's; plan_merge_kernel brings the splits to the largest
//              m and adds them, plan_merge_store below applies the same epilogue with the centre row (i / kXkRows) kXkRows.
//
// Passes of 64 coordinates (NCH = 2), a remainder of <= 32 as NCH = 1, as the soft-min gradient.
//   registers / LDS / scratch (gfx950, tools/kernel_resources.py, profiles/gauss_grad_xk.txt): 0 bytes of scratch in all eight
//   instantiations, LDS as the plan's (95.1 / 111.5 KiB).
#pragma once

#include "glhip_plan_apply_xk.h"

namespace glhip {

template <typename T>
struct XkGaussGradParams {
    const T* x;           // (B,N,D)
    const T* y;           // (B,M,D)
    const float* v;       // (B,M): the signed weights of the columns
    const float* g;       // (B,N): the incoming gradient; NULL (fwd_grad): 1
    float* gx;            // (B,N,D)
    float* out;           // (B,N): U_i, written on the pass with v0 == 0; NULL: not wanted
    float s2;             // log2(e) / blur^2
    float gscale;         // 1 / blur^2
    int v0;               // first coordinate of this pass
    int nv;               // coordinates of this pass, <= 32 NCH
};

// The gaussian gradient's end of plan_merge_kernel (glhip_plan_apply.h): the merged sums S of coordinate c and W of a row, both relative
// to 2^mx, put through the unnormalised epilogue of xk_plan_kernel.
template <typename T>
__device__ __forceinline__ void plan_merge_store(const XkGaussGradParams<T>& prm, int N, int D, long row, int c, float s, float w, float mx) {
    const long i = row % N;
    const long crow = row - i + (i / kXkRows) * kXkRows;      // the first row of the row block, within the batch item
    const float xc = to_f32<T>(prm.x[row * D + prm.v0 + c]) - to_f32<T>(prm.x[crow * D + prm.v0 + c]);
    const float e2m = fast_exp2(mx);
    const float gs = prm.g ? prm.g[row] * prm.gscale : prm.gscale;
    prm.gx[row * D + prm.v0 + c] = xk_gauss_grad_entry(s, w, xc, e2m, gs);
    if (c == 0 && prm.out && prm.v0 == 0) prm.out[row] = (e2m > 0.f) ? w * e2m : 0.f;
}

}  // namespace glhip
