// glhip_softmin_grad_xk.h — the gradient of a p = 2 soft-min with respect to the row points on the matrix cores, 17 <= D <= 4095:
//
//     grad_x[i][d] = g_i ( x_i[d] - sum_j w_ij y_j[d] / sum_j w_ij ),      w_ij as in glhip_plan_apply_xk.h
//
// i.e. the transport plan applied to the column cloud itself.  It runs xk_plan_kernel (glhip_plan_apply_xk.h) instantiated on
// XkGradParams: the exponent half, the weights relative to the running row maximum times 2^kWqShift, the mass from the fp32 weights,
// the two f16 pieces under a power-of-two scale per feature column and tile, six MFMAs per chunk into a fresh accumulator per
// 32-column block and the meeting of the two column halves are that kernel's; three things differ (`if constexpr (GRAD)` there).
//
//   features   feature c of a pass that starts at coordinate v0 is to_f32(y[j][v0 + c]) - to_f32(centre[v0 + c]), read in the cloud's
//              dtype: no feat pointer, no fp32 copy of a bf16 cloud.  centre = the first row of the row block, which the exponent half
//              centres on already.  Centred features keep x_i - ybar_i free of cancellation for clouds far from the origin: both
//              terms of the epilogue are of the size of the cloud's diameter.
//   epilogue   unsplit launches write grad_x[b][i][v0 + c] = g_i ((x_i[c] - centre[c]) - s / w); 0 for a row without mass (w == 0).
//              The division stays a division: a one-hot plan row gives x_i - y_j exactly.
//   splits     partials (sums of nv centred features, mass, m) as in the plan kernels; plan_merge_kernel brings the splits to the
//              largest m and adds, plan_merge_store below divides and applies the same epilogue — the centre row of row i is (i / kXkRows) kXkRows of its batch item.
//
// A pass covers 64 coordinates (NCH = 2), a remainder of <= 32 runs as NCH = 1: ceil(D / 64) passes, each with its own exponent half.
//   registers / LDS / scratch (gfx950, tools/kernel_resources.py, profiles/xk_shared_stage.txt): 0 bytes of scratch in all eight
//   instantiations, LDS as the plan's (95.1 / 111.5 KiB).
//
// This header keeps the parameter struct and its end of the merge of the column splits.  (One __global__ template, not a shared __device__ body
// behind two __global__ wrappers: that cost the plan kernel 30 VGPRs at NCH = 1 and spilled at NCH = 2 — glhip_plan_apply_xk.h.)
#pragma once

#include "glhip_plan_apply_xk.h"

namespace glhip {

template <typename T>
struct XkGradParams {
    const T* x;           // (B,N,D)
    const T* y;           // (B,M,D)
    const float* h;       // (B,M)
    const float* fwd;     // (B,N): the saved soft-min
    const float* g;       // (B,N): the incoming gradient
    float* gx;            // (B,N,D)
    float s2;             // log2(e) / eps
    float out_scale;      // -eps ln 2: LSE2_i = fwd_i / out_scale
    int v0;               // first coordinate of this pass
    int nv;               // coordinates of this pass, <= 32 NCH
};

// The gradient's end of plan_merge_kernel (glhip_plan_apply.h): the merged sum s of centred coordinate c and the mass w of a row, divided
// and put through the gradient epilogue of xk_plan_kernel.
template <typename T>
__device__ __forceinline__ void plan_merge_store(const XkGradParams<T>& prm, int N, int D, long row, int c, float s, float w, float) {
    const long i = row % N;
    const long crow = row - i + (i / kXkRows) * kXkRows;      // the first row of the row block, within the batch item
    const float xc = to_f32<T>(prm.x[row * D + prm.v0 + c]) - to_f32<T>(prm.x[crow * D + prm.v0 + c]);
    prm.gx[row * D + prm.v0 + c] = (w > 0.f) ? prm.g[row] * (xc - s / w) : 0.f;
}

}  // namespace glhip
