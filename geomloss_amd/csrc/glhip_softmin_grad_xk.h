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
//   splits     partials (sums of nv centred features, mass, m) as in the plan kernels; xk_grad_merge_kernel brings the splits to the
//              largest m, adds, divides and applies the same epilogue — the centre row of row i is (i / kXkRows) kXkRows of its batch item.
//
// A pass covers 64 coordinates (NCH = 2), a remainder of <= 32 runs as NCH = 1: ceil(D / 64) passes, each with its own exponent half.
//   registers / LDS / scratch (gfx950, tools/kernel_resources.py, profiles/xk_shared_stage.txt): 0 bytes of scratch in all eight
//   instantiations, LDS as the plan's (95.1 / 111.5 KiB).
//
// This header keeps the parameter struct and the merge of the column splits.  (One __global__ template, not a shared __device__ body
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

// Combines the column splits of a gradient pass: one thread per (row, coordinate).  The partials of a row are nv sums of centred
// coordinates and the mass — both relative to 2^m of their split — and m (plan_merge_kernel's format): brought to the largest m, added,
// divided, and put through the gradient epilogue of xk_plan_kernel.
template <typename T>
__global__ void __launch_bounds__(kBlock)
xk_grad_merge_kernel(XkGradParams<T> prm, int N, int D, long rows, SplitInfo sp) {
    const long id = (long)blockIdx.x * kBlock + threadIdx.x;
    const int nv = prm.nv;
    if (id >= rows * nv) return;
    const long row = id / nv;
    const int c = (int)(id - row * nv);
    const float* part = sp.workspace + row * (nv + 2);
    float mx = kMinusHuge;
    for (int k = 0; k < sp.n_splits; ++k) mx = fmaxf(mx, part[k * sp.split_stride + nv + 1]);
    float s = 0.f, w = 0.f;
    for (int k = 0; k < sp.n_splits; ++k) {
        const float rs = fast_exp2(part[k * sp.split_stride + nv + 1] - mx);
        s = __builtin_fmaf(part[k * sp.split_stride + c], rs, s);
        w = __builtin_fmaf(part[k * sp.split_stride + nv], rs, w);
    }
    const long i = row % N;
    const long crow = row - i + (i / kXkRows) * kXkRows;      // the first row of the row block, within the batch item
    const float xc = to_f32<T>(prm.x[row * D + prm.v0 + c]) - to_f32<T>(prm.x[crow * D + prm.v0 + c]);
    prm.gx[row * D + prm.v0 + c] = (w > 0.f) ? prm.g[row] * (xc - s / w) : 0.f;
}

}  // namespace glhip
