// glhip_api_distgrad_xk.hip — C-ABI part 13: the row gradients of the distance reductions of 17 <= D <= 4095 on the matrix cores
// (GLHIP_FLAG_XK_DIST_GRAD): xk_dist_grad_kernel (glhip_dist_grad_xk.h), launched by glhip_softmin_bwd_x with p = 1 (glhip_api_bwd.hip) and
// by glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad of the laplacian and energy kernels (glhip_api_convgrad.hip) where
// softmin_bwd_family / conv_family (glhip_family.h) say GLHIP_FAMILY_DIST beyond D = 16: what glhip_dist_grad_uses_xk reports.  A translation
// unit of its own: the parallel build does not get longer.
#include "glhip_grad_xk.h"
#include "glhip_launch_plan.h"
#include "glhip_dist_grad_xk.h"

namespace {

constexpr int kXkDistGradWidth = 32 * glhip::kXkDistGradChunks;      // coordinates per pass of xk_dist_grad_kernel

// The passes over the D coordinates, kXkDistGradWidth at a time: one chunk each
template <int MODE, typename T>
void launch_dist_grad_passes(const XkDistGradParams<MODE, T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_passes(prm, D, kXkDistGradWidth, [&](const XkDistGradParams<MODE, T>& pass, int) {
        launch_plan_pass(kXkRows, pass.nv + 2, kXkPlanSlots, B, N, M, sc, st,
            [&](dim3 grid, const SplitInfo& sp) {
                hipLaunchKernelGGL((xk_dist_grad_kernel<MODE, T, kXkDistGradChunks>), grid, dim3(kXkThreads), 0, st, pass, N, M, D, sp);
            },
            [&](const SplitInfo& sp) { launch_plan_merge(pass, B, N, D, sp, st); });
    });
}

}  // namespace

namespace glhip {

// The launch behind glhip_softmin_bwd_x (p = 1: op GLHIP_DIST_GRAD_SOFTMIN_P1, s = h, scale = eps), glhip_kernel_conv_bwd_x (out NULL) and
// glhip_kernel_conv_fwd_grad (g NULL) of the laplacian / energy kernels (s = v, scale = blur) under GLHIP_FLAG_XK_DIST_GRAD; the caller has
// checked the arguments and the family, and B, N > 0.
int dist_grad_xk_launch(int op, const void* x, const void* y, const float* s, const float* g, float* out, float* gx, int B, int N, int M, int D,
                        float scale, int in_dtype, void* workspace, size_t workspace_bytes, int flags, hipStream_t st) {
    return xk_grad_launch(gx, out, B, N, M, D, in_dtype, workspace, workspace_bytes, flags, st, [&](auto tag, const Scratch& sc) {
        using T = decltype(tag);
        const T* xp = static_cast<const T*>(x);
        const T* yp = static_cast<const T*>(y);
        if (op == GLHIP_DIST_GRAD_SOFTMIN_P1) {      // the scales of make_softmin_params with p = 1
            const float t = kLog2e / scale;
            launch_dist_grad_passes(XkDistGradParams<DM_SOFTMIN_P1, T>{xp, yp, s, g, gx, nullptr, t, 1e-8f * t * t, dist_guard(), 1.f, 0, 0}, B, N, M, D, sc, st);
        } else if (op == GLHIP_DIST_GRAD_LAPLACIAN) {
            const ConvParams<T> c = make_conv_params<T>(GLHIP_LAPLACIAN, x, y, s, out, g, gx, scale);
            launch_dist_grad_passes(XkDistGradParams<DM_LAPLACIAN, T>{xp, yp, s, g, gx, out, c.t, c.clamp2, dist_guard(), c.gscale, 0, 0}, B, N, M, D, sc, st);
        } else {
            const ConvParams<T> c = make_conv_params<T>(GLHIP_ENERGY, x, y, s, out, g, gx, scale);
            launch_dist_grad_passes(XkDistGradParams<DM_ENERGY, T>{xp, yp, s, g, gx, out, c.t, c.clamp2, dist_guard(), c.gscale, 0, 0}, B, N, M, D, sc, st);
        }
    });
}

}  // namespace glhip

extern "C" {

int glhip_dist_grad_uses_xk(int op, int B, long N, long M, int D, int dtype, int flags, int n_ranges) {
    if (op < GLHIP_DIST_GRAD_SOFTMIN_P1 || op > GLHIP_DIST_GRAD_ENERGY || plan_family_bad_args(B, N, M, D, dtype, n_ranges)) return GLHIP_EINVAL;
    const int fam = op == GLHIP_DIST_GRAD_SOFTMIN_P1 ? softmin_bwd_family(1, B, N, M, D, 1, flags, n_ranges)
                                                     : conv_family(op /* = kind */, 1, B, D, flags, n_ranges);
    return family_on_xk_route(fam, GLHIP_FAMILY_DIST, D);
}

size_t glhip_dist_grad_workspace_bytes(int B, int N, int M, int D, int flags) {
    return xk_grad_workspace_bytes(glhip_dist_grad_uses_xk(GLHIP_DIST_GRAD_SOFTMIN_P1, B, N, M, D, GLHIP_F32, flags, 0), B, N, M, D, flags, kXkDistGradWidth);
}

int glhip_dist_grad_pass_width(void) { return kXkDistGradWidth; }

}  // extern "C"
