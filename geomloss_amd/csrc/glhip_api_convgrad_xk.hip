// glhip_api_convgrad_xk.hip — C-ABI part 12: the gradient of the gaussian kernel product of 17 <= D <= 4095 on the matrix cores
// (GLHIP_FLAG_XK_GRAD): xk_plan_kernel on XkGaussGradParams (glhip_gauss_grad_xk.h), launched by glhip_kernel_conv_bwd_x and
// glhip_kernel_conv_fwd_grad (glhip_api_convgrad.hip) where conv_family (glhip_family.h) says GLHIP_FAMILY_XK: what
// glhip_kernel_conv_grad_uses_xk reports.  A translation unit of its own: the
// parallel build does not get longer.
#include "glhip_grad_xk.h"
#include "glhip_launch_plan.h"
#include "glhip_gauss_grad_xk.h"

namespace glhip {

// The launch behind glhip_kernel_conv_bwd_x (out NULL) and glhip_kernel_conv_fwd_grad (g NULL) under GLHIP_FLAG_XK_GRAD; the caller has
// checked the arguments and the family, and B, N > 0.
int gauss_grad_xk_launch(const void* x, const void* y, const float* v, const float* g, float* out, float* gx, int B, int N, int M, int D,
                         float blur, int in_dtype, void* workspace, size_t workspace_bytes, int flags, hipStream_t st) {
    return xk_grad_launch(gx, out, B, N, M, D, in_dtype, workspace, workspace_bytes, flags, st, [&](auto tag, const Scratch& sc) {
        using T = decltype(tag);
        const XkGaussGradParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), v, g, gx, out, kLog2e / (blur * blur),
                                       1.0f / (blur * blur), 0, 0};
        launch_xk_plan_passes(prm, D, B, N, M, D, sc, st);
    });
}

}  // namespace glhip

extern "C" {

int glhip_kernel_conv_grad_uses_xk(int kind, int B, long N, long M, int D, int dtype, int flags, int n_ranges) {
    if (kind < GLHIP_GAUSSIAN || kind > GLHIP_ENERGY || plan_family_bad_args(B, N, M, D, dtype, n_ranges)) return GLHIP_EINVAL;
    return family_on_xk_route(conv_family(kind, 1, B, D, flags, n_ranges), GLHIP_FAMILY_XK, D);
}

size_t glhip_kernel_conv_grad_workspace_bytes(int B, int N, int M, int D, int flags) {
    return xk_grad_workspace_bytes(glhip_kernel_conv_grad_uses_xk(GLHIP_GAUSSIAN, B, N, M, D, GLHIP_F32, flags, 0), B, N, M, D, flags, kXkPlanWidth);
}

}  // extern "C"
