// glhip_api_grad_xk.hip — C-ABI part 10: the p = 2 soft-min gradient of 17 <= D <= 4095 on the matrix cores (GLHIP_FLAG_XK_GRAD):
// xk_plan_kernel on XkGradParams (glhip_softmin_grad_xk.h), launched by glhip_softmin_bwd_x (glhip_api_bwd.hip) where softmin_bwd_family
// (glhip_family.h) says GLHIP_FAMILY_XK: what glhip_softmin_bwd_x_uses_plan reports.  A translation unit of its own: the parallel build
// does not get longer.
#include "glhip_grad_xk.h"
#include "glhip_launch_plan.h"
#include "glhip_softmin_grad_xk.h"

namespace glhip {

// The launch behind glhip_softmin_bwd_x under GLHIP_FLAG_XK_GRAD; the caller has checked the arguments and the family, and B, N > 0.
int softmin_grad_xk_launch(const void* x, const void* y, const float* h, const float* fwd, const float* g, float* gx, int B, int N, int M,
                           int D, float eps, int in_dtype, void* workspace, size_t workspace_bytes, int flags, hipStream_t st) {
    return xk_grad_launch(gx, nullptr, B, N, M, D, in_dtype, workspace, workspace_bytes, flags, st, [&](auto tag, const Scratch& sc) {
        using T = decltype(tag);
        const XkGradParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), h, fwd, g, gx, kLog2e / eps, -eps * kLn2, 0, 0};
        launch_xk_plan_passes(prm, D, B, N, M, D, sc, st);
    });
}

}  // namespace glhip

extern "C" {

int glhip_softmin_bwd_x_uses_plan(int B, long N, long M, int D, int p, int dtype, int flags, int n_ranges) {
    if (plan_family_bad_args(B, N, M, D, dtype, n_ranges) || (p != 1 && p != 2)) return GLHIP_EINVAL;
    return family_on_xk_route(softmin_bwd_family(1, B, N, M, D, p, flags, n_ranges), GLHIP_FAMILY_XK, D);
}

size_t glhip_softmin_bwd_x_workspace_bytes(int B, int N, int M, int D, int flags) {
    return xk_grad_workspace_bytes(glhip_softmin_bwd_x_uses_plan(B, N, M, D, 2, GLHIP_F32, flags, 0), B, N, M, D, flags, kXkPlanWidth);
}

}  // extern "C"
