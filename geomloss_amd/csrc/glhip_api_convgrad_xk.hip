// glhip_api_convgrad_xk.hip — C-ABI part 12: the gradient of the gaussian kernel product of 17 <= D <= 4095 on the matrix cores
// (GLHIP_FLAG_XK_GRAD): xk_plan_kernel on XkGaussGradParams (glhip_gauss_grad_xk.h), launched by glhip_kernel_conv_bwd_x and
// glhip_kernel_conv_fwd_grad (glhip_api_convgrad.hip) where glhip_kernel_conv_grad_uses_xk says so.  A translation unit of its own: the
// parallel build does not get longer.
#include "glhip_launch_plan.h"
#include "glhip_gauss_grad_xk.h"

namespace {

// THE predicate of the GLHIP_FLAG_XK_GRAD route of glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad, and what
// glhip_kernel_conv_grad_uses_xk reports.  Host arithmetic only.
inline int conv_grad_uses_xk(int kind, int B, long N, long M, int D, int dtype, int flags, int n_ranges) {
    if (kind < GLHIP_GAUSSIAN || kind > GLHIP_ENERGY || plan_family_bad_args(B, N, M, D, dtype, n_ranges)) return GLHIP_EINVAL;
    if (!(flags & GLHIP_FLAG_XK_GRAD) || (flags & (GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_DIRECT))) return 0;
    return (kind == GLHIP_GAUSSIAN && D > kXdMaxD && D <= kXkMaxD && n_ranges == 0 && B <= 65535) ? 1 : 0;
}

}  // namespace

namespace glhip {

// The launch behind glhip_kernel_conv_bwd_x (out NULL) and glhip_kernel_conv_fwd_grad (g NULL) under GLHIP_FLAG_XK_GRAD; the caller has
// checked the arguments and the predicate, and B, N > 0.
int gauss_grad_xk_launch(const void* x, const void* y, const float* v, const float* g, float* out, float* gx, int B, int N, int M, int D,
                         float blur, int in_dtype, void* workspace, size_t workspace_bytes, int flags, hipStream_t st) {
    if (M == 0) {      // no columns: empty sums
        (void)hipMemsetAsync(gx, 0, (size_t)B * N * D * sizeof(float), st);
        if (out) (void)hipMemsetAsync(out, 0, (size_t)B * N * sizeof(float), st);
        return GLHIP_OK;
    }
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, 0, N);
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const XkGaussGradParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), v, g, gx, out, kLog2e / (blur * blur),
                                       1.0f / (blur * blur), 0, 0};
        launch_xk_plan_passes(prm, D, B, N, M, D, sc, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return GLHIP_OK;
}

}  // namespace glhip

extern "C" {

int glhip_kernel_conv_grad_uses_xk(int kind, int B, long N, long M, int D, int dtype, int flags, int n_ranges) {
    return conv_grad_uses_xk(kind, B, N, M, D, dtype, flags, n_ranges);
}

size_t glhip_kernel_conv_grad_workspace_bytes(int B, int N, int M, int D, int flags) {
    if (B <= 0 || N <= 0 || M <= 0 || (flags & GLHIP_FLAG_NO_SPLIT)) return 0;
    if (conv_grad_uses_xk(GLHIP_GAUSSIAN, B, N, M, D, GLHIP_F32, flags, 0) != 1) return 0;
    return plan_pass_workspace_bytes(B, N, M, kXkRows, D < kXkPlanWidth ? D : kXkPlanWidth, {kXkPlanSlots});
}

}  // extern "C"
