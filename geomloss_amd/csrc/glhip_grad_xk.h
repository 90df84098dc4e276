// glhip_grad_xk.h — the launches behind the matrix-core gradient routes of 17 <= D <= 4095, each defined in a translation unit of its own
// and called by glhip_softmin_bwd_x (glhip_api_bwd.hip) and glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad (glhip_api_convgrad.hip) where
// softmin_bwd_family / conv_family (glhip_family.h) say GLHIP_FAMILY_XK, or GLHIP_FAMILY_DIST beyond D = 16.  The caller has checked the
// arguments and the family, and B, N > 0.
#pragma once

#include <cstddef>
#include <hip/hip_runtime.h>

namespace glhip {

// glhip_api_grad_xk.hip: GLHIP_FLAG_XK_GRAD, p = 2 soft-min (xk_plan_kernel on XkGradParams, glhip_softmin_grad_xk.h)
int softmin_grad_xk_launch(const void* x, const void* y, const float* h, const float* fwd, const float* g, float* gx, int B, int N, int M,
                           int D, float eps, int in_dtype, void* workspace, size_t workspace_bytes, int flags, hipStream_t st);
// glhip_api_convgrad_xk.hip: GLHIP_FLAG_XK_GRAD, gaussian product (xk_plan_kernel on XkGaussGradParams, glhip_gauss_grad_xk.h); bwd_x: out NULL,
// fwd_grad: g NULL
int gauss_grad_xk_launch(const void* x, const void* y, const float* v, const float* g, float* out, float* gx, int B, int N, int M, int D,
                         float blur, int in_dtype, void* workspace, size_t workspace_bytes, int flags, hipStream_t st);
// glhip_api_distgrad_xk.hip: GLHIP_FLAG_XK_DIST_GRAD (xk_dist_grad_kernel, glhip_dist_grad_xk.h); op GLHIP_DIST_GRAD_SOFTMIN_P1: s = h, scale = eps;
// laplacian / energy: s = v, scale = blur, bwd_x: out NULL, fwd_grad: g NULL
int dist_grad_xk_launch(int op, const void* x, const void* y, const float* s, const float* g, float* out, float* gx, int B, int N, int M, int D,
                        float scale, int in_dtype, void* workspace, size_t workspace_bytes, int flags, hipStream_t st);

}  // namespace glhip
