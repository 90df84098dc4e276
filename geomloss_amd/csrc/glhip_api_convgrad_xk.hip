// glhip_api_convgrad_xk.hip — C-ABI part 12: the gradient of the gaussian kernel product of 17 <= D <= 4095 on the matrix cores
// (GLHIP_FLAG_XK_GRAD): xk_plan_kernel on XkGaussGradParams (glhip_gauss_grad_xk.h), launched by glhip_kernel_conv_bwd_x and
// glhip_kernel_conv_fwd_grad (glhip_api_convgrad.hip) where glhip_kernel_conv_grad_uses_xk says so.  A translation unit of its own: the
// parallel build does not get longer.
#include "glhip_launch.h"
#include "glhip_gauss_grad_xk.h"

namespace {

constexpr size_t kGaussGradXkMaxWorkspace = (size_t)1 << 30;   // glhip_kernel_conv_grad_workspace_bytes never asks for more than 1 GiB (glhip.h)
constexpr long kXkGaussGradSlots = 256;                        // resident 8-wave workgroups: one per CU, as xk_plan_kernel
constexpr int kGaussGradXkWidth = 32 * kXkPlanMaxChunks;       // coordinates per pass

// THE predicate of the GLHIP_FLAG_XK_GRAD route of glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad, and what
// glhip_kernel_conv_grad_uses_xk reports.  Host arithmetic only.
inline int conv_grad_uses_xk(int kind, int B, long N, long M, int D, int dtype, int flags, int n_ranges) {
    if (kind < GLHIP_GAUSSIAN || kind > GLHIP_ENERGY || B < 0 || N < 0 || M < 0 || N > 0x7fffffffL || M > 0x7fffffffL || D < 1 ||
        n_ranges < 0 || (dtype != GLHIP_F32 && dtype != GLHIP_BF16))
        return GLHIP_EINVAL;
    if (!(flags & GLHIP_FLAG_XK_GRAD) || (flags & (GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_DIRECT))) return 0;
    return (kind == GLHIP_GAUSSIAN && D > kXdMaxD && D <= kXkMaxD && n_ranges == 0 && B <= 65535) ? 1 : 0;
}

template <typename T, int NCH, int L>
void launch_xk_gauss_grad_pass(const XkGaussGradParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    const Ranges none{nullptr, nullptr, nullptr, nullptr};
    SplitLaunch sl(none, 0, B, N, M, kXkRows, prm.nv + 2, sc.ws, sc.bytes, sc.cb, st);
    const PlanSplits ps = plan_splits(sl.row_blocks, M, sl.fit, sc.allow_split, kXkGaussGradSlots);
    if (!(ps.xcd && sl.take_xcd(ps.n)))      // (a grid beyond 2^31 workgroups stays on the plain 3-D grid)
        sl.sp.n_splits = ps.xcd ? choose_splits(sl.row_blocks, M, 0, sl.fit) : ps.n;
    const dim3 grid = sl.sp.xcd_grid_x > 0 ? dim3((unsigned)((long)sl.gx * B * sl.sp.n_splits), 1, 1) : dim3(sl.gx, B, sl.sp.n_splits);
    hipLaunchKernelGGL((xk_plan_kernel<T, NCH, L, XkGaussGradParams<T>>), grid, dim3(kXkThreads), 0, st, prm, N, M, D, sl.sp);
    if (sl.sp.n_splits > 1) {
        const long rows = (long)B * N, items = rows * prm.nv;
        hipLaunchKernelGGL((xk_gauss_grad_merge_kernel<T>), dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm, N, D, rows, sl.sp);
    }
}

template <typename T, int L>
void launch_xk_gauss_grad(XkGaussGradParams<T> prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    for (int v0 = 0; v0 < D; v0 += kGaussGradXkWidth) {
        prm.v0 = v0;
        prm.nv = D - v0 < kGaussGradXkWidth ? D - v0 : kGaussGradXkWidth;
        if (prm.nv > 32) launch_xk_gauss_grad_pass<T, 2, L>(prm, B, N, M, D, sc, st);
        else launch_xk_gauss_grad_pass<T, 1, L>(prm, B, N, M, D, sc, st);
    }
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
        if (sc.h2) launch_xk_gauss_grad<T, XL_F16X2>(prm, B, N, M, D, sc, st);
        else launch_xk_gauss_grad<T, XL_BF16X3>(prm, B, N, M, D, sc, st);
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
    const int nv = D < kGaussGradXkWidth ? D : kGaussGradXkWidth;      // the widest pass
    const size_t per_split = (size_t)B * N * (nv + 2) * sizeof(float);
    const long row_blocks = (long)B * ((N + kXkRows - 1) / kXkRows);
    long fit = (long)(kGaussGradXkMaxWorkspace / per_split);
    fit = fit < 32 ? fit : 32;
    const int ns = plan_splits(row_blocks, M, fit, true, kXkGaussGradSlots).n;
    return ns >= 2 ? (size_t)ns * per_split : 0;
}

}  // extern "C"
