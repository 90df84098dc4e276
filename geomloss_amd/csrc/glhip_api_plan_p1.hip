// glhip_api_plan_p1.hip — C-ABI part 14: the plan of a p = 1 soft-min applied to features, 1 <= D <= 4095 (glhip_plan_apply_p1):
// xk_dist_plan_kernel (glhip_dist_plan_xk.h), the exponent half of xk_dist_kernel joined with the plan half of xk_plan_kernel.  It
// normalises itself and returns the soft-min on the side, so no saved forward value comes in.  A translation unit of its own: the parallel
// build does not get longer.
#include "glhip_launch_plan.h"
#include "glhip_dist_plan_xk.h"

namespace {

constexpr int kXkDistPlanWidth = 32 * glhip::kXkDistPlanChunks;      // features per pass of xk_dist_plan_kernel

// THE predicate of glhip_plan_apply_p1, and what glhip_plan_apply_p1_supported reports.  Host arithmetic only.
inline int plan_p1_supported(int B, long N, long M, int D, int V, int dtype, int n_ranges) {
    if (plan_family_bad_args(B, N, M, D, dtype, n_ranges) || V < 0) return GLHIP_EINVAL;
    return (n_ranges > 0 || D > kXkMaxD || B > 65535) ? 0 : 1;
}

// The passes over the V feature columns, kXkDistPlanWidth at a time; a pass of <= 32 runs with one chunk.  V == 0 with a soft-min wanted:
// one pass without features and without column splits (the merge works per feature).
template <typename T>
void launch_dist_plan_passes(const XkDistPlanParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    auto one = [&](const XkDistPlanParams<T>& pass, int nch) {
        launch_plan_pass(kXkRows, pass.nv + 2, kXkPlanSlots, B, N, M, sc, st,
            [&](dim3 grid, const SplitInfo& sp) {
                if (nch > 1) hipLaunchKernelGGL((xk_dist_plan_kernel<T, kXkDistPlanChunks>), grid, dim3(kXkThreads), 0, st, pass, N, M, D, sp);
                else hipLaunchKernelGGL((xk_dist_plan_kernel<T, 1>), grid, dim3(kXkThreads), 0, st, pass, N, M, D, sp);
            },
            [&](const SplitInfo& sp) { launch_plan_merge(pass, B, N, D, sp, st); });
    };
    if (prm.V == 0) one(prm, 1);
    else launch_plan_passes(prm, prm.V, kXkDistPlanWidth, one);
}

}  // namespace

extern "C" {

int glhip_plan_apply_p1_supported(int B, long N, long M, int D, int V, int dtype, int n_ranges) {
    return plan_p1_supported(B, N, M, D, V, dtype, n_ranges);
}

int glhip_plan_apply_p1_pass_width(void) { return kXkDistPlanWidth; }

size_t glhip_plan_apply_p1_workspace_bytes(int B, int N, int M, int D, int V) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXkMaxD || V <= 0) return 0;
    return plan_pass_workspace_bytes(B, N, M, kXkRows, V < kXkDistPlanWidth ? V : kXkDistPlanWidth, {kXkPlanSlots});
}

int glhip_plan_apply_p1(const void* x, const void* y, const float* h, const float* feat, float* out, float* softmin,
                        int B, int N, int M, int D, int V, float eps, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream) {
    int rc = check_common("glhip_plan_apply_p1", x, y, h, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    const int ok = plan_p1_supported(B, N, M, D, V, in_dtype, n_ranges);
    if (ok == GLHIP_EINVAL) return fail(GLHIP_EINVAL, "glhip_plan_apply_p1: bad argument (V %d)", V);
    if (ok == 0)
        return fail(GLHIP_EUNSUPPORTED, "glhip_plan_apply_p1: only D <= %d, dense launches (got D %d, n_ranges %d)", kXkMaxD, D, n_ranges);
    if (B == 0 || N == 0 || (V == 0 && !softmin)) return GLHIP_OK;   // nothing to write
    if (V > 0 && !out) return fail(GLHIP_EINVAL, "glhip_plan_apply_p1: NULL out");
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "glhip_plan_apply_p1: eps must be > 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (M == 0) {      // an empty plan: zero sums; the soft-min of a row without mass is +inf
        if (V > 0 && hipMemsetAsync(out, 0, (size_t)B * N * V * sizeof(float), st) != hipSuccess) return check_launch("glhip_plan_apply_p1");
        if (softmin && hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(softmin), 0x7f800000, (size_t)B * N, st) != hipSuccess)
            return check_launch("glhip_plan_apply_p1");
        return check_launch("glhip_plan_apply_p1");
    }
    if (V > 0 && !feat) return fail(GLHIP_EINVAL, "glhip_plan_apply_p1: NULL feat");
    // GLHIP_FLAG_F16X2 is ignored: a squared distance needs all 24 bits
    const Scratch sc = make_scratch(workspace, workspace_bytes, V == 0 ? (flags | GLHIP_FLAG_NO_SPLIT) : flags, 0, N);
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const float t = kLog2e / eps;      // the scales of make_softmin_params with p = 1
        const XkDistPlanParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), h, feat, out, softmin,
                                      t, 1e-8f * t * t, dist_guard(), -eps * kLn2, V, 0, 0};
        launch_dist_plan_passes(prm, B, N, M, D, sc, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return check_launch("glhip_plan_apply_p1");
}

}  // extern "C"
