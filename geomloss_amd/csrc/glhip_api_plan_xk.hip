// glhip_api_plan_xk.hip — C-ABI part 9: plan application in any dimension up to 4095.  1 <= D <= 16 forwards to glhip_plan_apply
// (glhip_api_plan.hip); 17 <= D <= 4095 runs xk_plan_kernel (glhip_plan_apply_xk.h).  A translation unit of its own: the parallel
// build does not get longer.
#include "glhip_launch_plan.h"

namespace {

static_assert(PlanShape<4, 1, XL_BF16X3>::kMaxChunks == 4 && PlanShape<5, 1, XL_BF16X3>::kMaxChunks == 2 &&
              PlanShape<11, 1, XL_BF16X3>::kMaxChunks == 2 && PlanShape<12, 1, XL_BF16X3>::kMaxChunks == 1,
              "plan_nd_pass_width restates PlanShape::kMaxChunks");
inline int plan_nd_pass_width(int D) {
    if (D <= kXdMaxD) return D <= 4 ? 128 : (D <= 11 ? 64 : 32);
    return kXkPlanWidth;
}

// THE predicate of glhip_plan_apply_nd, and what glhip_plan_apply_nd_family reports.  Host arithmetic only.
inline int plan_nd_family(int B, long N, long M, int D, int V, int p, int dtype, int n_ranges) {
    if (plan_family_bad_args(B, N, M, D, dtype, n_ranges) || V < 0 || (p != 1 && p != 2)) return GLHIP_EINVAL;
    if (p != 2 || n_ranges > 0 || D > kXkMaxD || B > 65535) return GLHIP_EUNSUPPORTED;
    return D <= kXdMaxD ? GLHIP_FAMILY_XD : GLHIP_FAMILY_XK;
}

}  // namespace

extern "C" {

int glhip_plan_apply_nd_family(int B, long N, long M, int D, int V, int p, int dtype, int flags, int n_ranges) {
    (void)flags;      // both exponent layouts run the same family
    return plan_nd_family(B, N, M, D, V, p, dtype, n_ranges);
}

int glhip_plan_apply_nd_pass_width(int D) { return (D < 1 || D > kXkMaxD) ? 0 : plan_nd_pass_width(D); }

size_t glhip_plan_apply_nd_workspace_bytes(int B, int N, int M, int D, int V) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXkMaxD || V <= 0) return 0;
    if (D <= kXdMaxD) return glhip_plan_apply_workspace_bytes(B, N, M, D, V);
    return plan_pass_workspace_bytes(B, N, M, kXkRows, V < kXkPlanWidth ? V : kXkPlanWidth, {kXkPlanSlots});
}

int glhip_plan_apply_nd(const void* x, const void* y, const float* h, const float* fwd, const float* feat, float* out, float* mass,
                        int B, int N, int M, int D, int V, float eps, int p, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream) {
    int rc = check_common("glhip_plan_apply_nd", x, y, h, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    const int fam = plan_nd_family(B, N, M, D, V, p, in_dtype, n_ranges);
    if (fam == GLHIP_EINVAL) return fail(GLHIP_EINVAL, "glhip_plan_apply_nd: bad argument (V %d, p %d)", V, p);
    if (fam == GLHIP_EUNSUPPORTED)
        return fail(GLHIP_EUNSUPPORTED, "glhip_plan_apply_nd: only p = 2, D <= %d, dense launches (got p %d, D %d, n_ranges %d)", kXkMaxD, p, D, n_ranges);
    if (V == 0 && B > 0 && N > 0 && mass) {      // a zero-size feat: out is empty, mass is zeroed (any D; glhip_plan_apply leaves it untouched)
        if (hipMemsetAsync(mass, 0, (size_t)B * N * sizeof(float), static_cast<hipStream_t>(stream)) != hipSuccess) return check_launch("glhip_plan_apply_nd");
        return check_launch("glhip_plan_apply_nd");
    }
    if (fam == GLHIP_FAMILY_XD)      // the very launch of glhip_plan_apply
        return glhip_plan_apply(x, y, h, fwd, feat, out, mass, B, N, M, D, V, eps, p, in_dtype, ranges_i, slices_i, redranges_j, n_ranges,
                                workspace, workspace_bytes, flags, stream);
    if (B == 0 || N == 0 || V == 0) return GLHIP_OK;   // nothing to write
    if (!fwd || !out) return fail(GLHIP_EINVAL, "glhip_plan_apply_nd: NULL fwd / out");
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "glhip_plan_apply_nd: eps must be > 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (M == 0) {      // an empty plan: zero sums, zero mass
        if (hipMemsetAsync(out, 0, (size_t)B * N * V * sizeof(float), st) != hipSuccess) return check_launch("glhip_plan_apply_nd");
        if (mass && hipMemsetAsync(mass, 0, (size_t)B * N * sizeof(float), st) != hipSuccess) return check_launch("glhip_plan_apply_nd");
        return check_launch("glhip_plan_apply_nd");
    }
    if (!feat) return fail(GLHIP_EINVAL, "glhip_plan_apply_nd: NULL feat");
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, 0, N);
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const PlanParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), h, fwd, feat, out, mass,
                                kLog2e / eps, -eps * kLn2, V, 0, 0};
        launch_xk_plan_passes(prm, V, B, N, M, D, sc, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return check_launch("glhip_plan_apply_nd");
}

}  // extern "C"
