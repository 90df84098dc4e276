// glhip_api_plan.hip — C-ABI part 8: the transport plan of a p = 2 soft-min applied to a feature matrix (glhip_plan_apply.h).
#include "glhip_launch_plan.h"

namespace {

template <int D, typename T, int NCH, int L>
void launch_plan_d_pass(const PlanParams<T>& prm, int B, int N, int M, const Scratch& sc, hipStream_t st) {
    constexpr long kSlots = 256L * (PlanShape<D, NCH, L>::template waves<T>() / 2);      // resident 8-wave workgroups (PlanShape::waves)
    launch_plan_pass(kPlanRows, prm.nv + 2, kSlots, B, N, M, sc, st,
        [&](dim3 grid, const SplitInfo& sp) {
            hipLaunchKernelGGL((plan_apply_kernel<D, T, NCH, L>), grid, dim3(kPlanNW * 64), 0, st, prm, N, M, sp);
        },
        [&](const SplitInfo& sp) { launch_plan_merge(prm, B, N, D, sp, st); });
}

// (a loop of its own, not launch_xk_plan_passes: the pass width and the chunk counts depend on D)
template <int D, typename T, int L>
void launch_plan_d(PlanParams<T> prm, int B, int N, int M, int V, const Scratch& sc, hipStream_t st) {
    constexpr int kMax = PlanShape<D, 1, L>::kMaxChunks;       // passes of up to 128 (64) features
    for (int v0 = 0; v0 < V; v0 += 32 * kMax) {
        prm.v0 = v0;
        prm.nv = V - v0 < 32 * kMax ? V - v0 : 32 * kMax;
        if constexpr (kMax == 4) {
            if (prm.nv > 64) { launch_plan_d_pass<D, T, 4, L>(prm, B, N, M, sc, st); continue; }
        }
        if constexpr (kMax >= 2) {
            if (prm.nv > 32) { launch_plan_d_pass<D, T, 2, L>(prm, B, N, M, sc, st); continue; }
        }
        launch_plan_d_pass<D, T, 1, L>(prm, B, N, M, sc, st);
    }
}

template <typename T>
void launch_plan(const PlanParams<T>& prm, int B, int N, int M, int D, int V, const Scratch& sc, hipStream_t st) {
#define GL_PLAN(DD)                                                              \
    if (sc.h2) launch_plan_d<DD, T, XL_F16X2>(prm, B, N, M, V, sc, st);          \
    else launch_plan_d<DD, T, XL_BF16X3>(prm, B, N, M, V, sc, st)
    switch (D) {
        case 1: GL_PLAN(1); break;
        case 2: GL_PLAN(2); break;
        case 3: GL_PLAN(3); break;
        default: GLHIP_XD_DISPATCH(D, GL_PLAN)
    }
#undef GL_PLAN
}

}  // namespace

extern "C" {

size_t glhip_plan_apply_workspace_bytes(int B, int N, int M, int D, int V) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || V <= 0) return 0;
    // the widest pass any dimension takes, for either number of resident workgroups a kernel shape has
    return plan_pass_workspace_bytes(B, N, M, kPlanRows, V < 32 * kPlanMaxChunks ? V : 32 * kPlanMaxChunks, {256, 512});
}

int glhip_plan_apply(const void* x, const void* y, const float* h, const float* fwd, const float* feat, float* out, float* mass,
                     int B, int N, int M, int D, int V, float eps, int p, int in_dtype,
                     const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                     void* workspace, size_t workspace_bytes, int flags, void* stream) {
    int rc = check_common("glhip_plan_apply", x, y, h, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    if (V < 0) return fail(GLHIP_EINVAL, "glhip_plan_apply: bad size V=%d", V);
    if (p != 2 || D > kXdMaxD || n_ranges > 0)
        return fail(GLHIP_EUNSUPPORTED, "glhip_plan_apply: only p = 2, D <= 16, dense launches (got p %d, D %d, n_ranges %d)", p, D, n_ranges);
    if (B == 0 || N == 0 || V == 0) return GLHIP_OK;   // nothing to write
    if (!fwd || !out) return fail(GLHIP_EINVAL, "glhip_plan_apply: NULL fwd / out");
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "glhip_plan_apply: eps must be > 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (M == 0) {      // an empty plan: zero sums, zero mass
        if (hipMemsetAsync(out, 0, (size_t)B * N * V * sizeof(float), st) != hipSuccess) return check_launch("glhip_plan_apply");
        if (mass && hipMemsetAsync(mass, 0, (size_t)B * N * sizeof(float), st) != hipSuccess) return check_launch("glhip_plan_apply");
        return check_launch("glhip_plan_apply");
    }
    if (!feat) return fail(GLHIP_EINVAL, "glhip_plan_apply: NULL feat");
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, 0, N);
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const PlanParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), h, fwd, feat, out, mass,
                                kLog2e / eps, -eps * kLn2, V, 0, 0};
        launch_plan<T>(prm, B, N, M, D, V, sc, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return check_launch("glhip_plan_apply");
}

}  // extern "C"
