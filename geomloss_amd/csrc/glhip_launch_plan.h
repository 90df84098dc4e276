// glhip_launch_plan.h — host side of the reductions whose partial per row and column split is (sums[nv], mass, m), and of argmin, which
// shares their split policy: ONE pass launcher, ONE pass loop, ONE sizing rule and ONE argument prologue for glhip_api_plan.hip,
// glhip_api_plan_xk.hip, glhip_api_grad_xk.hip, glhip_api_convgrad_xk.hip, glhip_api_distgrad_xk.hip and glhip_api_argmin.hip; for the three
// gradient routes of 17 <= D <= 4095 also ONE workspace rule and ONE launch prologue.
// What the launcher takes and what the sizing calls promise must agree exactly: both read plan_splits, plan_pass_workspace_bytes and the
// resident-slot constants, which live with every other split rule in glhip_split_policy.h.
#pragma once

#include "glhip_launch.h"
#include "glhip_plan_apply_xk.h"

namespace {

constexpr int kXkPlanWidth = 32 * kXkPlanMaxChunks;       // features / coordinates per pass of xk_plan_kernel

// (the EINVAL prologue the predicates of the family share: plan_family_bad_args, glhip_family.h)

// One dense pass: `rows` per workgroup, `partial` floats per row and split, `slots` resident workgroups.  main(grid, sp) launches the
// reduction, merge(sp) the kernel that combines its column splits.
template <class Main, class Merge>
void launch_plan_pass(int rows, int partial, long slots, int B, int N, int M, const Scratch& sc, hipStream_t st, Main&& main, Merge&& merge) {
    const Ranges none{nullptr, nullptr, nullptr, nullptr};
    SplitLaunch sl(none, 0, B, N, M, rows, partial, sc.ws, sc.bytes, sc.cb, st);
    const PlanSplits ps = plan_splits(sl.row_blocks, M, sl.fit, sc.allow_split, slots);
    SplitPlan plan;
    if (!(ps.xcd && take_xcd(plan, sl, ps.n)))      // (a grid beyond 2^31 workgroups stays on the plain 3-D grid)
        plan.n_splits = ps.xcd ? choose_splits(sl.row_blocks, M, 0, sl.fit) : ps.n;
    sl.apply(plan);
    main(sl.sp.xcd_grid_x > 0 ? dim3((unsigned)((long)sl.gx * B * sl.sp.n_splits), 1, 1) : dim3(sl.gx, B, sl.sp.n_splits), sl.sp);
    if (sl.sp.n_splits > 1) merge(sl.sp);
}

// plan_merge_kernel on the parameter struct of the pass: one thread per (row, feature); its width is a run-time argument
template <class P>
void launch_plan_merge(const P& prm, int B, int N, int D, const SplitInfo& sp, hipStream_t st) {
    const long rows = (long)B * N, items = rows * prm.nv;
    hipLaunchKernelGGL((plan_merge_kernel<P>), dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm, N, D, rows, sp);
}

template <typename T, int NCH, int L, class P>
void launch_xk_plan_pass(const P& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_pass(kXkRows, prm.nv + 2, kXkPlanSlots, B, N, M, sc, st,
        [&](dim3 grid, const SplitInfo& sp) {
            hipLaunchKernelGGL((xk_plan_kernel<T, NCH, L, P>), grid, dim3(kXkThreads), 0, st, prm, N, M, D, sp);
        },
        [&](const SplitInfo& sp) { launch_plan_merge(prm, B, N, D, sp, st); });
}

// THE pass loop: `width` features (the plan: V) or coordinates (the gradients: D), `pass_width` at a time; pass(prm, nch) launches one
// pass with prm.v0 and prm.nv set, nch = the chunks of 32 it needs.
template <class P, class Pass>
void launch_plan_passes(P prm, int width, int pass_width, Pass&& pass) {
    for (int v0 = 0; v0 < width; v0 += pass_width) {
        prm.v0 = v0;
        prm.nv = width - v0 < pass_width ? width - v0 : pass_width;
        pass(prm, (prm.nv + 31) / 32);
    }
}

// The passes of xk_plan_kernel, kXkPlanWidth at a time; a pass of <= 32 runs with one chunk.  In the K layout the call asks for.
template <template <typename> class PP, typename T>
void launch_xk_plan_passes(const PP<T>& prm, int width, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_passes(prm, width, kXkPlanWidth, [&](const PP<T>& pass, int nch) {
        if (nch > 1) {
            if (sc.h2) launch_xk_plan_pass<T, 2, XL_F16X2>(pass, B, N, M, D, sc, st);
            else launch_xk_plan_pass<T, 2, XL_BF16X3>(pass, B, N, M, D, sc, st);
        } else {
            if (sc.h2) launch_xk_plan_pass<T, 1, XL_F16X2>(pass, B, N, M, D, sc, st);
            else launch_xk_plan_pass<T, 1, XL_BF16X3>(pass, B, N, M, D, sc, st);
        }
    });
}

// ---- The gradient routes of 17 <= D <= 4095 (glhip_api_grad_xk.hip, glhip_api_convgrad_xk.hip, glhip_api_distgrad_xk.hip) ----

// Which launch takes them is an arm of softmin_bwd_family / conv_family (glhip_family.h: xk_grad_route), which their exported predicates read.
// Their sizing rule: the widest pass carries min(D, pass_width) coordinates; `uses`: what the route's predicate answers for float32 clouds
inline size_t xk_grad_workspace_bytes(int uses, int B, int N, int M, int D, int flags, int pass_width) {
    if (B <= 0 || N <= 0 || M <= 0 || (flags & GLHIP_FLAG_NO_SPLIT) || uses != 1) return 0;
    return plan_pass_workspace_bytes(B, N, M, kXkRows, D < pass_width ? D : pass_width, {kXkPlanSlots});
}

// Their launch prologue: without columns the sums are empty (gx, and out where wanted, are zeroed); else run(T{}, scratch) on the cloud type
template <class Run>
int xk_grad_launch(float* gx, float* out, int B, int N, int M, int D, int in_dtype, void* workspace, size_t workspace_bytes, int flags,
                   hipStream_t st, Run&& run) {
    if (M == 0) {
        (void)hipMemsetAsync(gx, 0, (size_t)B * N * D * sizeof(float), st);
        if (out) (void)hipMemsetAsync(out, 0, (size_t)B * N * sizeof(float), st);
        return GLHIP_OK;
    }
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, 0, N);
    if (in_dtype == GLHIP_F32) run(float{}, sc); else run(bf16_t{}, sc);
    return GLHIP_OK;
}

}  // namespace
