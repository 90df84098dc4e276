// glhip_launch_plan.h — host side of the reductions whose partial per row and column split is (sums[nv], mass, m), and of argmin, which
// shares their split policy: ONE pass launcher, ONE pass loop over xk_plan_kernel (glhip_plan_apply_xk.h), ONE sizing rule and ONE
// argument prologue for glhip_api_plan.hip, glhip_api_plan_xk.hip, glhip_api_grad_xk.hip, glhip_api_convgrad_xk.hip and glhip_api_argmin.hip.
// What the launcher takes and what the sizing calls promise must agree exactly: both read plan_splits and the constants below.
// glhip_api_distgrad_xk.hip (xk_dist_grad_kernel, glhip_dist_grad_xk.h) uses launch_plan_pass, launch_plan_merge and the sizing rule with a
// pass loop of its own: its passes are 32 coordinates wide, and launch_xk_plan_passes below stays the loop of xk_plan_kernel alone.
#pragma once

#include <initializer_list>

#include "glhip_launch.h"
#include "glhip_plan_apply_xk.h"

namespace {

constexpr size_t kPlanMaxWorkspace = (size_t)1 << 30;     // no *_workspace_bytes call of this family asks for more than 1 GiB (glhip.h)
constexpr long kXkPlanSlots = 256;                        // resident 8-wave workgroups of xk_plan_kernel: one per CU (glhip_plan_apply_xk.h)
constexpr int kXkPlanWidth = 32 * kXkPlanMaxChunks;       // features / coordinates per pass of xk_plan_kernel

// The EINVAL prologue the predicates of the family share
inline bool plan_family_bad_args(int B, long N, long M, int D, int dtype, int n_ranges) {
    return B < 0 || N < 0 || M < 0 || N > 0x7fffffffL || M > 0x7fffffffL || D < 1 || n_ranges < 0 || (dtype != GLHIP_F32 && dtype != GLHIP_BF16);
}

// THE split policy of a pass, shared by the launcher and by the sizing calls: the rule of every split launch (choose_splits), or — dense
// launches with room for 8 splits over >= 65536 columns (SplitLaunch::xcd_eligible) — the XCD-aware grid with xcd_splits.
// `fit`: splits the workspace holds; `slots`: resident workgroups of the kernel shape.
struct PlanSplits { int n; bool xcd; };
inline PlanSplits plan_splits(long row_blocks, int M, long fit, bool allow_split, long slots) {
    if (!allow_split || fit < 2) return PlanSplits{1, false};
    if (fit >= 8 && M >= 65536) return PlanSplits{xcd_splits(row_blocks, M, slots, fit), true};
    return PlanSplits{choose_splits(row_blocks, M, 0, fit), false};
}

// One dense pass: `rows` per workgroup, `partial` floats per row and split, `slots` resident workgroups.  main(grid, sp) launches the
// reduction, merge(sp) the kernel that combines its column splits.
template <class Main, class Merge>
void launch_plan_pass(int rows, int partial, long slots, int B, int N, int M, const Scratch& sc, hipStream_t st, Main&& main, Merge&& merge) {
    const Ranges none{nullptr, nullptr, nullptr, nullptr};
    SplitLaunch sl(none, 0, B, N, M, rows, partial, sc.ws, sc.bytes, sc.cb, st);
    const PlanSplits ps = plan_splits(sl.row_blocks, M, sl.fit, sc.allow_split, slots);
    if (!(ps.xcd && sl.take_xcd(ps.n)))      // (a grid beyond 2^31 workgroups stays on the plain 3-D grid)
        sl.sp.n_splits = ps.xcd ? choose_splits(sl.row_blocks, M, 0, sl.fit) : ps.n;
    main(sl.sp.xcd_grid_x > 0 ? dim3((unsigned)((long)sl.gx * B * sl.sp.n_splits), 1, 1) : dim3(sl.gx, B, sl.sp.n_splits), sl.sp);
    if (sl.sp.n_splits > 1) merge(sl.sp);
}

// The workspace of the widest pass (nv sums) of a call: what launch_plan_pass would take with up to 1 GiB, for the largest of the
// resident-workgroup counts its kernel shapes have; 0 where the pass runs unsplit.
inline size_t plan_pass_workspace_bytes(int B, int N, int M, int rows, int nv, std::initializer_list<long> slots) {
    const size_t per_split = (size_t)B * N * (nv + 2) * sizeof(float);
    const long row_blocks = (long)B * ((N + rows - 1) / rows);
    long fit = (long)(kPlanMaxWorkspace / per_split);
    fit = fit < 32 ? fit : 32;
    int ns = 0;
    for (long s : slots) {
        const int n = plan_splits(row_blocks, M, fit, true, s).n;
        ns = n > ns ? n : ns;
    }
    return ns >= 2 ? (size_t)ns * per_split : 0;
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

// The passes of xk_plan_kernel over `width` features (the plan: V) or coordinates (the gradients: D), kXkPlanWidth at a time; a pass of
// <= 32 runs with one chunk.  In the K layout the call asks for.
template <template <typename> class PP, typename T>
void launch_xk_plan_passes(PP<T> prm, int width, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    for (int v0 = 0; v0 < width; v0 += kXkPlanWidth) {
        prm.v0 = v0;
        prm.nv = width - v0 < kXkPlanWidth ? width - v0 : kXkPlanWidth;
        if (prm.nv > 32) {
            if (sc.h2) launch_xk_plan_pass<T, 2, XL_F16X2>(prm, B, N, M, D, sc, st);
            else launch_xk_plan_pass<T, 2, XL_BF16X3>(prm, B, N, M, D, sc, st);
        } else {
            if (sc.h2) launch_xk_plan_pass<T, 1, XL_F16X2>(prm, B, N, M, D, sc, st);
            else launch_xk_plan_pass<T, 1, XL_BF16X3>(prm, B, N, M, D, sc, st);
        }
    }
}

}  // namespace
