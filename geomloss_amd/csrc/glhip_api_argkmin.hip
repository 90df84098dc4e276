// glhip_api_argkmin.hip — C-ABI part 12: the top-k arg-reduction glhip_argkmin (glhip_argkmin_xk.h) with its host-only support query,
// its limit on k, its pass count and its workspace sizing.  A translation unit of its own, like argmin's: the parallel build does not
// get longer.
#include "glhip_launch_plan.h"
#include "glhip_argkmin_xk.h"

namespace {

// THE predicate of glhip_argkmin, and what glhip_argkmin_supported reports.  Host arithmetic only.
inline int argkmin_supported(int B, long N, long M, int D, int k, int p, int dtype, int n_ranges) {
    if (plan_family_bad_args(B, N, M, D, dtype, n_ranges) || (p != 1 && p != 2) || k < 1) return GLHIP_EINVAL;
    return (p == 2 && n_ranges == 0 && D <= kXkMaxD && B <= 65535 && k <= kArgkminMaxK) ? 1 : 0;
}

// Resident workgroups of the kernel that serves k ranks in one pass, and its list capacity: the smallest compiled one that holds them
inline int argkmin_cap(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : 16; }
inline long argkmin_slots(int k) { return argkmin_occ(argkmin_cap(k)) >= 4 ? kXkSlots : kXkTopkSlots; }

// k <= kArgkminCap: one pass of the plain kernel.  Beyond: floored passes of kArgkminCap ranks, the last one of the remainder, on the
// smallest capacity that holds it (k = 20 = 16 + 4: the second pass runs at argmin's occupancy).
inline int argkmin_passes(int k) { return k <= kArgkminCap ? 1 : (k + kArgkminCap - 1) / kArgkminCap; }
// the floor buffer at the head of the workspace of a k > kArgkminCap call: one (u, index) pair per row
inline size_t argkmin_floor_bytes(int B, int N) { return align256((size_t)B * (size_t)N * 2 * sizeof(int32_t)); }

// The split policy is plan_splits (glhip_split_policy.h, through launch_plan_pass) with the resident workgroups of the kernel that runs
// (argkmin_slots); the partial of a row is the kc (exponent, index) pairs of the pass.
template <typename T, int CAP, bool FLOOR>
void launch_argkmin_cap(const ArgkminParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_pass(kXkRows, 2 * prm.kc, argkmin_slots(prm.kc), B, N, M, sc, st,
        [&](dim3 grid, const SplitInfo& sp) {
            hipLaunchKernelGGL((argkmin_xk_kernel<T, CAP, argkmin_occ(CAP), FLOOR>), grid, dim3(kXkThreads), 0, st, prm, N, M, D, sp);
        },
        [&](const SplitInfo& sp) {
            const long rows = (long)B * N;
            hipLaunchKernelGGL((argkmin_merge_kernel<CAP>), dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm.index, prm.value,
                               rows, prm.k, prm.r0, prm.kc, prm.floor, sp);
        });
}

// one pass: the ranks prm.r0 .. prm.r0 + prm.kc - 1
template <typename T, bool FLOOR>
void launch_argkmin_pass(const ArgkminParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    switch (argkmin_cap(prm.kc)) {
        case 4: launch_argkmin_cap<T, 4, FLOOR>(prm, B, N, M, D, sc, st); break;
        case 8: launch_argkmin_cap<T, 8, FLOOR>(prm, B, N, M, D, sc, st); break;
        default: launch_argkmin_cap<T, 16, FLOOR>(prm, B, N, M, D, sc, st); break;
    }
}

// `sc`: the split area (for k > kArgkminCap: what follows the floor buffer prm.floor).  The passes follow each other on the stream: a
// pass reads the floors the one before it wrote, and nothing else orders them.
template <typename T>
void launch_argkmin(ArgkminParams<T> prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    if (prm.k <= kArgkminCap) {
        launch_argkmin_pass<T, false>(prm, B, N, M, D, sc, st);
        return;
    }
    const long rows = (long)B * N;
    hipLaunchKernelGGL(argkmin_floor_fill_kernel, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm.floor, rows);
    for (prm.r0 = 0; prm.r0 < prm.k; prm.r0 += kArgkminCap) {
        prm.kc = prm.k - prm.r0 < kArgkminCap ? prm.k - prm.r0 : kArgkminCap;
        launch_argkmin_pass<T, true>(prm, B, N, M, D, sc, st);
    }
}

// The split area of one pass of kc ranks: room for either rule of plan_splits (as glhip_argmin_workspace_bytes), non-decreasing in M
inline size_t argkmin_split_bytes(int B, int N, int M, int kc) {
    const long row_blocks = (long)B * ((N + kXkRows - 1) / kXkRows);
    const size_t per_split = (size_t)B * (size_t)N * 2 * kc * sizeof(float);
    long fit = (long)(kPlanMaxWorkspace / per_split);      // never more than 1 GiB: the launch runs with the splits that fit
    fit = fit < 32 ? fit : 32;
    int ns = choose_splits(row_blocks, M, 0, fit);
    if (M >= 65536 && fit >= 8) {
        const int nx = xcd_splits(row_blocks, M, argkmin_slots(kc), fit);
        ns = ns > nx ? ns : nx;
        ns = ns > 8 ? ns : 8;
    }
    return ns >= 2 ? (size_t)ns * per_split : 0;
}

}  // namespace

extern "C" {

int glhip_argkmin_max_k(void) { return kArgkminMaxK; }

int glhip_argkmin_passes(int k) { return (k < 1 || k > kArgkminMaxK) ? GLHIP_EINVAL : argkmin_passes(k); }

int glhip_argkmin_supported(int B, long N, long M, int D, int k, int p, int dtype, int n_ranges) {
    return argkmin_supported(B, N, M, D, k, p, dtype, n_ranges);
}

size_t glhip_argkmin_workspace_bytes(int B, int N, int M, int D, int k) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXkMaxD || k < 1 || k > kArgkminMaxK) return 0;
    if (k <= kArgkminCap) return argkmin_split_bytes(B, N, M, k);
    // the floor buffer, then the largest split area of the passes: those of kArgkminCap ranks and the last one
    const size_t full = argkmin_split_bytes(B, N, M, kArgkminCap), last = argkmin_split_bytes(B, N, M, k - (argkmin_passes(k) - 1) * kArgkminCap);
    return argkmin_floor_bytes(B, N) + (full > last ? full : last);
}

int glhip_argkmin(const void* x, const void* y, const float* g, int32_t* index, float* value,
                  int B, int N, int M, int D, int k, int p, int in_dtype,
                  const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                  void* workspace, size_t workspace_bytes, int flags, void* stream) {
    // (g may be NULL: check_common sees y in its place)
    int rc = check_common("glhip_argkmin", x, y, y, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    const int ok = argkmin_supported(B, N, M, D, k, p, in_dtype, n_ranges);
    if (ok == GLHIP_EINVAL) return fail(GLHIP_EINVAL, "glhip_argkmin: bad argument (p %d, k %d)", p, k);
    if (ok == 0)
        return fail(GLHIP_EUNSUPPORTED, "glhip_argkmin: only p = 2, D <= %d, k <= %d, dense launches (got p %d, D %d, k %d, n_ranges %d)", kXkMaxD,
                    kArgkminMaxK, p, D, k, n_ranges);
    if (B == 0 || N == 0) return GLHIP_OK;   // nothing to write
    if (!index) return fail(GLHIP_EINVAL, "glhip_argkmin: NULL index");
    if (arg_family(B, N, M, D, k, p, in_dtype, n_ranges, flags) == GLHIP_FAMILY_XD)      // GLHIP_FLAG_XD_ARG: resident operands (glhip_arg_xd.h)
        return arg_xd_launch("glhip_argkmin", x, y, g, index, value, B, N, M, D, k, in_dtype, workspace, workspace_bytes, flags, stream);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // k > kArgkminCap: the floors of the passes live at the head of the workspace, whatever the flags; the splits take what follows
    int32_t* floor = nullptr;
    if (k > kArgkminCap) {
        const size_t head = argkmin_floor_bytes(B, N);
        if (!workspace || workspace_bytes < head || (reinterpret_cast<uintptr_t>(workspace) & 7))
            return fail(GLHIP_EINVAL, "glhip_argkmin: k = %d > %d runs in passes and needs an 8-byte aligned workspace of at least %zu bytes for their "
                        "floors (got %zu): size it with glhip_argkmin_workspace_bytes", k, kArgkminCap, head, workspace ? workspace_bytes : (size_t)0);
        floor = static_cast<int32_t*>(workspace);
        workspace_bytes -= head;
        workspace = workspace_bytes ? static_cast<char*>(workspace) + head : nullptr;
    }
    // GLHIP_FLAG_F16X2 is accepted and ignored: the kernel has the bf16 x 3 layout only.  M == 0 runs the kernel over no tile: index -1, value +inf.
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, 0, N);
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const ArgkminParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), g, index, value, k, 0, k, floor};
        launch_argkmin<T>(prm, B, N, M, D, sc, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return check_launch("glhip_argkmin");
}

}  // extern "C"
