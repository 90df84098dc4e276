// glhip_api_argkmin.hip — C-ABI part 12: the top-k arg-reduction glhip_argkmin (glhip_argkmin_xk.h) with its host-only support query,
// its limit on k and its workspace sizing.  A translation unit of its own, like argmin's: the parallel build does not get longer.
#include "glhip_launch_plan.h"
#include "glhip_argkmin_xk.h"

namespace {

// THE predicate of glhip_argkmin, and what glhip_argkmin_supported reports.  Host arithmetic only.
inline int argkmin_supported(int B, long N, long M, int D, int k, int p, int dtype, int n_ranges) {
    if (plan_family_bad_args(B, N, M, D, dtype, n_ranges) || (p != 1 && p != 2) || k < 1) return GLHIP_EINVAL;
    return (p == 2 && n_ranges == 0 && D <= kXkMaxD && B <= 65535 && k <= kArgkminMaxK) ? 1 : 0;
}

// Resident workgroups of the kernel that serves k, and its list capacity: the smallest compiled one that holds k
inline int argkmin_cap(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : 16; }
inline long argkmin_slots(int k) { return argkmin_occ(argkmin_cap(k)) >= 4 ? kXkSlots : kXkTopkSlots; }

// The split policy is plan_splits (glhip_split_policy.h, through launch_plan_pass) with the resident workgroups of the kernel that runs
// (argkmin_slots); the partial of a row is its k (exponent, index) pairs.
template <typename T, int CAP>
void launch_argkmin_cap(const ArgkminParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_pass(kXkRows, 2 * prm.k, argkmin_slots(prm.k), B, N, M, sc, st,
        [&](dim3 grid, const SplitInfo& sp) {
            hipLaunchKernelGGL((argkmin_xk_kernel<T, CAP, argkmin_occ(CAP)>), grid, dim3(kXkThreads), 0, st, prm, N, M, D, sp);
        },
        [&](const SplitInfo& sp) {
            const long rows = (long)B * N;
            hipLaunchKernelGGL((argkmin_merge_kernel<CAP>), dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm.index, prm.value,
                               rows, prm.k, sp);
        });
}

template <typename T>
void launch_argkmin(const ArgkminParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    switch (argkmin_cap(prm.k)) {
        case 4: launch_argkmin_cap<T, 4>(prm, B, N, M, D, sc, st); break;
        case 8: launch_argkmin_cap<T, 8>(prm, B, N, M, D, sc, st); break;
        default: launch_argkmin_cap<T, 16>(prm, B, N, M, D, sc, st); break;
    }
}

}  // namespace

extern "C" {

int glhip_argkmin_max_k(void) { return kArgkminMaxK; }

int glhip_argkmin_supported(int B, long N, long M, int D, int k, int p, int dtype, int n_ranges) {
    return argkmin_supported(B, N, M, D, k, p, dtype, n_ranges);
}

size_t glhip_argkmin_workspace_bytes(int B, int N, int M, int D, int k) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXkMaxD || k < 1 || k > kArgkminMaxK) return 0;
    const long row_blocks = (long)B * ((N + kXkRows - 1) / kXkRows);
    const size_t per_split = (size_t)B * (size_t)N * 2 * k * sizeof(float);
    long fit = (long)(kPlanMaxWorkspace / per_split);      // never more than 1 GiB: the launch runs with the splits that fit
    fit = fit < 32 ? fit : 32;
    // room for either rule of plan_splits (as glhip_argmin_workspace_bytes): non-decreasing in M
    int ns = choose_splits(row_blocks, M, 0, fit);
    if (M >= 65536 && fit >= 8) {
        const int nx = xcd_splits(row_blocks, M, argkmin_slots(k), fit);
        ns = ns > nx ? ns : nx;
        ns = ns > 8 ? ns : 8;
    }
    return ns >= 2 ? (size_t)ns * per_split : 0;
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
    hipStream_t st = static_cast<hipStream_t>(stream);
    // GLHIP_FLAG_F16X2 is accepted and ignored: the kernel has the bf16 x 3 layout only.  M == 0 runs the kernel over no tile: index -1, value +inf.
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, 0, N);
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const ArgkminParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), g, index, value, k};
        launch_argkmin<T>(prm, B, N, M, D, sc, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return check_launch("glhip_argkmin");
}

}  // extern "C"
