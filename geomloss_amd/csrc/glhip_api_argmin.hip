// glhip_api_argmin.hip — C-ABI part 11: the arg-reduction glhip_argmin (glhip_argmin_xk.h) with its host-only support query and its
// workspace sizing.  A translation unit of its own: the parallel build does not get longer.
#include "glhip_launch_plan.h"
#include "glhip_argmin_xk.h"

namespace {

// THE predicate of glhip_argmin, and what glhip_argmin_supported reports.  Host arithmetic only.
inline int argmin_supported(int B, long N, long M, int D, int p, int dtype, int n_ranges) {
    if (plan_family_bad_args(B, N, M, D, dtype, n_ranges) || (p != 1 && p != 2)) return GLHIP_EINVAL;
    return (p == 2 && n_ranges == 0 && D <= kXkMaxD && B <= 65535) ? 1 : 0;
}

// The split policy is plan_splits (glhip_split_policy.h, through launch_plan_pass) with the resident workgroups of the forward kernel of 17 <= D <= 4095; the partial of
// a row is (value, index).
template <typename T>
void launch_argmin(const ArgminParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_pass(kXkRows, 2, kXkSlots, B, N, M, sc, st,
        [&](dim3 grid, const SplitInfo& sp) { hipLaunchKernelGGL((argmin_xk_kernel<T>), grid, dim3(kXkThreads), 0, st, prm, N, M, D, sp); },
        [&](const SplitInfo& sp) {
            const long rows = (long)B * N;
            hipLaunchKernelGGL(argmin_merge_kernel, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm.index, prm.value, rows, sp);
        });
}

}  // namespace

extern "C" {

int glhip_argmin_supported(int B, long N, long M, int D, int p, int dtype, int n_ranges) {
    return argmin_supported(B, N, M, D, p, dtype, n_ranges);
}

size_t glhip_argmin_workspace_bytes(int B, int N, int M, int D) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXkMaxD) return 0;
    const long row_blocks = (long)B * ((N + kXkRows - 1) / kXkRows);
    // room for either rule of plan_splits (as glhip_workspace_bytes sizes the forward of 17 <= D <= 4095): non-decreasing in M
    int ns = choose_splits(row_blocks, M, 0, 32);
    if (M >= 65536) {
        const int nx = xcd_splits(row_blocks, M, kXkSlots, 32);
        ns = ns > nx ? ns : nx;
        ns = ns > 8 ? ns : 8;
    }
    return ns >= 2 ? (size_t)ns * (size_t)B * (size_t)N * 2 * sizeof(float) : 0;
}

int glhip_argmin(const void* x, const void* y, const float* g, int32_t* index, float* value,
                 int B, int N, int M, int D, int p, int in_dtype,
                 const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                 void* workspace, size_t workspace_bytes, int flags, void* stream) {
    // (g may be NULL: check_common sees y in its place)
    int rc = check_common("glhip_argmin", x, y, y, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    const int ok = argmin_supported(B, N, M, D, p, in_dtype, n_ranges);
    if (ok == GLHIP_EINVAL) return fail(GLHIP_EINVAL, "glhip_argmin: bad argument (p %d)", p);
    if (ok == 0)
        return fail(GLHIP_EUNSUPPORTED, "glhip_argmin: only p = 2, D <= %d, dense launches (got p %d, D %d, n_ranges %d)", kXkMaxD, p, D, n_ranges);
    if (B == 0 || N == 0) return GLHIP_OK;   // nothing to write
    if (!index) return fail(GLHIP_EINVAL, "glhip_argmin: NULL index");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // GLHIP_FLAG_F16X2 is accepted and ignored: the kernel has the bf16 x 3 layout only.  M == 0 runs the kernel over no tile: index -1, value +inf.
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, 0, N);
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const ArgminParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), g, index, value};
        launch_argmin<T>(prm, B, N, M, D, sc, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return check_launch("glhip_argmin");
}

}  // extern "C"
