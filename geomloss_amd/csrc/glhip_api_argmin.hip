// glhip_api_argmin.hip — C-ABI part 11: the arg-reduction glhip_argmin (glhip_argmin_xk.h) with its host-only support query and its
// workspace sizing.  A translation unit of its own: the parallel build does not get longer.
#include "glhip_launch.h"
#include "glhip_argmin_xk.h"

namespace {

// THE predicate of glhip_argmin, and what glhip_argmin_supported reports.  Host arithmetic only.
inline int argmin_supported(int B, long N, long M, int D, int p, int dtype, int n_ranges) {
    if (B < 0 || N < 0 || M < 0 || N > 0x7fffffffL || M > 0x7fffffffL || D < 1 || n_ranges < 0 || (p != 1 && p != 2) ||
        (dtype != GLHIP_F32 && dtype != GLHIP_BF16))
        return GLHIP_EINVAL;
    return (p == 2 && n_ranges == 0 && D <= kXkMaxD && B <= 65535) ? 1 : 0;
}

// THE split policy, shared by the launcher and the sizing call: the rule of launch_xk_l (glhip_launch.h) — choose_splits, or the
// XCD-aware grid with xcd_splits for dense launches with room for 8 splits over >= 65536 columns.  `fit`: splits the workspace holds.
struct ArgminSplits { int n; bool xcd; };
inline ArgminSplits argmin_splits(long row_blocks, int M, long fit, bool allow_split) {
    if (!allow_split || fit < 2) return ArgminSplits{1, false};
    if (fit >= 8 && M >= 65536) return ArgminSplits{xcd_splits(row_blocks, M, kXkSlots, fit), true};
    return ArgminSplits{choose_splits(row_blocks, M, 0, fit), false};
}

template <typename T>
void launch_argmin(const ArgminParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    const Ranges none{nullptr, nullptr, nullptr, nullptr};
    SplitLaunch sl(none, 0, B, N, M, kXkRows, 2, sc.ws, sc.bytes, sc.cb, st);
    const ArgminSplits as = argmin_splits(sl.row_blocks, M, sl.fit, sc.allow_split);
    if (!(as.xcd && sl.take_xcd(as.n)))      // (a grid beyond 2^31 workgroups stays on the plain 3-D grid)
        sl.sp.n_splits = as.xcd ? choose_splits(sl.row_blocks, M, 0, sl.fit) : as.n;
    const dim3 grid = sl.sp.xcd_grid_x > 0 ? dim3((unsigned)((long)sl.gx * B * sl.sp.n_splits), 1, 1) : dim3(sl.gx, B, sl.sp.n_splits);
    hipLaunchKernelGGL((argmin_xk_kernel<T>), grid, dim3(kXkThreads), 0, st, prm, N, M, D, sl.sp);
    if (sl.sp.n_splits > 1) {
        const long rows = (long)B * N;
        hipLaunchKernelGGL(argmin_merge_kernel, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm.index, prm.value, rows, sl.sp);
    }
}

}  // namespace

extern "C" {

int glhip_argmin_supported(int B, long N, long M, int D, int p, int dtype, int n_ranges) {
    return argmin_supported(B, N, M, D, p, dtype, n_ranges);
}

size_t glhip_argmin_workspace_bytes(int B, int N, int M, int D) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXkMaxD) return 0;
    const long row_blocks = (long)B * ((N + kXkRows - 1) / kXkRows);
    // room for either rule of argmin_splits (as glhip_workspace_bytes sizes the forward of 17 <= D <= 4095): non-decreasing in M
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
