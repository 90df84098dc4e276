// glhip_api_plan_bilinear.hip — C-ABI part 16: the plan of a p = 2 soft-min contracted with a bilinear per-pair weight, 1 <= D <= 4095
// (glhip_plan_bilinear): xk_bilinear_kernel (glhip_plan_bilinear_xk.h), the exponent half of xk_plan_kernel, a second run of the same
// chain over the features, and the plan half against the centred coordinates.  A translation unit of its own: the parallel build does
// not get longer.
#include "glhip_launch_plan.h"
#include "glhip_plan_bilinear_xk.h"

namespace {

constexpr int kXkBilinearWidth = 32 * glhip::kXkBilinearChunks;      // coordinates per pass of xk_bilinear_kernel

// THE predicate of glhip_plan_bilinear, and what glhip_plan_bilinear_supported reports.  Host arithmetic only.
inline int plan_bilinear_supported(int B, long N, long M, int D, int K, int p, int dtype, int n_ranges) {
    if (plan_family_bad_args(B, N, M, D, dtype, n_ranges) || K < 0 || (p != 1 && p != 2)) return GLHIP_EINVAL;
    return (p != 2 || n_ranges > 0 || D > kXkMaxD || K > kXkMaxD || B > 65535) ? 0 : 1;
}

// The passes over the D coordinates, kXkBilinearWidth at a time; the partial of a row and split is (T[nv], W, mass, m): the merge counts
// W as one more sum.  In the K layout the call asks for (the exponent half only).
template <typename T>
void launch_bilinear_passes(const XkBilinearParams<T>& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_passes(prm, D, kXkBilinearWidth, [&](const XkBilinearParams<T>& pass, int) {
        launch_plan_pass(kXkRows, pass.nv + 3, kXkPlanSlots, B, N, M, sc, st,
            [&](dim3 grid, const SplitInfo& sp) {
                if (sc.h2) hipLaunchKernelGGL((xk_bilinear_kernel<T, kXkBilinearChunks, XL_F16X2>), grid, dim3(kXkThreads), 0, st, pass, N, M, D, sp);
                else hipLaunchKernelGGL((xk_bilinear_kernel<T, kXkBilinearChunks, XL_BF16X3>), grid, dim3(kXkThreads), 0, st, pass, N, M, D, sp);
            },
            [&](const SplitInfo& sp) {
                XkBilinearParams<T> mrg = pass;
                mrg.nv = pass.nv + 1;
                launch_plan_merge(mrg, B, N, D, sp, st);
            });
    });
}

}  // namespace

extern "C" {

int glhip_plan_bilinear_supported(int B, long N, long M, int D, int K, int p, int dtype, int n_ranges) {
    return plan_bilinear_supported(B, N, M, D, K, p, dtype, n_ranges);
}

int glhip_plan_bilinear_pass_width(void) { return kXkBilinearWidth; }

size_t glhip_plan_bilinear_workspace_bytes(int B, int N, int M, int D, int K) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXkMaxD || K < 1 || K > kXkMaxD) return 0;
    return plan_pass_workspace_bytes(B, N, M, kXkRows, (D < kXkBilinearWidth ? D : kXkBilinearWidth) + 1, {kXkPlanSlots});
}

int glhip_plan_bilinear(const void* x, const void* y, const float* h, const float* fwd, const float* rowfeat, const float* colfeat,
                        float* out, float* wsum, int B, int N, int M, int D, int K, float eps, int p, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream) {
    int rc = check_common("glhip_plan_bilinear", x, y, h, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    const int ok = plan_bilinear_supported(B, N, M, D, K, p, in_dtype, n_ranges);
    if (ok == GLHIP_EINVAL) return fail(GLHIP_EINVAL, "glhip_plan_bilinear: bad argument (K %d, p %d)", K, p);
    if (ok == 0)
        return fail(GLHIP_EUNSUPPORTED, "glhip_plan_bilinear: only p = 2, D <= %d, K <= %d, dense launches (got p %d, D %d, K %d, n_ranges %d)",
                    kXkMaxD, kXkMaxD, p, D, K, n_ranges);
    if (B == 0 || N == 0) return GLHIP_OK;             // nothing to write
    if (!out) return fail(GLHIP_EINVAL, "glhip_plan_bilinear: NULL out");
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "glhip_plan_bilinear: eps must be > 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (M == 0 || K == 0) {      // an empty plan or an empty weight: zero sums
        if (hipMemsetAsync(out, 0, (size_t)B * N * D * sizeof(float), st) != hipSuccess) return check_launch("glhip_plan_bilinear");
        if (wsum && hipMemsetAsync(wsum, 0, (size_t)B * N * sizeof(float), st) != hipSuccess) return check_launch("glhip_plan_bilinear");
        return check_launch("glhip_plan_bilinear");
    }
    if (!fwd || !rowfeat || !colfeat) return fail(GLHIP_EINVAL, "glhip_plan_bilinear: NULL fwd / rowfeat / colfeat");
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, 0, N);
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const XkBilinearParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), h, fwd, rowfeat, colfeat, out, wsum,
                                      kLog2e / eps, -eps * kLn2, K, 0, 0};
        launch_bilinear_passes(prm, B, N, M, D, sc, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return check_launch("glhip_plan_bilinear");
}

}  // extern "C"
