// glhip_api_conv.hip — C-ABI part 3: kernel products (gaussian / laplacian / energy).
#include "glhip_autosort.h"
#include "glhip_launch.h"

extern "C" {

int glhip_kernel_conv_fwd_family(int kind, int B, long N, long M, int D, int dtype, int flags, int n_ranges) {
    if (B < 0 || N < 0 || M < 0 || N > 0x7fffffffL || M > 0x7fffffffL || D < 1 || n_ranges < 0 || kind < GLHIP_GAUSSIAN || kind > GLHIP_ENERGY ||
        (dtype != GLHIP_F32 && dtype != GLHIP_BF16))
        return GLHIP_EINVAL;
    if (kind != GLHIP_GAUSSIAN && autosort_applies(B, (int)N, (int)M, D, n_ranges, flags))   // the inner launch over slabs of sorted rows
        return conv_family(kind, 0, 1, D, flags | GLHIP_FLAG_MFMA_DIST | GLHIP_FLAG_NO_SORT, (int)((N + kSortSlab - 1) / kSortSlab));
    return conv_family(kind, 0, B, D, flags, n_ranges);
}

int glhip_kernel_conv_fwd(int kind, const void* x, const void* y, const float* v, float* out, int B, int N, int M,
                          int D, float blur, int in_dtype, const int32_t* ranges_i, const int32_t* slices_i,
                          const int32_t* redranges_j, int n_ranges, void* workspace, size_t workspace_bytes,
                          int flags, void* stream) {
    int rc = check_common("glhip_kernel_conv_fwd", x, y, v, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    if (B == 0 || N == 0) return GLHIP_OK;   // nothing to write
    if (!out) return fail(GLHIP_EINVAL, "glhip_kernel_conv_fwd: NULL out");
    if (kind < GLHIP_GAUSSIAN || kind > GLHIP_ENERGY) return fail(GLHIP_EINVAL, "glhip_kernel_conv_fwd: bad kind %d", kind);
    if (kind != GLHIP_ENERGY && !(blur > 0.f)) return fail(GLHIP_EINVAL, "glhip_kernel_conv_fwd: blur must be > 0");
    const Ranges rg{ranges_i, slices_i, redranges_j};
    hipStream_t st = static_cast<hipStream_t>(stream);
    // laplacian / energy, big dense launches: sorted clouds -> distances on the matrix cores (autosort_conv, glhip_autosort.h)
    if (kind != GLHIP_GAUSSIAN && autosort_applies(B, N, M, D, n_ranges, flags)) {
        bool ran;
        rc = autosort_conv("glhip_kernel_conv_fwd", x, y, v, out, nullptr, N, M, D, in_dtype, workspace, workspace_bytes, flags, st, &ran,
                           [&](const AutoSort& a, int inner_flags) {
                               return glhip_kernel_conv_fwd(kind, a.xs, a.ys, a.col0, a.out, 1, N, M, D, blur, in_dtype, a.ranges_i, a.slices_i, a.red,
                                                            a.C, a.inner_ws, a.inner_bytes, inner_flags, stream);
                           });
        if (rc || ran) return rc;
    }
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, n_ranges, N);
    const int fam = conv_family(kind, 0, B, D, flags, n_ranges);
    rc = (in_dtype == GLHIP_F32)
             ? conv_typed<0, float>(fam, kind, x, y, v, out, nullptr, nullptr, B, N, M, D, blur, rg, n_ranges, sc, flags, st)
             : conv_typed<0, bf16_t>(fam, kind, x, y, v, out, nullptr, nullptr, B, N, M, D, blur, rg, n_ranges, sc, flags, st);
    return rc ? rc : check_launch("glhip_kernel_conv_fwd");
}

}  // extern "C"
