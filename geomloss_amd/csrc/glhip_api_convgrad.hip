// glhip_api_convgrad.hip — C-ABI part 4: gradients of the kernel products.
#include "glhip_autosort.h"
#include "glhip_grad_xk.h"
#include "glhip_launch.h"

extern "C" {

int glhip_kernel_conv_bwd_x(int kind, const void* x, const void* y, const float* v, const float* g, float* grad_x,
                            int B, int N, int M, int D, float blur, int in_dtype, const int32_t* ranges_i,
                            const int32_t* slices_i, const int32_t* redranges_j, int n_ranges, void* workspace,
                            size_t workspace_bytes, int flags, void* stream) {
    int rc = check_common("glhip_kernel_conv_bwd_x", x, y, v, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    if (B == 0 || N == 0) return GLHIP_OK;   // nothing to write
    if (!g || !grad_x) return fail(GLHIP_EINVAL, "glhip_kernel_conv_bwd_x: NULL g / grad_x");
    if (kind < GLHIP_GAUSSIAN || kind > GLHIP_ENERGY) return fail(GLHIP_EINVAL, "glhip_kernel_conv_bwd_x: bad kind %d", kind);
    if (kind != GLHIP_ENERGY && !(blur > 0.f)) return fail(GLHIP_EINVAL, "glhip_kernel_conv_bwd_x: blur must be > 0");
    const Ranges rg{ranges_i, slices_i, redranges_j};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int fam = conv_family(kind, 1, B, D, flags, n_ranges);
    if (fam == GLHIP_FAMILY_XK) {      // GLHIP_FLAG_XK_GRAD: gaussian, 17 <= D <= 4095, dense
        rc = gauss_grad_xk_launch(x, y, v, g, nullptr, grad_x, B, N, M, D, blur, in_dtype, workspace, workspace_bytes, flags, st);
    } else if (fam == GLHIP_FAMILY_DIST && D > kXdMaxD) {      // GLHIP_FLAG_XK_DIST_GRAD: laplacian / energy (the op is the kind), 17 <= D <= 4095, dense
        rc = dist_grad_xk_launch(kind, x, y, v, g, nullptr, grad_x, B, N, M, D, blur, in_dtype, workspace, workspace_bytes, flags, st);
    } else {
        const Scratch sc = make_scratch(workspace, workspace_bytes, flags, n_ranges, N);
        rc = (in_dtype == GLHIP_F32)
                 ? conv_typed<1, float>(fam, kind, x, y, v, nullptr, g, grad_x, B, N, M, D, blur, rg, n_ranges, sc, flags, st)
                 : conv_typed<1, bf16_t>(fam, kind, x, y, v, nullptr, g, grad_x, B, N, M, D, blur, rg, n_ranges, sc, flags, st);
    }
    return rc ? rc : check_launch("glhip_kernel_conv_bwd_x");
}

int glhip_kernel_conv_fwd_grad(int kind, const void* x, const void* y, const float* v, float* out, float* grad_unit,
                               int B, int N, int M, int D, float blur, int in_dtype, const int32_t* ranges_i,
                               const int32_t* slices_i, const int32_t* redranges_j, int n_ranges, void* workspace,
                               size_t workspace_bytes, int flags, void* stream) {
    int rc = check_common("glhip_kernel_conv_fwd_grad", x, y, v, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    if (kind < GLHIP_GAUSSIAN || kind > GLHIP_ENERGY)
        return fail(GLHIP_EINVAL, "glhip_kernel_conv_fwd_grad: unknown kernel id %d", kind);
    const int fam = conv_family(kind, 2, B, D, flags, n_ranges);
    if (fam == GLHIP_EUNSUPPORTED)
        return fail(GLHIP_EUNSUPPORTED, "glhip_kernel_conv_fwd_grad: D <= 3 (gaussian on the matrix cores: D <= 16; 17 <= D <= 4095 "
                                        "under GLHIP_FLAG_XK_GRAD; laplacian / energy of 17 <= D <= 4095 under GLHIP_FLAG_XK_DIST_GRAD) only (got kind %d, D %d, flags %d): call glhip_kernel_conv_fwd + "
                                        "glhip_kernel_conv_bwd_x", kind, D, flags);
    if (B == 0 || N == 0) return GLHIP_OK;
    if (!out || !grad_unit) return fail(GLHIP_EINVAL, "glhip_kernel_conv_fwd_grad: NULL out / grad_unit");
    if (kind != GLHIP_ENERGY && !(blur > 0.f)) return fail(GLHIP_EINVAL, "glhip_kernel_conv_fwd_grad: blur must be > 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (fam == GLHIP_FAMILY_XK) {      // GLHIP_FLAG_XK_GRAD: gaussian, 17 <= D <= 4095, dense: the passes of glhip_gauss_grad_xk.h
        rc = gauss_grad_xk_launch(x, y, v, nullptr, out, grad_unit, B, N, M, D, blur, in_dtype, workspace, workspace_bytes, flags, st);
        return rc ? rc : check_launch("glhip_kernel_conv_fwd_grad");
    }
    if (fam == GLHIP_FAMILY_DIST && D > kXdMaxD) {      // GLHIP_FLAG_XK_DIST_GRAD: laplacian / energy (the op is the kind): the passes of glhip_dist_grad_xk.h
        rc = dist_grad_xk_launch(kind, x, y, v, nullptr, out, grad_unit, B, N, M, D, blur, in_dtype, workspace, workspace_bytes, flags, st);
        return rc ? rc : check_launch("glhip_kernel_conv_fwd_grad");
    }
    const Ranges rg{ranges_i, slices_i, redranges_j};
    if (kind != GLHIP_GAUSSIAN && autosort_applies(B, N, M, D, n_ranges, flags)) {      // as glhip_kernel_conv_fwd (autosort_conv, glhip_autosort.h)
        bool ran;
        rc = autosort_conv("glhip_kernel_conv_fwd_grad", x, y, v, out, grad_unit, N, M, D, in_dtype, workspace, workspace_bytes, flags, st, &ran,
                           [&](const AutoSort& a, int inner_flags) {
                               return glhip_kernel_conv_fwd_grad(kind, a.xs, a.ys, a.col0, a.out, a.out_rows, 1, N, M, D, blur, in_dtype, a.ranges_i,
                                                                 a.slices_i, a.red, a.C, a.inner_ws, a.inner_bytes, inner_flags, stream);
                           });
        if (rc || ran) return rc;
    }
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, n_ranges, N);
    rc = (in_dtype == GLHIP_F32)
             ? conv_typed<2, float>(fam, kind, x, y, v, out, nullptr, grad_unit, B, N, M, D, blur, rg, n_ranges, sc, flags, st)
             : conv_typed<2, bf16_t>(fam, kind, x, y, v, out, nullptr, grad_unit, B, N, M, D, blur, rg, n_ranges, sc, flags, st);
    return rc ? rc : check_launch("glhip_kernel_conv_fwd_grad");
}

}  // extern "C"
