// glhip_family.h — WHICH kernel family serves a launch: one host predicate per entry-point family, stated once.  The bodies of
// glhip_launch.h switch on the value, the exported predicates report it, the entry points read their routes of 17 <= D <= 4095 from it.
//   soft-min forward / half-step    softmin_fwd_family -> softmin_fwd_typed      (reported by glhip_softmin_fwd_family)
//   soft-min gradient, two modes    softmin_bwd_family -> softmin_bwd_typed      (glhip_softmin_bwd_x_uses_plan, glhip_dist_grad_uses_xk)
//   kernel products, three modes    conv_family        -> conv_typed<MODE>       (glhip_kernel_conv_fwd_family, glhip_kernel_conv_grad_uses_xk,
//                                                                                 glhip_dist_grad_uses_xk)
// Plain C++ (no HIP header, no HIP type: a host compiler builds a stand-alone program around it, tests/test_grad_family_cpu.py), like
// glhip_split_policy.h, which lends the dimension limits.  Values are the GLHIP_FAMILY_* codes of include/glhip.h.
#pragma once

#include "glhip.h"
#include "glhip_split_policy.h"

namespace glhip {

// The EINVAL prologue the exported predicates of the plan family and of the gradients share
inline bool plan_family_bad_args(int B, long N, long M, int D, int dtype, int n_ranges) {
    return B < 0 || N < 0 || M < 0 || N > 0x7fffffffL || M > 0x7fffffffL || D < 1 || n_ranges < 0 || (dtype != GLHIP_F32 && dtype != GLHIP_BF16);
}

// Which matrix-core forward family serves a p = 2 soft-min / half-step / gaussian product in dimension D > 3 under `flags`
// (GLHIP_FLAG_NO_MFMA / _DIRECT: none — the generic kernel)
inline int highd_p2_family(int D, int flags) {
    if (flags & (GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_DIRECT)) return GLHIP_FAMILY_GENERIC;
    if (D <= kXdMaxD) return GLHIP_FAMILY_XD;
    return D <= kSizedMaxD ? GLHIP_FAMILY_XK : GLHIP_FAMILY_GENERIC;
}

// ... and a distance reduction (p = 1 soft-min / half-step, laplacian / energy product) in dimension D > 3: glhip_dist_xd.h up to D = 16,
// glhip_dist_xk.h for 17 <= D <= 4095 on the caller's word (GLHIP_FLAG_XK_DIST); dense launches only
inline bool highd_dist_applies(int B, int D, int flags, int n_ranges) {
    if (n_ranges != 0 || (flags & (GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_DIRECT))) return false;
    return D <= kXdMaxD || ((flags & GLHIP_FLAG_XK_DIST) && D <= kSizedMaxD && B <= 65535);
}

inline bool use_mfma_dist(int flags, int n_ranges, int B, int D) {
    return (flags & GLHIP_FLAG_MFMA_DIST) != 0 && n_ranges > 0 && B == 1 && D <= 3;
}

// The gradient routes of 17 <= D <= 4095 (glhip_grad_xk.h): the flag that opts in, none that opts out of the matrix cores, a dimension of
// the K-chunked kernels, a dense launch within the grid's batch limit
inline int xk_grad_route(int opt_in, int flags, int B, int D, int n_ranges) {
    if (!(flags & opt_in) || (flags & (GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_DIRECT))) return 0;
    return (D > kXdMaxD && D <= kSizedMaxD && n_ranges == 0 && B <= 65535) ? 1 : 0;
}

// The kernel family of a soft-min forward / fused half-step launch: THE predicate of softmin_fwd_typed, and what glhip_softmin_fwd_family
// reports.  Host arithmetic only.
inline int softmin_fwd_family(int B, long N, long M, int D, int p, int flags, int n_ranges) {
    if (D <= 3) {
        if (p == 1 && use_mfma_dist(flags, n_ranges, B, D)) return GLHIP_FAMILY_DIST;
        const bool direct = (flags & GLHIP_FLAG_DIRECT) != 0, mfma = (flags & GLHIP_FLAG_NO_MFMA) == 0;
        // GLHIP_FLAG_F16X2, big dense launches: the kernel of glhip_softmin_xd.h instantiated for D <= 3 (see softmin_fwd_typed)
        const bool ab_flag = (flags & (GLHIP_FLAG_F32_MFMA | GLHIP_FLAG_XDL16)) != 0;
        if (p == 2 && (flags & GLHIP_FLAG_F16X2) && !direct && mfma && !ab_flag && n_ranges == 0 && M >= 65536 && (double)B * N * M >= 5e8)
            return GLHIP_FAMILY_XD;
        return (p == 2 && !direct && mfma) ? GLHIP_FAMILY_X32 : GLHIP_FAMILY_VALU;
    }
    if (p == 1) return highd_dist_applies(B, D, flags, n_ranges) ? GLHIP_FAMILY_DIST : GLHIP_FAMILY_GENERIC;
    return highd_p2_family(D, flags);
}

// ... of a soft-min gradient: THE predicate of softmin_bwd_typed.  `mode` 1: the gradient (glhip_softmin_bwd_x); 2: value and unit gradient
// (glhip_softmin_fwd_grad, p = 2 on the matrix-core kernels of D <= 16 only: GLHIP_EUNSUPPORTED elsewhere).  p = 2: GLHIP_FAMILY_X32 stands for
// glhip_wsum_mfma.h (D <= 3), _XD for the transposed kernel of 4 <= D <= 16 (glhip_wsum_t32.h, block-sparse included), _XK for xk_plan_kernel
// under GLHIP_FLAG_XK_GRAD.  p = 1: GLHIP_FAMILY_DIST is dist_xd_grad_kernel (4 <= D <= 16, dense) and, under GLHIP_FLAG_XK_DIST_GRAD,
// xk_dist_grad_kernel (17 <= D <= 4095); D <= 3 stays on the VALU skeleton.
inline int softmin_bwd_family(int mode, int B, long /*N*/, long /*M*/, int D, int p, int flags, int n_ranges) {
    const bool mfma = !(flags & (GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_DIRECT));
    if (mode == 2 && (p != 2 || D > kXdMaxD || !mfma)) return GLHIP_EUNSUPPORTED;
    if (D <= 3) return (p == 2 && mfma) ? GLHIP_FAMILY_X32 : GLHIP_FAMILY_VALU;
    if (D <= kXdMaxD) {
        if (!mfma || (p == 1 && n_ranges != 0)) return GLHIP_FAMILY_GENERIC;
        return p == 2 ? GLHIP_FAMILY_XD : GLHIP_FAMILY_DIST;
    }
    if (p == 2) return xk_grad_route(GLHIP_FLAG_XK_GRAD, flags, B, D, n_ranges) ? GLHIP_FAMILY_XK : GLHIP_FAMILY_GENERIC;
    return xk_grad_route(GLHIP_FLAG_XK_DIST_GRAD, flags, B, D, n_ranges) ? GLHIP_FAMILY_DIST : GLHIP_FAMILY_GENERIC;
}

// ... and of a kernel product: THE predicate of conv_typed<MODE>.  `mode` is ConvOp's MODE: 0 product (glhip_kernel_conv_fwd; what
// glhip_kernel_conv_fwd_family reports), 1 gradient (glhip_kernel_conv_bwd_x), 2 product and unit gradient (glhip_kernel_conv_fwd_grad,
// which has no generic kernel: GLHIP_EUNSUPPORTED where the others say GLHIP_FAMILY_GENERIC).
// Gaussian: GLHIP_FAMILY_X32 stands for the matrix-core kernels of D <= 3 (glhip_wsum_x32.h / glhip_wsum_mfma.h), GLHIP_FAMILY_XD in
// modes 1 and 2 for the transposed kernel of 4 <= D <= 16 (glhip_wsum_t32.h), _XK there for xk_plan_kernel under GLHIP_FLAG_XK_GRAD.
// Laplacian / energy, modes 1 and 2: GLHIP_FAMILY_DIST in 17 <= D <= 4095 is xk_dist_grad_kernel under GLHIP_FLAG_XK_DIST_GRAD.  Mode 0 reads
// neither gradient flag.
inline int conv_family(int kind, int mode, int B, int D, int flags, int n_ranges) {
    const bool mfma = !(flags & GLHIP_FLAG_NO_MFMA);
    if (D <= 3) {
        if (kind == GLHIP_GAUSSIAN) return mfma ? GLHIP_FAMILY_X32 : GLHIP_FAMILY_VALU;
        return use_mfma_dist(flags, n_ranges, B, D) ? GLHIP_FAMILY_DIST : GLHIP_FAMILY_VALU;
    }
    const int none = mode == 2 ? GLHIP_EUNSUPPORTED : GLHIP_FAMILY_GENERIC;
    if (kind != GLHIP_GAUSSIAN) {    // laplacian / energy: distances on the matrix cores, dense launches of D <= 16 ...
        if (mode != 2 && D <= kXdMaxD && n_ranges == 0 && mfma) return GLHIP_FAMILY_DIST;
        // ... and of 17 <= D <= 4095: the product under GLHIP_FLAG_XK_DIST (glhip_dist_xk.h), its gradients under GLHIP_FLAG_XK_DIST_GRAD
        if (mode == 0) return (D > kXdMaxD && highd_dist_applies(B, D, flags, n_ranges)) ? GLHIP_FAMILY_DIST : none;
        return xk_grad_route(GLHIP_FLAG_XK_DIST_GRAD, flags, B, D, n_ranges) ? GLHIP_FAMILY_DIST : none;
    }
    if (mode == 0) return highd_p2_family(D, flags & ~GLHIP_FLAG_DIRECT);      // (_DIRECT means nothing to a kernel product)
    if (xk_grad_route(GLHIP_FLAG_XK_GRAD, flags, B, D, n_ranges)) return GLHIP_FAMILY_XK;
    return (D <= kXdMaxD && mfma) ? GLHIP_FAMILY_XD : none;
}

// the op of a laplacian / energy gradient (glhip_dist_grad_uses_xk, dist_grad_xk_launch) is its kind
static_assert(GLHIP_DIST_GRAD_LAPLACIAN == GLHIP_LAPLACIAN && GLHIP_DIST_GRAD_ENERGY == GLHIP_ENERGY, "include/glhip.h");

// What the exported gradient predicates answer from a gradient family value: 1 on its route of 17 <= D <= 4095 (`route`: GLHIP_FAMILY_XK or
// GLHIP_FAMILY_DIST, which below D = 17 names other kernels)
inline int family_on_xk_route(int fam, int route, int D) { return (fam == route && D > kXdMaxD) ? 1 : 0; }

}  // namespace glhip
