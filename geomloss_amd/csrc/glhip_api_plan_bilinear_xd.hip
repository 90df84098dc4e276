// glhip_api_plan_bilinear_xd.hip — C-ABI part 17: the resident-operand bilinear plan reduction of 1 <= D <= 16, 1 <= K <= 32
// (glhip_plan_bilinear_xd.h) behind GLHIP_FLAG_XD_BILINEAR: the exported family predicate of glhip_plan_bilinear, the workspace sizing of the
// new family and its launch, which glhip_plan_bilinear calls where the predicate says GLHIP_FAMILY_XD.  A translation unit of its own: the
// parallel build does not get longer.
#include "glhip_launch_plan.h"
#include "glhip_plan_bilinear_xd.h"

static_assert(kPlanBilinearXdMaxK == kXdBilinearMaxK, "glhip_family.h");

namespace {

// ---- the workspace of a call: [packed rows] [packed row features] [x - centre] [packed columns] [group scales] [split partials], each
// rounded to 256 bytes ----
struct XdBilinearLayout {
    size_t xrec, rrec, xc, yrec, yinv, head;      // byte offsets; head = where the split area begins
    long xstride, rstride, ystride;
    int NM, NMK;
};
inline XdBilinearLayout xd_bilinear_layout(int B, int N, int M, int D, int K) {
    XdBilinearLayout l;
    l.NM = xd_bilinear_num_mfma(D);
    l.NMK = xd_bilinear_num_mfma_k(K);
    const int yrecs = xd_bilinear_group_recs(l.NM, l.NMK) / 32;      // records per column
    l.xstride = packed_stride(N, 2 * l.NM);
    l.rstride = packed_stride(N, 2 * l.NMK);
    l.ystride = packed_stride(M, yrecs);
    l.xrec = 0;
    l.rrec = l.xrec + align256(packed_cols_bytes(B, N, 2 * l.NM));
    l.xc = l.rrec + align256(packed_cols_bytes(B, N, 2 * l.NMK));
    l.yrec = l.xc + align256((size_t)B * (size_t)N * D * sizeof(float));
    l.yinv = l.yrec + align256(packed_cols_bytes(B, M, yrecs));
    l.head = l.yinv + align256((size_t)B * (size_t)((M + 31) / 32) * sizeof(float));
    return l;
}

inline size_t xd_bilinear_workspace_bytes(int B, int N, int M, int D, int K) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXdMaxD || K < 1 || K > kXdBilinearMaxK) return 0;
    const XdBilinearLayout l = xd_bilinear_layout(B, N, M, D, K);
    // the split area of either kernel shape, so that the size does not fall where a larger K moves to the shape with fewer resident workgroups
    return l.head + plan_pass_workspace_bytes(B, N, M, kXdBilinearRows, D + 1, {256, 512});
}

template <int NM, int NMK>
void launch_xd_bilinear(const XdBilinearParams& prm, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_pass(kXdBilinearRows, D + 3, xd_bilinear_slots(NM, NMK), B, N, M, sc, st,
        [&](dim3 grid, const SplitInfo& sp) {
            hipLaunchKernelGGL((xd_bilinear_kernel<NM, NMK>), grid, dim3(kXdBilinearThreads), 0, st, prm, N, M, D, sp);
        },
        [&](const SplitInfo& sp) { launch_plan_merge(prm, B, N, D, sp, st); });
}

template <int NM>
void launch_xd_bilinear_k(const XdBilinearParams& prm, int NMK, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    switch (NMK) {
        case 2: launch_xd_bilinear<NM, 2>(prm, B, N, M, D, sc, st); break;
        case 3: launch_xd_bilinear<NM, 3>(prm, B, N, M, D, sc, st); break;
        case 6: launch_xd_bilinear<NM, 6>(prm, B, N, M, D, sc, st); break;
        default: launch_xd_bilinear<NM, 12>(prm, B, N, M, D, sc, st); break;
    }
}

// both clouds into records, once per call: the only kernels of the family that know D and the cloud's dtype
template <int D, typename T>
void launch_xd_bilinear_pack(const T* x, const T* y, const float* h, const float* fwd, int B, int N, int M, float s2, float out_scale,
                             const XdBilinearLayout& l, char* ws, hipStream_t st) {
    const XdPacked xp{reinterpret_cast<uint4*>(ws + l.xrec), l.xstride}, yp{reinterpret_cast<uint4*>(ws + l.yrec), l.ystride};
    hipLaunchKernelGGL((xd_bilinear_pack_rows_kernel<D, T>), dim3((N + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, x, fwd, N, s2, out_scale, xp,
                       reinterpret_cast<float*>(ws + l.xc));
    hipLaunchKernelGGL((xd_bilinear_pack_cols_kernel<D, T>), dim3((M + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, x, y, h, N, M, s2, yp,
                       xd_bilinear_group_recs(l.NM, l.NMK), 64 * (l.NM + l.NMK), reinterpret_cast<float*>(ws + l.yinv));
}

#define GLHIP_XD_BILINEAR_D_DISPATCH(D, CALL)                                                                             \
    switch (D) {                                                                                                          \
        case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;              \
        case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;              \
        case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;            \
        case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; default: CALL(16); break;            \
    }

}  // namespace

namespace glhip {

int plan_bilinear_xd_launch(const void* x, const void* y, const float* h, const float* fwd, const float* rowfeat, const float* colfeat, float* out,
                            float* wsum, int B, int N, int M, int D, int K, float eps, int in_dtype, void* workspace, size_t workspace_bytes,
                            int flags, void* stream) {
    const char* fn = "glhip_plan_bilinear";
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t need = xd_bilinear_workspace_bytes(B, N, M, D, K);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return fail(GLHIP_EINVAL, "%s: GLHIP_FLAG_XD_BILINEAR packs both clouds and both feature matrices into the workspace and needs a 16-byte "
                    "aligned one of at least %zu bytes (got %zu): size it with glhip_plan_bilinear_xd_workspace_bytes", fn, need,
                    workspace ? workspace_bytes : (size_t)0);
    const XdBilinearLayout l = xd_bilinear_layout(B, N, M, D, K);
    char* ws = static_cast<char*>(workspace);
    const float s2 = kLog2e / eps, out_scale = -eps * kLn2;
#define GLHIP_PACK(D_)                                                                                                                          \
    if (in_dtype == GLHIP_F32) launch_xd_bilinear_pack<D_, float>(static_cast<const float*>(x), static_cast<const float*>(y), h, fwd, B, N, M, s2, \
                                                                  out_scale, l, ws, st);                                                        \
    else launch_xd_bilinear_pack<D_, bf16_t>(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(y), h, fwd, B, N, M, s2, out_scale, l, ws, st)
    GLHIP_XD_BILINEAR_D_DISPATCH(D, GLHIP_PACK)
#undef GLHIP_PACK
    // the two weight chains: one workgroup row per record
    uint4* rrec = reinterpret_cast<uint4*>(ws + l.rrec);
    uint4* yrec = reinterpret_cast<uint4*>(ws + l.yrec);
    hipLaunchKernelGGL((xd_bilinear_pack_feat_kernel<true>), dim3((N + 31 + kBlock) / kBlock, 2 * l.NMK, B), dim3(kBlock), 0, st, rowfeat, N, K, rrec,
                       l.rstride, 64 * l.NMK, 0);
    hipLaunchKernelGGL((xd_bilinear_pack_feat_kernel<false>), dim3((M + 31 + kBlock) / kBlock, 2 * l.NMK, B), dim3(kBlock), 0, st, colfeat, M, K, yrec,
                       l.ystride, xd_bilinear_group_recs(l.NM, l.NMK), 64 * l.NM);
    // the splits take what follows the operands
    const size_t rest = workspace_bytes - l.head;
    const Scratch sc = make_scratch(rest ? ws + l.head : nullptr, rest, flags, 0, N);
    const XdBilinearParams prm{reinterpret_cast<const uint4*>(ws + l.xrec), l.xstride, rrec, l.rstride, yrec, l.ystride,
                               reinterpret_cast<const float*>(ws + l.yinv), reinterpret_cast<const float*>(ws + l.xc), out, wsum, D + 1};
    switch (l.NM) {
        case 1: launch_xd_bilinear_k<1>(prm, l.NMK, B, N, M, D, sc, st); break;
        case 2: launch_xd_bilinear_k<2>(prm, l.NMK, B, N, M, D, sc, st); break;
        case 3: launch_xd_bilinear_k<3>(prm, l.NMK, B, N, M, D, sc, st); break;
        case 4: launch_xd_bilinear_k<4>(prm, l.NMK, B, N, M, D, sc, st); break;
        case 5: launch_xd_bilinear_k<5>(prm, l.NMK, B, N, M, D, sc, st); break;
        case 6: launch_xd_bilinear_k<6>(prm, l.NMK, B, N, M, D, sc, st); break;
        default: launch_xd_bilinear_k<7>(prm, l.NMK, B, N, M, D, sc, st); break;
    }
    return check_launch(fn);
}

}  // namespace glhip

extern "C" {

int glhip_plan_bilinear_family(int B, long N, long M, int D, int K, int p, int dtype, int n_ranges, int flags) {
    return plan_bilinear_family(B, N, M, D, K, p, dtype, n_ranges, flags);
}

size_t glhip_plan_bilinear_xd_workspace_bytes(int B, int N, int M, int D, int K) { return xd_bilinear_workspace_bytes(B, N, M, D, K); }

}  // extern "C"
