// glhip_api_plan_p1_xd.hip — C-ABI part 18: the resident-operand p = 1 plan application of 1 <= D <= 16 (glhip_dist_plan_xd.h) behind
// GLHIP_FLAG_XD_PLAN_P1: the exported family predicate of glhip_plan_apply_p1, the pass width and the workspace sizing of the new family
// and its launch, which glhip_plan_apply_p1 calls where the predicate says GLHIP_FAMILY_XD.  A translation unit of its own: the parallel
// build does not get longer.
#include "glhip_launch_plan.h"
#include "glhip_dist_plan_xd.h"

namespace {

// features one pass carries: the widest instantiation without scratch (all of them, see the table in glhip_dist_plan_xd.h)
inline int xd_dist_plan_pass_width(int) { return 32 * kXdDistPlanMaxChunks; }

// ---- the workspace of a call: [packed rows] [n_i] [packed columns] [S_j] [feature pieces of a pass] [their inverse scales] [split
// partials], each rounded to 256 bytes.  The feature area is sized for the widest pass of the call: `chunks` chunks of 32 features. ----
struct XdDistPlanLayout {
    size_t xrec, nrow, yrec, ys, qrec, qinv, head;      // byte offsets; head = where the split area begins
    long xstride, ystride;
    int NM, chunks;
};
inline XdDistPlanLayout xd_dist_plan_layout(int B, int N, int M, int D, int V) {
    XdDistPlanLayout l;
    l.NM = xd_dist_plan_num_mfma(D);
    const int width = xd_dist_plan_pass_width(D), wv = V < width ? V : width;
    l.chunks = xd_dist_plan_inst_chunks((wv + 31) / 32);
    const size_t groups = (size_t)((M + 31) / 32);
    l.xstride = packed_stride(N, 2 * l.NM);
    l.ystride = packed_stride(M, 2 * l.NM);
    l.xrec = 0;
    l.nrow = l.xrec + align256(packed_cols_bytes(B, N, 2 * l.NM));
    l.yrec = l.nrow + align256((size_t)B * (size_t)N * sizeof(float));
    l.ys = l.yrec + align256(packed_cols_bytes(B, M, 2 * l.NM));
    l.qrec = l.ys + align256((size_t)B * groups * 32 * sizeof(float));
    l.qinv = l.qrec + align256((size_t)B * groups * 256 * l.chunks * 16);
    l.head = l.qinv + align256((size_t)B * groups * 32 * l.chunks * sizeof(float));
    return l;
}

inline size_t xd_dist_plan_workspace_bytes(int B, int N, int M, int D, int V) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXdMaxD || V < 0) return 0;
    const XdDistPlanLayout l = xd_dist_plan_layout(B, N, M, D, V);
    if (V == 0) return l.head;      // the soft-min alone: one pass without features and without column splits
    const int width = xd_dist_plan_pass_width(D);
    // the split area of either kernel shape, so that the size does not fall where a wider V moves to the shape with fewer resident workgroups
    return l.head + ((plan_pass_workspace_bytes(B, N, M, kXdDistPlanRows, V < width ? V : width, {256, 512}) + 15) & ~(size_t)15);
}

template <int NM, int NCH>
void launch_xd_dist_plan(const XdDistPlanParams& pass, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    launch_plan_pass(kXdDistPlanRows, pass.nv + 2, xd_dist_plan_slots(NM, NCH), B, N, M, sc, st,
        [&](dim3 grid, const SplitInfo& sp) {
            hipLaunchKernelGGL((xd_dist_plan_kernel<NM, NCH>), grid, dim3(kXdDistPlanThreads), 0, st, pass, N, M, D, sp);
        },
        [&](const SplitInfo& sp) { launch_plan_merge(pass, B, N, D, sp, st); });
}

template <int NM>
void launch_xd_dist_plan_ch(const XdDistPlanParams& pass, int nch, int B, int N, int M, int D, const Scratch& sc, hipStream_t st) {
    switch (nch) {
        case 1: launch_xd_dist_plan<NM, 1>(pass, B, N, M, D, sc, st); break;
        case 2: launch_xd_dist_plan<NM, 2>(pass, B, N, M, D, sc, st); break;
        default: launch_xd_dist_plan<NM, 4>(pass, B, N, M, D, sc, st); break;
    }
}

// both clouds into records, once per call: the only kernels of the family that know D and the cloud's dtype
template <int D, typename T>
void launch_xd_dist_plan_pack(const T* x, const T* y, const float* h, int B, int N, int M, float t, const XdDistPlanLayout& l, char* ws,
                              hipStream_t st) {
    const XdPacked xp{reinterpret_cast<uint4*>(ws + l.xrec), l.xstride}, yp{reinterpret_cast<uint4*>(ws + l.yrec), l.ystride};
    hipLaunchKernelGGL((xd_dist_plan_pack_rows_kernel<D, T>), dim3((N + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, x, N, t, xp,
                       reinterpret_cast<float*>(ws + l.nrow));
    hipLaunchKernelGGL((xd_dist_plan_pack_cols_kernel<D, T>), dim3((M + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, x, y, h, N, M, t, yp,
                       reinterpret_cast<float*>(ws + l.ys));
}

#define GLHIP_XD_PLAN_P1_D_DISPATCH(D, CALL)                                                                              \
    switch (D) {                                                                                                          \
        case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;              \
        case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;              \
        case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;            \
        case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; default: CALL(16); break;            \
    }

}  // namespace

namespace glhip {

int plan_p1_xd_launch(const void* x, const void* y, const float* h, const float* feat, float* out, float* softmin, int B, int N, int M, int D,
                      int V, float eps, int in_dtype, void* workspace, size_t workspace_bytes, int flags, void* stream) {
    const char* fn = "glhip_plan_apply_p1";
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t need = xd_dist_plan_workspace_bytes(B, N, M, D, V);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return fail(GLHIP_EINVAL, "%s: GLHIP_FLAG_XD_PLAN_P1 packs both clouds and the features of a pass into the workspace and needs a 16-byte "
                    "aligned one of at least %zu bytes (got %zu): size it with glhip_plan_apply_p1_xd_workspace_bytes", fn, need,
                    workspace ? workspace_bytes : (size_t)0);
    const XdDistPlanLayout l = xd_dist_plan_layout(B, N, M, D, V);
    char* ws = static_cast<char*>(workspace);
    const float t = kLog2e / eps;      // the scales of make_softmin_params with p = 1
#define GLHIP_PACK(D_)                                                                                                                   \
    if (in_dtype == GLHIP_F32) launch_xd_dist_plan_pack<D_, float>(static_cast<const float*>(x), static_cast<const float*>(y), h, B, N, M, t, \
                                                                   l, ws, st);                                                           \
    else launch_xd_dist_plan_pack<D_, bf16_t>(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(y), h, B, N, M, t, l, ws, st)
    GLHIP_XD_PLAN_P1_D_DISPATCH(D, GLHIP_PACK)
#undef GLHIP_PACK
    // the splits take what follows the operands; V == 0: one pass without features and without column splits (the merge works per feature)
    const size_t rest = workspace_bytes - l.head;
    const Scratch sc = make_scratch(rest ? ws + l.head : nullptr, rest, V == 0 ? (flags | GLHIP_FLAG_NO_SPLIT) : flags, 0, N);
    uint4* qrec = reinterpret_cast<uint4*>(ws + l.qrec);
    float* qinv = reinterpret_cast<float*>(ws + l.qinv);
    const float* ys = reinterpret_cast<const float*>(ws + l.ys);
    const int groups = (M + 31) / 32;
    const XdDistPlanParams prm{reinterpret_cast<const uint4*>(ws + l.xrec), l.xstride, reinterpret_cast<const float*>(ws + l.nrow),
                               reinterpret_cast<const uint4*>(ws + l.yrec), l.ystride, ys, qrec, 0, qinv, x, y, out, softmin,
                               t, 1e-8f * t * t, dist_guard(), -eps * kLn2, in_dtype == GLHIP_BF16 ? 1 : 0, V, 0, 0};
    auto one = [&](XdDistPlanParams pass, int nch) {
        const int inst = xd_dist_plan_inst_chunks(nch), VC = 32 * inst;      // inst <= l.chunks: the pass fits the feature area
        pass.qstride = (long)groups * 256 * inst;
        const long items = (long)groups * VC;
        hipLaunchKernelGGL(xd_dist_plan_pack_feat_kernel, dim3((unsigned)((items + kBlock - 1) / kBlock), B, 1), dim3(kBlock), 0, st, feat, ys, M, V,
                           pass.v0, pass.nv, VC, qrec, pass.qstride, qinv);
        switch (l.NM) {
            case 1: launch_xd_dist_plan_ch<1>(pass, inst, B, N, M, D, sc, st); break;
            case 2: launch_xd_dist_plan_ch<2>(pass, inst, B, N, M, D, sc, st); break;
            case 3: launch_xd_dist_plan_ch<3>(pass, inst, B, N, M, D, sc, st); break;
            case 4: launch_xd_dist_plan_ch<4>(pass, inst, B, N, M, D, sc, st); break;
            case 5: launch_xd_dist_plan_ch<5>(pass, inst, B, N, M, D, sc, st); break;
            case 6: launch_xd_dist_plan_ch<6>(pass, inst, B, N, M, D, sc, st); break;
            default: launch_xd_dist_plan_ch<7>(pass, inst, B, N, M, D, sc, st); break;
        }
    };
    if (V == 0) one(prm, 1);
    else launch_plan_passes(prm, V, xd_dist_plan_pass_width(D), one);
    return check_launch(fn);
}

}  // namespace glhip

extern "C" {

int glhip_plan_apply_p1_family(int B, long N, long M, int D, int V, int dtype, int n_ranges, int flags) {
    return plan_p1_family(B, N, M, D, V, dtype, n_ranges, flags);
}

int glhip_plan_apply_p1_xd_pass_width(int D) { return (D < 1 || D > kXdMaxD) ? 0 : xd_dist_plan_pass_width(D); }

size_t glhip_plan_apply_p1_xd_workspace_bytes(int B, int N, int M, int D, int V) { return xd_dist_plan_workspace_bytes(B, N, M, D, V); }

}  // extern "C"
