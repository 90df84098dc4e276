// glhip_api_arg_xd.hip — C-ABI part 13: the resident-operand arg-reductions of 1 <= D <= 16 (glhip_arg_xd.h) behind GLHIP_FLAG_XD_ARG:
// the family predicate of glhip_argmin / glhip_argkmin, the workspace sizing of the new family and its launch, which those two entry
// points call where the predicate says GLHIP_FAMILY_XD.  A translation unit of its own: the parallel build does not get longer.
#include "glhip_launch_plan.h"
#include "glhip_arg_xd.h"

static_assert(kArgMaxK == kArgkminMaxK, "glhip_family.h");

namespace {

// ---- the workspace of a call: [floors (k > 16)] [packed rows] [|xt|^2 / 2] [packed columns] [split partials], each rounded to 256 bytes ----
struct ArgXdLayout {
    size_t floors, xrec, hn, yrec, head;      // byte offsets; head = where the split area begins
    long xstride, ystride;
};
inline ArgXdLayout arg_xd_layout(int B, int N, int M, int D, int k) {
    const int nbp = 2 * arg_xd_num_mfma(D);
    ArgXdLayout l;
    l.xstride = packed_stride(N, nbp);
    l.ystride = packed_stride(M, nbp);
    l.floors = 0;
    l.xrec = k > kArgkminCap ? align256((size_t)B * (size_t)N * 2 * sizeof(int32_t)) : 0;
    l.hn = l.xrec + align256(packed_cols_bytes(B, N, nbp));
    l.yrec = l.hn + align256((size_t)B * (size_t)N * sizeof(float));
    l.head = l.yrec + align256(packed_cols_bytes(B, M, nbp));
    return l;
}

// The split area of one pass of kc ranks: room for either rule of plan_splits with this family's row blocks and resident workgroups
inline size_t arg_xd_split_bytes(int B, int N, int M, int NM, int kc) {
    const int rows = arg_xd_rows(arg_xd_cap(kc), NM);
    const long row_blocks = (long)B * ((N + rows - 1) / rows);
    const size_t per_split = (size_t)B * (size_t)N * 2 * kc * sizeof(float);
    long fit = (long)(kPlanMaxWorkspace / per_split);
    fit = fit < 32 ? fit : 32;
    int ns = choose_splits(row_blocks, M, 0, fit);
    if (M >= 65536 && fit >= 8) {
        const int nx = xcd_splits(row_blocks, M, kArgXdSlots, fit);
        ns = ns > nx ? ns : nx;
        ns = ns > 8 ? ns : 8;
    }
    return ns >= 2 ? (size_t)ns * per_split : 0;
}

inline size_t arg_xd_workspace_bytes(int B, int N, int M, int D, int k) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kXdMaxD || k < 1 || k > kArgkminMaxK) return 0;
    // the largest split area of the passes: those of kArgkminCap ranks and the last one; of every smaller k too, so that the size does
    // not fall where a larger k moves to the kernel shape with fewer row blocks
    size_t split = 0;
    for (int kc = 1; kc <= (k < kArgkminCap ? k : kArgkminCap); ++kc) {
        const size_t s = arg_xd_split_bytes(B, N, M, arg_xd_num_mfma(D), kc);
        split = s > split ? s : split;
    }
    return arg_xd_layout(B, N, M, D, k).head + split;
}

template <int NM, int CAP>
void launch_arg_xd_cap(const ArgXdParams& prm, int B, int N, int M, const Scratch& sc, hipStream_t st) {
    launch_plan_pass(arg_xd_rows(CAP, NM), 2 * prm.kc, kArgXdSlots, B, N, M, sc, st,
        [&](dim3 grid, const SplitInfo& sp) { hipLaunchKernelGGL((arg_xd_kernel<NM, CAP>), grid, dim3(kArgXdThreads), 0, st, prm, N, M, sp); },
        [&](const SplitInfo& sp) {
            const long rows = (long)B * N;
            hipLaunchKernelGGL((argkmin_merge_kernel<CAP>), dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm.index, prm.value,
                               rows, prm.k, prm.r0, prm.kc, prm.floor, sp);
        });
}

// one pass: the ranks prm.r0 .. prm.r0 + prm.kc - 1 on the smallest capacity that holds them
template <int NM>
void launch_arg_xd_pass(const ArgXdParams& prm, int B, int N, int M, const Scratch& sc, hipStream_t st) {
    switch (arg_xd_cap(prm.kc)) {
        case 1: launch_arg_xd_cap<NM, 1>(prm, B, N, M, sc, st); break;
        case 4: launch_arg_xd_cap<NM, 4>(prm, B, N, M, sc, st); break;
        case 8: launch_arg_xd_cap<NM, 8>(prm, B, N, M, sc, st); break;
        default: launch_arg_xd_cap<NM, 16>(prm, B, N, M, sc, st); break;
    }
}

// k <= kArgkminCap: one plain pass.  Beyond: floored passes of kArgkminCap ranks, the last one of the remainder, as glhip_api_argkmin.hip
template <int NM>
void launch_arg_xd(ArgXdParams prm, int B, int N, int M, const Scratch& sc, hipStream_t st) {
    if (prm.k <= kArgkminCap) {
        prm.floor = nullptr;
        launch_arg_xd_pass<NM>(prm, B, N, M, sc, st);
        return;
    }
    const long rows = (long)B * N;
    hipLaunchKernelGGL(argkmin_floor_fill_kernel, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm.floor, rows);
    for (prm.r0 = 0; prm.r0 < prm.k; prm.r0 += kArgkminCap) {
        prm.kc = prm.k - prm.r0 < kArgkminCap ? prm.k - prm.r0 : kArgkminCap;
        launch_arg_xd_pass<NM>(prm, B, N, M, sc, st);
    }
}

// both clouds into records, once per call: the only kernels of the family that know D and the cloud's dtype
template <int D, typename T>
void launch_arg_xd_pack(const T* x, const T* y, const float* g, int B, int N, int M, const XdPacked& xp, const XdPacked& yp, float* hn, hipStream_t st) {
    hipLaunchKernelGGL((arg_xd_pack_rows_kernel<D, T>), dim3((N + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, x, N, xp, hn);
    SoftminParams<T> sp{};
    sp.x = x;
    sp.y = y;
    sp.h = g;
    hipLaunchKernelGGL((xd_pack_kernel<XD_ARG, D, T>), dim3((M + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, sp, N, M, yp);
}

#define GLHIP_ARG_XD_D_DISPATCH(D, CALL)                                                                                  \
    switch (D) {                                                                                                          \
        case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;              \
        case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;              \
        case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;            \
        case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; default: CALL(16); break;            \
    }

}  // namespace

namespace glhip {

int arg_xd_launch(const char* fn, const void* x, const void* y, const float* g, int32_t* index, float* value, int B, int N, int M, int D, int k,
                  int in_dtype, void* workspace, size_t workspace_bytes, int flags, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long ranks = (long)B * N * k;
    if (M == 0) {      // no column: index -1, value +inf
        hipLaunchKernelGGL(arg_xd_none_kernel, dim3((unsigned)((ranks + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, index, value, ranks);
        return check_launch(fn);
    }
    const size_t need = arg_xd_workspace_bytes(B, N, M, D, k);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return fail(GLHIP_EINVAL, "%s: GLHIP_FLAG_XD_ARG packs both clouds into the workspace and needs a 16-byte aligned one of at least %zu bytes "
                    "(got %zu): size it with glhip_arg_xd_workspace_bytes", fn, need, workspace ? workspace_bytes : (size_t)0);
    const ArgXdLayout l = arg_xd_layout(B, N, M, D, k);
    char* ws = static_cast<char*>(workspace);
    const XdPacked xp{reinterpret_cast<uint4*>(ws + l.xrec), l.xstride}, yp{reinterpret_cast<uint4*>(ws + l.yrec), l.ystride};
    float* hn = reinterpret_cast<float*>(ws + l.hn);
#define GLHIP_PACK(D_)                                                                                                                             \
    if (in_dtype == GLHIP_F32) launch_arg_xd_pack<D_, float>(static_cast<const float*>(x), static_cast<const float*>(y), g, B, N, M, xp, yp, hn, st); \
    else launch_arg_xd_pack<D_, bf16_t>(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(y), g, B, N, M, xp, yp, hn, st)
    GLHIP_ARG_XD_D_DISPATCH(D, GLHIP_PACK)
#undef GLHIP_PACK
    // the splits take what follows the operands
    const size_t rest = workspace_bytes - l.head;
    const Scratch sc = make_scratch(rest ? ws + l.head : nullptr, rest, flags, 0, N);
    const ArgXdParams prm{xp.rec, xp.stride, yp.rec, yp.stride, hn, index, value, k, 0, k, reinterpret_cast<int32_t*>(ws + l.floors)};
    switch (arg_xd_num_mfma(D)) {
        case 1: launch_arg_xd<1>(prm, B, N, M, sc, st); break;
        case 2: launch_arg_xd<2>(prm, B, N, M, sc, st); break;
        case 3: launch_arg_xd<3>(prm, B, N, M, sc, st); break;
        case 4: launch_arg_xd<4>(prm, B, N, M, sc, st); break;
        case 5: launch_arg_xd<5>(prm, B, N, M, sc, st); break;
        case 6: launch_arg_xd<6>(prm, B, N, M, sc, st); break;
        default: launch_arg_xd<7>(prm, B, N, M, sc, st); break;
    }
    return check_launch(fn);
}

}  // namespace glhip

extern "C" {

int glhip_arg_family(int B, long N, long M, int D, int k, int p, int dtype, int n_ranges, int flags) {
    return arg_family(B, N, M, D, k, p, dtype, n_ranges, flags);
}

size_t glhip_arg_xd_workspace_bytes(int B, int N, int M, int D, int k) { return arg_xd_workspace_bytes(B, N, M, D, k); }

}  // extern "C"
