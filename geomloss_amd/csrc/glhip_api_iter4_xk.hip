// glhip_api_iter4_xk.hip — C-ABI part 14: the one-launch Sinkhorn iteration of 17 <= D <= 4095 on pre-packed operands
// (glhip_softmin_xkp.h): the sizing entry point glhip_sinkhorn_iter4_workspace_bytes, the pack launch and the reducing launch that
// glhip_sinkhorn_iter4 / glhip_sinkhorn_anneal (glhip_api.hip) call; and the same for p = 1 under GLHIP_FLAG_XK_ITER_DIST (glhip_dist_xkp.h):
// glhip_sinkhorn_iter4_dist_workspace_bytes and the P = 1 instantiation of the reducing kernel.  A translation unit of its own: the
// parallel build does not get longer.
#include "glhip_launch.h"
#include "glhip_softmin_xkp.h"

static_assert(kXkpRows == kRowsNW4, "MultiSplit counts the row blocks of 128 rows");

namespace {

template <typename T>
void pack_typed(const void* x, const void* y, int B, int N, int M, int D, char* ws, const XkpLayout& l, hipStream_t st) {
    const int n = N > M ? N : M;
    auto rec = [&](size_t off) { return reinterpret_cast<uint4*>(ws + off); };
    hipLaunchKernelGGL((xkp_pack_kernel<T>), dim3((n + 31 + kBlock - 1) / kBlock, B, 2 * xkp_num_stages(D)), dim3(kBlock), 0, st,
                       static_cast<const T*>(x), static_cast<const T*>(y), N, M, D, rec(l.xr), rec(l.xc), rec(l.yr), rec(l.yc),
                       reinterpret_cast<float*>(ws + l.n2x), reinterpret_cast<float*>(ws + l.n2y));
}

template <typename T>
void reduce_typed(SoftminMulti<T>& m, int B, int N, int M, int D, int p, void* ws, size_t bytes, bool allow_split, hipStream_t st) {
    const XkpLayout l(B, N, M, D);
    char* base = static_cast<char*>(ws);
    auto rec = [&](size_t off) { return reinterpret_cast<const uint4*>(base + off); };
    const float* n2x = reinterpret_cast<const float*>(base + l.n2x);
    const float* n2y = reinterpret_cast<const float*>(base + l.n2y);
    // rows / columns of the problems: x / y, y / x, x / x, y / y
    const XkpOperands ops{{rec(l.xr), rec(l.yr), rec(l.xr), rec(l.yr)}, {rec(l.yc), rec(l.xc), rec(l.xc), rec(l.yc)},
                          {n2x, n2y, n2x, n2y}, {n2y, n2x, n2x, n2y}, dist_guard()};
    for (int k = m.count; k < 4; ++k) { m.p[k] = m.p[0]; m.N[k] = 0; m.M[k] = m.M[0]; }      // unused slots: no rows
    // the split partials live behind the operands
    const Scratch sc{bytes > l.partials ? base + l.partials : nullptr, bytes > l.partials ? bytes - l.partials : 0, allow_split, false, false, false,
                     ChunkBuf(), Level2()};
    MultiSplit<T> ms(m, B, kXkpRows, sc, MULTI_XD);
    if (p == 1) {
        hipLaunchKernelGGL((xkp_fwd_multi_kernel<T, 1>), ms.grid(m.count), dim3(kXkpThreads), 0, st, m, ops, D, ms.sp);
        ms.template merge<SoftminFwdOp<1, 1, true, 1, T>>(m, st);
    } else {
        hipLaunchKernelGGL((xkp_fwd_multi_kernel<T, 2>), ms.grid(m.count), dim3(kXkpThreads), 0, st, m, ops, D, ms.sp);
        ms.template merge<SoftminFwdOp<1, 2, false, 1, T>>(m, st);
    }
}

}  // namespace

namespace glhip {

bool xkp_pack(const void* x, const void* y, int B, int N, int M, int D, int in_dtype, void* ws, size_t bytes, hipStream_t st) {
    const XkpLayout l(B, N, M, D);
    if (!ws || bytes < l.partials) return false;
    if (in_dtype == GLHIP_F32) pack_typed<float>(x, y, B, N, M, D, static_cast<char*>(ws), l, st);
    else pack_typed<bf16_t>(x, y, B, N, M, D, static_cast<char*>(ws), l, st);
    return true;
}

void xkp_reduce(SoftminMulti<float>& m, int B, int N, int M, int D, int p, void* ws, size_t bytes, bool allow_split, hipStream_t st) {
    reduce_typed<float>(m, B, N, M, D, p, ws, bytes, allow_split, st);
}
void xkp_reduce(SoftminMulti<bf16_t>& m, int B, int N, int M, int D, int p, void* ws, size_t bytes, bool allow_split, hipStream_t st) {
    reduce_typed<bf16_t>(m, B, N, M, D, p, ws, bytes, allow_split, st);
}

}  // namespace glhip

extern "C" size_t glhip_sinkhorn_iter4_workspace_bytes(int B, int N, int M, int D, int p) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || (p != 1 && p != 2)) return 0;
    const int n = N > M ? N : M;
    if (D <= kXdMaxD) return 4 * glhip_workspace_bytes(B, n, n, D, 0);
    if (p != 2 || D > kXkMaxD) return 0;
    return XkpLayout(B, N, M, D).partials + xkp_partial_bytes(B, N, M);
}

// p = 1 under GLHIP_FLAG_XK_ITER_DIST: the same packed operands and split partials (glhip_sinkhorn_iter4_workspace_bytes keeps answering
// 0 for p = 1 beyond D = 16: the route is opt-in)
extern "C" size_t glhip_sinkhorn_iter4_dist_workspace_bytes(int B, int N, int M, int D) {
    if (B <= 0 || N <= 0 || M <= 0 || D <= kXdMaxD || D > kXkMaxD) return 0;
    return XkpLayout(B, N, M, D).partials + xkp_partial_bytes(B, N, M);
}
