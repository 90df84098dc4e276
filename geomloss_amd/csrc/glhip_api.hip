// glhip_api.hip — C-ABI of libgeomloss_hip.so (include/glhip.h), part 1: version / errors / scratch size and the soft-min FORWARD family
// (glhip_softmin_fwd, glhip_sinkhorn_step, glhip_sinkhorn_step_perm, glhip_sinkhorn_iter4, glhip_sinkhorn_anneal, glhip_sinkhorn_extrapolate4).  gfx950 only.
#include "glhip_autosort.h"
#include "glhip_launch.h"

namespace glhip {
thread_local char g_err[512] = "";
}

// XdShape<D>::NBP of the default layout for a run-time D (0 outside 4 <= D <= 16)
#define GL_NBP(DD) XdShape<DD>::NBP
static const int kXdNBP[] = {GL_NBP(4), GL_NBP(5), GL_NBP(6), GL_NBP(7), GL_NBP(8), GL_NBP(9), GL_NBP(10), GL_NBP(11), GL_NBP(12), GL_NBP(13), GL_NBP(14), GL_NBP(15), GL_NBP(16)};
#undef GL_NBP
static_assert(sizeof kXdNBP / sizeof kXdNBP[0] == kXdMaxD - 3, "one entry per dimension of the xd kernels");

extern "C" {

int glhip_version(void) { return GLHIP_VERSION; }

size_t glhip_workspace_bytes(int B, int N, int M, int D, int n_ranges) {
    // the launches' own splits and packed columns: forward_workspace_bytes (glhip_split_policy.h), with the kernels' record counts
    const int nr = X32Layout<XL_BF16X3>::NR, nbp = (D > 3 && D <= kXdMaxD) ? kXdNBP[D - 4] : 0;
    size_t bytes = forward_workspace_bytes(B, N, M, D, n_ranges, nr, nbp);
    if (bytes > 0 && autosort_applies(B, N, M, D, n_ranges, 0)) {
        // big dense distance reductions (p = 1, laplacian, energy) sort their clouds inside the workspace and run as a block-sparse launch
        // over slabs of 256 rows (glhip_autosort.h): the sorted copies + what that inner launch asks for
        const size_t sorted = autosort_bytes(N, M, D) + forward_workspace_bytes(1, N, M, D, (N + kSortSlab - 1) / kSortSlab, nr, nbp);
        bytes = bytes > sorted ? bytes : sorted;
    }
    return bytes;
}

const char* glhip_last_error(void) { return g_err; }

// big dense D <= 3 launches that sort their clouds first (glhip_autosort.h): p = 1 — compact row blocks -> distances on the matrix
// cores; p = 2 — only the column blocks that can change a float32 result (exact block pruning)
static bool softmin_sorts(int B, int N, int M, int D, int p, int n_ranges, int flags) {
    return (p == 1 || prune_applies(N, M)) && autosort_applies(B, N, M, D, n_ranges, flags);
}

// The inner launch of a sorted call: the block-sparse launch over the slabs of the sorted clouds, on the rest of the workspace.  p = 2:
// with the records of the second pruning level (glhip_softmin_x32.h), which only this path hands to a kernel.
static int sorted_inner(const char* fn, const AutoSort& a, const void* x, const float* h, int N, int M, int D, float eps, int p, int in_dtype,
                        int flags, hipStream_t st, const StepArgs& step) {
    const int inner = flags | (p == 1 ? GLHIP_FLAG_MFMA_DIST : 0) | GLHIP_FLAG_NO_SORT;
    Scratch sc = make_scratch(a.inner_ws, a.inner_bytes, inner, a.C, N);
    if (p == 2) {
        sc.l2.groups = static_cast<const GroupBox*>(a.groups);
        sc.l2.home = a.home;
        sc.l2.t2 = a.t2;
        sc.l2.list_takes = a.list_takes;
        sc.l2.centre_x = x;
        sc.l2.n_groups = (M + 31) / 32;
        sc.l2.L2 = (float)(prune_L(M) * 1.4426950408889634);
    }
    const Ranges rg{a.ranges_i, a.slices_i, a.red};
    return (in_dtype == GLHIP_F32) ? softmin_fwd_typed<float>(fn, a.xs, a.ys, h, a.out, 1, N, M, D, eps, p, rg, a.C, sc, inner, st, step)
                                   : softmin_fwd_typed<bf16_t>(fn, a.xs, a.ys, h, a.out, 1, N, M, D, eps, p, rg, a.C, sc, inner, st, step);
}

int glhip_softmin_fwd_family(int B, long N, long M, int D, int p, int dtype, int flags, int n_ranges) {
    if (B < 0 || N < 0 || M < 0 || N > 0x7fffffffL || M > 0x7fffffffL || D < 1 || n_ranges < 0 || (p != 1 && p != 2) ||
        (dtype != GLHIP_F32 && dtype != GLHIP_BF16))
        return GLHIP_EINVAL;
    if (softmin_sorts(B, (int)N, (int)M, D, p, n_ranges, flags))   // the inner launch: slabs of kSortSlab sorted rows as row blocks
        return softmin_fwd_family(1, N, M, D, p, flags | (p == 1 ? GLHIP_FLAG_MFMA_DIST : 0) | GLHIP_FLAG_NO_SORT, (int)((N + kSortSlab - 1) / kSortSlab));
    return softmin_fwd_family(B, N, M, D, p, flags, n_ranges);
}

int glhip_softmin_perm_applies(int B, long N, long M, int D, int p, int dtype, int flags, int n_ranges) {
    if (B < 0 || N < 0 || M < 0 || N > 0x7fffffffL || M > 0x7fffffffL || D < 1 || n_ranges < 0 || (p != 1 && p != 2) ||
        (dtype != GLHIP_F32 && dtype != GLHIP_BF16))
        return GLHIP_EINVAL;
    return p == 2 && softmin_sorts(B, (int)N, (int)M, D, p, n_ranges, flags) ? 1 : 0;
}

// The body of glhip_sinkhorn_step_perm, of glhip_sinkhorn_step (no permutation buffers) and of glhip_softmin_fwd, which is the step with
// pot = prev = NULL and damping = 1.  `fn`: the entry point the caller used, for messages.  perm_x / perm_y / perm_flags: the reused
// permutations of the sorted p = 2 call (autosort_prepare), ignored by every other call.
static int softmin_step(const char* fn, const void* x, const void* y, const float* logw, const float* pot, const float* prev, float* out, int B,
                        int N, int M, int D, float eps, float damping, int p, int in_dtype, const int32_t* ranges_i, const int32_t* slices_i,
                        const int32_t* redranges_j, int n_ranges, void* workspace, size_t workspace_bytes, int flags, void* stream,
                        int32_t* perm_x = nullptr, int32_t* perm_y = nullptr, int perm_flags = 0) {
    int rc = check_common(fn, x, y, logw, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    if (B == 0 || N == 0) return GLHIP_OK;   // nothing to write
    if (!out) return fail(GLHIP_EINVAL, "%s: NULL out", fn);
    if (out == prev) return fail(GLHIP_EINVAL, "%s: out must not alias prev (updates are simultaneous)", fn);
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "%s: eps must be > 0", fn);
    if (p != 1 && p != 2) return fail(GLHIP_EUNSUPPORTED, "%s: p must be 1 or 2 (got %d)", fn, p);
    hipStream_t st = static_cast<hipStream_t>(stream);
    StepArgs step{pot, prev, prev ? 0.5f * damping : damping, prev ? 0.5f : 0.f};
    if (softmin_sorts(B, N, M, D, p, n_ranges, flags)) {
        AutoSort a;
        const int C = (N + kSortSlab - 1) / kSortSlab;
        rc = autosort_prepare(a, x, y, N, M, D, in_dtype, workspace, workspace_bytes, glhip_workspace_bytes(1, N, M, D, C), st, p == 1, perm_x,
                              perm_y, perm_flags);
        if (rc) return rc;
        if (a.on) {      // the potentials travel with their clouds
            gather_f32(logw, a.perm_y, a.col0, M, st, a.hint_y);
            if (pot) { gather_f32(pot, a.perm_y, a.col1, M, st, a.hint_y); step.pot = a.col1; }
            if (prev) { gather_f32(prev, a.perm_x, a.row0, N, st, a.hint_x); step.prev = a.row0; }
            // (the bound takes the column vector the kernels form: logw + pot / eps)
            if (p == 2)
                prune_ranges(a.xs, a.ys, a.col0, step.pot, 1.0f / eps, N, M, D, in_dtype, eps, a.ranges_i, a.slices_i, a.red, a.blocks, a.groups, a.home,
                             a.t2, a.mlb, a.t1, a.refs, st);
            rc = sorted_inner(fn, a, x, a.col0, N, M, D, eps, p, in_dtype, flags, st, step);
            if (rc) return rc;
            scatter_f32(a.out, a.perm_x, out, N, st, 1, a.hint_x);
            return check_launch(fn);
        }
    }
    const Ranges rg{ranges_i, slices_i, redranges_j};
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags, n_ranges, N);
    rc = (in_dtype == GLHIP_F32) ? softmin_fwd_typed<float>(fn, x, y, logw, out, B, N, M, D, eps, p, rg, n_ranges, sc, flags, st, step)
                                 : softmin_fwd_typed<bf16_t>(fn, x, y, logw, out, B, N, M, D, eps, p, rg, n_ranges, sc, flags, st, step);
    return rc ? rc : check_launch(fn);
}

int glhip_softmin_fwd(const void* x, const void* y, const float* h, float* out, int B, int N, int M, int D,
                      float eps, int p, int in_dtype, const int32_t* ranges_i, const int32_t* slices_i,
                      const int32_t* redranges_j, int n_ranges, void* workspace, size_t workspace_bytes, int flags,
                      void* stream) {
    return softmin_step("glhip_softmin_fwd", x, y, h, nullptr, nullptr, out, B, N, M, D, eps, 1.f, p, in_dtype, ranges_i, slices_i, redranges_j,
                        n_ranges, workspace, workspace_bytes, flags, stream);
}

int glhip_sinkhorn_step(const void* x, const void* y, const float* logw, const float* pot, const float* prev,
                        float* out, int B, int N, int M, int D, float eps, float damping, int p, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream) {
    return softmin_step("glhip_sinkhorn_step", x, y, logw, pot, prev, out, B, N, M, D, eps, damping, p, in_dtype, ranges_i, slices_i, redranges_j,
                        n_ranges, workspace, workspace_bytes, flags, stream);
}

int glhip_sinkhorn_step_perm(const void* x, const void* y, const float* logw, const float* pot, const float* prev,
                             float* out, int B, int N, int M, int D, float eps, float damping, int p, int in_dtype,
                             const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                             void* workspace, size_t workspace_bytes, int flags, void* stream, int32_t* perm_x, int32_t* perm_y,
                             int perm_flags) {
    return softmin_step("glhip_sinkhorn_step_perm", x, y, logw, pot, prev, out, B, N, M, D, eps, damping, p, in_dtype, ranges_i, slices_i,
                        redranges_j, n_ranges, workspace, workspace_bytes, flags, stream, perm_x, perm_y, perm_flags);
}

int glhip_prune_inspect_slots(int M) { return M > 0 ? prune_plan(M).S : GLHIP_EINVAL; }

int glhip_prune_inspect(const void* x, const void* y, const float* logw, const float* pot, int N, int M, int D, float eps, int in_dtype,
                        int32_t* perm_x, int32_t* perm_y, double* mlb, double* t1, int32_t* home, int32_t* intervals, float* t2,
                        void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "glhip_prune_inspect";
    int rc = check_common(fn, x, y, logw, 1, N, M, D, in_dtype, nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "%s: eps must be > 0", fn);
    if (!softmin_sorts(1, N, M, D, 2, 0, 0))
        return fail(GLHIP_EUNSUPPORTED, "%s: a p = 2 call of this shape is not pruned (N = %d, M = %d, D = %d)", fn, N, M, D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AutoSort a;
    const int C = (N + kSortSlab - 1) / kSortSlab;
    rc = autosort_prepare(a, x, y, N, M, D, in_dtype, workspace, workspace_bytes, glhip_workspace_bytes(1, N, M, D, C), st, false);
    if (rc) return rc;
    if (!a.on) return fail(GLHIP_EINVAL, "%s: needs a workspace of glhip_workspace_bytes(1, N, M, D, 0)", fn);
    gather_f32(logw, a.perm_y, a.col0, M, st);
    if (pot) gather_f32(pot, a.perm_y, a.col1, M, st);
    // -inf marks the thresholds of the tiles no kernel writes (slabs without a home block)
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.t2), (int)0xFF800000u, (size_t)((N + 31) / 32), st) != hipSuccess)
        return fail(GLHIP_ELAUNCH, "%s: memset failed: %s", fn, hipGetErrorString(hipGetLastError()));
    prune_ranges(a.xs, a.ys, a.col0, pot ? a.col1 : nullptr, 1.0f / eps, N, M, D, in_dtype, eps, a.ranges_i, a.slices_i, a.red, a.blocks, a.groups,
                 a.home, a.t2, a.mlb, a.t1, a.refs, st);
    auto copy = [&](void* dst, const void* src, size_t bytes) {
        return !dst || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
    };
    const bool ok = copy(perm_x, a.perm_x, (size_t)N * 4) && copy(perm_y, a.perm_y, (size_t)M * 4) && copy(mlb, a.mlb, (size_t)C * 8) &&
                    copy(t1, a.t1, (size_t)C * 8) && copy(home, a.home, (size_t)C * 4) &&
                    copy(intervals, a.red, (size_t)C * prune_plan(M).S * 8) && copy(t2, a.t2, (size_t)((N + 31) / 32) * 4);
    if (!ok) return fail(GLHIP_ELAUNCH, "%s: copy failed: %s", fn, hipGetErrorString(hipGetLastError()));
    return check_launch(fn);
}

int glhip_sinkhorn_iter4(const void* x, const void* y, const float* a_log, const float* b_log, const float* f_ba,
                         const float* g_ab, const float* f_aa, const float* g_bb, float* f_ba_out, float* g_ab_out,
                         float* f_aa_out, float* g_bb_out, int B, int N, int M, int D, float eps, float damping, int p,
                         int in_dtype, int first, void* workspace, size_t workspace_bytes, int flags, void* stream) {
    int rc = check_common("glhip_sinkhorn_iter4", x, y, b_log, B, N, M, D, in_dtype, nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    if ((p != 1 && p != 2) || D > kXdMaxD) return fail(GLHIP_EUNSUPPORTED, "glhip_sinkhorn_iter4: only p = 1, 2 and D <= 16 (got p = %d, D = %d)", p, D);
    if (flags & (GLHIP_FLAG_DIRECT | GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_F32_MFMA | GLHIP_FLAG_XDL16))
        return fail(GLHIP_EUNSUPPORTED, "glhip_sinkhorn_iter4: runs on the default 32x32x16 kernel only (flags = %d)", flags);
    if (B == 0 || N == 0 || M == 0) return GLHIP_OK;
    if (!a_log || !f_ba_out || !g_ab_out) return fail(GLHIP_EINVAL, "glhip_sinkhorn_iter4: NULL a_log / f_ba_out / g_ab_out");
    if ((f_aa_out == nullptr) != (g_bb_out == nullptr)) return fail(GLHIP_EINVAL, "glhip_sinkhorn_iter4: f_aa_out and g_bb_out go together");
    if (first < 0 || first > 2) return fail(GLHIP_EINVAL, "glhip_sinkhorn_iter4: first must be 0, 1 or 2 (got %d)", first);
    if (first != 1 && (!f_ba || !g_ab || (f_aa_out && (!f_aa || !g_bb))))
        return fail(GLHIP_EINVAL, "glhip_sinkhorn_iter4: NULL potential (only allowed with first = 1)");
    if (first != 1 && (f_ba_out == f_ba || g_ab_out == g_ab || (f_aa_out && (f_aa_out == f_aa || g_bb_out == g_bb))))
        return fail(GLHIP_EINVAL, "glhip_sinkhorn_iter4: outputs must not alias inputs (updates are simultaneous)");
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "glhip_sinkhorn_iter4: eps must be > 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags & ~GLHIP_FLAG_PREPACK, 0, N);
    rc = (in_dtype == GLHIP_F32)
             ? iter4_typed<float>(x, y, a_log, b_log, f_ba, g_ab, f_aa, g_bb, f_ba_out, g_ab_out, f_aa_out, g_bb_out, B, N, M, D, eps, damping, p, first, sc, st)
             : iter4_typed<bf16_t>(x, y, a_log, b_log, f_ba, g_ab, f_aa, g_bb, f_ba_out, g_ab_out, f_aa_out, g_bb_out, B, N, M, D, eps, damping, p, first, sc, st);
    return rc ? rc : check_launch("glhip_sinkhorn_iter4");
}

int glhip_sinkhorn_anneal(const void* x, const void* y, const float* a_log, const float* b_log, float* const* set0, float* const* set1,
                          int B, int N, int M, int D, const float* eps, const float* damping, int n_eps, int p, int in_dtype,
                          void* workspace, size_t workspace_bytes, int flags, float f16x2_min_eps, void* stream) {
    const char* fn = "glhip_sinkhorn_anneal";
    int rc = check_common(fn, x, y, b_log, B, N, M, D, in_dtype, nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    if ((p != 1 && p != 2) || D > kXdMaxD) return fail(GLHIP_EUNSUPPORTED, "%s: only p = 1, 2 and D <= 16 (got p = %d, D = %d)", fn, p, D);
    if (flags & (GLHIP_FLAG_DIRECT | GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_F32_MFMA | GLHIP_FLAG_XDL16))
        return fail(GLHIP_EUNSUPPORTED, "%s: runs on the default 32x32x16 kernel only (flags = %d)", fn, flags);
    if (n_eps < 1 || !eps || !damping) return fail(GLHIP_EINVAL, "%s: needs n_eps >= 1 temperatures and dampings (n_eps = %d)", fn, n_eps);
    if (B == 0 || N == 0 || M == 0) return GLHIP_OK;
    if (!a_log || !set0 || !set1) return fail(GLHIP_EINVAL, "%s: NULL a_log / set0 / set1", fn);
    float* const* sets[2] = {set0, set1};
    const bool debias = set0[2] != nullptr;
    for (int s = 0; s < 2; ++s) {
        if (!sets[s][0] || !sets[s][1]) return fail(GLHIP_EINVAL, "%s: NULL f_ba / g_ab buffer in set%d", fn, s);
        if ((sets[s][2] != nullptr) != debias || (sets[s][3] != nullptr) != debias)
            return fail(GLHIP_EINVAL, "%s: the f_aa / g_bb buffers go together, in both sets or in neither", fn);
    }
    for (int i = 0; i < 8; ++i)
        for (int j = i + 1; j < 8; ++j)
            if (sets[i / 4][i % 4] && sets[i / 4][i % 4] == sets[j / 4][j % 4])
                return fail(GLHIP_EINVAL, "%s: a buffer appears twice in set0 / set1 (updates are simultaneous)", fn);
    for (int i = 0; i < n_eps; ++i)
        if (!(eps[i] > 0.f)) return fail(GLHIP_EINVAL, "%s: eps[%d] must be > 0", fn, i);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto one = [&](int i, int first, float* const* src, float* const* dst) {
        int fl = flags & ~GLHIP_FLAG_PREPACK;
        if (!(eps[i] >= f16x2_min_eps)) fl &= ~GLHIP_FLAG_F16X2;
        const Scratch sc = make_scratch(workspace, workspace_bytes, fl, 0, N);
        const float* s0 = src ? src[0] : nullptr; const float* s1 = src ? src[1] : nullptr;
        const float* s2 = src ? src[2] : nullptr; const float* s3 = src ? src[3] : nullptr;
        return (in_dtype == GLHIP_F32)
                   ? iter4_typed<float>(x, y, a_log, b_log, s0, s1, s2, s3, dst[0], dst[1], dst[2], dst[3], B, N, M, D, eps[i], damping[i], p, first, sc, st)
                   : iter4_typed<bf16_t>(x, y, a_log, b_log, s0, s1, s2, s3, dst[0], dst[1], dst[2], dst[3], B, N, M, D, eps[i], damping[i], p, first, sc, st);
    };
    rc = one(0, 1, nullptr, set0);      // initial potentials at the first temperature
    for (int i = 0; i < n_eps && !rc; ++i) rc = one(i, 0, sets[i % 2], sets[(i + 1) % 2]);
    return rc ? rc : check_launch(fn);
}

int glhip_sinkhorn_extrapolate4(const void* x, const void* y, const void* xc, const void* yc, const float* a_log_c, const float* b_log_c,
                                const float* f_ba, const float* g_ab, const float* f_aa, const float* g_bb, float* f_ba_out,
                                float* g_ab_out, float* f_aa_out, float* g_bb_out, int B, int N, int M, int Nc, int Mc, int D, float eps,
                                float damping, int p, int in_dtype, void* workspace, size_t workspace_bytes, int flags, void* stream) {
    const char* fn = "glhip_sinkhorn_extrapolate4";
    int rc = check_common(fn, x, yc, b_log_c, B, N, Mc, D, in_dtype, nullptr, nullptr, nullptr, 0);
    if (!rc) rc = check_common(fn, y, xc, a_log_c, B, M, Nc, D, in_dtype, nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    if ((p != 1 && p != 2) || D > kXdMaxD) return fail(GLHIP_EUNSUPPORTED, "%s: only p = 1, 2 and D <= 16 (got p = %d, D = %d)", fn, p, D);
    if (flags & (GLHIP_FLAG_DIRECT | GLHIP_FLAG_NO_MFMA | GLHIP_FLAG_F32_MFMA | GLHIP_FLAG_XDL16))
        return fail(GLHIP_EUNSUPPORTED, "%s: runs on the default 32x32x16 kernel only (flags = %d)", fn, flags);
    if (B == 0 || (N == 0 && M == 0)) return GLHIP_OK;
    if (Nc == 0 || Mc == 0) return fail(GLHIP_EINVAL, "%s: empty coarse measure (Nc = %d, Mc = %d)", fn, Nc, Mc);
    if (!f_ba_out || !g_ab_out || !f_ba || !g_ab) return fail(GLHIP_EINVAL, "%s: NULL f_ba / g_ab / f_ba_out / g_ab_out", fn);
    if ((f_aa_out == nullptr) != (g_bb_out == nullptr)) return fail(GLHIP_EINVAL, "%s: f_aa_out and g_bb_out go together", fn);
    if (f_aa_out && (!f_aa || !g_bb)) return fail(GLHIP_EINVAL, "%s: NULL f_aa / g_bb", fn);
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "%s: eps must be > 0", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Scratch sc = make_scratch(workspace, workspace_bytes, flags & ~GLHIP_FLAG_PREPACK, 0, N > M ? N : M);
    rc = (in_dtype == GLHIP_F32)
             ? extrapolate4_typed<float>(x, y, xc, yc, a_log_c, b_log_c, f_ba, g_ab, f_aa, g_bb, f_ba_out, g_ab_out, f_aa_out, g_bb_out, B, N, M, Nc, Mc, D, eps, damping, p, sc, st)
             : extrapolate4_typed<bf16_t>(x, y, xc, yc, a_log_c, b_log_c, f_ba, g_ab, f_aa, g_bb, f_ba_out, g_ab_out, f_aa_out, g_bb_out, B, N, M, Nc, Mc, D, eps, damping, p, sc, st);
    return rc ? rc : check_launch(fn);
}

}  // extern "C"
