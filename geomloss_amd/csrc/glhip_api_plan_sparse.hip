// glhip_api_plan_sparse.hip — C-ABI part 18: the transport plan of a p = 2 soft-min applied to a feature matrix on the caller's
// block-sparse ranges, 1 <= D <= 16 (glhip_plan_apply_sparse.h).  A translation unit of its own: the parallel build does not get longer.
#include "glhip_launch_plan.h"
#include "glhip_plan_apply_sparse.h"

namespace {

constexpr int kSparseWidth = 32 * kPlanMaxChunks;      // the widest pass of any dimension

// THE predicate of glhip_plan_apply_sparse, and what glhip_plan_apply_sparse_supported reports.  Host arithmetic only.
inline int plan_sparse_supported(int B, long N, long M, int D, int V, int p, int dtype, int n_ranges) {
    if (plan_family_bad_args(B, N, M, D, dtype, n_ranges) || V < 0 || (p != 1 && p != 2)) return GLHIP_EINVAL;
    return (p == 2 && D <= kXdMaxD && B == 1 && n_ranges >= 1) ? 1 : 0;
}

// The row-chunk table of a launch: 256-row chunks, at the front of the workspace
inline size_t sparse_table_bytes(int n_ranges, int N) { return chunk_table_bytes(n_ranges, N, kPlanRows); }

// Column splits.  The host sees the row blocks, not their slices: it counts at least max(n_ranges, ceil(N / 256)) chunks.  A launch with
// a chunk per resident workgroup takes no split (its chunks are its parallelism; at N = 1e5 the voxel rule gives 2000 row blocks); a
// smaller one takes the rule of every block-sparse launch on its chunks.
inline int plan_sparse_splits(int n_ranges, int N, int M, long fit, bool allow_split, long slots) {
    const long by_rows = ((long)N + kPlanRows - 1) / kPlanRows;
    const long chunks = n_ranges > by_rows ? n_ranges : by_rows;
    if (chunks >= slots) return 1;
    return rule_splits(chunks, M, n_ranges, fit, allow_split);
}

// Gathered tiles or one piece of an interval per tile.  The intervals live on the device; the host's stand-in for their mean length is
// the mean row block, as in SplitGeom::gather: voxel clusters of both clouds have one scale.  Below four tiles per block the tail of
// an interval is a quarter of its tiles and more: gather.
inline int plan_sparse_gather(int n_ranges, int N) { return (N / n_ranges < 4 * 128) ? 1 : 0; }

template <int D, typename T, int NCH, int L>
void launch_sparse_pass(const PlanParams<T>& prm, const SplitLaunch& sl, int N, int M, bool allow_split, hipStream_t st) {
    constexpr long kSlots = 256L * (PlanShape<D, NCH, L>::template waves<T>() / 2);      // resident 8-wave workgroups (PlanShape::waves)
    SplitInfo sp = sl.sp;
    sp.n_splits = plan_sparse_splits(sl.n_ranges, N, M, sl.fit, allow_split, kSlots);
    sp.gather = plan_sparse_gather(sl.n_ranges, N);
    const long cells = sp.n_splits > 1 ? (long)N * (prm.nv + 2) * sp.n_splits : (long)N * prm.nv;
    hipLaunchKernelGGL((plan_sparse_fill_kernel<T>), dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, prm, (long)N, sp);
    hipLaunchKernelGGL((plan_apply_sparse_kernel<D, T, NCH, L>), dim3(sl.chunk_grid, 1, sp.n_splits), dim3(kPlanNW * 64), 0, st, prm, sl.rgc, N, M, sp);
    if (sp.n_splits > 1) launch_plan_merge(prm, 1, N, D, sp, st);
}

// (the pass loop of launch_plan_d, glhip_api_plan.hip, on plan_sparse_max_chunks)
template <int D, typename T, int L>
void launch_sparse_d(PlanParams<T> prm, const SplitLaunch& sl, int N, int M, int V, bool allow_split, hipStream_t st) {
    constexpr int kMax = plan_sparse_max_chunks<D, L>();
    for (int v0 = 0; v0 < V; v0 += 32 * kMax) {
        prm.v0 = v0;
        prm.nv = V - v0 < 32 * kMax ? V - v0 : 32 * kMax;
        if constexpr (kMax == 4) {
            if (prm.nv > 64) { launch_sparse_pass<D, T, 4, L>(prm, sl, N, M, allow_split, st); continue; }
        }
        if constexpr (kMax >= 2) {
            if (prm.nv > 32) { launch_sparse_pass<D, T, 2, L>(prm, sl, N, M, allow_split, st); continue; }
        }
        launch_sparse_pass<D, T, 1, L>(prm, sl, N, M, allow_split, st);
    }
}

template <typename T>
void launch_sparse(const PlanParams<T>& prm, const SplitLaunch& sl, int N, int M, int D, int V, bool h2, bool allow_split, hipStream_t st) {
#define GL_SPARSE(DD)                                                                   \
    if (h2) launch_sparse_d<DD, T, XL_F16X2>(prm, sl, N, M, V, allow_split, st);        \
    else launch_sparse_d<DD, T, XL_BF16X3>(prm, sl, N, M, V, allow_split, st)
    switch (D) {
        case 1: GL_SPARSE(1); break;
        case 2: GL_SPARSE(2); break;
        case 3: GL_SPARSE(3); break;
        default: GLHIP_XD_DISPATCH(D, GL_SPARSE)
    }
#undef GL_SPARSE
}

}  // namespace

extern "C" {

int glhip_plan_apply_sparse_supported(int B, long N, long M, int D, int V, int p, int dtype, int n_ranges) {
    return plan_sparse_supported(B, N, M, D, V, p, dtype, n_ranges);
}

size_t glhip_plan_apply_sparse_workspace_bytes(int B, int N, int M, int D, int V, int n_ranges) {
    if (B != 1 || N <= 0 || M <= 0 || D < 1 || D > kXdMaxD || V <= 0 || n_ranges <= 0) return 0;
    const int nv = V < kSparseWidth ? V : kSparseWidth;
    const size_t per_split = (size_t)N * (nv + 2) * sizeof(float);
    long fit = (long)(kPlanMaxWorkspace / per_split);
    fit = fit < 32 ? fit : 32;
    const int ns = plan_sparse_splits(n_ranges, N, M, fit, true, 512);      // the larger of the kernel shapes' resident-workgroup counts
    return sparse_table_bytes(n_ranges, N) + (ns >= 2 ? (size_t)ns * per_split : 0);
}

int glhip_plan_apply_sparse(const void* x, const void* y, const float* h, const float* fwd, const float* feat, float* out, float* mass,
                            int B, int N, int M, int D, int V, float eps, int p, int in_dtype,
                            const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                            void* workspace, size_t workspace_bytes, int flags, void* stream) {
    int rc = check_common("glhip_plan_apply_sparse", x, y, h, B, N, M, D, in_dtype, ranges_i, slices_i, redranges_j, n_ranges);
    if (rc) return rc;
    const int ok = plan_sparse_supported(B, N, M, D, V, p, in_dtype, n_ranges);
    if (ok == GLHIP_EINVAL) return fail(GLHIP_EINVAL, "glhip_plan_apply_sparse: bad argument (V %d, p %d)", V, p);
    if (ok == 0)
        return fail(GLHIP_EUNSUPPORTED, "glhip_plan_apply_sparse: only p = 2, D <= %d, B = 1, n_ranges >= 1 (got p %d, D %d, B %d, n_ranges %d)",
                    kXdMaxD, p, D, B, n_ranges);
    if (N == 0 || V == 0) return GLHIP_OK;   // nothing to write
    if (!fwd || !out) return fail(GLHIP_EINVAL, "glhip_plan_apply_sparse: NULL fwd / out");
    if (!(eps > 0.f)) return fail(GLHIP_EINVAL, "glhip_plan_apply_sparse: eps must be > 0");
    if (M > 0 && !feat) return fail(GLHIP_EINVAL, "glhip_plan_apply_sparse: NULL feat");
    const size_t table = sparse_table_bytes(n_ranges, N);
    if (!workspace || workspace_bytes < table)
        return fail(GLHIP_EINVAL, "glhip_plan_apply_sparse: the workspace must hold the row-chunk table (%zu bytes; glhip_plan_apply_sparse_workspace_bytes)", table);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ChunkBuf cb{static_cast<int32_t*>(workspace), (long)n_ranges + N / kPlanRows + 1};
    const size_t rest = workspace_bytes - table;
    const Ranges rg{ranges_i, slices_i, redranges_j, nullptr};
    const int nvmax = V < kSparseWidth ? V : kSparseWidth;
    // one chunk table and one partial layout (that of the widest pass) for every pass of the call
    const SplitLaunch sl(rg, n_ranges, 1, N, M, kPlanRows, nvmax + 2, rest ? static_cast<char*>(workspace) + table : nullptr, rest, cb, st);
    const bool allow_split = (flags & GLHIP_FLAG_NO_SPLIT) == 0, h2 = (flags & GLHIP_FLAG_F16X2) != 0;
    auto run = [&](auto tag) {
        using T = decltype(tag);
        const PlanParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), h, fwd, feat, out, mass,
                                kLog2e / eps, -eps * kLn2, V, 0, 0};
        launch_sparse<T>(prm, sl, N, M, D, V, h2, allow_split, st);
    };
    if (in_dtype == GLHIP_F32) run(float{}); else run(bf16_t{});
    return check_launch("glhip_plan_apply_sparse");
}

}  // extern "C"
