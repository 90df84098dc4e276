// glhip_launch.h — host side shared by the translation units of libgeomloss_hip.so: argument checks, scratch layout, kernel
// selection and launch templates.  Everything lives in an anonymous namespace on purpose: each .hip file includes this header and
// instantiates only the templates its entry points use (forward / gradient / kernel-product kernels compile in parallel).
//
// Which kernel runs is a host predicate per entry-point family, stated once (glhip_family.h) and switched on by the body that launches:
//   soft-min forward / half-step   softmin_fwd_family -> softmin_fwd_typed         (reported by glhip_softmin_fwd_family)
//   soft-min gradient, two modes   softmin_bwd_family -> softmin_bwd_typed         (glhip_softmin_bwd_x_uses_plan / glhip_dist_grad_uses_xk read it)
//   kernel products, three modes   conv_family        -> conv_typed<MODE>          (mode 0 reported by glhip_kernel_conv_fwd_family)
// The gradient routes of 17 <= D <= 4095 are arms of the same values; their launches live in translation units of their own
// (glhip_grad_xk.h) and the entry points call them where the family says GLHIP_FAMILY_XK, or _DIST beyond D = 16.
// Parameters come from one builder each (make_softmin_params, make_conv_params: the only place that names the scales of a kernel
// kind); the one-thread-per-row fallback of the three bodies is launch_generic.  The plan family: glhip_launch_plan.h.
// How many column splits a launch takes, whether it moves to the XCD-aware grid and where it places pre-packed columns is decided in
// glhip_split_policy.h (plain C++, one plan function per policy; glhip_workspace_bytes is assembled from the same pieces): a launcher here
// builds its SplitPlan, hands it to SplitLaunch::apply and launches.
#pragma once

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "glhip_error.h"
#include "glhip_family.h"
#include "glhip_generic.h"
#include "glhip_kconv_ops.h"
#include "glhip_softmin_ops.h"
#include "glhip_wsum_mfma.h"
#include "glhip_softmin_x32.h"
#include "glhip_softmin_list.h"
#include "glhip_wsum_x32.h"
#include "glhip_dist_x32.h"
#include "glhip_dist_grad_x32.h"
#include "glhip_softmin_xd.h"
#include "glhip_softmin_xk.h"
#include "glhip_wsum_t32.h"
#include "glhip_dist_xd.h"
#include "glhip_dist_xk.h"

using namespace glhip;

namespace {

int check_common(const char* fn, const void* x, const void* y, const void* s, int B, int N, int M, int D,
                 int in_dtype, const int32_t* ri, const int32_t* si, const int32_t* rj, int n_ranges) {
    if (B < 0 || N < 0 || M < 0 || D < 1) return fail(GLHIP_EINVAL, "%s: bad sizes B=%d N=%d M=%d D=%d", fn, B, N, M, D);
    // empty clouds may come with NULL pointers (a torch tensor with no elements has none)
    if ((!x && (long)B * N > 0) || ((!y || !s) && (long)B * M > 0)) return fail(GLHIP_EINVAL, "%s: NULL input pointer", fn);
    if (in_dtype != GLHIP_F32 && in_dtype != GLHIP_BF16) return fail(GLHIP_EINVAL, "%s: bad in_dtype %d", fn, in_dtype);
    if (n_ranges < 0) return fail(GLHIP_EINVAL, "%s: n_ranges < 0", fn);
    if (n_ranges > 0) {
        if (!ri || !si || !rj) return fail(GLHIP_EINVAL, "%s: block-sparse mode needs ranges_i, slices_i, redranges_j", fn);
        if (B != 1) return fail(GLHIP_EUNSUPPORTED, "%s: block-sparse mode requires B == 1 (got %d)", fn, B);
    }
    if (B > 65535) return fail(GLHIP_EUNSUPPORTED, "%s: B=%d exceeds the grid.y limit 65535", fn, B);
    return GLHIP_OK;
}

struct Scratch {
    void* ws;
    size_t bytes;
    bool allow_split;
    bool force_pre;     // GLHIP_FLAG_PREPACK
    bool small_rows;    // GLHIP_FLAG_SMALL_ROW_BLOCKS
    bool h2;            // GLHIP_FLAG_F16X2: exponents from f16 x 2 pieces (glhip_softmin_xd.h) where a kernel has that layout
    ChunkBuf cb;        // block-sparse launches: room for the row-chunk table, carved off the front of the workspace
    Level2 l2;          // the sorted p = 2 launches of glhip_softmin_fwd / glhip_sinkhorn_step: second pruning level (glhip_softmin_x32.h)
    // what the plan functions of glhip_split_policy.h read
    SplitFlags policy() const { return SplitFlags{ws != nullptr, allow_split, force_pre, prepack_min_pairs()}; }
    static double prepack_min_pairs() {     // tuning knob: GLHIP_PREPACK_MIN (pairs per launch)
        static const double v = getenv("GLHIP_PREPACK_MIN") ? atof(getenv("GLHIP_PREPACK_MIN")) : kPrepackMinPairs;
        return v;
    }
};

// Scratch of one API call.  Block-sparse calls reserve the front of the workspace for the row-chunk table (chunk_table_rows,
// glhip_split_policy.h); the rest serves the column splits and the packed columns as before.
Scratch make_scratch(void* workspace, size_t bytes, int flags, int n_ranges, int N) {
    Scratch sc{workspace, bytes, (flags & GLHIP_FLAG_NO_SPLIT) == 0, (flags & GLHIP_FLAG_PREPACK) != 0,
               (flags & GLHIP_FLAG_SMALL_ROW_BLOCKS) != 0, (flags & GLHIP_FLAG_F16X2) != 0, ChunkBuf(), Level2()};
    const int rows = (n_ranges > 0 && workspace) ? chunk_table_rows(bytes, n_ranges, N, sc.small_rows) : 0;
    if (rows > 0) {
        const size_t need = chunk_table_bytes(n_ranges, N, rows);
        sc.cb.buf = static_cast<int32_t*>(workspace);
        sc.cb.capacity = (long)n_ranges + N / rows + 1;
        sc.ws = static_cast<char*>(workspace) + need;
        sc.bytes = bytes - need;
        if (sc.bytes == 0) sc.ws = nullptr;
    }
    return sc;
}

// the workgroup heights and the last dimension glhip_split_policy.h sizes the workspace with (and glhip_family.h routes by) are the kernels' own
static_assert(kRowsValu2 == 2 * kBlock && kRowsNW8 == kMfmaRowsPerBlock && kRowsXk == kXkRows && kSizedMaxD == kXkMaxD, "glhip_split_policy.h");

// rows per thread: 2 keeps the LDS read rate at half a ds_read_b128 per row-column step while leaving
// enough workgroups to fill 256 CUs; small problems use 1 to expose more workgroups.
inline bool use_two_rows(int B, int N, int n_ranges, const Scratch& sc) {
    if (n_ranges > 0) return true;
    if (sc.ws && sc.allow_split) return (long)B * N >= 4 * kBlock;   // column splits provide the parallelism
    const long blocks2 = (long)B * ((N + 2 * kBlock - 1) / (2 * kBlock));
    return blocks2 >= 1024;
}

// dimension dispatch: D = 1, 2, 3 (the kernels of the low-dimensional paths) and 4 <= D <= 16 (the matrix-core xd kernels)
#define GLHIP_D3_DISPATCH(D, CALL)                                                                                        \
    switch (D) {                                                                                                          \
        case 1: CALL(1); break;   case 2: CALL(2); break;   default: CALL(3); break;                                      \
    }

#define GLHIP_XD_DISPATCH(D, CALL)                                                                                        \
    switch (D) {                                                                                                          \
        case 4: CALL(4); break;   case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;              \
        case 8: CALL(8); break;   case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break;            \
        case 12: CALL(12); break; case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break;            \
        default: CALL(16); break;                                                                                         \
    }

// ---- softmin ---------------------------------------------------------------------------------------

template <int D, int P, bool DIRECT, bool BWD, typename T>
void launch_softmin_r(const SoftminParams<T>& prm, const Ranges& rg, int n_ranges, int B, int N, int M,
                      const Scratch& sc, hipStream_t st) {
    if (use_two_rows(B, N, n_ranges, sc)) {
        if constexpr (BWD) launch_mapreduce<SoftminBwdOp<D, P, DIRECT, 2, T>>(prm, rg, n_ranges, B, N, M, sc.ws, sc.bytes, sc.allow_split, st, sc.cb);
        else launch_mapreduce<SoftminFwdOp<D, P, DIRECT, 2, T>>(prm, rg, n_ranges, B, N, M, sc.ws, sc.bytes, sc.allow_split, st, sc.cb);
    } else {
        if constexpr (BWD) launch_mapreduce<SoftminBwdOp<D, P, DIRECT, 1, T>>(prm, rg, n_ranges, B, N, M, sc.ws, sc.bytes, sc.allow_split, st, sc.cb);
        else launch_mapreduce<SoftminFwdOp<D, P, DIRECT, 1, T>>(prm, rg, n_ranges, B, N, M, sc.ws, sc.bytes, sc.allow_split, st, sc.cb);
    }
}

// p = 2 forward on the matrix cores: bf16x3 on 32x32x16 MFMAs, transposed blocks (glhip_softmin_x32.h); same partial format /
// merge kernel as the VALU op.
template <int D, typename T, int NW, int L = XL_BF16X3>
void launch_softmin_mfma_nw(const SoftminParams<T>& prm, const Ranges& rg, int n_ranges, int B, int N, int M,
                            const Scratch& sc, hipStream_t st) {
    constexpr int NR = X32Layout<L>::NR;
    using MergeOp = SoftminFwdOp<D, 2, false, 1, T>;   // the forward merge does not use the row-pass centre
    constexpr int kRowsPerBlock = NW * 32;             // 32 rows per wavefront
    // block-sparse: one workgroup per row chunk of kRowsPerBlock rows (build_row_chunks_kernel)
    // 4 wavefronts on the 32x32x16 kernel, f16 x 2 layout: chunks of whole groups of 4 row tiles, leftover row tiles carried (glhip_softmin_x32.h)
    // (profiles/r06_carried_tiles_ab.txt)
    // the second pruning level rides on the workgroup shape the sorted launches get (launch_softmin_mfma): f16 x 2 on 4 wavefronts,
    // bf16 x 3 on 8; its kernel carries no leftover tiles (slabs of 256 rows are whole chunks)
    constexpr bool kP2Shape = (L == XL_F16X2) ? NW == 4 : NW == 8;
    const bool p2 = kP2Shape && n_ranges > 0 && sc.l2.groups && sc.l2.home && sc.l2.centre_x && sc.l2.t2 && sc.l2.list_takes;
    const int share = (NW == 4 && L == XL_F16X2 && n_ranges > 0 && !p2) ? 1 : 0;
    SplitLaunch sl(rg, n_ranges, B, N, M, kRowsPerBlock, 2, sc.ws, sc.bytes, sc.cb, st, share);
    const SplitPlan plan = plan_x32_fwd(sl, sc.policy(), NW, NR, share && sl.rgc.chunks);
    sl.apply(plan);
    // Dense launches of the x32 kernel with enough work to pay for one more (tiny) launch split the columns into
    // bf16x3 MFMA records ONCE, in workspace behind the split partials, instead of once per workgroup.
    PackedCols pk{nullptr, packed_stride(M, NR)};
    const bool pre = plan.pre;
    const bool use_p2 = pre && p2 && !sl.sp.gather;
    if (pre) {
        pk.rec = sl.packed<uint4>(plan);
        SoftminParams<T> pprm = prm;      // (the pack kernel reads the rows for the launch's centre only: the one the main kernel takes)
        if (use_p2) pprm.x = static_cast<const T*>(sc.l2.centre_x);
        // the sorted p = 2 launch on the f16 x 2 layout reads group-major columns, like the dense one (its intervals are whole blocks of
        // 256 sorted columns: softmin_fwd_x32_body, GSRC); the other block-sparse launches gather theirs from [M][NR]
        if (use_p2 && L == XL_F16X2) hipLaunchKernelGGL((pack_columns_kernel<D, T, true, L>), dim3((M + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, pprm, N, M, pk);
        else if (n_ranges > 0) hipLaunchKernelGGL((pack_columns_kernel<D, T, false, L>), dim3((M + kBlock - 1) / kBlock, B, 1), dim3(kBlock), 0, st, pprm, N, M, pk);
        else hipLaunchKernelGGL((pack_columns_kernel<D, T, true, L>), dim3((M + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, prm, N, M, pk);
    }
    auto main_kernel = [&](auto sparse, dim3 grid, const Ranges& r) {
        constexpr bool SP = decltype(sparse)::value;
        if constexpr (SP && kP2Shape) {
            if (use_p2) {
                // f16 x 2: two sweeps back to back on the same grid, and ONE of them does the launch's work (list_takes_launch,
                // glhip_list_cursor.h: decided on the device from the records, once, by list_decide in front of them) — the list-driven
                // kernel (glhip_softmin_list.h) where the first level keeps little or no slab has a home block, the staged one
                // otherwise; the workgroups of the other return on the int it wrote.  bf16 x 3: the staged kernel alone (the int is
                // not read).
                // GLHIP_LIST_KEEP: the rule's threshold in percent (tuning knob, read per launch: 100 = always list-driven, 0 = only without home blocks)
                if constexpr (L == XL_F16X2) {
                    const char* knob = getenv("GLHIP_LIST_KEEP");
                    const int keep_pct = knob ? atoi(knob) : kListKeepPct;
                    list_decide(r.slices_i, r.redranges_j, sc.l2.home, n_ranges, M, keep_pct, sc.l2.list_takes, st);
                    hipLaunchKernelGGL((softmin_fwd_list_p2_kernel<D, T>), grid, dim3(NW * 64), 0, st, prm, r, N, M, sl.sp, pk, sc.l2);
                }
                hipLaunchKernelGGL((softmin_fwd_x32_p2_kernel<D, T, NW, L>), grid, dim3(NW * 64), 0, st, prm, r, N, M, sl.sp, pk, sc.l2);
                return;
            }
        }
        if (pre) hipLaunchKernelGGL((softmin_fwd_x32_kernel<D, T, SP, 1, NW, true, L>), grid, dim3(NW * 64), 0, st, prm, r, N, M, sl.sp, pk);
        else hipLaunchKernelGGL((softmin_fwd_x32_kernel<D, T, SP, 1, NW, false, L>), grid, dim3(NW * 64), 0, st, prm, r, N, M, sl.sp, PackedCols{nullptr, 0});
    };
    if constexpr (NW == 2) sl.launch_sparse<MergeOp>(main_kernel, prm, st);   // block-sparse launches on row blocks of up to 64 points only (launch_softmin_mfma)
    else sl.launch<MergeOp>(main_kernel, prm, st);
}

template <int D, typename T>
void launch_softmin_mfma(const SoftminParams<T>& prm, const Ranges& rg, int n_ranges, int B, int N, int M,
                         const Scratch& sc, hipStream_t st) {
    // Workgroup height of the bf16x3 kernels: 8 wavefronts (256 rows per pass) for launches big enough to run with
    // pre-packed columns — dense (1-4 % faster than 4 there, measured from B x N = 256 x 4096 to 1 x 1e6) and
    // block-sparse with row blocks of a few hundred points (multiscale at 1e6: 0.27 vs 0.30 s); 4 wavefronts when
    // every workgroup packs its own tiles or the row blocks are small, where more, smaller workgroups win.
    static const int forced_nw = getenv("GLHIP_FWD_NW") ? atoi(getenv("GLHIP_FWD_NW")) : 0;   // tuning knob (4 or 8)
    if (sc.h2) {      // GLHIP_FLAG_F16X2: the same kernel on the f16 x 2 layout (one MFMA per block); same workgroup shapes
        // f16 x 2 (16 KB tiles): block-sparse launches run 4-wavefront workgroups whatever the cluster size — at N = 1e6 (clusters of
        // ~455 rows) 236 ms per two-scale loss against 241 with 8 wavefronts and 297 with 2 (round 6; with 32-KB bf16 x 3 tiles
        // 8 wavefronts won: the rule below); 2 x 2 row tiles per wavefront and 2 .. 12 column splits made no difference
        if (n_ranges > 0 && ((sc.small_rows && !forced_nw) || forced_nw == 2)) launch_softmin_mfma_nw<D, T, 2, XL_F16X2>(prm, rg, n_ranges, B, N, M, sc, st);
        else if (forced_nw ? forced_nw == 8 : (n_ranges == 0 && (double)B * N * M >= 5e8 && (long)B * N >= 32768))
            launch_softmin_mfma_nw<D, T, 8, XL_F16X2>(prm, rg, n_ranges, B, N, M, sc, st);
        else launch_softmin_mfma_nw<D, T, 4, XL_F16X2>(prm, rg, n_ranges, B, N, M, sc, st);
        return;
    }
    if (n_ranges > 0 && sc.small_rows && !forced_nw)
        // the caller says the pairs sit in row blocks of up to 64 points (GLHIP_FLAG_SMALL_ROW_BLOCKS): 2 wavefronts x 256-column
        // tiles — in a 4-wavefront workgroup half the wavefronts would own no row and only stage and wait.  Not inferred from the
        // MEAN block (N / n_ranges): clusters of a cloud sampled on a surface average 47 points at N = 1e5 while most pairs
        // belong to blocks of hundreds, which 64-row workgroups cut into twice the chunks (measured: 12.2 -> 18.1 ms per loss)
        launch_softmin_mfma_nw<D, T, 2>(prm, rg, n_ranges, B, N, M, sc, st);
    else if (forced_nw ? forced_nw == 8
                       : ((double)B * N * M >= 5e8 && (n_ranges == 0 ? (long)B * N >= 32768 : N / n_ranges >= 192)))
        launch_softmin_mfma_nw<D, T, 8>(prm, rg, n_ranges, B, N, M, sc, st);
    else
        launch_softmin_mfma_nw<D, T, 4>(prm, rg, n_ranges, B, N, M, sc, st);
}

// weighted-sum matrix-core kernels; MergeOp is the VALU operator with the same partial format.
//   x32 = true: glhip_wsum_x32.h (32x32x16 MFMAs, pre-packed columns when the launch is big enough) — the default;
//   x32 = false: glhip_wsum_mfma.h (16x16x32 MFMAs, GLHIP_FLAG_XDL16).
// The 32x32x16 form pays for the one-component reduction (gaussian product: 1 exp2 + 1 fma per pair, 89.8 vs 92.4 ms
// at 1e6).  With D + 1 accumulators per row it needs 64 accumulator registers per lane and its bare loop measures
// 22.8 cycles per 64 pairs (tools/ubench/overlap.hip) — what the 16x16x32 kernel already delivers end to end
// (23.3); the shipped x32 gradient kernels were slower (188 vs 148 ms), so the gradients stay on glhip_wsum_mfma.h.
template <int MODE> constexpr bool wsum_uses_x32() { return MODE == WS_GAUSS_FWD; }

template <int MODE, int D, typename T, bool SPARSE>
void launch_wsum_kernel(bool x32, bool pre, dim3 grid, hipStream_t st, const WsumParams<T>& prm, const Ranges& rg, int N, int M,
                        const SplitInfo& sp, const PackedCols& pk, const PackedQ& pq) {
    if constexpr (wsum_uses_x32<MODE>()) {
        if (x32 && pre) { hipLaunchKernelGGL((wsum_x32_kernel<MODE, D, T, SPARSE, true>), grid, dim3(kWsumNW * 64), 0, st, prm, rg, N, M, sp, pk, pq); return; }
        if (x32) { hipLaunchKernelGGL((wsum_x32_kernel<MODE, D, T, SPARSE, false>), grid, dim3(kWsumNW * 64), 0, st, prm, rg, N, M, sp, pk, pq); return; }
    }
    // block-sparse soft-min gradient / value + gradient: 2 row tiles x 8 wavefronts (119 VGPRs, 4 wavefronts per SIMD; the last
    // wavefronts of a partial chunk own no rows and skip the arithmetic) — 42.2 -> 40.4 ms at N = 1e6; dense launches are faster on
    // 4 x 4 (149 vs 160 ms), the gaussian modes indifferent (164 vs 163)
    if constexpr (SPARSE && MODE == WS_SOFTMIN_BWD) hipLaunchKernelGGL((wsum_mfma_kernel<MODE, D, T, SPARSE, 2, 8>), grid, dim3(512), 0, st, prm, rg, N, M, sp);
    else hipLaunchKernelGGL((wsum_mfma_kernel<MODE, D, T, SPARSE>), grid, dim3(kBlock), 0, st, prm, rg, N, M, sp);
}

template <int MODE, int D, typename T, class MergeOp>
void launch_wsum(const WsumParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int B,
                 int N, int M, const Scratch& sc, bool x32, hipStream_t st) {
    static_assert(WsumShape<MODE, D>::kPart == MergeOp::kPartial, "partial formats differ");
    constexpr int NQ = WsumShape<MODE, D>::kNQ;
    constexpr int NR = X32Layout<XL_BF16X3>::NR;
    SplitLaunch sl(rg, n_ranges, B, N, M, kMfmaRowsPerBlock, MergeOp::kPartial, sc.ws, sc.bytes, sc.cb, st);
    const SplitPlan plan = plan_wsum(sl, sc.policy(), wsum_uses_x32<MODE>() && x32, NR, NQ);
    sl.apply(plan);
    // pre-packed column records + q vectors behind the split partials (see launch_softmin_mfma_nw)
    PackedCols pk{nullptr, packed_stride(M, NR)};
    PackedQ pq{nullptr, (long)B * M};
    const bool pre = plan.pre;
    if constexpr (wsum_uses_x32<MODE>()) {
        if (pre) {
            pk.rec = sl.packed<uint4>(plan);
            pq.q = sl.packed<float>(plan, packed_cols_bytes(B, M, NR));
            if (n_ranges > 0) hipLaunchKernelGGL((wsum_pack_kernel<MODE, D, T, false>), dim3((M + kBlock - 1) / kBlock, B, 1), dim3(kBlock), 0, st, prm, N, M, pk, pq);
            else hipLaunchKernelGGL((wsum_pack_kernel<MODE, D, T, true>), dim3((M + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, prm, N, M, pk, pq);
        }
    }
    sl.launch<MergeOp>([&](auto sparse, dim3 grid, const Ranges& r) {
        launch_wsum_kernel<MODE, D, T, decltype(sparse)::value>(x32, pre, grid, st, prm, r, N, M, sl.sp, pk, pq);
    }, mprm, st);
}

// the soft-min gradient (and value + gradient) as a weighted sum: the transport plan row times (y_j, 1)
template <typename T>
WsumParams<T> softmin_wsum_params(const SoftminParams<T>& prm) {
    return WsumParams<T>{prm.x, prm.y, prm.h, prm.fwd, prm.g, prm.out, prm.gx, prm.s2, prm.out_scale, 1.f, prm.shift2};
}

// ... and the gaussian product / gradient: weights exp2(-s/2 |x - y|^2), s = log2(e) / blur^2
template <typename T>
WsumParams<T> gauss_wsum_params(const ConvParams<T>& prm, float blur) {
    return WsumParams<T>{prm.x, prm.y, prm.v, nullptr, prm.g, prm.out, prm.gx, kLog2e / (blur * blur), 1.f, -1.0f / (blur * blur), prm.t};
}

// p = 1 soft-min / laplacian / energy with the squared distance on the matrix cores (glhip_dist_x32.h): block-sparse launches whose
// row blocks are spatially compact, on the caller's word (GLHIP_FLAG_MFMA_DIST).  Row chunks, column splits and the merge as above.
constexpr int kDistNW = 8;
inline float dist_guard() {   // GLHIP_DIST_GUARD: test knob (1e30 = every pair on explicit differences, 0 = none)
    static const float g = getenv("GLHIP_DIST_GUARD") ? (float)atof(getenv("GLHIP_DIST_GUARD")) : 1.0f / 256.0f;
    return g;
}

// the distance kernels' parameters of a kernel product ...
template <typename T>
DistParams<T> dist_params(const ConvParams<T>& c) {
    return DistParams<T>{c.x, c.y, c.v, nullptr, nullptr, c.out, c.t, c.clamp2, 1.f, 0.f, 1.f, 0.f, dist_guard()};
}
// ... and of a p = 1 soft-min (make_softmin_params with p = 1: t = log2(e) / eps)
template <typename T>
DistParams<T> dist_params(const SoftminParams<T>& s) {
    return DistParams<T>{s.x, s.y, s.h, s.pot, s.prev, s.out, s.t, s.clamp2, s.out_scale, s.pot_scale, s.alpha, s.beta, dist_guard()};
}

template <int MODE, int D, typename T, class MergeOp, bool FAMILY = false>
void launch_dist(const DistParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int N, int M,
                 const Scratch& sc, hipStream_t st) {
    SplitLaunch sl(rg, n_ranges, 1, N, M, kDistNW * 32, MergeOp::kPartial, sc.ws, sc.bytes, sc.cb, st);
    sl.apply(plan_rule(sl, sc.allow_split));
    sl.launch_sparse<MergeOp>([&](auto, dim3 grid, const Ranges& r) {
        hipLaunchKernelGGL((dist_x32_kernel<MODE, D, T, kDistNW, FAMILY>), grid, dim3(kDistNW * 64), 0, st, prm, r, N, M, sl.sp);
    }, mprm, st);
}

// laplacian / energy product + gradient (GM = DG_FWDGRAD) or gradient (DG_BWD) on matrix-core distances (glhip_dist_grad_x32.h);
// MergeOp = ConvOp<KIND, D, 1, T, 2 | 1>: same partial formats as the direct-difference operators
template <int KIND, int GM, int D, typename T>
void launch_dist_grad(const ConvParams<T>& prm, const Ranges& rg, int n_ranges, int N, int M, const Scratch& sc, hipStream_t st) {
    using MergeOp = ConvOp<KIND, D, 1, T, GM == DG_FWDGRAD ? 2 : 1>;
    const DistGradParams<T> gp{dist_params(prm), prm.g, prm.gx, prm.gscale};
    SplitLaunch sl(rg, n_ranges, 1, N, M, kDistNW * 32, MergeOp::kPartial, sc.ws, sc.bytes, sc.cb, st);
    sl.apply(plan_rule(sl, sc.allow_split));
    sl.launch_sparse<MergeOp>([&](auto, dim3 grid, const Ranges& r) {
        hipLaunchKernelGGL((dist_grad_x32_kernel<KIND, GM, D, T, kDistNW>), grid, dim3(kDistNW * 64), 0, st, gp, r, N, M, sl.sp);
    }, prm, st);
}

template <int KIND, int GM, typename T>
void launch_dist_grad_d(const ConvParams<T>& prm, const Ranges& rg, int n_ranges, int N, int M, int D, const Scratch& sc, hipStream_t st) {
#define GL_D(DD) launch_dist_grad<KIND, GM, DD, T>(prm, rg, n_ranges, N, M, sc, st)
    GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
}

// ---- 4 <= D <= 16 on the matrix cores (glhip_softmin_xd.h): soft-min forward / fused half-step (MODE XD_SOFTMIN) and gaussian
// product (XD_GAUSS).  Column splits, XCD-aware 1-D grid for big dense launches, row chunks for block-sparse ones and the merge
// kernels are those of the D <= 3 kernels; there is no pre-packed column copy.
template <int MODE, int D, typename T, class MergeOp, int RT, int NW, int L>
void launch_xd_cfg(const SoftminParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int B, int N,
                   int M, const Scratch& sc, hipStream_t st) {
    using S = XdShape<D, L>;
    constexpr int kPart = MODE == XD_SOFTMIN ? 2 : 1;
    static_assert(MergeOp::kPartial == kPart, "partial formats differ");
    constexpr int kRows = RT * NW * 32;
    SplitLaunch sl(rg, n_ranges, B, N, M, kRows, kPart, sc.ws, sc.bytes, sc.cb, st);
    // splits by the rule, by the free-split rule or on the XCD-aware grid; pre-packed columns (glhip_softmin_xd.h): the records of all
    // columns once, in workspace behind the split partials
    const SplitPlan plan = plan_xd(sl, sc.policy(), NW, S::NBP);
    sl.apply(plan);
    XdPacked pk{nullptr, packed_stride(M, S::NBP)};
    static_assert(S::kGroupRecs == 32 * S::NBP, "packed_stride counts whole groups of 32 columns");
    if (plan.pre) {
        pk.rec = sl.packed<uint4>(plan);
        hipLaunchKernelGGL((xd_pack_kernel<MODE, D, T, L>), dim3((M + 31 + kBlock) / kBlock, B, 1), dim3(kBlock), 0, st, prm, N, M, pk);
    }
    auto main_kernel = [&](auto sparse, dim3 grid, const Ranges& r) {
        constexpr bool SP = decltype(sparse)::value;
        if constexpr (NW == 8 && !SP) {
            if (pk.rec) { hipLaunchKernelGGL((xd_fwd_kernel<MODE, D, T, false, RT, NW, true, L>), grid, dim3(NW * 64), 0, st, prm, r, N, M, sl.sp, pk); return; }
        }
        hipLaunchKernelGGL((xd_fwd_kernel<MODE, D, T, SP, RT, NW, false, L>), grid, dim3(NW * 64), 0, st, prm, r, N, M, sl.sp, XdPacked{nullptr, 0});
    };
    if constexpr (NW == 8) {
        if (plan.pre) { sl.launch_dense<MergeOp>(main_kernel, mprm, st); return; }      // (pre-packed launches are dense)
    }
    sl.launch<MergeOp>(main_kernel, mprm, st);
}

template <int MODE, int D, typename T, class MergeOp, int L>
void launch_xd_l(const SoftminParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int B, int N, int M,
                 const Scratch& sc, hipStream_t st) {
    // big launches: 8 wavefronts x 2 row tiles (the two tiles share the LDS reads of a column group; 512 rows share the bf16
    // pieces of a column when they are packed on the fly) while the x-side operands of two tiles fit 128 VGPRs — 4 waves per
    // SIMD: up to 5 chained MFMAs (D <= 12) on dense launches, 4 (D <= 9) on block-sparse ones, 1 tile beyond; small launches:
    // 4 wavefronts x 1 tile, more workgroups
    constexpr int NM = XdShape<D, L>::NM;
    const bool big = (double)B * N * M >= 5e8 && (n_ranges == 0 ? (long)B * N >= 32768 : N / n_ranges >= 192);
    if (big) {      // (constexpr where the shape decides: the configurations a dimension never takes are not compiled)
        if constexpr (NM <= 4) {
            launch_xd_cfg<MODE, D, T, MergeOp, 2, 8, L>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
        } else if constexpr (NM == 5) {
            if (n_ranges == 0) launch_xd_cfg<MODE, D, T, MergeOp, 2, 8, L>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
            else launch_xd_cfg<MODE, D, T, MergeOp, 1, 8, L>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
        } else {
            launch_xd_cfg<MODE, D, T, MergeOp, 1, 8, L>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
        }
    } else {
        launch_xd_cfg<MODE, D, T, MergeOp, 1, 4, L>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
    }
}

// ... in the K layout the call asks for: bf16 x 3 (default) or f16 x 2 (GLHIP_FLAG_F16X2: the caller vouches for the range)
template <int MODE, int D, typename T, class MergeOp>
void launch_xd(const SoftminParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int B, int N, int M,
               const Scratch& sc, hipStream_t st) {
    if (sc.h2) launch_xd_l<MODE, D, T, MergeOp, XL_F16X2>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
    else launch_xd_l<MODE, D, T, MergeOp, XL_BF16X3>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
}

// ---- 17 <= D <= 4095 on the matrix cores (glhip_softmin_xk.h): the same two operators with D as a run-time argument.  Column splits,
// the XCD-aware grid of big dense launches, row chunks of block-sparse launches and the merge kernels as above (the merge operators
// do not look at the coordinates: they are instantiated for D = 1); tiles are staged on the fly, there is no pre-packed copy, so
// the workspace holds split partials only and a launch without one runs unsplit.
template <int MODE, typename T, class MergeOp, int L>
void launch_xk_l(const SoftminParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int B, int N, int M, int D,
                 const Scratch& sc, hipStream_t st) {
    constexpr int kPart = MODE == XD_SOFTMIN ? 2 : 1;
    static_assert(MergeOp::kPartial == kPart, "partial formats differ");
    SplitLaunch sl(rg, n_ranges, B, N, M, kXkRows, kPart, sc.ws, sc.bytes, sc.cb, st);
    sl.apply(plan_rule(sl, sc.allow_split, kXkSlots, false, true));   // small clusters: gathered tiles, as in launch_softmin_mfma_nw
    sl.launch<MergeOp>([&](auto sparse, dim3 grid, const Ranges& r) {
        hipLaunchKernelGGL((xk_fwd_kernel<MODE, T, decltype(sparse)::value, L>), grid, dim3(kXkThreads), 0, st, prm, r, N, M, D, sl.sp);
    }, mprm, st);
}

// ... in the K layout the call asks for
template <int MODE, typename T, class MergeOp>
void launch_xk(const SoftminParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int B, int N, int M, int D,
               const Scratch& sc, hipStream_t st) {
    if (sc.h2) launch_xk_l<MODE, T, MergeOp, XL_F16X2>(prm, mprm, rg, n_ranges, B, N, M, D, sc, st);
    else launch_xk_l<MODE, T, MergeOp, XL_BF16X3>(prm, mprm, rg, n_ranges, B, N, M, D, sc, st);
}

// ... and the distance reductions of the same dimensions (glhip_dist_xk.h, GLHIP_FLAG_XK_DIST): p = 1 soft-min / fused half-step, laplacian
// and energy products, dense and batched launches, bf16 x 3 only.  Splits, XCD rule and merge as launch_xk_l.
template <int MODE, typename T, class MergeOp>
void launch_xk_dist(const DistParams<T>& prm, const typename MergeOp::Params& mprm, int B, int N, int M, int D, const Scratch& sc,
                    hipStream_t st) {
    static_assert(MergeOp::kPartial == (MODE == DM_SOFTMIN_P1 ? 2 : 1), "partial formats differ");
    SplitLaunch sl(Ranges{nullptr, nullptr, nullptr, nullptr}, 0, B, N, M, kXkRows, MergeOp::kPartial, sc.ws, sc.bytes, sc.cb, st);
    sl.apply(plan_rule(sl, sc.allow_split, kXkSlots));
    sl.launch_dense<MergeOp>([&](auto, dim3 grid, const Ranges&) {
        hipLaunchKernelGGL((xk_dist_kernel<MODE, T>), grid, dim3(kXkThreads), 0, st, prm, N, M, D, sl.sp);
    }, mprm, st);
}

// (plan application, the D > 16 gradients and argmin: glhip_launch_plan.h)

// distance reductions for 4 <= D <= 16, dense launches (glhip_dist_xd.h): soft-min p = 1 / fused half-step, laplacian and energy products
// (small launches split their columns further: dist_small_launch_splits, glhip_split_policy.h)
template <int MODE, int D, typename T, class MergeOp>
void launch_dist_xd(const DistParams<T>& prm, const typename MergeOp::Params& mprm, int B, int N, int M, const Scratch& sc, hipStream_t st) {
    constexpr int NW = 8;
    static_assert(MergeOp::kPartial == (MODE == DM_SOFTMIN_P1 ? 2 : 1), "partial formats differ");
    SplitLaunch sl(Ranges{nullptr, nullptr, nullptr, nullptr}, 0, B, N, M, NW * 32, MergeOp::kPartial, sc.ws, sc.bytes, sc.cb, st);
    sl.apply(plan_rule(sl, sc.allow_split, 0, true));
    sl.launch_dense<MergeOp>([&](auto, dim3 grid, const Ranges&) {
        hipLaunchKernelGGL((dist_xd_kernel<MODE, D, T, NW>), grid, dim3(NW * 64), 0, st, prm, N, M, sl.sp);
    }, mprm, st);
}

// ... and their gradients with respect to the row points (dist_xd_grad_kernel); no small-launch rule here
template <int MODE, int D, typename T, class MergeOp>
void launch_dist_xd_grad(const DistXdGradParams<T>& gp, const typename MergeOp::Params& mprm, int B, int N, int M, const Scratch& sc,
                         hipStream_t st) {
    constexpr int NW = 8;
    static_assert(MergeOp::kPartial == (MODE == DM_SOFTMIN_P1 ? D + 1 : D), "partial formats differ");
    SplitLaunch sl(Ranges{nullptr, nullptr, nullptr, nullptr}, 0, B, N, M, NW * 32, MergeOp::kPartial, sc.ws, sc.bytes, sc.cb, st);
    sl.apply(plan_rule(sl, sc.allow_split));
    sl.launch_dense<MergeOp>([&](auto, dim3 grid, const Ranges&) {
        hipLaunchKernelGGL((dist_xd_grad_kernel<MODE, D, T, NW>), grid, dim3(NW * 64), 0, st, gp, N, M, sl.sp);
    }, mprm, st);
}

// weighted-sum reductions on transposed 32 x 32 blocks (glhip_wsum_t32.h), 1 <= D <= 16; splits / grids / merges as launch_wsum
// WQ: the weighted sums on the matrix cores too (wsum_t32q_kernel: soft-min gradient, f16 x 2, one row tile per wavefront)
template <int MODE, int D, typename T, class MergeOp, int RT, int L, bool WQ = false>
void launch_wsum_t32_rt(const WsumParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int B, int N,
                     int M, const Scratch& sc, hipStream_t st) {
    static_assert(MergeOp::kPartial == ((MODE == WS_GAUSS_BWD) ? D : D + 1), "partial formats differ");
    constexpr int NW = 8 / RT;       // 256 rows per workgroup either way
    SplitLaunch sl(rg, n_ranges, B, N, M, kMfmaRowsPerBlock, MergeOp::kPartial, sc.ws, sc.bytes, sc.cb, st);
    sl.apply(plan_rule(sl, sc.allow_split, kXdSlots));
    sl.launch<MergeOp>([&](auto sparse, dim3 grid, const Ranges& r) {
        constexpr bool SP = decltype(sparse)::value;
        if constexpr (WQ) hipLaunchKernelGGL((wsum_t32q_kernel<D, T, SP, NW>), grid, dim3(NW * 64), 0, st, prm, r, N, M, sl.sp);
        else hipLaunchKernelGGL((wsum_t32_kernel<MODE, D, T, SP, RT, NW, L>), grid, dim3(NW * 64), 0, st, prm, r, N, M, sl.sp);
    }, mprm, st);
}

template <int MODE, int D, typename T, class MergeOp>
void launch_wsum_t32(const WsumParams<T>& prm, const typename MergeOp::Params& mprm, const Ranges& rg, int n_ranges, int B, int N,
                     int M, const Scratch& sc, hipStream_t st) {
    // 2 row tiles per wavefront share the LDS reads of a column group (4 wavefronts x 64 rows) up to D = 8 — measured 3-16 % faster
    // than 1 tile there (profiles/r03_grad_kernels_ab.txt); beyond, the x-side operands of two tiles no longer fit 128 VGPRs
    if constexpr (MODE == WS_SOFTMIN_BWD) {
        constexpr int wq_min_d = 7;      // (measured in round 5: the matrix-core weighted sums pay from D = 7 on)
        if (sc.h2 && D >= wq_min_d) {
            launch_wsum_t32_rt<MODE, D, T, MergeOp, 1, XL_F16X2, true>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
            return;
        }
    }
    if (sc.h2) launch_wsum_t32_rt<MODE, D, T, MergeOp, (D <= 8 ? 2 : 1), XL_F16X2>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
    else launch_wsum_t32_rt<MODE, D, T, MergeOp, (D <= 8 ? 2 : 1), XL_BF16X3>(prm, mprm, rg, n_ranges, B, N, M, sc, st);
}

// gaussian gradient (FWDGRAD = false) or product + unit gradient (true) through the transposed kernel
template <int D, bool FWDGRAD, typename T>
void launch_gauss_grad_t32(const ConvParams<T>& prm, float blur, const Ranges& rg, int n_ranges, int B, int N, int M, const Scratch& sc,
                           hipStream_t st) {
    if constexpr (FWDGRAD) launch_wsum_t32<WS_GAUSS_FWDGRAD, D, T, GaussFwdGradMerge<D, T>>(gauss_wsum_params(prm, blur), prm, rg, n_ranges, B, N, M, sc, st);
    else launch_wsum_t32<WS_GAUSS_BWD, D, T, ConvOp<GLHIP_GAUSSIAN, D, 1, T, 1>>(gauss_wsum_params(prm, blur), prm, rg, n_ranges, B, N, M, sc, st);
}

template <typename T>
SoftminParams<T> make_softmin_params(const void* x, const void* y, const float* h, float* out, float eps, int p,
                                     const float* pot, const float* prev, float alpha, float beta) {
    const float s2 = kLog2e / eps;
    SoftminParams<T> prm;
    prm.x = static_cast<const T*>(x);
    prm.y = static_cast<const T*>(y);
    prm.h = h;
    prm.out = out;
    prm.fwd = nullptr;
    prm.g = nullptr;
    prm.gx = nullptr;
    prm.s2 = s2;
    prm.t = (p == 1) ? s2 : std::sqrt(0.5f * s2);
    prm.inv_t = 1.0f / prm.t;
    prm.out_scale = -eps * kLn2;
    prm.clamp2 = 1e-8f * prm.t * prm.t;
    prm.pot = pot;
    prm.prev = prev;
    prm.pot_scale = 1.0f / eps;
    prm.alpha = alpha;
    prm.beta = beta;
    prm.shift2 = 0.f;
    return prm;
}

// The parameters of a kernel product / its gradient: the one place that names the scales of a kind (glhip_kconv_ops.h).  `t` scales the
// coordinates into base-2 units, `gscale` takes the direction sum of the scaled coordinates back to d/dx, `clamp2` = 1e-8 t^2 floors the
// scaled squared distance under a square root.  A route that reads only some of the fields (a forward merge: `out`) gets them all.
template <typename T>
ConvParams<T> make_conv_params(int kind, const void* x, const void* y, const float* v, float* out, const float* g, float* gx, float blur) {
    ConvParams<T> prm{static_cast<const T*>(x), static_cast<const T*>(y), v, out, g, gx, 1.0f, -1.0f, 1e-8f};      // energy
    if (kind == GLHIP_GAUSSIAN) {
        prm.t = std::sqrt(0.5f * kLog2e) / blur;
        prm.gscale = -1.0f / (prm.t * blur * blur);
        prm.clamp2 = 0.f;
    } else if (kind == GLHIP_LAPLACIAN) {
        prm.t = kLog2e / blur;
        prm.gscale = -1.0f / blur;
        prm.clamp2 = 1e-8f * kLog2e * kLog2e;   // the reference clamps |x/blur - y/blur|^2
    }
    return prm;
}

// the one-thread-per-row kernel of glhip_generic.h: one workgroup per row range (block-sparse) or per kBlock rows of a problem
template <int GM, bool BWD, typename T>
void launch_generic(const GenericParams<T>& prm, const Ranges& rg, int n_ranges, int B, int N, int M, int D, hipStream_t st) {
    if (n_ranges > 0) hipLaunchKernelGGL((generic_kernel<GM, BWD, true, T>), dim3(n_ranges, 1, 1), dim3(kBlock), 0, st, prm, rg, N, M, D);
    else hipLaunchKernelGGL((generic_kernel<GM, BWD, false, T>), dim3((N + kBlock - 1) / kBlock, B, 1), dim3(kBlock), 0, st, prm, rg, N, M, D);
}

// glhip_sinkhorn_iter4: `count` dense reductions in one launch of a multi kernel + one merge launch.  What the three launchers share:
// the extent of the problems (multi_geom, glhip_split_policy.h), the plan of their kind (plan_multi), the split workspace and the merge.
template <typename T>
struct MultiSplit {
    SplitGeom g;
    size_t packed[4] = {0, 0, 0, 0};      // MULTI_X32: where each problem's pre-packed columns go
    SplitPlan plan;
    SplitInfo sp;
    // `nr`: records per column of the x32 forward (MULTI_X32)
    MultiSplit(SoftminMulti<T>& m, int B, int rows, const Scratch& sc, int kind, int nr = 0)
        : g(multi_geom(m.count, m.N, m.M, B, rows, sc.ws != nullptr, sc.bytes)), plan(plan_multi(g, sc.policy(), kind, m.count, m.N, m.M, nr, packed)),
          sp{plan.n_splits, static_cast<float*>(sc.ws), 0, 0, 0} {      // (the split stride is per problem, set in the kernels)
        m.ws_stride = (long)sp.n_splits * B * g.N * 2;      // floats of split workspace per problem
    }
    dim3 grid(int count) const { return dim3(g.gx, g.B, sp.n_splits * count); }
    template <class MergeOp>
    void merge(const SoftminMulti<T>& m, hipStream_t st) const {
        if (sp.n_splits > 1)
            hipLaunchKernelGGL((merge_multi_kernel<MergeOp, T>), dim3((g.N + kBlock - 1) / kBlock, g.B, m.count), dim3(kBlock), 0, st, m, sp);
    }
};

// p = 2, D <= 3: the multi launch of the x32 forward kernel, with pre-packed columns where they pay (plan_multi)
template <int D, typename T, int L = XL_BF16X3>
void launch_iter4(SoftminMulti<T>& m, int B, const Scratch& sc, hipStream_t st) {
    constexpr int NR = X32Layout<L>::NR;
    constexpr int NW = 4;
    MultiSplit<T> ms(m, B, NW * 32, sc, MULTI_X32, NR);
    int maxM = 0;
    for (int k = 0; k < m.count; ++k) {
        maxM = m.M[k] > maxM ? m.M[k] : maxM;
        m.pk[k] = PackedCols{ms.plan.pre ? reinterpret_cast<uint4*>(static_cast<char*>(sc.ws) + ms.packed[k]) : nullptr, packed_stride(m.M[k], NR)};
    }
    if (ms.plan.pre) {
        hipLaunchKernelGGL((pack_columns_multi_kernel<D, T, L>), dim3((maxM + 31 + kBlock) / kBlock, B, m.count), dim3(kBlock), 0, st, m);
        hipLaunchKernelGGL((softmin_fwd_x32_multi_kernel<D, T, NW, true, L>), ms.grid(m.count), dim3(NW * 64), 0, st, m, ms.sp);
    } else {
        hipLaunchKernelGGL((softmin_fwd_x32_multi_kernel<D, T, NW, false, L>), ms.grid(m.count), dim3(NW * 64), 0, st, m, ms.sp);
    }
    ms.template merge<SoftminFwdOp<D, 2, false, 1, T>>(m, st);
}

// the same for 4 <= D <= 16: the multi launch of the xd kernel (glhip_softmin_xd.h), columns packed on the fly, 4 wavefronts x 1 row tile
template <int D, typename T, int L>
void launch_iter4_xd(SoftminMulti<T>& m, int B, const Scratch& sc, hipStream_t st) {
    constexpr int NW = 4;
    for (int k = 0; k < m.count; ++k) m.pk[k] = PackedCols{nullptr, 0};
    MultiSplit<T> ms(m, B, NW * 32, sc, MULTI_XD);
    hipLaunchKernelGGL((xd_fwd_multi_kernel<D, T, NW, L>), ms.grid(m.count), dim3(NW * 64), 0, st, m, ms.sp);
    ms.template merge<SoftminFwdOp<D, 2, false, 1, T>>(m, st);
}

// p = 1 (round 5): the multi launch of the dense distance kernel (glhip_dist_xd.h), any D <= 16
template <int D, typename T>
void launch_iter4_dist(SoftminMulti<T>& m, int B, const Scratch& sc, hipStream_t st) {
    constexpr int NW = 8;
    DistMulti<T> dm;
    dm.count = m.count;
    for (int k = 0; k < 4; ++k) {
        dm.p[k] = dist_params(m.p[k]);
        dm.N[k] = m.N[k];
        dm.M[k] = m.M[k];
    }
    MultiSplit<T> ms(m, B, NW * 32, sc, MULTI_DIST);
    dm.ws_stride = m.ws_stride;
    hipLaunchKernelGGL((dist_xd_multi_kernel<D, T, NW>), ms.grid(m.count), dim3(NW * 64), 0, st, dm, ms.sp);
    ms.template merge<SoftminFwdOp<D, 1, true, 1, T>>(m, st);
}

// every problem of a SoftminMulti in one launch, on the kernel family of (p, D, layout)
template <typename T>
int multi_dispatch(SoftminMulti<T>& m, int B, int D, int p, const Scratch& sc, hipStream_t st) {
    if (m.count < 4) {      // unused slots: no rows
        for (int k = m.count; k < 4; ++k) { m.p[k] = m.p[0]; m.N[k] = 0; m.M[k] = m.M[0]; }
    }
    if (p == 1) {      // distances: one kernel for every D <= 16
#define GL_D(DD) launch_iter4_dist<DD, T>(m, B, sc, st)
        if (D <= 3) { GLHIP_D3_DISPATCH(D, GL_D) }
        else { GLHIP_XD_DISPATCH(D, GL_D) }
#undef GL_D
        return GLHIP_OK;
    }
    // GLHIP_FLAG_F16X2: the iteration on the f16 x 2 layout, like the half-steps it replaces; 4 <= D <= 16 on the xd kernel (round 5)
#define GL_D(DD) \
    if (sc.h2) launch_iter4<DD, T, XL_F16X2>(m, B, sc, st); \
    else launch_iter4<DD, T>(m, B, sc, st)
#define GL_XD(DD) \
    if (sc.h2) launch_iter4_xd<DD, T, XL_F16X2>(m, B, sc, st); \
    else launch_iter4_xd<DD, T, XL_BF16X3>(m, B, sc, st)
    if (D <= 3) { GLHIP_D3_DISPATCH(D, GL_D) }
    else { GLHIP_XD_DISPATCH(D, GL_XD) }
#undef GL_XD
#undef GL_D
    return GLHIP_OK;
}

template <typename T>
int iter4_typed(const void* x, const void* y, const float* a_log, const float* b_log, const float* f_ba, const float* g_ab,
                const float* f_aa, const float* g_bb, float* f_ba_out, float* g_ab_out, float* f_aa_out, float* g_bb_out,
                int B, int N, int M, int D, float eps, float damping, int p, int first, const Scratch& sc, hipStream_t st) {
    // first = 0: averaged update;  1: initial potentials (no pot, no prev);  2: plain extrapolation (pot, no prev)
    const float alpha = first ? damping : 0.5f * damping, beta = 0.5f;
    auto one = [&](const void* rows, const void* cols, const float* logw, const float* pot, const float* prev, float* out) {
        return make_softmin_params<T>(rows, cols, logw, out, eps, p, first == 1 ? nullptr : pot, first ? nullptr : prev, alpha, beta);
    };
    SoftminMulti<T> m;
    m.count = f_aa_out ? 4 : 2;
    m.p[0] = one(x, y, b_log, g_ab, f_ba, f_ba_out); m.N[0] = N; m.M[0] = M;
    m.p[1] = one(y, x, a_log, f_ba, g_ab, g_ab_out); m.N[1] = M; m.M[1] = N;
    if (m.count == 4) {
        m.p[2] = one(x, x, a_log, f_aa, f_aa, f_aa_out); m.N[2] = N; m.M[2] = N;
        m.p[3] = one(y, y, b_log, g_bb, g_bb, g_bb_out); m.N[3] = M; m.M[3] = M;
    }
    return multi_dispatch<T>(m, B, D, p, sc, st);
}

// The coarse-to-fine jump of the two-scale loop: every potential carried from the coarse measures to the fine points,
//     f_ba(x_i) = damping * softmin(eps, C(x_i, y_c), b_log_c + g_ab_c / eps)   and its three companions,
// as ONE launch of the same multi kernels (rows: fine clouds, columns: coarse clouds).
template <typename T>
int extrapolate4_typed(const void* x, const void* y, const void* xc, const void* yc, const float* a_log_c, const float* b_log_c,
                       const float* f_ba, const float* g_ab, const float* f_aa, const float* g_bb, float* f_ba_out, float* g_ab_out,
                       float* f_aa_out, float* g_bb_out, int B, int N, int M, int Nc, int Mc, int D, float eps, float damping, int p,
                       const Scratch& sc, hipStream_t st) {
    auto one = [&](const void* rows, const void* cols, const float* logw, const float* pot, float* out) {
        return make_softmin_params<T>(rows, cols, logw, out, eps, p, pot, nullptr, damping, 0.5f);
    };
    SoftminMulti<T> m;
    m.count = f_aa_out ? 4 : 2;
    m.p[0] = one(x, yc, b_log_c, g_ab, f_ba_out); m.N[0] = N; m.M[0] = Mc;
    m.p[1] = one(y, xc, a_log_c, f_ba, g_ab_out); m.N[1] = M; m.M[1] = Nc;
    if (m.count == 4) {
        m.p[2] = one(x, xc, a_log_c, f_aa, f_aa_out); m.N[2] = N; m.M[2] = Nc;
        m.p[3] = one(y, yc, b_log_c, g_bb, g_bb_out); m.N[3] = M; m.M[3] = Mc;
    }
    return multi_dispatch<T>(m, B, D, p, sc, st);
}

// D <= 3 on the VALU skeleton: p = 1, and p = 2 on explicit differences (GLHIP_FLAG_DIRECT) or in the expanded form (GLHIP_FLAG_NO_MFMA)
template <int D, bool BWD, typename T>
void launch_softmin_valu(const SoftminParams<T>& prm, const Ranges& rg, int n_ranges, int B, int N, int M, int p, int flags, const Scratch& sc,
                         hipStream_t st) {
    if (p == 1) launch_softmin_r<D, 1, true, BWD, T>(prm, rg, n_ranges, B, N, M, sc, st);
    else if (flags & GLHIP_FLAG_DIRECT) launch_softmin_r<D, 2, true, BWD, T>(prm, rg, n_ranges, B, N, M, sc, st);
    else launch_softmin_r<D, 2, false, BWD, T>(prm, rg, n_ranges, B, N, M, sc, st);
}

struct StepArgs {   // fused Sinkhorn half-step; all-default = plain soft-min
    const float* pot = nullptr;
    const float* prev = nullptr;
    float alpha = 1.f, beta = 0.f;
};

// The body of glhip_softmin_fwd / glhip_sinkhorn_step: a switch on softmin_fwd_family (glhip_family.h).  `fn`: the entry point, for messages.
template <typename T>
int softmin_fwd_typed(const char* fn, const void* x, const void* y, const float* h, float* out, int B, int N, int M, int D, float eps, int p,
                      const Ranges& rg, int n_ranges, const Scratch& sc, int flags, hipStream_t st, const StepArgs& step) {
    const SoftminParams<T> prm = make_softmin_params<T>(x, y, h, out, eps, p, step.pot, step.prev, step.alpha, step.beta);
    switch (softmin_fwd_family(B, N, M, D, p, flags, n_ranges)) {
    case GLHIP_FAMILY_VALU:
#define GL_D(DD) launch_softmin_valu<DD, false, T>(prm, rg, n_ranges, B, N, M, p, flags, sc, st)
        GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
        break;
    case GLHIP_FAMILY_X32:      // p = 2, D <= 3
#define GL_D(DD) launch_softmin_mfma<DD, T>(prm, rg, n_ranges, B, N, M, sc, st)
        GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
        break;
    case GLHIP_FAMILY_DIST: {   // p = 1: distances on the matrix cores
        const DistParams<T> dp = dist_params(prm);
        if (D <= 3) {           // block-sparse (use_mfma_dist)
#define GL_D(DD) launch_dist<DM_SOFTMIN_P1, DD, T, SoftminFwdOp<DD, 1, true, 1, T>>(dp, prm, rg, n_ranges, N, M, sc, st)
            GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
        } else if (D > kXdMaxD) {   // dense, 17 <= D <= 4095, GLHIP_FLAG_XK_DIST: K-chunked (glhip_dist_xk.h)
            launch_xk_dist<DM_SOFTMIN_P1, T, SoftminFwdOp<1, 1, true, 1, T>>(dp, prm, B, N, M, D, sc, st);
        } else {                    // dense, 4 <= D <= 16 (glhip_dist_xd.h)
#define GL_XD(DD) launch_dist_xd<DM_SOFTMIN_P1, DD, T, SoftminFwdOp<DD, 1, true, 1, T>>(dp, prm, B, N, M, sc, st)
            GLHIP_XD_DISPATCH(D, GL_XD)
#undef GL_XD
        }
        break;
    }
    case GLHIP_FAMILY_XD:       // p = 2 on the kernel of glhip_softmin_xd.h
        if (D <= 3) {
            // GLHIP_FLAG_F16X2, D <= 3: 3 D + 6 <= 15 K slots = ONE v_mfma_f32_32x32x16_f16 per 1024 exponents (bf16 x 3: two), 32 bytes
            // of LDS per column (64) — the kernel of glhip_softmin_xd.h instantiated for D <= 3
            // Big dense launches only (pre-packed columns, XCD-aware grid): that is where it was measured to win — 87.1 -> 79.2 ms at
            // 1e6 x 1e6, 36.8 -> 35.0 ms per online loss at 1e5; batches of 4096 x 4096 problems lose 4 % to the x32 kernel's staging
            // (B = 256: 16.2 -> 17.0 ms per loss), and block-sparse launches keep the gathered pre-packed tiles of glhip_softmin_x32.h.
            // (block-sparse launches through this kernel, packing their tiles on the fly in 512-row workgroups: 281 vs 244 ms per two-scale
            // loss at 1e6, round 6)
            // (mid-size launches, 16384 <= M < 65536, through this kernel with pre-packed columns and a free split count: 0.164 -> 0.191 ms
            // at N = M = 4e4, 0.242 -> 0.250 at 5e4, round 6: they stay on the x32 kernel)
            // GLHIP_FLAG_F32_MFMA / GLHIP_FLAG_XDL16 keep these launches on the x32 kernel too.
#define GL_D(DD) launch_xd_l<XD_SOFTMIN, DD, T, SoftminFwdOp<DD, 2, false, 1, T>, XL_F16X2>(prm, prm, rg, n_ranges, B, N, M, sc, st)
            GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
        } else {                // 4 <= D <= 16
#define GL_XD(DD) launch_xd<XD_SOFTMIN, DD, T, SoftminFwdOp<DD, 2, false, 1, T>>(prm, prm, rg, n_ranges, B, N, M, sc, st)
            GLHIP_XD_DISPATCH(D, GL_XD)
#undef GL_XD
        }
        break;
    case GLHIP_FAMILY_XK:       // p = 2, 17 <= D <= 4095: K-chunked (glhip_softmin_xk.h)
        launch_xk<XD_SOFTMIN, T, SoftminFwdOp<1, 2, false, 1, T>>(prm, prm, rg, n_ranges, B, N, M, D, sc, st);
        break;
    default: {                  // GLHIP_FAMILY_GENERIC: D > 3, a plain soft-min only
        if (step.pot || step.prev || step.alpha != 1.f)
            return fail(GLHIP_EUNSUPPORTED, "%s: no fused kernel for D=%d, p=%d, flags=%d (D > 3: the matrix-core kernels only — "
                                            "p = 2 up to D = 4095, dense p = 1 up to D = 16, and up to D = 4095 under GLHIP_FLAG_XK_DIST): use glhip_softmin_fwd", fn, D, p, flags);
        const GenericParams<T> gp{prm.x, prm.y, h, out, nullptr, nullptr, nullptr, (p == 1) ? prm.s2 : 0.5f * prm.s2, prm.out_scale, 1.f, 1e-8f};
        if (p == 2) launch_generic<GM_SOFTMIN_P2, false, T>(gp, rg, n_ranges, B, N, M, D, st);
        else launch_generic<GM_SOFTMIN_P1, false, T>(gp, rg, n_ranges, B, N, M, D, st);
    }
    }
    return GLHIP_OK;
}

// The body of glhip_softmin_bwd_x (out NULL) and glhip_softmin_fwd_grad (g NULL; `shift2`: how far, in units of LSE2, the guess `fwd` may lie
// below the value's upper bound): a switch on `fam` = softmin_bwd_family (glhip_family.h), which the entry point has evaluated — it keeps the
// arms of 17 <= D <= 4095 (GLHIP_FAMILY_XK, and _DIST beyond D = 16: glhip_grad_xk.h) and the refusal of mode 2 to itself.
template <typename T>
int softmin_bwd_typed(int fam, const void* x, const void* y, const float* h, float* out, const float* fwd, const float* g, float* gx, int B,
                      int N, int M, int D, float eps, int p, const Ranges& rg, int n_ranges, const Scratch& sc, int flags, hipStream_t st,
                      float shift2 = 0.f) {
    SoftminParams<T> prm = make_softmin_params<T>(x, y, h, out, eps, p, nullptr, nullptr, 1.f, 0.f);
    prm.fwd = fwd; prm.g = g; prm.gx = gx; prm.shift2 = shift2;
    switch (fam) {
    case GLHIP_FAMILY_VALU:
#define GL_D(DD) launch_softmin_valu<DD, true, T>(prm, rg, n_ranges, B, N, M, p, flags, sc, st)
        GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
        break;
    case GLHIP_FAMILY_X32: {    // p = 2, D <= 3: the 16x16x32 kernel only (x32 = false)
        const WsumParams<T> w = softmin_wsum_params(prm);
#define GL_D(DD) launch_wsum<WS_SOFTMIN_BWD, DD, T, SoftminBwdOp<DD, 2, false, 1, T>>(w, prm, rg, n_ranges, B, N, M, sc, false, st)
        GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
        break;
    }
    case GLHIP_FAMILY_XD: {     // p = 2, gradient (+ value), 4 <= D <= 16
        const WsumParams<T> w = softmin_wsum_params(prm);
#define GL_XD(DD) launch_wsum_t32<WS_SOFTMIN_BWD, DD, T, SoftminBwdOp<DD, 2, false, 1, T>>(w, prm, rg, n_ranges, B, N, M, sc, st)
        GLHIP_XD_DISPATCH(D, GL_XD)
#undef GL_XD
        break;
    }
    case GLHIP_FAMILY_DIST: {   // p = 1 gradient, dense, 4 <= D <= 16
        const DistXdGradParams<T> gp{dist_params(prm), fwd, g, gx, 1.f};
#define GL_XD(DD) launch_dist_xd_grad<DM_SOFTMIN_P1, DD, T, SoftminBwdOp<DD, 1, true, 1, T>>(gp, prm, B, N, M, sc, st)
        GLHIP_XD_DISPATCH(D, GL_XD)
#undef GL_XD
        break;
    }
    default: {                  // GLHIP_FAMILY_GENERIC
        const GenericParams<T> gp{prm.x, prm.y, h, out, fwd, g, gx, (p == 1) ? prm.s2 : 0.5f * prm.s2, prm.out_scale, 1.f, 1e-8f};
        if (p == 2) launch_generic<GM_SOFTMIN_P2, true, T>(gp, rg, n_ranges, B, N, M, D, st);
        else launch_generic<GM_SOFTMIN_P1, true, T>(gp, rg, n_ranges, B, N, M, D, st);
    }
    }
    return GLHIP_OK;
}

// ---- kernel products ---------------------------------------------------------------------------------

template <int KIND, int D, int BWD, typename T>   // BWD: ConvOp's MODE (0 product, 1 gradient, 2 both)
void launch_conv_r(const ConvParams<T>& prm, const Ranges& rg, int n_ranges, int B, int N, int M, const Scratch& sc,
                   hipStream_t st) {
    if (use_two_rows(B, N, n_ranges, sc))
        launch_mapreduce<ConvOp<KIND, D, 2, T, BWD>>(prm, rg, n_ranges, B, N, M, sc.ws, sc.bytes, sc.allow_split, st, sc.cb);
    else
        launch_mapreduce<ConvOp<KIND, D, 1, T, BWD>>(prm, rg, n_ranges, B, N, M, sc.ws, sc.bytes, sc.allow_split, st, sc.cb);
}

template <int KIND, int BWD, typename T>
void launch_conv_d(const ConvParams<T>& prm, const Ranges& rg, int n_ranges, int B, int N, int M, int D,
                   const Scratch& sc, hipStream_t st) {
#define GL_D(DD) launch_conv_r<KIND, DD, BWD, T>(prm, rg, n_ranges, B, N, M, sc, st)
    GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
}

template <int D, bool BWD, typename T>
void launch_gauss_mfma(const ConvParams<T>& prm, float blur, const Ranges& rg, int n_ranges, int B, int N, int M,
                       const Scratch& sc, bool x32, hipStream_t st) {
    const WsumParams<T> w = gauss_wsum_params(prm, blur);
    if constexpr (BWD) launch_wsum<WS_GAUSS_BWD, D, T, ConvOp<GLHIP_GAUSSIAN, D, 1, T, true>>(w, prm, rg, n_ranges, B, N, M, sc, x32, st);
    else launch_wsum<WS_GAUSS_FWD, D, T, ConvOp<GLHIP_GAUSSIAN, D, 1, T, false>>(w, prm, rg, n_ranges, B, N, M, sc, x32, st);
}

// gaussian product + its row gradient in one pass (WS_GAUSS_FWDGRAD; prm.g = NULL)
template <int D, typename T>
void launch_gauss_fwdgrad(const ConvParams<T>& prm, float blur, const Ranges& rg, int n_ranges, int B, int N, int M,
                          const Scratch& sc, hipStream_t st) {
    launch_wsum<WS_GAUSS_FWDGRAD, D, T, GaussFwdGradMerge<D, T>>(gauss_wsum_params(prm, blur), prm, rg, n_ranges, B, N, M, sc, false, st);
}

// the distance kernels' mode (glhip_dist_x32.h, glhip_dist_xd.h) of a laplacian / energy kernel
template <int KIND> constexpr int kConvDistMode = KIND == GLHIP_LAPLACIAN ? DM_LAPLACIAN : DM_ENERGY;

// laplacian / energy on the family conv_family chose, GLHIP_FAMILY_GENERIC aside
template <int KIND, int MODE, typename T>
void launch_conv_dist_kind(int fam, const ConvParams<T>& prm, const Ranges& rg, int n_ranges, int B, int N, int M, int D, const Scratch& sc,
                           int flags, hipStream_t st) {
    constexpr int DM = kConvDistMode<KIND>;
    const bool grad_family = (flags & GLHIP_FLAG_GRAD_FAMILY) != 0;      // products rounded like MODE 2: |.| = m rsq(m) (glhip_kconv_ops.h)
    if (fam == GLHIP_FAMILY_VALU) {
        if constexpr (MODE == 0) {
            if (grad_family) { launch_conv_d<KIND, 3, T>(prm, rg, n_ranges, B, N, M, D, sc, st); return; }
        }
        launch_conv_d<KIND, MODE, T>(prm, rg, n_ranges, B, N, M, D, sc, st);
    } else if (D <= 3) {      // GLHIP_FAMILY_DIST, block-sparse (use_mfma_dist)
        if constexpr (MODE == 0) {
            const DistParams<T> dp = dist_params(prm);
#define GL_DIST(DD) \
    if (grad_family) launch_dist<DM, DD, T, ConvOp<KIND, DD, 1, T, 0>, true>(dp, prm, rg, n_ranges, N, M, sc, st); \
    else launch_dist<DM, DD, T, ConvOp<KIND, DD, 1, T, 0>, false>(dp, prm, rg, n_ranges, N, M, sc, st)
            GLHIP_D3_DISPATCH(D, GL_DIST)
#undef GL_DIST
        } else {
            launch_dist_grad_d<KIND, MODE == 2 ? DG_FWDGRAD : DG_BWD, T>(prm, rg, n_ranges, N, M, D, sc, st);
        }
    } else if constexpr (MODE == 0) {      // GLHIP_FAMILY_DIST, dense: 4 <= D <= 16 (glhip_dist_xd.h), beyond K-chunked (glhip_dist_xk.h)
        const DistParams<T> dp = dist_params(prm);
        if (D > kXdMaxD) {
            launch_xk_dist<DM, T, ConvOp<KIND, 1, 1, T, 0>>(dp, prm, B, N, M, D, sc, st);
            return;
        }
#define GL_XD(DD) launch_dist_xd<DM, DD, T, ConvOp<KIND, DD, 1, T, 0>>(dp, prm, B, N, M, sc, st)
        GLHIP_XD_DISPATCH(D, GL_XD)
#undef GL_XD
    } else if constexpr (MODE == 1) {
        const DistXdGradParams<T> gp{dist_params(prm), nullptr, prm.g, prm.gx, prm.gscale};
#define GL_XD(DD) launch_dist_xd_grad<DM, DD, T, ConvOp<KIND, DD, 1, T, 1>>(gp, prm, B, N, M, sc, st)
        GLHIP_XD_DISPATCH(D, GL_XD)
#undef GL_XD
    }
}

// The body of the three kernel-product entry points: MODE 0 glhip_kernel_conv_fwd (g, gx NULL), 1 glhip_kernel_conv_bwd_x (out NULL),
// 2 glhip_kernel_conv_fwd_grad (g NULL).  A switch on `fam` = conv_family(kind, MODE, ...) (glhip_family.h), which the entry point has
// evaluated: modes 1 and 2 keep the arms of 17 <= D <= 4095 (GLHIP_FAMILY_XK, and _DIST beyond D = 16: glhip_grad_xk.h) to themselves.
// `if constexpr (MODE ...)` where a translation unit must not instantiate the other modes' kernels.
template <int MODE, typename T>
int conv_typed(int fam, int kind, const void* x, const void* y, const float* v, float* out, const float* g, float* gx,
               int B, int N, int M, int D, float blur, const Ranges& rg, int n_ranges, const Scratch& sc,
               int flags, hipStream_t st) {
    const ConvParams<T> prm = make_conv_params<T>(kind, x, y, v, out, g, gx, blur);
    if (fam == GLHIP_FAMILY_GENERIC) {
        if constexpr (MODE != 2) {      // unscaled coordinates: the scales sit on the distance, the clamp is the reference's own 1e-8
            GenericParams<T> gp{prm.x, prm.y, v, out, nullptr, g, gx, 1.f, 1.f, -1.0f, 1e-8f};      // energy
            if (kind == GLHIP_GAUSSIAN) {
                gp.dscale = 0.5f * kLog2e / (blur * blur);
                gp.gscale = -1.0f / (blur * blur);
                launch_generic<GM_GAUSS, MODE == 1, T>(gp, rg, n_ranges, B, N, M, D, st);
            } else if (kind == GLHIP_LAPLACIAN) {
                gp.dscale = kLog2e / blur;
                gp.gscale = -1.0f / blur;
                gp.clamp2 = 1e-8f * blur * blur;
                launch_generic<GM_LAPLACE, MODE == 1, T>(gp, rg, n_ranges, B, N, M, D, st);
            } else {
                launch_generic<GM_ENERGY, MODE == 1, T>(gp, rg, n_ranges, B, N, M, D, st);
            }
        }
    } else if (fam == GLHIP_EUNSUPPORTED) {      // MODE 2 only; the entry point has said so with a message
        return fam;
    } else if (kind == GLHIP_LAPLACIAN) {
        launch_conv_dist_kind<GLHIP_LAPLACIAN, MODE, T>(fam, prm, rg, n_ranges, B, N, M, D, sc, flags, st);
    } else if (kind == GLHIP_ENERGY) {
        launch_conv_dist_kind<GLHIP_ENERGY, MODE, T>(fam, prm, rg, n_ranges, B, N, M, D, sc, flags, st);
    } else if (fam == GLHIP_FAMILY_VALU) {      // gaussian from here on
        launch_conv_d<GLHIP_GAUSSIAN, MODE, T>(prm, rg, n_ranges, B, N, M, D, sc, st);
    } else if (fam == GLHIP_FAMILY_X32) {       // D <= 3 on the matrix cores
        if constexpr (MODE == 2) {
#define GL_D(DD) launch_gauss_fwdgrad<DD, T>(prm, blur, rg, n_ranges, B, N, M, sc, st)
            GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
        } else {
            const bool x32 = (flags & GLHIP_FLAG_XDL16) == 0;
#define GL_D(DD) launch_gauss_mfma<DD, MODE == 1, T>(prm, blur, rg, n_ranges, B, N, M, sc, x32, st)
            GLHIP_D3_DISPATCH(D, GL_D)
#undef GL_D
        }
    } else if constexpr (MODE == 0) {           // 4 <= D <= 16 (glhip_softmin_xd.h) and 17 <= D <= 4095 (K-chunked, glhip_softmin_xk.h)
        // the gaussian exponent -|x-y|^2 / (2 blur^2) is the soft-min's with eps = blur^2 and h = 0; `h` carries v; the merge takes prm
        const SoftminParams<T> sprm = make_softmin_params<T>(x, y, v, out, blur * blur, 2, nullptr, nullptr, 1.f, 0.f);
        if (fam == GLHIP_FAMILY_XK) {
            launch_xk<XD_GAUSS, T, ConvOp<GLHIP_GAUSSIAN, 1, 1, T, 0>>(sprm, prm, rg, n_ranges, B, N, M, D, sc, st);
        } else {
#define GL_XD(DD) launch_xd<XD_GAUSS, DD, T, ConvOp<GLHIP_GAUSSIAN, DD, 1, T, 0>>(sprm, prm, rg, n_ranges, B, N, M, sc, st)
            GLHIP_XD_DISPATCH(D, GL_XD)
#undef GL_XD
        }
    } else {                                    // 4 <= D <= 16: the transposed 32x32x16 kernel (glhip_wsum_t32.h)
#define GL_XD(DD) launch_gauss_grad_t32<DD, MODE == 2, T>(prm, blur, rg, n_ranges, B, N, M, sc, st)
        GLHIP_XD_DISPATCH(D, GL_XD)
#undef GL_XD
    }
    return GLHIP_OK;
}

}  // namespace
