// glhip_dist_xkp.h — the p = 1 Sinkhorn iteration on PRE-PACKED operands for clouds of dimension 17 <= D <= 4095: the DISTANCE epilogue of
// xkp_fwd_multi_kernel (glhip_softmin_xkp.h), opted into with GLHIP_FLAG_XK_ITER_DIST.  float32 / bfloat16 clouds, batched or not.
//
// What is shared.  The records xkp_pack_kernel writes are temperature-free centred points and serve a distance as well as a dot product:
//     d2_ij = n_i + N_j - 2 <xt_i, yt_j>,      n_i = |xt_i|^2,  N_j = |yt_j|^2  (stored once per point by the pack kernel),
// so the pack stage, the workspace layout (XkpLayout), the grid, the 128 x 128 tile, the LDS-DMA stage loop and the meeting of the column
// halves are those of the p = 2 kernel: ONE body, xkp_fwd_multi_kernel<T, P>, with two epilogues chosen by `if constexpr`.  The P = 2
// instantiation's compiler report did not move with the change (126 VGPRs, 0 scratch, 52224 bytes of LDS, 3 waves per SIMD).
//
// What is new, all in this header.
//   columns  : at a tile's first stage 128 threads write S_j = log2(e) (logw_j + pot_j / eps) and N_j to LDS (padding: S_j = kNegBig,
//              N_j = 0) — xkp_dist_columns; 1 KiB more LDS than P = 2 (two tiles in flight), 53248 bytes: still three workgroups per CU.
//   rows     : n_i of a lane's two rows, two VGPRs loaded once per workgroup; rows past the cloud carry the threshold -inf, so that
//              whatever their accumulators hold (a row group past the cloud is not staged) never reaches the repair.
//   epilogue : xkp_dist_exponents, per row tile after the last stage of a column tile:
//                d2 = fma(-2, acc, n_i + N_j);  near pairs patched (below);  dist = v_sqrt_f32(v_med3(d2, 1e-8, 3e38))  (utils.py:61);
//                u = fma(-s, dist, S_j),  s = log2(e) / eps.
//              The accumulators then hold exponents and join the lazy explicit running maximum and sum exactly as for P = 2.  Distances
//              are in the caller's units — the temperature enters with the one FMA, so one pack serves every temperature of an anneal.
//   tail     : no row constant (r_i = 0); finish_value or the (max, sum) partial of SoftminFwdOp<1, 1, true, 1, T>.
//
// Near pairs.  The rule of glhip_dist_xk.h: a pair with d2 < max(guard n_i, 4 clamp2) (guard = 2^-8, GLHIP_DIST_GUARD) is re-evaluated
// on explicit differences of the caller's own points (xk_dist_exact_d2, a run-time loop over D from global memory through the problem's
// row and column pointers, t = 1), clamped from below.  xkp_dist_patch_near is xk_dist_patch_near with the column index computed
// (tile origin + reg_column) instead of read from an index array: that array would be a third KiB of LDS per tile in flight and push the
// kernel to two workgroups per CU.  Columns past the split's end are never re-evaluated.
//
// Why the rule still bounds the error with ONE centre per batch item (x[b, 0, :]) instead of the row block's first row.  The rule never
// uses where the centre is, only n_i: the expanded form errs by about eps32 (n_i + N_j) (float32 accumulation; the dropped bf16 products
// are smaller), and by the triangle inequality sqrt(N_j) <= sqrt(n_i) + sqrt(d2).  For a pair that is NOT re-evaluated, d2 >= n_i / 256:
// either N_j <= 4 n_i, then n_i + N_j <= 5 n_i <= 1280 d2, or N_j > 4 n_i, then d2 >= (sqrt(N_j) - sqrt(n_i))^2 >= N_j / 4 and
// n_i + N_j <= 5 d2.  The relative error of d2 is below 1280 eps32 either way, that of the distance half of it — the bound of
// xk_dist_kernel, for any centre.  What the centre does change is the size of n_i: both clouds are at most one diameter of their union
// from x[b, 0, :] (the assumption of the p = 2 error bound, glhip_softmin_xk.h), where a block's first row gives the same scale; the
// rule is not widened to max(n_i, N_j).  The row x[b, 0, :] itself has zero records: acc = 0 and d2 = N_j, exact like a near pair.
// The x-x and y-y problems have a near pair on every diagonal: one exact evaluation per row (each lane patches its own pairs, a wavefront
// waits for its slowest lane: one pair on a diagonal block).
//
// Resources as the compiler reports them (the translation unit prints them with every build): DESIGN.md §4.
#pragma once

#include "glhip_dist_xk.h"

namespace glhip {

constexpr float kXkpDistClamp2 = 1e-8f;      // the floor of utils.py:61 on the unscaled squared distance

// S_j and N_j of one column of a tile (thread `c` of the tile's first 128; `on`: the column exists)
template <typename T>
__device__ __forceinline__ void xkp_dist_columns(const SoftminParams<T>& prm, const float* __restrict__ cn2, long col, bool on, float* S,
                                                 float* Nj) {
    *S = on ? dual_entry(prm, col) * kLog2e : kNegBig;
    *Nj = on ? cn2[col] : 0.f;
}

// xk_dist_patch_near for a group whose columns are col0 .. col0 + 31 of the cloud, those >= col_end being padding
template <typename T>
__device__ __forceinline__ void xkp_dist_patch_near(f32x16& d2, uint32_t near, const T* xi, const T* yb, int col0, int col_end, int half,
                                                    int D) {
    while (near != 0u) {
        const int k = __builtin_ctz(near);
        near &= near - 1u;
        const int j = col0 + reg_column(k, half);
        if (j < col_end) {
            const float e = fmaxf(xk_dist_exact_d2<T>(xi, yb + (long)j * D, D, 1.f), kXkpDistClamp2);
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) d2[kk] = (kk == k) ? e : d2[kk];
        }
    }
}

// The accumulators of one row tile (dot products of the centred points against the wavefront's two column groups) become exponents.
//   Sv / Nv : the tile's S_j / N_j in LDS, at the wavefront's first column;   ni : n_i of this lane's row, thr : its near-pair threshold
//   (-inf for a row past the cloud);   xb / yb : the problem's rows / columns of this batch item;   rbase : first row of the tile,
//   clamped to N - 1 per lane;   col0 : cloud index of the wavefront's first column, col_end : end of the split's columns
template <typename T>
__device__ __forceinline__ void xkp_dist_exponents(f32x16 (&acc)[2], const float* Sv, const float* Nv, float ni, float thr, float s2, bool cg1,
                                                   const T* xb, const T* yb, int rbase, int N, int col0, int col_end, int half, int D) {
#pragma unroll
    for (int cg = 0; cg < 2; ++cg) {
        if (cg == 1 && !cg1) continue;      // (the wavefront's second column group may lie past the tile: never staged)
        f32x16& d2 = acc[cg];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const float4 v = *reinterpret_cast<const float4*>(&Nv[cg * 32 + g4 * 8 + half * 4]);
            d2[4 * g4] = __builtin_fmaf(-2.f, d2[4 * g4], ni + v.x);
            d2[4 * g4 + 1] = __builtin_fmaf(-2.f, d2[4 * g4 + 1], ni + v.y);
            d2[4 * g4 + 2] = __builtin_fmaf(-2.f, d2[4 * g4 + 2], ni + v.z);
            d2[4 * g4 + 3] = __builtin_fmaf(-2.f, d2[4 * g4 + 3], ni + v.w);
        }
        if (__any(min16(d2) < thr)) {
            uint32_t near = 0u;
#pragma unroll
            for (int k = 15; k >= 0; --k) near = (near << 1) | (d2[k] < thr ? 1u : 0u);
            // the lane, re-derived on this rare path (as xk_dist_kernel: nothing is kept in registers for it across the stage loop)
            int ln;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
            const T* xi = xb + (long)min(rbase + (ln & 31), N - 1) * D;
            xkp_dist_patch_near<T>(d2, near, xi, yb, col0 + cg * 32, col_end, ln >> 5, D);
        }
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const float4 v = *reinterpret_cast<const float4*>(&Sv[cg * 32 + g4 * 8 + half * 4]);
            const float sv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dist = fast_sqrt(__builtin_amdgcn_fmed3f(d2[4 * g4 + r], kXkpDistClamp2, 3.0e38f));
                d2[4 * g4 + r] = __builtin_fmaf(-s2, dist, sv[r]);
            }
        }
    }
}

}  // namespace glhip
