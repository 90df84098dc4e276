// glhip_plan_apply_xk.h — the transport plan of a p = 2 soft-min applied to a feature matrix on the matrix cores, 17 <= D <= 4095:
//
//     out[i][v] = sum_j w_ij feat[j][v] / sum_j w_ij,      w_ij = 2^( u_ij + C_i ),  u_ij = H_j + s xt_i.yt_j,  C_i = r_i - fwd_i / out_scale
//
// glhip_plan_apply.h keeps the x-side operands of the whole exponent in registers and is templated on D <= 16.  Here D is a RUN-TIME
// argument and the kernel is the union of two that the tree already has:
//
//   exponent half = xk_fwd_kernel (glhip_softmin_xk.h), MODE soft-min: the 256 x 128 block of 8 wavefronts as 4 x 2, K stages of 6
//   MFMAs, points centred on the first row of the row block and split on the fly (xk_pack_half, xk_norms, glhip_klayout.h), padded
//   columns at -1e30 (f16 x 2: the floor), both layouts.  That kernel calls mfma(Y, X, acc): after the last stage lane (half, i) of a
//   wavefront holds, for each of its 2 x 2 blocks, row i for the 16 columns col(half, r) = 8 (r / 4) + 4 half + r % 4 —
//   the layout plan_apply_kernel feeds to its second product as the B operand.
//
//   plan half = the discipline of plan_apply_kernel (glhip_plan_apply.h), after the last K stage of a column tile, block by block:
//   C_i joins the exponents on the VALU, together with a per-column mask (0, or -inf for padded columns and columns with h = -inf:
//   they weigh exactly 0 in either layout, whatever the staging put in their H slot and whatever fwd_i is); weights relative to the
//   running maximum of their row times 2^kWqShift; the mass from the unsplit fp32 weights; weights in two f16 pieces; six
//   v_mfma_f32_32x32x16_f16 per chunk of 32 features against A operands staged in LDS (two f16 pieces under a power-of-two scale per
//   feature column and tile: plan_scale_exponent); a fresh accumulator per 32-column block, folded into the running sums with one
//   v_fma_f32 per register; a new row maximum rescales the running sums and the mass.  The largest weight of a row is 2^13 exactly:
//   a one-hot plan row returns its features bit for bit.
//
// Feature staging costs no barrier of its own: a tile's features are loaded and their maxima taken (ds_max_u32) between the first
// two barriers of the tile, scaled, split and written to LDS between the second and the third — the barriers xk_fwd_kernel has for
// the column indices and norms.  The two column halves of a workgroup (wc = 0, 1) carry separate (sums, mass, m) for the same rows
// and meet in LDS after the last tile ([feature][row] in the stage buffer), as (m, s) do in xk_fwd_kernel.  Column splits: the
// partial format of plan_apply_kernel — (sums[nv], mass, m) — and its plan_merge_kernel, unchanged.
//
// Chunks per pass: NCH = 1 or 2 chunks of 32 features, i.e. up to 64 features per pass (launch); wider feature matrices take
// further passes, a remainder is a pass of its own.  A wavefront carries 2 row tiles x NCH accumulators of 16 registers next to its
// 64 registers of exponents; four chunks would need 128 + 64 before any operand and 130 KiB for the meeting of the halves.
// One workgroup per CU: __launch_bounds__(512, 2).
//   registers / LDS / scratch (gfx950, tools/kernel_resources.py, profiles/xk_shared_stage.txt), float32 and bfloat16 clouds, plan and
//   gradient:
//     NCH = 1, both layouts:  199 VGPRs, 95.1 KiB of LDS (97 408 B), 0 bytes of scratch
//     NCH = 2, both layouts:  252-256 VGPRs, 111.5 KiB of LDS (114 176 B), 0 bytes of scratch
//     gaussian gradient (profiles/gauss_grad_xk.txt):  207 / 253-256 VGPRs, the same LDS, 0 bytes of scratch
//     LDS: 78.75 KiB of xk_fwd_kernel + 16 KiB of feature pieces per chunk + 384 B per chunk of maxima and inverse scales
//
// Cost model: per 32 x 32 block NM >= 7 MFMAs of exponent (NM = ceil((6 + kPer D) / 16)) + 6 NCH MFMAs of product + ~50 VALU
// instructions of exponentials and piece conversions shared by the chunks + 16 NCH v_fma_f32.  The staging of the exponent half
// (the splitting of 384 points per stage) is what a pass shares with a forward reduction, and it dominates both.
//
// The exponent half is xk_exponent_blocks (glhip_softmin_xk.h), the stage loop xk_fwd_kernel runs, without that kernel's sched_barrier
// between the two half groups of f16 x 2 (there for a 128-VGPR budget this kernel does not have).
//
// glhip_softmin_bwd_x of 17 <= D <= 4095 — g_i (x_i - sum_j P_ij y_j) is a plan application too — runs this kernel under
// GLHIP_FLAG_XK_GRAD, instantiated on XkGradParams (glhip_softmin_grad_xk.h): the centred column cloud as its features and the
// gradient's epilogue, chosen with `if constexpr` at four sites.  The two must stay ONE __global__ template: the same body as a
// __device__ __forceinline__ function behind two thin __global__ wrappers cost 30 VGPRs at NCH = 1 and spilled 112-180 bytes per lane
// at NCH = 2 (profiles/xk_shared_stage.txt).  Out of scope here: block-sparse plans, p = 1, float64 clouds and autograd through the
// application.
//
// glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad of the gaussian kernel, 17 <= D <= 4095, are the third instantiation, on
// XkGaussGradParams (glhip_gauss_grad_xk.h, sites marked GAUSS): the exponents of the gaussian product, features v_j (y_j - centre),
// the signed mass sum_j w_ij v_j (lds.xk.v carries v_j), and an epilogue that multiplies the sums by 2^m instead of normalising them.
//
// Pieces of the plan half shared with plan_apply_kernel and xk_dist_grad_kernel: plan_store_pieces, plan_rescale, plan_split_weights and
// plan_chunk_mfma (glhip_plan_apply.h), reg_column / reg_feature (glhip_klayout.h).  Pieces, never bodies: see above and
// profiles/xk_plan_pieces.txt for what stayed inline here (feature load, staging loop, fold, parking of the wc == 1 half) and why.
#pragma once

#include "glhip_plan_apply.h"
#include "glhip_softmin_xk.h"

namespace glhip {

constexpr int kXkPlanMaxChunks = 2;                      // feature chunks per pass

template <typename T> struct XkGaussGradParams;          // glhip_gauss_grad_xk.h

// GAUSS: one entry of the gradient from sums relative to 2^m (e2m = 2^m, gs = g_i / blur^2).  A row that no column reached (e2m == 0)
// writes 0.  The signed mass w can be 0 where s is not: it is never a test for an empty row.
__device__ __forceinline__ float xk_gauss_grad_entry(float s, float w, float xc, float e2m, float gs) {
    return (e2m > 0.f) ? gs * (e2m * __builtin_fmaf(-xc, w, s)) : 0.f;
}

template <int NCH>
struct XkPlanLds {
    XkLds xk;                                            // the exponent half (xk.v: the column mask, 0 or -inf)
    uint4 q[(kXkCols / 32) * NCH * 4 * 64];              // feature A operands: [group][chunk][piece][instruction][lane = 32 h + c] x 8 f16
    uint32_t fmax[2][32 * NCH];                          // largest |f| bit pattern per feature, tiles of even / odd index
    __attribute__((aligned(16))) float inv[32 * NCH];    // 2^-13 / scale of the current tile, per feature
    uint32_t live[4];                                    // the current tile's columns with mass (h_j > -inf), one bit each: plan_live_features
};

// P = PlanParams<T>: the plan applied to prm.feat.  P = XkGradParams<T> (glhip_softmin_grad_xk.h): the gradient with respect to the row
// points — the same body at four sites marked GRAD: the feature load, the output row, the unsplit epilogue and the mass output.
// P = XkGaussGradParams<T> (glhip_gauss_grad_xk.h): the gradient of the gaussian product — GRAD's feature load and output row, and its own
// arms marked GAUSS: C_i and H_j without dual or forward value, v_j in lds.xk.v, the signed mass and the unnormalised epilogue.
template <typename T, int NCH, int L, typename P>
__global__ void __launch_bounds__(kXkThreads, 2)
xk_plan_kernel(P prm, int N, int M, int D, SplitInfo sp) {
    constexpr bool GRAD = !std::is_same<P, PlanParams<T>>::value;
    constexpr bool GAUSS = std::is_same<P, XkGaussGradParams<T>>::value;
    constexpr bool H2 = (L == XL_F16X2);
    constexpr int VC = 32 * NCH;
    constexpr int kQRecs = NCH * 4 * 64;                      // feature records per column group
    constexpr int kFItems = (kXkCols / 4) * VC / kXkThreads;  // (column quad, feature) items per thread and tile: 2, 4
    static_assert(NCH == 1 || NCH == 2, "1 or 2 chunks of 32 features per pass");
    static_assert(kFItems * kXkThreads == (kXkCols / 4) * VC, "whole items per thread");
    static_assert((VC + 2) * kXkRows * sizeof(float) <= sizeof(XkLds::buf), "the column halves meet in the stage buffer");
    __shared__ XkPlanLds<NCH> lds;

    int bx, b, split;
    workgroup_coords(sp, bx, b, split);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / kXkWC, wc = wave % kXkWC;
    const int half = lane >> 5, l31 = lane & 31;
    const int ns = sp.n_splits;
    const int NM = xk_num_mfma(D, L), NG = xk_num_groups(D, L);
    const float xscale = H2 ? __builtin_sqrtf(prm.s2) : prm.s2;
    const float yscale = H2 ? __builtin_sqrtf(prm.s2) : 1.0f;
    const T* xb = prm.x + (long)b * N * D;
    const T* yb = prm.y + (long)b * M * D;
    const Ranges none{nullptr, nullptr, nullptr, nullptr};

    int row_begin, row_end, q_begin, q_end;
    block_extent<false>(none, N, kXkRows, row_begin, row_end, q_begin, q_end, bx);
    if (row_begin >= row_end) return;
    const int row0 = row_begin;
    const T* centre = xb + (long)row0 * D;
    const int nrows = row_end - row0;
    const int nr32 = (nrows + 31) & ~31;                      // row slots that are packed

    if (tid < 2 * VC) lds.fmax[tid / VC][tid % VC] = 0u;
    if (tid < kXkRows) lds.xk.idx[tid] = min(row0 + tid, row_end - 1);
    __syncthreads();
    xk_norms<T>(xb, centre, D, lds.xk.idx, 0, kXkRows, lds.xk.n2row, tid);
    __syncthreads();
    if (tid < kXkRows) lds.xk.scal[tid] = 0.f;                // soft-min: the x-side scalar is 0, r_i joins with C_i

    const int wave_row0 = row0 + wr * (kXkRT * 32);
    const bool wave_rows = wave_row0 < row_end;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 pacc[kXkRT][NCH];                                  // running sums, relative to 2^m
    float mass4[kXkRT][4], m[kXkRT], cst[kXkRT];
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) pacc[rt][ch] = zero16;
#pragma unroll
        for (int k = 0; k < 4; ++k) mass4[rt][k] = 0.f;
        m[rt] = kMinusHuge;      // running maximum of the row's exponents (both lane halves of a row hold the same value)
        // C_i = r_i - LSE2_i, r_i = -s/2 |xt_i|^2, LSE2_i = fwd_i / out_scale.  fwd_i = +inf is a row without mass; a huge fwd_i (the
        // forward counted its padded columns into such a row) must stay finite here: it meets the -inf of the column mask
        const int i = min(wave_row0 + rt * 32 + l31, row_end - 1);
        if constexpr (GAUSS) {                                // C_i = r_i: the exponents of the gaussian product
            cst[rt] = -0.5f * prm.s2 * lds.xk.n2row[i - row0];
        } else {
            const float fw = prm.fwd[(long)b * N + i];
            const float c = -0.5f * prm.s2 * lds.xk.n2row[i - row0] - fw / prm.out_scale;
            cst[rt] = (fw == __builtin_inff()) ? kNegBig : __builtin_fminf(c, -kNegBig);
        }
    }

    int js, je;
    column_interval<false>(none, M, 0, split, ns, js, je);
    int parity = 0;
    for (int j0 = js; j0 < je; j0 += kXkCols, parity ^= 1) {
        const int n = min(kXkCols, je - j0);                  // real columns, in the slots kXkRows .. kXkRows + n - 1
        const int ncg = (n + 31) >> 5;                        // column groups that are packed and multiplied
        const int col = (tid < n) ? j0 + tid : -1;            // this thread's column (tid < kXkCols), -1 = padding
        if constexpr (!GRAD && !GAUSS) {   // which of the tile's columns carry mass (h_j > -inf): read by the feature staging between the next two barriers
            const float hcol = (col >= 0) ? prm.h[(long)b * M + col] : -__builtin_inff();
            const unsigned long long live = __ballot(hcol != -__builtin_inff());
            if (lane == 0 && wave < 2) {
                lds.live[2 * wave] = (uint32_t)live;
                lds.live[2 * wave + 1] = (uint32_t)(live >> 32);
            }
        }
        __syncthreads();                                      // the previous tile (and the row scalars) are settled
        if (tid < kXkCols) lds.xk.idx[kXkRows + tid] = col;
        // features: item (column quad cq, feature c of the pass) — c runs fastest, so the loads of a wavefront are contiguous runs of
        // feat rows (plan_apply_kernel).  GRAD: the centred coordinates v0 .. v0 + nv - 1 of the tile's columns, runs of y rows
        float fv[kFItems][4];
        bool voids = false;                                   // (nearly every tile: all n columns carry mass)
        if constexpr (!GRAD && !GAUSS) voids = __popc(lds.live[0]) + __popc(lds.live[1]) + __popc(lds.live[2]) + __popc(lds.live[3]) != n;
#pragma unroll
        for (int k = 0; k < kFItems; ++k) {
            const int it = tid + k * kXkThreads;
            const int cq = it / VC, c = it - cq * VC;
            const int t = cq << 2;
            float cen = 0.f;
            if constexpr (GRAD) cen = (c < prm.nv) ? to_f32<T>(centre[prm.v0 + c]) : 0.f;
            uint32_t mx = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float f = 0.f;
                if (t + q < n && c < prm.nv) {
                    if constexpr (GRAD) f = to_f32<T>(yb[(long)(j0 + t + q) * D + prm.v0 + c]) - cen;
                    else f = prm.feat[((long)b * M + j0 + t + q) * prm.V + prm.v0 + c];
                    if constexpr (GAUSS) f *= prm.v[(long)b * M + j0 + t + q];      // v_j (y_j - centre)
                }
                fv[k][q] = f;
            }
            if (voids) plan_live_features(fv[k], lds.live, t);
#pragma unroll
            for (int q = 0; q < 4; ++q) mx = max(mx, __float_as_uint(fv[k][q]) & 0x7FFFFFFFu);
            if (mx) atomicMax(&lds.fmax[parity][c], mx);
        }
        __syncthreads();                                      // the tile's indices and feature maxima are complete
        xk_norms<T>(yb, centre, D, lds.xk.idx, kXkRows, ncg * 32, &lds.xk.scal[kXkRows], tid);
        if (tid < VC) {
            const uint32_t se = plan_scale_exponent(lds.fmax[parity][tid]);
            lds.inv[tid] = __uint_as_float((254u - (uint32_t)kWqShift - se) << 23);
            lds.fmax[parity ^ 1][tid] = 0u;      // for the next tile: last read before the first barrier of this one
        }
        // columns 4 cq .. 4 cq + 3 of a group are K slots s0 .. s0 + 3 of one lane half and one instruction
#pragma unroll
        for (int k = 0; k < kFItems; ++k) {
            const int it = tid + k * kXkThreads;
            const int cq = it / VC, c = it - cq * VC;
            const int t = cq << 2;
            if (t < ncg * 32) {
                const float sc = __uint_as_float(plan_scale_exponent(lds.fmax[parity][c]) << 23);
                const int jj = t & 31;
                const int r = (jj >> 3) << 2, hq = (jj >> 2) & 1;
                uint2* qb = reinterpret_cast<uint2*>(&lds.q[(t >> 5) * kQRecs + (c >> 5) * (4 * 64) + (r >> 3) * 64 + hq * 32 + (c & 31)]) + ((r & 7) >> 2);
                plan_store_pieces(fv[k], sc, qb);
            }
        }
        __syncthreads();
        if (tid < ncg * 32) {                                 // |yt|^2 -> H_j, and the column's mask
            float H = kNegBig, mask = -__builtin_inff();
            if constexpr (GAUSS) {                            // lds.xk.v: v_j, 0 for a padded column (its features are 0 too)
                mask = 0.f;
                if (col >= 0) {
                    H = -0.5f * prm.s2 * lds.xk.scal[kXkRows + tid];
                    mask = prm.v[(long)b * M + col];
                }
            } else if (col >= 0) {
                const float hj = prm.h[(long)b * M + col];
                H = __builtin_fmaf(-0.5f * prm.s2, lds.xk.scal[kXkRows + tid], hj * kLog2e);
                if (hj != -__builtin_inff()) mask = 0.f;
            }
            if (H2) H = __builtin_fmaxf(H, kH2Floor);
            lds.xk.scal[kXkRows + tid] = H;
            lds.xk.v[tid] = mask;
        }

        const bool wave_on = wave_rows && wc * kXkCG < ncg;
        f32x16 acc[kXkRT][kXkCG];
        xk_exponent_blocks<T, L, false>(lds.xk, xb, yb, centre, D, NM, NG, nr32, ncg, xscale, yscale, wave_on, wr, wc, half, l31, tid, acc);
        if (!wave_on) continue;

        // ---- plan half: the weights of this wavefront's 2 x 2 blocks times the tile's features (column groups >= ncg were not packed) ----
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) {
#pragma unroll
            for (int cg = 0; cg < kXkCG; ++cg) {
                const int G = wc * kXkCG + cg;
                if (G >= ncg) continue;
                // register r <-> column reg_column(r, half) of the group: four broadcast 16-byte reads of the mask
                f32x16 u;
                const float* mk = &lds.xk.v[G * 32 + half * 4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if constexpr (GAUSS) {                    // no mask: the running maximum is taken over the exponents, never over v
#pragma unroll
                        for (int k = 0; k < 4; ++k) u[4 * q + k] = acc[rt][cg][4 * q + k] + cst[rt];
                    } else {
                        const float4 k4 = *reinterpret_cast<const float4*>(mk + q * 8);
                        u[4 * q + 0] = (acc[rt][cg][4 * q + 0] + cst[rt]) + k4.x;
                        u[4 * q + 1] = (acc[rt][cg][4 * q + 1] + cst[rt]) + k4.y;
                        u[4 * q + 2] = (acc[rt][cg][4 * q + 2] + cst[rt]) + k4.z;
                        u[4 * q + 3] = (acc[rt][cg][4 * q + 3] + cst[rt]) + k4.w;
                    }
                }
                // weights relative to the running maximum of the row: w' = 2^13 2^(u - m) <= 8192 whatever fwd is worth, and the largest
                // weight of a row is 2^13 EXACTLY.  A new maximum rescales the running sums (factor exactly 1 for the rows that keep theirs)
                float bm = max16(u);
                bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
                plan_rescale(bm, m[rt], pacc[rt], mass4[rt]);
                Pack16h whi[2], wlo[2];
#pragma unroll
                for (int k = 0; k < 16; k += 2) {
                    const f32x2_t w = {fast_exp2(u[k] - m[rt]) * (float)(1 << kWqShift), fast_exp2(u[k + 1] - m[rt]) * (float)(1 << kWqShift)};
                    if constexpr (GAUSS) {                    // the signed mass: the unsplit fp32 weights times v_j
                        const float2 v2 = *reinterpret_cast<const float2*>(mk + reg_column(k, 0));      // (mk carries the lane half)
                        mass4[rt][k & 3] = __builtin_fmaf(w[0], v2.x, mass4[rt][k & 3]);
                        mass4[rt][(k & 3) + 1] = __builtin_fmaf(w[1], v2.y, mass4[rt][(k & 3) + 1]);
                    } else {
                        mass4[rt][k & 3] += w[0];
                        mass4[rt][(k & 3) + 1] += w[1];
                    }
                    plan_split_weights(w, k, whi, wlo);
                }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const f32x16 t = plan_chunk_mfma(&lds.q[G * kQRecs + ch * (4 * 64) + lane], whi, wlo);
                    // register r <-> feature reg_feature(r, half) of the chunk: four broadcast 16-byte reads of the inverse scales
                    const float* ig = &lds.inv[ch * 32 + half * 4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 i4 = *reinterpret_cast<const float4*>(ig + q * 8);
                        pacc[rt][ch][4 * q + 0] = __builtin_fmaf(t[4 * q + 0], i4.x, pacc[rt][ch][4 * q + 0]);
                        pacc[rt][ch][4 * q + 1] = __builtin_fmaf(t[4 * q + 1], i4.y, pacc[rt][ch][4 * q + 1]);
                        pacc[rt][ch][4 * q + 2] = __builtin_fmaf(t[4 * q + 2], i4.z, pacc[rt][ch][4 * q + 2]);
                        pacc[rt][ch][4 * q + 3] = __builtin_fmaf(t[4 * q + 3], i4.w, pacc[rt][ch][4 * q + 3]);
                    }
                }
            }
        }
    }

    // ---- the two column halves of the workgroup meet in LDS (the stage buffer is free now): [feature | mass | m][row] ----
    __syncthreads();
    float* mrg = reinterpret_cast<float*>(lds.xk.buf);
    float mass[kXkRT];
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
        float s = (mass4[rt][0] + mass4[rt][1]) + (mass4[rt][2] + mass4[rt][3]);
        s += __shfl_xor(s, 32, 64);                          // the two 16-column halves
        mass[rt] = s * (1.0f / (float)(1 << kWqShift));      // relative to 2^m
        if (wc == 1) {
            const int r_local = wr * (kXkRT * 32) + rt * 32 + l31;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mrg[(32 * ch + reg_feature(r, half)) * kXkRows + r_local] = pacc[rt][ch][r];
            }
            if (half == 0) {
                mrg[VC * kXkRows + r_local] = mass[rt];
                mrg[(VC + 1) * kXkRows + r_local] = m[rt];
            }
        }
    }
    __syncthreads();
    if (wc != 0 || !wave_rows) return;
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
        const int r_local = wr * (kXkRT * 32) + rt * 32 + l31;
        const int i = row0 + r_local;
        if (i >= row_end) continue;
        // the halves are brought to the larger m (factor exactly 1 for the half that holds it, 0 for a half without mass)
        const float m2 = mrg[(VC + 1) * kXkRows + r_local];
        const float mn = fmaxf(m[rt], m2);
        const float rs1 = fast_exp2(m[rt] - mn), rs2 = fast_exp2(m2 - mn);
        const float w = __builtin_fmaf(mrg[VC * kXkRows + r_local], rs2, mass[rt] * rs1);
        const long idx = (long)b * N + i;
        float* orow;
        float gi = 0.f;                                       // GRAD: the incoming gradient of the row
        float e2m = 0.f;                                      // GAUSS: 2^m, and gi = g_i / blur^2
        if constexpr (GAUSS) {
            orow = prm.gx + idx * D + prm.v0;
            if (ns == 1) {
                gi = prm.g ? prm.g[idx] * prm.gscale : prm.gscale;
                e2m = fast_exp2(mn);
            }
        } else if constexpr (GRAD) {
            orow = prm.gx + idx * D + prm.v0;
            if (ns == 1) gi = prm.g[idx];
        } else {
            orow = prm.out + idx * prm.V + prm.v0;
        }
        float* part = sp.workspace + split * sp.split_stride + idx * (prm.nv + 2);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * ch + reg_feature(r, half);
                if (c < prm.nv) {
                    const float s = __builtin_fmaf(mrg[c * kXkRows + r_local], rs2, pacc[rt][ch][r] * rs1);
                    if (ns > 1) {
                        part[c] = s;
                    } else if constexpr (GAUSS) {     // nothing is normalised: g_i / blur^2 2^m (S - xc W); a row no column reached gets 0
                        const float xc = to_f32<T>(xb[(long)i * D + prm.v0 + c]) - to_f32<T>(centre[prm.v0 + c]);
                        orow[c] = xk_gauss_grad_entry(s, w, xc, e2m, gi);
                    } else if constexpr (GRAD) {      // g_i ((x_i - centre) - ybar_i); a row without mass gets 0
                        const float xc = to_f32<T>(xb[(long)i * D + prm.v0 + c]) - to_f32<T>(centre[prm.v0 + c]);
                        orow[c] = (w > 0.f) ? gi * (xc - s / w) : 0.f;
                    } else {
                        orow[c] = (w > 0.f) ? s / w : 0.f;      // a division: exact where the quotient is
                    }
                }
            }
        }
        if (half == 0) {
            if (ns > 1) {
                part[prm.nv] = w;
                part[prm.nv + 1] = mn;
            } else if constexpr (GAUSS) {
                if (prm.out && prm.v0 == 0) prm.out[idx] = (e2m > 0.f) ? w * e2m : 0.f;
            } else if constexpr (!GRAD) {
                if (prm.mass && prm.v0 == 0) prm.mass[idx] = w * fast_exp2(mn);
            }
        }
    }
}

}  // namespace glhip
