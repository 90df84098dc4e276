// glhip_dist_grad_xk.h — the row gradients of the DISTANCE reductions (p = 1 soft-min, laplacian and energy kernel products) on the matrix
// cores, 17 <= D <= 4095, float32 / bfloat16 clouds, dense and batched launches (GLHIP_FLAG_XK_DIST_GRAD):
//
//     grad_x[i] = g_i gscale ( xs_i W_i - S_i ) / Z_i,     W_i = sum_j w_ij,   S_i = sum_j w_ij ys_j,   xs = t (x - c),  ys = t (y - c)
//     soft-min p = 1 : w_ij = e_ij / dist_ij,  e_ij = 2^(S_j - dist_ij),  Z_i = sum_j e_ij (this launch: self-normalising),  gscale = 1
//     laplacian      : w_ij = v_j 2^(-dist_ij) / dist_ij,  Z = 1,  gscale = -1 / blur        energy : w_ij = v_j / dist_ij,  Z = 1,  gscale = -1
// with dist_ij = sqrt(max(d2_ij, clamp2)), t the coordinate scale of DistParams and c the first row of the 256-row block.  A new
// __global__ template that joins two halves the tree already has:
//
//   exponent half = xk_dist_kernel (glhip_dist_xk.h): d2 from the chain with xscale = -2 t, yscale = t, n_i, N_j (xk_exponent_blocks,
//   xk_norms, bf16 x 3 only); pairs below thr = max(guard n_i, 4 clamp2) re-evaluated on explicit differences from global memory.
//
//   plan half = the discipline of xk_plan_kernel (glhip_plan_apply_xk.h): features (y_j - c) of the coordinates v0 .. v0 + nv - 1, times
//   v_j for the products (XkGaussGradParams: the weights stay positive), in two f16 pieces under a per-column power-of-two scale
//   (XkPlanLds, plan_scale_exponent); weights in two f16 pieces times 2^kWqShift; six v_mfma_f32_32x32x16_f16 per chunk into a fresh
//   accumulator per 32-column block; W, the scalar (Z, or the product for glhip_kernel_conv_fwd_grad) and the running maximum from the
//   unsplit fp32 weights on the VALU.  The coordinate scale t joins in the epilogue: the sums are linear in it.
//
// Weight range: 1 / dist is unbounded above, so the lazy running row maximum m is taken over u~ = u - 0.5 log2(d2) (u = S_j - dist,
// -dist or 0), not over u: w' = 2^13 2^(u~ - m) <= 2^13 as in xk_plan_kernel.  Pairs inside the clamp (d2 <= clamp2) get no direction —
// what sqrt(clamp_min(., 1e-8)) gives under autograd (glhip_dist_grad_x32.h) — and enter the maximum with u~ = u: they still count in Z
// and in the product, with 2^(u - m) <= 1.  Columns that weigh nothing (padding, h = -inf, v = 0) enter it with -inf.
//
// Near pairs (below thr: the set the forward repairs) must not enter xs_i W - S: that difference would lose |ys_j| / dist_ij in relative
// accuracy.  They get weight 0 in the f16 pieces and in W; their exact contribution w_ij (x_i - y_j)[c] joins the running sums on the
// VALU.  No atomics and no order that depends on timing: lane (half, row) holds its row's sums for 16 of the 32 features of a chunk;
// the two lanes of a row exchange their 16-bit near masks (__shfl_xor 32), both walk the same pairs — first those of half 0, then of
// half 1, each in ascending register order —, each recomputes d2 on explicit differences and adds the direction to its own 16 NCH
// features in an unrolled loop.  Rare and divergent, like the `while (near)` loop of the forward.
//
// Epilogue: T_c = (x_i - c)[c] W - S_c is formed before anything is written; the two column halves of the workgroup meet in LDS on
// (T[nv], scalar, m); a column split writes the same nv + 2 floats, plan_merge_kernel (glhip_plan_apply.h) is reused unchanged and
// plan_merge_store below applies the epilogue (no centre row needed: T is already formed).  Rows that no column reached, rows whose duals
// are all -inf (Z == 0), padded columns and columns with h = -inf write / contribute 0, never NaN.
//
// Width of a pass: ONE chunk of 32 coordinates (kXkDistGradChunks = 1).  Next to the state of xk_plan_kernel a wavefront carries the
// scalar, the distances of the block (the scalar needs them after the maximum is known) and the near masks; with two chunks every
// instantiation spills (256 VGPRs and 48 bytes of scratch per lane for the soft-min, 80 for the products), so NCH = 2 is not shipped.
//   registers / LDS / scratch / occupancy (gfx950, tools/kernel_resources.py, profiles/dist_grad_xk.txt), float32 and bfloat16 clouds alike:
//     soft-min p = 1 : 227 VGPRs, 95.1 KiB of LDS (97 408 B), 0 bytes of scratch, 2 waves per SIMD (one workgroup per CU)
//     laplacian      : 229 VGPRs, the same LDS, 0 bytes of scratch, 2 waves per SIMD
//     energy         : 231 VGPRs, the same LDS, 0 bytes of scratch, 2 waves per SIMD
//
// Shared pieces: the near-pair repair is xk_dist_exact_d2 / xk_dist_patch_near of glhip_dist_xk.h (the owner's patch; the second walk below
// keeps its structure and uses xk_dist_exact_d2 alone); the plan half calls plan_store_pieces, plan_rescale (with z4 as a second scalar),
// plan_split_weights and plan_chunk_mfma of glhip_plan_apply.h and the register maps of glhip_klayout.h (profiles/xk_plan_pieces.txt).
#pragma once

#include "glhip_dist_xk.h"
#include "glhip_plan_apply_xk.h"

namespace glhip {

constexpr int kXkDistGradChunks = 1;                     // chunks of 32 coordinates per pass (two spill, see above)

template <int MODE, typename T>
struct XkDistGradParams {
    const T* x;           // (B,N,D)
    const T* y;           // (B,M,D)
    const float* s;       // (B,M): the dual vector h (soft-min) or the signed weights v (products)
    const float* g;       // (B,N): the incoming gradient; NULL (fwd_grad): 1
    float* gx;            // (B,N,D)
    float* out;           // products, (B,N): sum_j k_ij v_j, written on the pass with v0 == 0; NULL: not wanted
    float t;              // coordinate scale (DistParams)
    float clamp2;         // 1e-8 t^2
    float guard;          // near pairs: d2 < max(guard n_i, 4 clamp2)
    float gscale;         // 1 (soft-min), -1 / blur (laplacian), -1 (energy)
    int v0;               // first coordinate of this pass
    int nv;               // coordinates of this pass, <= 32 NCH
};

// One entry of the gradient from T (unscaled coordinates), the scalar z and m, all relative to 2^m.
template <int MODE, typename T>
__device__ __forceinline__ float xk_dist_grad_entry(const XkDistGradParams<MODE, T>& prm, long row, float tc, float z, float e2m) {
    const float gs = (prm.g ? prm.g[row] : 1.f) * (prm.gscale * prm.t);
    if (MODE == DM_SOFTMIN_P1) return (z > 0.f) ? gs * (tc / z) : 0.f;
    return (e2m > 0.f) ? gs * (e2m * tc) : 0.f;
}

// The end of plan_merge_kernel (glhip_plan_apply.h): the merged T of coordinate c and the scalar of a row, both relative to 2^mx.
template <int MODE, typename T>
__device__ __forceinline__ void plan_merge_store(const XkDistGradParams<MODE, T>& prm, int, int D, long row, int c, float s, float w, float mx) {
    const float e2m = (MODE == DM_SOFTMIN_P1) ? 1.f : fast_exp2(mx);
    prm.gx[row * D + prm.v0 + c] = xk_dist_grad_entry(prm, row, s, w, e2m);
    if (MODE != DM_SOFTMIN_P1 && c == 0 && prm.out && prm.v0 == 0) prm.out[row] = (e2m > 0.f) ? w * e2m : 0.f;
}

template <int MODE, typename T, int NCH>
__global__ void __launch_bounds__(kXkThreads, 2)
xk_dist_grad_kernel(XkDistGradParams<MODE, T> prm, int N, int M, int D, SplitInfo sp) {
    constexpr int L = XL_BF16X3;
    constexpr bool SM = MODE == DM_SOFTMIN_P1;
    constexpr int VC = 32 * NCH;
    constexpr int kQRecs = NCH * 4 * 64;                      // feature records per column group
    constexpr int kFItems = (kXkCols / 4) * VC / kXkThreads;  // (column quad, feature) items per thread and tile
    static_assert(NCH == 1 || NCH == 2, "1 or 2 chunks of 32 coordinates per pass");
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
    const float t2 = prm.t * prm.t;
    const float kInf = __builtin_inff();
    const T* xb = prm.x + (long)b * N * D;
    const T* yb = prm.y + (long)b * M * D;

    const int row0 = bx * kXkRows;
    const int row_end = min(N, row0 + kXkRows);
    if (row0 >= row_end) return;
    const T* centre = xb + (long)row0 * D;
    const int nrows = row_end - row0;
    const int nr32 = (nrows + 31) & ~31;                      // row slots that are packed

    if (tid < 2 * VC) lds.fmax[tid / VC][tid % VC] = 0u;
    if (tid < kXkRows) lds.xk.idx[tid] = min(row0 + tid, row_end - 1);
    __syncthreads();
    xk_norms<T>(xb, centre, D, lds.xk.idx, 0, kXkRows, lds.xk.n2row, tid);
    __syncthreads();
    if (tid < kXkRows) lds.xk.scal[tid] = t2 * lds.xk.n2row[tid];      // n_i

    const int wave_row0 = row0 + wr * (kXkRT * 32);
    const bool wave_rows = wave_row0 < row_end;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 pacc[kXkRT][NCH];                                  // running sums S (unscaled centred coordinates), relative to 2^m
    float mass4[kXkRT][4], z4[kXkRT][4], m[kXkRT];            // W and the scalar, times 2^kWqShift; the running maximum of u~
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) pacc[rt][ch] = zero16;
#pragma unroll
        for (int k = 0; k < 4; ++k) { mass4[rt][k] = 0.f; z4[rt][k] = 0.f; }
        m[rt] = kMinusHuge;
    }

    int js, je;
    column_interval<false>(Ranges{nullptr, nullptr, nullptr, nullptr}, M, 0, split, ns, js, je);
    int parity = 0;
    for (int j0 = js; j0 < je; j0 += kXkCols, parity ^= 1) {
        const int n = min(kXkCols, je - j0);
        const int ncg = (n + 31) >> 5;                        // column groups that are packed and multiplied
        const int col = (tid < n) ? j0 + tid : -1;            // this thread's column (tid < kXkCols), -1 = padding
        __syncthreads();                                      // the previous tile (and the row scalars) are settled
        if (tid < kXkCols) lds.xk.idx[kXkRows + tid] = col;
        // features (xk_plan_kernel, GRAD / GAUSS): the centred coordinates v0 .. v0 + nv - 1 of the tile's columns, times v_j for the products
        float fv[kFItems][4];
#pragma unroll
        for (int k = 0; k < kFItems; ++k) {
            const int it = tid + k * kXkThreads;
            const int cq = it / VC, c = it - cq * VC;
            const int t = cq << 2;
            const float cen = (c < prm.nv) ? to_f32<T>(centre[prm.v0 + c]) : 0.f;
            uint32_t mx = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float f = 0.f;
                if (t + q < n && c < prm.nv) {
                    f = to_f32<T>(yb[(long)(j0 + t + q) * D + prm.v0 + c]) - cen;
                    if (!SM) f *= prm.s[(long)b * M + j0 + t + q];
                }
                fv[k][q] = f;
                mx = max(mx, __float_as_uint(f) & 0x7FFFFFFFu);
            }
            if (mx) atomicMax(&lds.fmax[parity][c], mx);
        }
        __syncthreads();                                      // the tile's indices and feature maxima are complete
        xk_norms<T>(yb, centre, D, lds.xk.idx, kXkRows, ncg * 32, &lds.xk.scal[kXkRows], tid);
        if (tid < VC) {
            const uint32_t se = plan_scale_exponent(lds.fmax[parity][tid]);
            lds.inv[tid] = __uint_as_float((254u - (uint32_t)kWqShift - se) << 23);
            lds.fmax[parity ^ 1][tid] = 0u;      // for the next tile: last read before the first barrier of this one
        }
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
        if (tid < ncg * 32) {                                 // |y_j - c|^2 -> N_j; the dual value / weight of the column (padding: -inf / 0)
            float Nj = 0.f, sj = SM ? -kInf : 0.f;
            if (col >= 0) {
                Nj = t2 * lds.xk.scal[kXkRows + tid];
                sj = prm.s[(long)b * M + col];
                if (SM) sj *= kLog2e;
            }
            lds.xk.scal[kXkRows + tid] = Nj;
            lds.xk.v[tid] = sj;
        }

        const bool wave_on = wave_rows && wc * kXkCG < ncg;
        f32x16 acc[kXkRT][kXkCG];
        xk_exponent_blocks<T, L, false>(lds.xk, xb, yb, centre, D, NM, NG, nr32, ncg, -2.f * prm.t, prm.t, wave_on, wr, wc, half, l31, tid, acc);
        if (!wave_on) continue;

#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) {
            if (wave_row0 + rt * 32 >= row_end) continue;     // a row tile past the block: not packed
            const int rslot = wr * (kXkRT * 32) + rt * 32 + l31;
            const float thr = fmaxf(prm.guard * lds.xk.scal[rslot], 4.f * prm.clamp2);
#pragma unroll
            for (int cg = 0; cg < kXkCG; ++cg) {
                const int G = wc * kXkCG + cg;
                if (G >= ncg) continue;
                const int cslot0 = G * 32;
                f32x16& d2 = acc[rt][cg];
                // ---- near pairs, as xk_dist_kernel: the owner patches its d2 with the exact value
                uint32_t near = 0u;
                const bool any_near = prm.guard > 0.f && __any(min16(d2) < thr);
                if (any_near) {
#pragma unroll
                    for (int k = 15; k >= 0; --k) near = (near << 1) | (d2[k] < thr ? 1u : 0u);
                    xk_dist_patch_near<T>(d2, near, xb + (long)lds.xk.idx[rslot] * D, yb, &lds.xk.idx[kXkRows + cslot0], half, D, prm.t, prm.clamp2);
                }
                // ---- u~ = u - 0.5 log2(d2) in place; ds: dist, or -1 for a pair inside the clamp
                const float* sg = &lds.xk.v[cslot0 + half * 4];
                f32x16 ds;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 s4 = *reinterpret_cast<const float4*>(sg + q * 8);
                    const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float dc = d2[q * 4 + r];
                        const bool cl = !(dc > prm.clamp2);
                        const float dist = fast_sqrt(__builtin_amdgcn_fmed3f(dc, prm.clamp2, 3.0e38f));
                        float ut = SM ? sv[r] - dist : (MODE == DM_LAPLACIAN ? -dist : 0.f);
                        ut = cl ? ut : __builtin_fmaf(-0.5f, fast_log2(dc), ut);
                        if (!SM) ut = (sv[r] != 0.f) ? ut : -kInf;
                        ds[q * 4 + r] = cl ? -1.f : dist;
                        d2[q * 4 + r] = ut;
                    }
                }
                float bm = max16(d2);
                bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
                plan_rescale(bm, m[rt], pacc[rt], mass4[rt], z4[rt]);      // lazy: only when the maximum grew
                // ---- the exact direction of the near pairs of the row: both lanes of the row walk the same pairs
                if (any_near) {
                    const uint32_t other = __shfl_xor(near, 32, 64);
                    if ((near | other) != 0u) {
                        const int irow = lds.xk.idx[rslot];
                        const T* xi = xb + (long)irow * D;
                        for (int hs = 0; hs < 2; ++hs) {
                            uint32_t todo = (hs == half) ? near : other;
                            while (todo != 0u) {
                                const int k = __builtin_ctz(todo);
                                todo &= todo - 1u;
                                const int cs = cslot0 + reg_column(k, hs);
                                const int j = lds.xk.idx[kXkRows + cs];
                                if (j < 0) continue;
                                const T* yj = yb + (long)j * D;
                                const float e = xk_dist_exact_d2<T>(xi, yj, D, prm.t);
                                if (!(e > prm.clamp2)) continue;      // inside the clamp: no direction
                                const float sj = lds.xk.v[cs];
                                const float dist = fast_sqrt(e);
                                float ut = SM ? sj - dist : (MODE == DM_LAPLACIAN ? -dist : 0.f);
                                ut = __builtin_fmaf(-0.5f, fast_log2(e), ut);
                                float wn = fast_exp2(ut - m[rt]);
                                if (!SM) wn = (sj != 0.f) ? wn * sj : 0.f;
#pragma unroll
                                for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
                                    for (int r = 0; r < 16; ++r) {
                                        const int c = 32 * ch + reg_feature(r, half);
                                        if (c < prm.nv) {     // S -= w (x_i - y_j): T = (x_i - c) W - S gains w (x_i - y_j)
                                            const float dy = to_f32<T>(yj[prm.v0 + c]) - to_f32<T>(xi[prm.v0 + c]);
                                            pacc[rt][ch][r] = __builtin_fmaf(wn, dy, pacc[rt][ch][r]);
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
                // ---- weights: W and the scalar from the unsplit fp32 weights, two f16 pieces for the product
                const float csq = fast_sqrt(prm.clamp2);
                Pack16h whi[2], wlo[2];
#pragma unroll
                for (int k = 0; k < 16; k += 2) {
                    const f32x2_t w = {fast_exp2(d2[k] - m[rt]) * (float)(1 << kWqShift), fast_exp2(d2[k + 1] - m[rt]) * (float)(1 << kWqShift)};
                    f32x2_t wd;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float dk = ds[k + e];
                        const bool cl = dk < 0.f;
                        float zf = cl ? 1.f : dk;                                   // 2^(u - m) = w' dist outside the clamp, w' inside
                        if (MODE == DM_ENERGY) zf *= cl ? -csq : -dk;               // energy: -dist v_j
                        wd[e] = (cl || ((near >> (k + e)) & 1u)) ? 0.f : w[e];
                        if (SM) {
                            z4[rt][(k & 3) + e] = __builtin_fmaf(w[e], zf, z4[rt][(k & 3) + e]);
                            mass4[rt][(k & 3) + e] += wd[e];
                        } else {
                            const float vj = sg[reg_column(k + e, 0)];      // (sg carries the lane half)
                            z4[rt][(k & 3) + e] = __builtin_fmaf(w[e] * zf, vj, z4[rt][(k & 3) + e]);
                            mass4[rt][(k & 3) + e] = __builtin_fmaf(wd[e], vj, mass4[rt][(k & 3) + e]);
                        }
                    }
                    plan_split_weights(wd, k, whi, wlo);
                }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const f32x16 t = plan_chunk_mfma(&lds.q[G * kQRecs + ch * (4 * 64) + lane], whi, wlo);
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

    // ---- T = (x_i - c) W - S, then the two column halves of the workgroup meet in LDS (the stage buffer is free now): [T | scalar | m][row] ----
    __syncthreads();
    float* mrg = reinterpret_cast<float*>(lds.xk.buf);
    float zs[kXkRT];
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
        float w = (mass4[rt][0] + mass4[rt][1]) + (mass4[rt][2] + mass4[rt][3]);
        float z = (z4[rt][0] + z4[rt][1]) + (z4[rt][2] + z4[rt][3]);
        w += __shfl_xor(w, 32, 64);                          // the two 16-column halves
        z += __shfl_xor(z, 32, 64);
        w *= 1.0f / (float)(1 << kWqShift);                  // relative to 2^m
        zs[rt] = z * (1.0f / (float)(1 << kWqShift));
        const int r_local = wr * (kXkRT * 32) + rt * 32 + l31;
        const int i = min(row0 + r_local, row_end - 1);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * ch + reg_feature(r, half);
                float xc = 0.f;
                if (c < prm.nv) xc = to_f32<T>(xb[(long)i * D + prm.v0 + c]) - to_f32<T>(centre[prm.v0 + c]);
                pacc[rt][ch][r] = __builtin_fmaf(xc, w, -pacc[rt][ch][r]);
            }
        }
        if (wc == 1) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mrg[(32 * ch + reg_feature(r, half)) * kXkRows + r_local] = pacc[rt][ch][r];
            }
            if (half == 0) {
                mrg[VC * kXkRows + r_local] = zs[rt];
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
        // the halves are brought to the larger m (factor exactly 1 for the half that holds it, 0 for a half no column reached)
        const float m2 = mrg[(VC + 1) * kXkRows + r_local];
        const float mn = fmaxf(m[rt], m2);
        const float rs1 = fast_exp2(m[rt] - mn), rs2 = fast_exp2(m2 - mn);
        const float z = __builtin_fmaf(mrg[VC * kXkRows + r_local], rs2, zs[rt] * rs1);
        const long idx = (long)b * N + i;
        const float e2m = (SM || ns > 1) ? 1.f : fast_exp2(mn);
        float* orow = prm.gx + idx * D + prm.v0;
        float* part = sp.workspace + split * sp.split_stride + idx * (prm.nv + 2);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * ch + reg_feature(r, half);
                if (c < prm.nv) {
                    const float s = __builtin_fmaf(mrg[c * kXkRows + r_local], rs2, pacc[rt][ch][r] * rs1);
                    if (ns > 1) part[c] = s;
                    else orow[c] = xk_dist_grad_entry(prm, idx, s, z, e2m);
                }
            }
        }
        if (half == 0) {
            if (ns > 1) {
                part[prm.nv] = z;
                part[prm.nv + 1] = mn;
            } else if (!SM) {
                if (prm.out && prm.v0 == 0) prm.out[idx] = (e2m > 0.f) ? z * e2m : 0.f;
            }
        }
    }
}

}  // namespace glhip
