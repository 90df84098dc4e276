// glhip_dist_xk.h — the DISTANCE reductions (soft-min with p = 1 incl. the fused Sinkhorn half-step, laplacian and energy kernel
// products) for clouds of dimension 17 <= D <= 4095, float32 / bfloat16 clouds, dense and batched launches (GLHIP_FLAG_XK_DIST).
//
// glhip_softmin_xk.h and glhip_dist_xd.h joined: the workgroup, the LDS and the stage loop are those of xk_fwd_kernel (256 rows x 128
// columns, 8 wavefronts as 4 x 2, XkLds, xk_exponent_blocks with D a run-time argument), the operands and the epilogue those of
// dist_xd_body.  With t the coordinate scale of DistParams and c the first row of the row block,
//     d2_ij = n_i + N_j + sum_d (-2 t (x_i - c)_d) (t (y_j - c)_d),      n_i = t^2 |x_i - c|^2,  N_j = t^2 |y_j - c|^2,
// is what the accumulators hold after the last stage: xscale = -2 t, yscale = t, row scalar n_i, column scalar N_j (xk_norms).  bf16 x 3
// only — a squared distance is a difference of large terms and needs all 24 bits; GLHIP_FLAG_F16X2 is ignored.
//
// Epilogue, per wavefront on its 2 x 2 blocks: near pairs (d2 < max(guard n_i, 4 clamp2): the expanded form has lost its bits there,
// see glhip_dist_xd.h; the debiasing terms of a Sinkhorn loss are x against x) are re-evaluated on explicit differences of the points
// themselves, a run-time loop over D from global memory with the row / column indices of lds.idx; then the clamp of utils.py:61
// (v_med3), v_sqrt_f32 and
//     soft-min  : u = S_j - dist, S_j = log2(e) (s_j + pot_scale pot_j) from lds.v; explicit lazy running maximum as xk_fwd_kernel
//     laplacian : exp2(-dist) v_j          energy : -dist v_j          (v_j from lds.v as broadcast float4)
// Padded columns contribute nothing: S_j = kNegBig, v_j = 0 (their d2 is n_i: no coordinates, scalar 0), and they are never re-evaluated.
// The two column halves of the workgroup meet in LDS; partials of a column split are (m, s) resp. s: the formats of
// SoftminFwdOp<1, 1, true, 1, T> / ConvOp<KIND, 1, 1, T, 0>.
//
// The first row of a block is its centre: n_i = 0 and d2 = N_j, a float32 chain on explicit differences — exact like a near pair.
//
// The near-pair repair is two __device__ __forceinline__ pieces below, xk_dist_exact_d2 and xk_dist_patch_near, shared with
// xk_dist_grad_kernel (glhip_dist_grad_xk.h); the v_mbcnt re-derivation of the lane stays at this kernel's call site.
#pragma once

#include "glhip_dist_xd.h"
#include "glhip_softmin_xk.h"

namespace glhip {

// ---- The near-pair repair, shared with xk_dist_grad_kernel (glhip_dist_grad_xk.h) and xk_dist_plan_kernel (glhip_dist_plan_xk.h) ----

// t^2 |x_i - y_j|^2 on explicit differences of the points themselves: a run-time loop over D from global memory
template <typename T>
__device__ __forceinline__ float xk_dist_exact_d2(const T* xi, const T* yj, int D, float t) {
    float e = 0.f;
    for (int d = 0; d < D; ++d) {
        const float df = (to_f32<T>(xi[d]) - to_f32<T>(yj[d])) * t;
        e = __builtin_fmaf(df, df, e);
    }
    return e;
}

// The owner of a block's near pairs (mask `near`: bit k = register k of d2, column reg_column(k, half) of the group whose column
// indices are cidx[0 .. 31], -1 = padding, never re-evaluated) patches its d2 with the exact value, clamped from below: one pair per
// lane and turn.
template <typename T>
__device__ __forceinline__ void xk_dist_patch_near(f32x16& d2, uint32_t near, const T* xi, const T* yb, const int* cidx, int half, int D,
                                                   float t, float clamp2) {
    while (near != 0u) {
        const int k = __builtin_ctz(near);
        near &= near - 1u;
        const int j = cidx[reg_column(k, half)];
        if (j >= 0) {
            const float e = fmaxf(xk_dist_exact_d2<T>(xi, yb + (long)j * D, D, t), clamp2);
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) d2[kk] = (kk == k) ? e : d2[kk];
        }
    }
}

template <int MODE, typename T>
__global__ void __launch_bounds__(kXkThreads, 4)
xk_dist_kernel(DistParams<T> prm, int N, int M, int D, SplitInfo sp) {
    constexpr int L = XL_BF16X3;
    constexpr bool SM = MODE == DM_SOFTMIN_P1;
    __shared__ XkLds lds;

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
    const T* xb = prm.x + (long)b * N * D;
    const T* yb = prm.y + (long)b * M * D;

    const int row0 = bx * kXkRows;
    const int row_end = min(N, row0 + kXkRows);
    if (row0 >= row_end) return;
    const T* centre = xb + (long)row0 * D;
    const int nrows = row_end - row0;
    const int nr32 = (nrows + 31) & ~31;                      // row slots that are packed
    if (tid < kXkRows) lds.idx[tid] = min(row0 + tid, row_end - 1);
    __syncthreads();
    xk_norms<T>(xb, centre, D, lds.idx, 0, kXkRows, lds.n2row, tid);
    __syncthreads();
    if (tid < kXkRows) lds.scal[tid] = t2 * lds.n2row[tid];  // n_i

    const int wave_row0 = row0 + wr * (kXkRT * 32);
    const bool wave_rows = wave_row0 < row_end;
    float m[kXkRT], ssum[kXkRT];                              // soft-min: running maximum and sum;  products: ssum only
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) { m[rt] = kMinusHuge; ssum[rt] = 0.f; }

    int js, je;
    column_interval<false>(Ranges{nullptr, nullptr, nullptr, nullptr}, M, 0, split, ns, js, je);
    for (int j0 = js; j0 < je; j0 += kXkCols) {
        const int n = min(kXkCols, je - j0);
        const int ncg = (n + 31) >> 5;                        // column groups that are packed and multiplied
        const int col = (tid < n) ? j0 + tid : -1;            // this thread's column (tid < kXkCols), -1 = padding
        __syncthreads();                                      // the previous tile (and the row scalars) are settled
        if (tid < kXkCols) lds.idx[kXkRows + tid] = col;
        __syncthreads();
        xk_norms<T>(yb, centre, D, lds.idx, kXkRows, ncg * 32, &lds.scal[kXkRows], tid);
        __syncthreads();
        if (tid < ncg * 32) {                                 // |y_j - c|^2 -> N_j; the dual value / weight of the column
            float Nj = 0.f, sj = SM ? kNegBig : 0.f;
            if (col >= 0) {
                Nj = t2 * lds.scal[kXkRows + tid];
                sj = prm.s[(long)b * M + col];
                if (SM) {
                    if (prm.pot) sj = __builtin_fmaf(prm.pot[(long)b * M + col], prm.pot_scale, sj);
                    sj *= kLog2e;
                }
            }
            lds.scal[kXkRows + tid] = Nj;
            lds.v[tid] = sj;
        }

        const bool wave_on = wave_rows && wc * kXkCG < ncg;
        f32x16 acc[kXkRT][kXkCG];
        xk_exponent_blocks<T, L, false>(lds, xb, yb, centre, D, NM, NG, nr32, ncg, -2.f * prm.t, prm.t, wave_on, wr, wc, half, l31, tid, acc);
        if (!wave_on) continue;

        // ---- epilogue: the squared distances of this wavefront's 2 x 2 blocks join the row sums (column groups >= ncg were not packed) ----
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) {
            if (wave_row0 + rt * 32 >= row_end) continue;     // a row tile past the block: not packed
            const int rslot = wr * (kXkRT * 32) + rt * 32 + l31;
            const float thr = fmaxf(prm.guard * lds.scal[rslot], 4.f * prm.clamp2);
            float um = kMinusHuge;
#pragma unroll
            for (int cg = 0; cg < kXkCG; ++cg) {
                const int cslot0 = (wc * kXkCG + cg) * 32;
                if (cslot0 >= ncg * 32) continue;
                f32x16& d2 = acc[rt][cg];
                // near pairs and everything below 4 x the floor of utils.py:61, which only an exact value may decide: one pair per
                // lane and turn (xk_dist_patch_near)
                if (prm.guard > 0.f && __any(min16(d2) < thr)) {
                    uint32_t near = 0u;
#pragma unroll
                    for (int k = 15; k >= 0; --k) near = (near << 1) | (d2[k] < thr ? 1u : 0u);      // (v_lshl_or: no 1 << k constants in VGPRs)
                    // the lane, re-derived on this rare path: the LDS addresses below, hoisted out of the tile loop and kept for it,
                    // cost the soft-min instantiations 8 bytes of scratch
                    int ln;
                    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
                    const int nh = ln >> 5;
                    const T* xi = xb + (long)lds.idx[wr * (kXkRT * 32) + rt * 32 + (ln & 31)] * D;
                    xk_dist_patch_near<T>(d2, near, xi, yb, &lds.idx[kXkRows + cslot0], nh, D, prm.t, prm.clamp2);
                }
                const float* sg = &lds.v[cslot0 + half * 4];
                float a4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 s4 = *reinterpret_cast<const float4*>(sg + q * 8);
                    const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float dist = fast_sqrt(__builtin_amdgcn_fmed3f(d2[q * 4 + r], prm.clamp2, 3.0e38f));
                        if (SM) d2[q * 4 + r] = sv[r] - dist;
                        else if (MODE == DM_LAPLACIAN) a4[r] = __builtin_fmaf(fast_exp2(-dist), sv[r], a4[r]);
                        else a4[r] = __builtin_fmaf(-dist, sv[r], a4[r]);
                    }
                }
                if (SM) um = fmaxf(um, max16(d2));
                else ssum[rt] += (a4[0] + a4[1]) + (a4[2] + a4[3]);
            }
            if (SM) {
                um = fmaxf(um, __shfl_xor(um, 32, 64));
                if (um > m[rt]) {                             // lazy: rescale only when the maximum grew
                    ssum[rt] *= fast_exp2(m[rt] - um);
                    m[rt] = um;
                }
#pragma unroll
                for (int cg = 0; cg < kXkCG; ++cg)
                    if (wc * kXkCG + cg < ncg) ssum[rt] += sum_exp2_16(acc[rt][cg], m[rt]);
            }
        }
    }

    // ---- the two column halves of the workgroup meet in LDS (the tile buffer is free now): [wc][row] of (m, s) ----
    __syncthreads();
    float* mrg = reinterpret_cast<float*>(lds.buf);
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
        const float s = ssum[rt] + __shfl_xor(ssum[rt], 32, 64);      // the lane halves hold the two 16-column halves of every block
        if (half == 0) {
            const int r = wr * (kXkRT * 32) + rt * 32 + l31;
            mrg[(wc * kXkRows + r) * 2] = m[rt];
            mrg[(wc * kXkRows + r) * 2 + 1] = s;
        }
    }
    __syncthreads();
    if (tid < nrows) {
        float mt = mrg[tid * 2], s = mrg[tid * 2 + 1];
#pragma unroll
        for (int w = 1; w < kXkWC; ++w) {
            const float m2 = mrg[(w * kXkRows + tid) * 2], s2 = mrg[(w * kXkRows + tid) * 2 + 1];
            if (SM) {
                const float mn = fmaxf(mt, m2);
                s = s * fast_exp2(mt - mn) + s2 * fast_exp2(m2 - mn);
                mt = mn;
            } else {
                s += s2;
            }
        }
        const long idx = (long)b * N + row0 + tid;
        if (SM) {
            if (ns == 1) {
                float f = prm.alpha * (prm.out_scale * (mt + fast_log2(s)));
                if (prm.prev) f = __builtin_fmaf(prm.beta, prm.prev[idx], f);
                prm.out[idx] = f;
            } else {
                float* dst = sp.workspace + split * sp.split_stride + idx * 2;
                dst[0] = mt;
                dst[1] = s;
            }
        } else {
            if (ns == 1) prm.out[idx] = s;
            else sp.workspace[split * sp.split_stride + idx] = s;
        }
    }
}

}  // namespace glhip
