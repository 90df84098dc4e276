// glhip_dist_plan_xk.h — the transport plan of a p = 1 soft-min applied to a feature matrix on the matrix cores, 1 <= D <= 4095,
// float32 / bfloat16 clouds, dense and batched launches (glhip_plan_apply_p1):
//
//     out[i][v]  = sum_j w_ij feat[j][v] / sum_j w_ij,      w_ij = 2^( S_j - dist_ij ),   S_j = log2(e) h_j,
//     softmin[i] = -eps ln 2 log2 sum_j w_ij                (optional)
// with dist_ij = sqrt(max(d2_ij, clamp2)), d2 = t^2 |x_i - y_j|^2, t = log2(e) / eps the coordinate scale of DistParams and clamp2 =
// 1e-8 t^2 the floor of utils.py:61.  A new __global__ template that joins two halves the tree already has, as xk_dist_grad_kernel
// (glhip_dist_grad_xk.h) does for one particular feature matrix and weight — here the caller's features and the plain weight, and none of
// that kernel's machinery (no u~ maximum, no second walk over near pairs, no xs W - S cancellation):
//
//   exponent half = xk_dist_kernel (glhip_dist_xk.h): d2 from the chain with xscale = -2 t, yscale = t, n_i, N_j (xk_exponent_blocks,
//   xk_norms, bf16 x 3 only: a squared distance needs all 24 bits), centred on the first row of the 256-row block; pairs below
//   thr = max(guard n_i, 4 clamp2) re-evaluated on explicit differences from global memory (xk_dist_patch_near); then v_med3, v_sqrt_f32,
//   u = S_j - dist.  Padded columns and columns with h = -inf carry S_j = -inf: they weigh exactly 0.
//
//   plan half = the discipline of xk_plan_kernel (glhip_plan_apply_xk.h): the features of the pass in two f16 pieces under a per-column
//   power-of-two scale (XkPlanLds, plan_scale_exponent, plan_store_pieces); weights relative to the lazy running row maximum times
//   2^kWqShift in two f16 pieces (plan_rescale, plan_split_weights); six v_mfma_f32_32x32x16_f16 per chunk of 32 features into a fresh
//   accumulator per 32-column block (plan_chunk_mfma); the row sum Z and the maximum from the unsplit fp32 weights on the VALU.  The
//   largest weight of a row is 2^13 exactly: a one-hot plan row returns its features bit for bit.
//
// The kernel normalises itself (no saved forward value comes in) and returns the soft-min it has computed on the side, (m, Z), on the
// pass with v0 == 0.  The two column halves of the workgroup meet in LDS on (sums[nv], Z, m); a column split writes the same nv + 2
// floats and plan_merge_kernel (glhip_plan_apply.h) is reused unchanged, with plan_merge_store below.  No atomics on results and no order
// that depends on timing: bit-identical run to run.  Rows that no column reached, rows whose duals are all -inf (Z == 0), padded columns
// and columns with h = -inf write / contribute 0, never NaN; the soft-min of a row without mass is +inf.
//
// ONE kernel for 1 <= D <= 4095: below D = 17 the chain is a single stage (NM = 1 at D = 1, 6 = one whole stage at D = 15); a
// resident-operand variant for D <= 16 is a follow-up.
//
// Width of a pass: TWO chunks of 32 features (kXkDistPlanChunks = 2), a pass of <= 32 features runs the one-chunk instantiation; wider
// feature matrices take further passes (launch_plan_passes), a remainder is a pass of its own.  Next to the state of xk_plan_kernel a
// wavefront carries only the near mask of the block it is repairing — no saved forward value, no second scalar, no distances kept for
// later — so, unlike xk_dist_grad_kernel, two chunks fit without scratch.
//   registers / LDS / scratch / occupancy (gfx950, tools/kernel_resources.py, profiles/dist_plan_xk.txt), float32 and bfloat16 clouds alike:
//     NCH = 1 : 206 VGPRs,  95.1 KiB of LDS  (97 408 B), 0 bytes of scratch, 2 waves per SIMD (one workgroup per CU)
//     NCH = 2 : 246 VGPRs, 111.5 KiB of LDS (114 176 B), 0 bytes of scratch, 2 waves per SIMD
//     plan_merge_kernel on XkDistPlanParams: 15 VGPRs, no LDS, no scratch
#pragma once

#include "glhip_dist_xk.h"
#include "glhip_plan_apply_xk.h"

namespace glhip {

constexpr int kXkDistPlanChunks = 2;                     // chunks of 32 features per pass (both fit without scratch, see above)

template <typename T>
struct XkDistPlanParams {
    const T* x;           // (B,N,D)
    const T* y;           // (B,M,D)
    const float* h;       // (B,M): the dual vector
    const float* feat;    // (B,M,V)
    float* out;           // (B,N,V)
    float* softmin;       // (B,N): -eps log sum_j exp(h_j - c_ij / eps), written on the pass with v0 == 0; NULL: not wanted
    float t;              // coordinate scale log2(e) / eps (DistParams)
    float clamp2;         // 1e-8 t^2
    float guard;          // near pairs: d2 < max(guard n_i, 4 clamp2)
    float out_scale;      // -eps ln 2: softmin = out_scale (m + log2 Z)
    int V;                // feature columns of feat / out
    int v0;               // first feature of this pass
    int nv;               // features of this pass, <= 32 NCH
};

// The soft-min of a row from its sum z relative to 2^m; z == 0 (no mass): +inf
template <typename T>
__device__ __forceinline__ float xk_dist_plan_softmin(const XkDistPlanParams<T>& prm, float z, float m) {
    return (z > 0.f) ? prm.out_scale * (m + fast_log2(z)) : __builtin_inff();
}

// The end of plan_merge_kernel (glhip_plan_apply.h): the merged sum s of feature c and the row sum w, both relative to 2^mx — divided.
template <typename T>
__device__ __forceinline__ void plan_merge_store(const XkDistPlanParams<T>& prm, int, int, long row, int c, float s, float w, float mx) {
    prm.out[row * prm.V + prm.v0 + c] = (w > 0.f) ? s / w : 0.f;
    if (c == 0 && prm.v0 == 0 && prm.softmin) prm.softmin[row] = xk_dist_plan_softmin(prm, w, mx);
}

template <typename T, int NCH>
__global__ void __launch_bounds__(kXkThreads, 2)
xk_dist_plan_kernel(XkDistPlanParams<T> prm, int N, int M, int D, SplitInfo sp) {
    constexpr int L = XL_BF16X3;
    constexpr int VC = 32 * NCH;
    constexpr int kQRecs = NCH * 4 * 64;                      // feature records per column group
    constexpr int kFItems = (kXkCols / 4) * VC / kXkThreads;  // (column quad, feature) items per thread and tile
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
    const float t2 = prm.t * prm.t;
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
    f32x16 pacc[kXkRT][NCH];                                  // running sums, relative to 2^m
    float mass4[kXkRT][4], m[kXkRT];                          // Z times 2^kWqShift; the running maximum of u
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) pacc[rt][ch] = zero16;
#pragma unroll
        for (int k = 0; k < 4; ++k) mass4[rt][k] = 0.f;
        m[rt] = kMinusHuge;      // (both lane halves of a row hold the same value)
    }

    int js, je;
    column_interval<false>(Ranges{nullptr, nullptr, nullptr, nullptr}, M, 0, split, ns, js, je);
    int parity = 0;
    for (int j0 = js; j0 < je; j0 += kXkCols, parity ^= 1) {
        const int n = min(kXkCols, je - j0);
        const int ncg = (n + 31) >> 5;                        // column groups that are packed and multiplied
        const int col = (tid < n) ? j0 + tid : -1;            // this thread's column (tid < kXkCols), -1 = padding
        {   // which of the tile's columns carry mass (h_j > -inf): read by the feature staging between the next two barriers
            const float hcol = (col >= 0) ? prm.h[(long)b * M + col] : -__builtin_inff();
            const unsigned long long live = __ballot(hcol != -__builtin_inff());
            if (lane == 0 && wave < 2) {
                lds.live[2 * wave] = (uint32_t)live;
                lds.live[2 * wave + 1] = (uint32_t)(live >> 32);
            }
        }
        __syncthreads();                                      // the previous tile (and the row scalars) are settled
        if (tid < kXkCols) lds.xk.idx[kXkRows + tid] = col;
        // features (xk_plan_kernel): item (column quad cq, feature c of the pass) — c runs fastest: contiguous runs of feat rows
        float fv[kFItems][4];
        const bool voids = __popc(lds.live[0]) + __popc(lds.live[1]) + __popc(lds.live[2]) + __popc(lds.live[3]) != n;      // (rare)
#pragma unroll
        for (int k = 0; k < kFItems; ++k) {
            const int it = tid + k * kXkThreads;
            const int cq = it / VC, c = it - cq * VC;
            const int t = cq << 2;
            uint32_t mx = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float f = 0.f;
                if (t + q < n && c < prm.nv) f = prm.feat[((long)b * M + j0 + t + q) * prm.V + prm.v0 + c];
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
        if (tid < ncg * 32) {                                 // |y_j - c|^2 -> N_j; the dual value of the column (padding, h = -inf: -inf)
            float Nj = 0.f, sj = -__builtin_inff();
            if (col >= 0) {
                Nj = t2 * lds.xk.scal[kXkRows + tid];
                sj = prm.h[(long)b * M + col] * kLog2e;
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
                if (prm.guard > 0.f && __any(min16(d2) < thr)) {
                    uint32_t near = 0u;
#pragma unroll
                    for (int k = 15; k >= 0; --k) near = (near << 1) | (d2[k] < thr ? 1u : 0u);
                    xk_dist_patch_near<T>(d2, near, xb + (long)lds.xk.idx[rslot] * D, yb, &lds.xk.idx[kXkRows + cslot0], half, D, prm.t, prm.clamp2);
                }
                // ---- u = S_j - dist in place: four broadcast 16-byte reads of the dual values
                const float* sg = &lds.xk.v[cslot0 + half * 4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 s4 = *reinterpret_cast<const float4*>(sg + q * 8);
                    const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float dist = fast_sqrt(__builtin_amdgcn_fmed3f(d2[q * 4 + r], prm.clamp2, 3.0e38f));
                        d2[q * 4 + r] = sv[r] - dist;
                    }
                }
                float bm = max16(d2);
                bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
                plan_rescale(bm, m[rt], pacc[rt], mass4[rt]);      // lazy: only when the maximum grew
                // ---- weights: Z from the unsplit fp32 weights, two f16 pieces for the product
                Pack16h whi[2], wlo[2];
#pragma unroll
                for (int k = 0; k < 16; k += 2) {
                    const f32x2_t w = {fast_exp2(d2[k] - m[rt]) * (float)(1 << kWqShift), fast_exp2(d2[k + 1] - m[rt]) * (float)(1 << kWqShift)};
                    mass4[rt][k & 3] += w[0];
                    mass4[rt][(k & 3) + 1] += w[1];
                    plan_split_weights(w, k, whi, wlo);
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

    // ---- the two column halves of the workgroup meet in LDS (the stage buffer is free now): [feature | Z | m][row] ----
    __syncthreads();
    float* mrg = reinterpret_cast<float*>(lds.xk.buf);
    float zs[kXkRT];
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
        float z = (mass4[rt][0] + mass4[rt][1]) + (mass4[rt][2] + mass4[rt][3]);
        z += __shfl_xor(z, 32, 64);                          // the two 16-column halves
        zs[rt] = z * (1.0f / (float)(1 << kWqShift));        // relative to 2^m
        if (wc == 1) {
            const int r_local = wr * (kXkRT * 32) + rt * 32 + l31;
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
        float* orow = prm.out + idx * prm.V + prm.v0;
        float* part = sp.workspace + split * sp.split_stride + idx * (prm.nv + 2);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * ch + reg_feature(r, half);
                if (c < prm.nv) {
                    const float s = __builtin_fmaf(mrg[c * kXkRows + r_local], rs2, pacc[rt][ch][r] * rs1);
                    if (ns > 1) part[c] = s;
                    else orow[c] = (z > 0.f) ? s / z : 0.f;      // a division: exact where the quotient is
                }
            }
        }
        if (half == 0) {
            if (ns > 1) {
                part[prm.nv] = z;
                part[prm.nv + 1] = mn;
            } else if (prm.softmin && prm.v0 == 0) {
                prm.softmin[idx] = xk_dist_plan_softmin(prm, z, mn);
            }
        }
    }
}

}  // namespace glhip
