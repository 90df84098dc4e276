// glhip_plan_bilinear_xk.h — the transport plan of a p = 2 soft-min contracted with a per-pair bilinear weight, on the matrix cores,
// 1 <= D <= 4095, 1 <= K <= 4095, float32 / bfloat16 clouds, float32 features, dense and batched launches (glhip_plan_bilinear):
//
//     w_ij   = exp(h_j - |x_i - y_j|^2 / (2 eps) + fwd_i / eps),      pi_ij = w_ij / sum_j w_ij,      tau_ij = <rowfeat_i, colfeat_j>
//     out[i][:] = sum_j pi_ij tau_ij (y_j - x_i)                      wsum[i] = sum_j pi_ij tau_ij
//
// the one reduction behind the gradients of P @ S and of the barycentric map with respect to the points and the potentials
// (geomloss_amd/transport.py).  ONE kernel for the whole range of D, a __global__ body of its own that joins pieces the tree already has,
// the way xk_dist_grad_kernel (glhip_dist_grad_xk.h) was built; xk_plan_kernel is not touched.  Per column tile:
//
//   exponent half = that of xk_plan_kernel (glhip_plan_apply_xk.h): xk_exponent_blocks over (x, y, D), clouds centred on the first row of
//   the row block, C_i and the -inf column mask on the VALU, both layouts (GLHIP_FLAG_F16X2 applies to this half only).
//
//   weight half = a SECOND run of xk_exponent_blocks over (rowfeat, colfeat, K) through the same stage buffer: uncentred (CENTRED = false),
//   unit scale, zero scalars, always bf16 x 3 — arbitrary features carry no f16 range contract.  It leaves tau of the same 2 x 2 blocks of
//   32 x 32 pairs in the same register layout, at float32 accuracy (the error model of glhip_softmin_xk.h with s |xt| |yt| read as
//   |rowfeat_i| |colfeat_j|).
//
//   product: TWO running maxima per row.  m, over the exponents u, carries the mass sum_j w_ij (unsplit fp32 weights, 2^(u - m)), as in
//   every plan kernel.  mq, over u + log2 |tau| — the lazy maximum of xk_dist_grad_kernel's u~ —, carries the signed sums: the product
//   q_ij = tau_ij 2^13 2^(u_ij - mq_i) is <= 2^13 in magnitude whatever the features are worth, is split into two f16 pieces
//   (plan_split_weights) and multiplies the centred coordinates (y_j - centre) of the pass, staged as xk_plan_kernel's GRAD features
//   (plan_store_pieces, plan_scale_exponent), in plan_chunk_mfma.  Features of any magnitude neither overflow nor flush: a common factor of
//   tau moves mq and nothing else (2^(u - mq) is capped at 2^110: |tau| down to 2^-110 of a row's largest product still counts in full).
//   W_i = sum_j q_ij is summed in fp32 from the unsplit products, as GAUSS sums its signed mass.  A pair whose weight is 0 (h_j = -inf,
//   padding) has q = 0 by a select, whatever finite tau it holds; a row whose tau are all 0 keeps mq at its floor and sums zeros.
//
//   epilogue: T_c = S_c - (x_i - centre)_c W is formed before anything is written (xk_dist_grad_kernel); the two column halves of the
//   workgroup meet in LDS on (T[nv], W, mass, mq, m), are brought to the larger mq and the larger m, and then to ONE scale:
//   2^(mq - m) multiplies T and W.  out = T / mass, wsum = W / mass; a row without mass gets 0 in both.  A column split writes
//   (T[nv], W, mass, m): nv + 3 floats, merged by plan_merge_kernel (glhip_plan_apply.h, unchanged) on a copy of the parameters whose
//   nv counts W as one more sum; plan_merge_store below divides.  No atomics on floats: bit-identical run to run.
//
// Cost model per 32 x 32 block and pass: NM(D) + NM(K) chained MFMAs of the two halves + 6 NCH of the product + ~110 VALU instructions
// (32 exponentials, 16 logarithms, the piece conversions); a pass re-stages both halves, so D > 32 NCH pays the chains once per pass.
//
// Width of a pass: ONE chunk of 32 coordinates (kXkBilinearChunks = 1; glhip_plan_bilinear_pass_width() reports 32).  Next to the state
// of xk_plan_kernel a wavefront holds the 64 registers of tau while the plan half consumes them, a second maximum and a second
// four-register scalar per row tile.  All four tau blocks are held at once — forming them per column group would re-stage the rows of the
// weight half — and that fits the 256 VGPRs of 8 wavefronts per workgroup exactly; with two chunks every instantiation spills, so 64 per
// pass is not shipped (as in glhip_dist_grad_xk.h).
//   registers / LDS / scratch / occupancy (gfx950, tools/kernel_resources.py on the -Rpass-analysis=kernel-resource-usage remarks the
//   Makefile prints for this translation unit), float32 and bfloat16 clouds, both exponent layouts alike:
//     NCH = 1 (shipped): 256 VGPRs, 95.1 KiB of LDS (97 424 B), 0 bytes of scratch, 2 waves per SIMD (one workgroup per CU)
//     NCH = 2 (not shipped): 256 VGPRs, 111.5 KiB of LDS (114 192 B), 140 bytes of scratch per lane
//   xk_plan_kernel (199-207 / 245-256 VGPRs) and xk_dist_grad_kernel (227-231) keep their figures: the only shared text that changed is
//   the CENTRED parameter of xk_exponent_blocks, whose default leaves their code as it was.
//
// Out of scope: p = 1, block-sparse ranges (the arguments are in the ABI), float64, D or K > 4095, second derivatives, a
// resident-operand variant for D <= 16, and routing hip._plan_moments (the Cov_i V_i of the p = 2 double backward: the same reduction with
// rowfeat = V, colfeat = y) through this kernel.
#pragma once

#include "glhip_plan_apply_xk.h"

namespace glhip {

constexpr int kXkBilinearChunks = 1;                     // chunks of 32 coordinates per pass (see above)

template <typename T>
struct XkBilinearParams {
    const T* x;           // (B,N,D)
    const T* y;           // (B,M,D)
    const float* h;       // (B,M)
    const float* fwd;     // (B,N): the saved soft-min
    const float* rowfeat; // (B,N,K)
    const float* colfeat; // (B,M,K)
    float* out;           // (B,N,D)
    float* wsum;          // (B,N) or NULL
    float s2;             // log2(e) / eps
    float out_scale;      // -eps ln 2: LSE2_i = fwd_i / out_scale
    int K;                // features of the weight half
    int v0;               // first coordinate of this pass
    int nv;               // coordinates of this pass, <= 32 NCH (the merge: + 1, W counts as the last sum)
};

// The end of plan_merge_kernel: prm.nv - 1 coordinates and W of a row, merged sum s and mass w relative to the same 2^mx — divided.
template <typename T>
__device__ __forceinline__ void plan_merge_store(const XkBilinearParams<T>& prm, int, int D, long row, int c, float s, float w, float) {
    const float q = (w > 0.f) ? s / w : 0.f;
    if (c < prm.nv - 1) prm.out[row * D + prm.v0 + c] = q;
    else if (prm.v0 == 0 && prm.wsum) prm.wsum[row] = q;
}

constexpr float kBilinearMaxLift = 110.f;                // cap of u - mq: 2^110 2^13 |tau| stays finite

template <typename T, int NCH, int L>
__global__ void __launch_bounds__(kXkThreads, 2)
xk_bilinear_kernel(XkBilinearParams<T> prm, int N, int M, int D, SplitInfo sp) {
    constexpr bool H2 = (L == XL_F16X2);
    constexpr int VC = 32 * NCH;
    constexpr int kQRecs = NCH * 4 * 64;                      // feature records per column group
    constexpr int kFItems = (kXkCols / 4) * VC / kXkThreads;  // (column quad, coordinate) items per thread and tile
    static_assert(NCH == 1 || NCH == 2, "1 or 2 chunks of 32 coordinates per pass");
    static_assert(kFItems * kXkThreads == (kXkCols / 4) * VC, "whole items per thread");
    static_assert((VC + 4) * kXkRows * sizeof(float) <= sizeof(XkLds::buf), "the column halves meet in the stage buffer");
    __shared__ XkPlanLds<NCH> lds;

    int bx, b, split;
    workgroup_coords(sp, bx, b, split);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / kXkWC, wc = wave % kXkWC;
    const int half = lane >> 5, l31 = lane & 31;
    const int ns = sp.n_splits;
    const int K = prm.K;
    const int NM = xk_num_mfma(D, L), NG = xk_num_groups(D, L);
    const int NMK = xk_num_mfma(K, XL_BF16X3), NGK = xk_num_groups(K, XL_BF16X3);
    const float xscale = H2 ? __builtin_sqrtf(prm.s2) : prm.s2;
    const float yscale = H2 ? __builtin_sqrtf(prm.s2) : 1.0f;
    const T* xb = prm.x + (long)b * N * D;
    const T* yb = prm.y + (long)b * M * D;
    const float* rfb = prm.rowfeat + (long)b * N * K;
    const float* cfb = prm.colfeat + (long)b * M * K;

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
    if (tid < kXkRows) lds.xk.scal[tid] = 0.f;                // both halves: the x-side scalar is 0, r_i joins with C_i

    const int wave_row0 = row0 + wr * (kXkRT * 32);
    const bool wave_rows = wave_row0 < row_end;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 pacc[kXkRT][NCH];                                  // running sums S (centred coordinates), relative to 2^mq
    float mass4[kXkRT][4], w4[kXkRT][4];                      // the mass (relative to 2^m) and W (relative to 2^mq), times 2^kWqShift
    float m[kXkRT], mq[kXkRT], cst[kXkRT];
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) pacc[rt][ch] = zero16;
#pragma unroll
        for (int k = 0; k < 4; ++k) { mass4[rt][k] = 0.f; w4[rt][k] = 0.f; }
        m[rt] = kMinusHuge;
        mq[rt] = kMinusHuge;
        // C_i = r_i - LSE2_i as in xk_plan_kernel: fwd_i = +inf is a row without mass, a huge fwd_i stays finite against the -inf mask
        const int i = min(wave_row0 + rt * 32 + l31, row_end - 1);
        const float fw = prm.fwd[(long)b * N + i];
        const float c = -0.5f * prm.s2 * lds.xk.n2row[i - row0] - fw / prm.out_scale;
        cst[rt] = (fw == __builtin_inff()) ? kNegBig : __builtin_fminf(c, -kNegBig);
    }

    int js, je;
    column_interval<false>(Ranges{nullptr, nullptr, nullptr, nullptr}, M, 0, split, ns, js, je);
    int parity = 0;
    for (int j0 = js; j0 < je; j0 += kXkCols, parity ^= 1) {
        const int n = min(kXkCols, je - j0);                  // real columns, in the slots kXkRows .. kXkRows + n - 1
        const int ncg = (n + 31) >> 5;                        // column groups that are packed and multiplied
        const int col = (tid < n) ? j0 + tid : -1;            // this thread's column (tid < kXkCols), -1 = padding
        __syncthreads();                                      // the previous tile (and the row scalars) are settled
        if (tid < kXkCols) lds.xk.idx[kXkRows + tid] = col;
        // features (xk_plan_kernel, GRAD): the centred coordinates v0 .. v0 + nv - 1 of the tile's columns, runs of y rows
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
                if (t + q < n && c < prm.nv) f = to_f32<T>(yb[(long)(j0 + t + q) * D + prm.v0 + c]) - cen;
                fv[k][q] = f;
                mx = max(mx, __float_as_uint(f) & 0x7FFFFFFFu);
            }
            if (mx) atomicMax(&lds.fmax[parity][c], mx);
        }
        __syncthreads();                                      // the tile's indices and coordinate maxima are complete
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
        if (tid < ncg * 32) {                                 // |yt|^2 -> H_j, and the column's mask
            float H = kNegBig, mask = -__builtin_inff();
            if (col >= 0) {
                const float hj = prm.h[(long)b * M + col];
                H = __builtin_fmaf(-0.5f * prm.s2, lds.xk.scal[kXkRows + tid], hj * kLog2e);
                if (hj != -__builtin_inff()) mask = 0.f;
            }
            if (H2) H = __builtin_fmaxf(H, kH2Floor);
            lds.xk.scal[kXkRows + tid] = H;
            lds.xk.v[tid] = mask;
        }

        const bool wave_on = wave_rows && wc * kXkCG < ncg;
        // ---- exponent half, then the weight half through the same stage buffer: no scalar on either side, no centre, unit scale.  The
        // column scalars are last read before the second barrier of the exponent half's last stage, and the weight half opens with a barrier
        f32x16 acc[kXkRT][kXkCG], tau[kXkRT][kXkCG];
        xk_exponent_blocks<T, L, false>(lds.xk, xb, yb, centre, D, NM, NG, nr32, ncg, xscale, yscale, wave_on, wr, wc, half, l31, tid, acc);
        if (tid < ncg * 32) lds.xk.scal[kXkRows + tid] = 0.f;
        xk_exponent_blocks<float, XL_BF16X3, false, false>(lds.xk, rfb, cfb, nullptr, K, NMK, NGK, nr32, ncg, 1.f, 1.f, wave_on, wr, wc, half, l31, tid, tau);
        if (!wave_on) continue;

        // ---- plan half: the products of this wavefront's 2 x 2 blocks times the tile's centred coordinates ----
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) {
#pragma unroll
            for (int cg = 0; cg < kXkCG; ++cg) {
                const int G = wc * kXkCG + cg;
                if (G >= ncg) continue;
                // register r <-> column reg_column(r, half) of the group: four broadcast 16-byte reads of the mask
                f32x16& u = acc[rt][cg];
                const f32x16& tb = tau[rt][cg];
                const float* mk = &lds.xk.v[G * 32 + half * 4];
                float bm = kMinusHuge, bq = kMinusHuge;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 k4 = *reinterpret_cast<const float4*>(mk + q * 8);
                    const float kv[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float uu = (u[4 * q + r] + cst[rt]) + kv[r];
                        u[4 * q + r] = uu;
                        bm = fmaxf(bm, uu);
                        bq = fmaxf(bq, uu + fast_log2(__builtin_fabsf(tb[4 * q + r])));      // tau == 0 or no mass: -inf
                    }
                }
                bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
                bq = fmaxf(bq, __shfl_xor(bq, 32, 64));
                if (__any(bm > m[rt])) {                      // plan_rescale for the mass alone
                    const float mn = fmaxf(m[rt], bm);
                    const float rs = fast_exp2(m[rt] - mn);
#pragma unroll
                    for (int k = 0; k < 4; ++k) mass4[rt][k] *= rs;
                    m[rt] = mn;
                }
                plan_rescale(bq, mq[rt], pacc[rt], w4[rt]);
                Pack16h whi[2], wlo[2];
#pragma unroll
                for (int k = 0; k < 16; k += 2) {
                    f32x2_t qq;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        mass4[rt][(k & 3) + e] += fast_exp2(u[k + e] - m[rt]) * (float)(1 << kWqShift);
                        const float ex = fast_exp2(__builtin_fminf(u[k + e] - mq[rt], kBilinearMaxLift)) * (float)(1 << kWqShift);
                        qq[e] = (ex > 0.f) ? tb[k + e] * ex : 0.f;      // no weight: exactly 0, whatever tau holds
                        w4[rt][(k & 3) + e] += qq[e];
                    }
                    plan_split_weights(qq, k, whi, wlo);
                }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const f32x16 t = plan_chunk_mfma(&lds.q[G * kQRecs + ch * (4 * 64) + lane], whi, wlo);
                    // register r <-> coordinate reg_feature(r, half) of the chunk: four broadcast 16-byte reads of the inverse scales
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

    // ---- T = S - (x_i - centre) W, then the two column halves of the workgroup meet in LDS (the stage buffer is free now):
    // [T | W | mass | mq | m][row] ----
    __syncthreads();
    float* mrg = reinterpret_cast<float*>(lds.xk.buf);
    float mass[kXkRT], ws[kXkRT];
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt) {
        float s = (mass4[rt][0] + mass4[rt][1]) + (mass4[rt][2] + mass4[rt][3]);
        float w = (w4[rt][0] + w4[rt][1]) + (w4[rt][2] + w4[rt][3]);
        s += __shfl_xor(s, 32, 64);                          // the two 16-column halves
        w += __shfl_xor(w, 32, 64);
        mass[rt] = s * (1.0f / (float)(1 << kWqShift));      // relative to 2^m
        ws[rt] = w * (1.0f / (float)(1 << kWqShift));        // relative to 2^mq
        const int r_local = wr * (kXkRT * 32) + rt * 32 + l31;
        const int i = min(row0 + r_local, row_end - 1);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * ch + reg_feature(r, half);
                float xc = 0.f;
                if (c < prm.nv) xc = to_f32<T>(xb[(long)i * D + prm.v0 + c]) - to_f32<T>(centre[prm.v0 + c]);
                pacc[rt][ch][r] = __builtin_fmaf(-xc, ws[rt], pacc[rt][ch][r]);
            }
        }
        if (wc == 1) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mrg[(32 * ch + reg_feature(r, half)) * kXkRows + r_local] = pacc[rt][ch][r];
            }
            if (half == 0) {
                mrg[VC * kXkRows + r_local] = ws[rt];
                mrg[(VC + 1) * kXkRows + r_local] = mass[rt];
                mrg[(VC + 2) * kXkRows + r_local] = mq[rt];
                mrg[(VC + 3) * kXkRows + r_local] = m[rt];
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
        // the halves are brought to the larger mq and the larger m (factor exactly 1 for the half that holds it, 0 for a half without
        // mass), then the signed sums to the scale of the mass
        const float mq2 = mrg[(VC + 2) * kXkRows + r_local], m2 = mrg[(VC + 3) * kXkRows + r_local];
        const float mqn = fmaxf(mq[rt], mq2), mn = fmaxf(m[rt], m2);
        const float lift = fast_exp2(__builtin_fminf(mqn - mn, 126.f));      // (finite: it meets factors that are exactly 0)
        const float rq1 = fast_exp2(mq[rt] - mqn) * lift, rq2 = fast_exp2(mq2 - mqn) * lift;
        const float rs1 = fast_exp2(m[rt] - mn), rs2 = fast_exp2(m2 - mn);
        const float w = __builtin_fmaf(mrg[(VC + 1) * kXkRows + r_local], rs2, mass[rt] * rs1);
        const float W = __builtin_fmaf(mrg[VC * kXkRows + r_local], rq2, ws[rt] * rq1);
        const long idx = (long)b * N + i;
        float* orow = prm.out + idx * D + prm.v0;
        float* part = sp.workspace + split * sp.split_stride + idx * (prm.nv + 3);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * ch + reg_feature(r, half);
                if (c < prm.nv) {
                    const float s = __builtin_fmaf(mrg[c * kXkRows + r_local], rq2, pacc[rt][ch][r] * rq1);
                    if (ns > 1) part[c] = s;
                    else orow[c] = (w > 0.f) ? s / w : 0.f;
                }
            }
        }
        if (half == 0) {
            if (ns > 1) {
                part[prm.nv] = W;
                part[prm.nv + 1] = w;
                part[prm.nv + 2] = mn;
            } else if (prm.wsum && prm.v0 == 0) {
                prm.wsum[idx] = (w > 0.f) ? W / w : 0.f;
            }
        }
    }
}

}  // namespace glhip
