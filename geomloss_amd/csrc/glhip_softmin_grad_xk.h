// glhip_softmin_grad_xk.h — the gradient of a p = 2 soft-min with respect to the row points on the matrix cores, 17 <= D <= 4095:
//
//     grad_x[i][d] = g_i ( x_i[d] - sum_j w_ij y_j[d] / sum_j w_ij ),      w_ij as in glhip_plan_apply_xk.h
//
// i.e. the transport plan applied to the column cloud itself.  xk_grad_kernel is xk_plan_kernel (glhip_plan_apply_xk.h) with three
// differences; everything else — the exponent half, the weights relative to the running row maximum times 2^kWqShift, the mass from
// the fp32 weights, the two f16 pieces under a power-of-two scale per feature column and tile, six MFMAs per chunk into a fresh
// accumulator per 32-column block, the meeting of the two column halves — is that kernel's, restated.
//
//   features   feature c of a pass that starts at coordinate v0 is to_f32(y[j][v0 + c]) - to_f32(centre[v0 + c]), read in the cloud's
//              dtype: no feat pointer, no fp32 copy of a bf16 cloud.  centre = the first row of the row block, which the exponent half
//              centres on already.  Centred features keep x_i - ybar_i free of cancellation for clouds far from the origin: both
//              terms of the epilogue are of the size of the cloud's diameter.
//   epilogue   unsplit launches write grad_x[b][i][v0 + c] = g_i ((x_i[c] - centre[c]) - s / w); 0 for a row without mass (w == 0).
//              The division stays a division: a one-hot plan row gives x_i - y_j exactly.
//   splits     partials (sums of nv centred features, mass, m) as in the plan kernels; xk_grad_merge_kernel brings the splits to the
//              largest m, adds, divides and applies the same epilogue — the centre row of row i is (i / kXkRows) kXkRows of its batch item.
//
// A pass covers 64 coordinates (NCH = 2), a remainder of <= 32 runs as NCH = 1: ceil(D / 64) passes, each with its own exponent half.
//   registers / LDS / scratch (gfx950, tools/kernel_resources.py, profiles/softmin_grad_xk.txt): see that file; 0 bytes of scratch in
//   all eight instantiations, LDS as xk_plan_kernel (95.1 / 111.5 KiB).
//
// Kept in step by hand: this body duplicates xk_plan_kernel's (a mode parameter there would have to leave the resources of its eight
// instantiations untouched; a copy does so by construction), whose stage loop in turn restates xk_fwd_kernel's.
#pragma once

#include "glhip_plan_apply_xk.h"

namespace glhip {

template <typename T>
struct XkGradParams {
    const T* x;           // (B,N,D)
    const T* y;           // (B,M,D)
    const float* h;       // (B,M)
    const float* fwd;     // (B,N): the saved soft-min
    const float* g;       // (B,N): the incoming gradient
    float* gx;            // (B,N,D)
    float s2;             // log2(e) / eps
    float out_scale;      // -eps ln 2: LSE2_i = fwd_i / out_scale
    int v0;               // first coordinate of this pass
    int nv;               // coordinates of this pass, <= 32 NCH
};

template <typename T, int NCH, int L>
__global__ void __launch_bounds__(kXkThreads, 2)
xk_grad_kernel(XkGradParams<T> prm, int N, int M, int D, SplitInfo sp) {
    constexpr bool H2 = (L == XL_F16X2);
    constexpr int kItems = H2 ? 8 : 4;                        // items (coordinates) of a 24-slot group
    constexpr int kLead = H2 ? 2 : 1;                         // items taken by the scalar item
    constexpr int VC = 32 * NCH;
    constexpr int kQRecs = NCH * 4 * 64;                      // feature records per column group
    constexpr int kFItems = (kXkCols / 4) * VC / kXkThreads;  // (column quad, feature) items per thread and tile: 2, 4
    static_assert(NCH == 1 || NCH == 2, "1 or 2 chunks of 32 features per pass");
    static_assert(kFItems * kXkThreads == (kXkCols / 4) * VC, "whole items per thread");
    static_assert((VC + 2) * kXkRows * sizeof(float) <= sizeof(XkLds::buf), "the column halves meet in the stage buffer");
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
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
        const float fw = prm.fwd[(long)b * N + i];
        const float c = -0.5f * prm.s2 * lds.xk.n2row[i - row0] - fw / prm.out_scale;
        cst[rt] = (fw == __builtin_inff()) ? kNegBig : __builtin_fminf(c, -kNegBig);
    }

    int js, je;
    column_interval<false>(none, M, 0, split, ns, js, je);
    int parity = 0;
    for (int j0 = js; j0 < je; j0 += kXkCols, parity ^= 1) {
        const int n = min(kXkCols, je - j0);                  // real columns, in the slots kXkRows .. kXkRows + n - 1
        const int ncg = (n + 31) >> 5;                        // column groups that are packed and multiplied
        const int col = (tid < n) ? j0 + tid : -1;            // this thread's column (tid < kXkCols), -1 = padding
        __syncthreads();                                      // the previous tile (and the row scalars) are settled
        if (tid < kXkCols) lds.xk.idx[kXkRows + tid] = col;
        // features = the centred coordinates v0 .. v0 + nv - 1 of the tile's columns: item (column quad cq, coordinate c of the pass) —
        // c runs fastest, so the loads of a wavefront are contiguous runs of y rows
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
                const f32x2_t v01 = {fv[k][0] * sc, fv[k][1] * sc}, v23 = {fv[k][2] * sc, fv[k][3] * sc};
                const f16x2_t h01 = __builtin_convertvector(v01, f16x2_t), h23 = __builtin_convertvector(v23, f16x2_t);
                const f16x2_t l01 = __builtin_convertvector(v01 - __builtin_convertvector(h01, f32x2_t), f16x2_t);
                const f16x2_t l23 = __builtin_convertvector(v23 - __builtin_convertvector(h23, f32x2_t), f16x2_t);
                const int jj = t & 31;
                const int r = (jj >> 3) << 2, hq = (jj >> 2) & 1;
                uint2* qb = reinterpret_cast<uint2*>(&lds.q[(t >> 5) * kQRecs + (c >> 5) * (4 * 64) + (r >> 3) * 64 + hq * 32 + (c & 31)]) + ((r & 7) >> 2);
                // [piece][instruction][lane]: 128 records = 256 uint2 per piece
                qb[0] = uint2{__builtin_bit_cast(uint32_t, h01), __builtin_bit_cast(uint32_t, h23)};
                qb[256] = uint2{__builtin_bit_cast(uint32_t, l01), __builtin_bit_cast(uint32_t, l23)};
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
        f32x16 acc[kXkRT][kXkCG];
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt)
#pragma unroll
            for (int cg = 0; cg < kXkCG; ++cg) acc[rt][cg] = zero16;

        const int npts = nr32 + ncg * 32;
        for (int g0 = 0; g0 < NG; g0 += kXkStageGroups) {
            __syncthreads();                                  // the previous stage is consumed (first stage: the scalars are written)
            // ---- split: work item = (point, group of the stage), as xk_fwd_kernel ----
            for (int t = tid; t < npts * kXkStageGroups; t += kXkThreads) {
                const int pt = t / kXkStageGroups, gi = t % kXkStageGroups;
                const int g = g0 + gi;
                if (g >= NG) continue;
                const bool isrow = pt < nr32;
                const int slot = isrow ? pt : kXkRows + (pt - nr32);
                const int i = lds.xk.idx[slot];
                const T* p = (isrow ? xb : yb) + (long)max(i, 0) * D;
                const float scale = isrow ? xscale : yscale;
                const int d0 = kItems * g - kLead;
                const float sc = lds.xk.scal[slot];
                uint32_t w[2][6];
                auto half_group = [&](auto hsel) {            // items d0 + kItems / 2 * HALF ... of the point -> six dwords
                    constexpr int HALF = decltype(hsel)::value;
                    float val[kItems / 2];
#pragma unroll
                    for (int q = 0; q < kItems / 2; ++q) {
                        const int d = d0 + HALF * (kItems / 2) + q;
                        val[q] = (d >= 0 && d < D && i >= 0) ? (to_f32<T>(p[d]) - to_f32<T>(centre[d])) * scale : 0.f;
                    }
                    if (isrow) xk_pack_half<true, L, HALF>(g == 0, sc, val, w[HALF]);
                    else xk_pack_half<false, L, HALF>(g == 0, sc, val, w[HALF]);
                };
                half_group(std::integral_constant<int, 0>{});
                half_group(std::integral_constant<int, 1>{});
                const uint4 rec[3] = {uint4{w[0][0], w[0][1], w[0][2], w[0][3]}, uint4{w[0][4], w[0][5], w[1][0], w[1][1]},
                                      uint4{w[1][2], w[1][3], w[1][4], w[1][5]}};
                uint4* dst = &lds.xk.buf[((slot >> 5) * kXkStageRecs + 3 * gi) * kXkRecStride + (slot & 31)];
#pragma unroll
                for (int r = 0; r < 3; ++r) dst[r * kXkRecStride] = rec[r];
            }
            __syncthreads();
            // ---- multiply: K chunk c of the stage = records 2 c (lane half 0) and 2 c + 1 (half 1) ----
            if (wave_on) {
                const int nch = min(kXkStageChunks, NM - (g0 / kXkStageGroups) * kXkStageChunks);
                const uint4* rbase = &lds.xk.buf[((wr * kXkRT) * kXkStageRecs + half) * kXkRecStride + l31];
                const uint4* cbase = &lds.xk.buf[((kXkRows / 32 + wc * kXkCG) * kXkStageRecs + half) * kXkRecStride + l31];
#pragma unroll
                for (int c = 0; c < kXkStageChunks; ++c) {
                    if (c < nch) {
                        uint4 X[kXkRT], Y[kXkCG];
#pragma unroll
                        for (int rt = 0; rt < kXkRT; ++rt) X[rt] = rbase[(rt * kXkStageRecs + 2 * c) * kXkRecStride];
#pragma unroll
                        for (int cg = 0; cg < kXkCG; ++cg) Y[cg] = cbase[(cg * kXkStageRecs + 2 * c) * kXkRecStride];
#pragma unroll
                        for (int rt = 0; rt < kXkRT; ++rt)
#pragma unroll
                            for (int cg = 0; cg < kXkCG; ++cg)
                                acc[rt][cg] = H2 ? mfma_h32(Y[cg], X[rt], acc[rt][cg]) : mfma_x32(Y[cg], X[rt], acc[rt][cg]);
                    }
                }
            }
        }
        if (!wave_on) continue;

        // ---- plan half: the weights of this wavefront's 2 x 2 blocks times the tile's features (column groups >= ncg were not packed) ----
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) {
#pragma unroll
            for (int cg = 0; cg < kXkCG; ++cg) {
                const int G = wc * kXkCG + cg;
                if (G >= ncg) continue;
                // register r <-> column 8 (r >> 2) + 4 half + (r & 3) of the group: four broadcast 16-byte reads of the mask
                f32x16 u;
                const float* mk = &lds.xk.v[G * 32 + half * 4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 k4 = *reinterpret_cast<const float4*>(mk + q * 8);
                    u[4 * q + 0] = (acc[rt][cg][4 * q + 0] + cst[rt]) + k4.x;
                    u[4 * q + 1] = (acc[rt][cg][4 * q + 1] + cst[rt]) + k4.y;
                    u[4 * q + 2] = (acc[rt][cg][4 * q + 2] + cst[rt]) + k4.z;
                    u[4 * q + 3] = (acc[rt][cg][4 * q + 3] + cst[rt]) + k4.w;
                }
                // weights relative to the running maximum of the row: w' = 2^13 2^(u - m) <= 8192 whatever fwd is worth, and the largest
                // weight of a row is 2^13 EXACTLY.  A new maximum rescales the running sums (factor exactly 1 for the rows that keep theirs)
                float bm = max16(u);
                bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
                if (__any(bm > m[rt])) {
                    const float mn = fmaxf(m[rt], bm);
                    const float rs = fast_exp2(m[rt] - mn);
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) pacc[rt][ch][r] *= rs;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) mass4[rt][k] *= rs;
                    m[rt] = mn;
                }
                Pack16h whi[2], wlo[2];
#pragma unroll
                for (int k = 0; k < 16; k += 2) {      // pairs: one v_cvt_pk_f16_f32 per two high pieces, both read back from it
                    const f32x2_t w = {fast_exp2(u[k] - m[rt]) * (float)(1 << kWqShift), fast_exp2(u[k + 1] - m[rt]) * (float)(1 << kWqShift)};
                    mass4[rt][k & 3] += w[0];
                    mass4[rt][(k & 3) + 1] += w[1];
                    const f16x2_t hh = __builtin_convertvector(w, f16x2_t);
                    const f32x2_t back = __builtin_convertvector(hh, f32x2_t);
                    const f16x2_t ll = __builtin_convertvector(w - back, f16x2_t);
                    whi[k >> 3].v[k & 7] = hh[0];
                    whi[k >> 3].v[(k & 7) + 1] = hh[1];
                    wlo[k >> 3].v[k & 7] = ll[0];
                    wlo[k >> 3].v[(k & 7) + 1] = ll[1];
                }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const uint4* qg = &lds.q[G * kQRecs + ch * (4 * 64) + lane];      // piece p, instruction I: qg[p * 128 + I * 64]
                    Pack16h qh0, qh1, ql0, ql1;
                    qh0.u = qg[0]; qh1.u = qg[64]; ql0.u = qg[128]; ql1.u = qg[192];
                    // smallest products first: lo hi, hi lo, hi hi
                    f32x16 t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ql0.v, whi[0].v, zero16, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ql1.v, whi[1].v, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh0.v, wlo[0].v, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh1.v, wlo[1].v, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh0.v, whi[0].v, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh1.v, whi[1].v, t, 0, 0, 0);
                    // register r <-> feature (r & 3) + 8 (r >> 2) + 4 half of the chunk: four broadcast 16-byte reads of the inverse scales
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
                for (int r = 0; r < 16; ++r) mrg[(32 * ch + (r & 3) + 8 * (r >> 2) + 4 * half) * kXkRows + r_local] = pacc[rt][ch][r];
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
        const T* xrow = xb + (long)i * D + prm.v0;
        float* orow = prm.gx + idx * D + prm.v0;
        float* part = sp.workspace + split * sp.split_stride + idx * (prm.nv + 2);
        const float gi = (ns == 1) ? prm.g[idx] : 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * ch + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (c < prm.nv) {
                    const float s = __builtin_fmaf(mrg[c * kXkRows + r_local], rs2, pacc[rt][ch][r] * rs1);
                    if (ns == 1) {      // g_i ((x_i - centre) - ybar_i): a division, exact where the quotient is; a row without mass gets 0
                        const float xc = to_f32<T>(xrow[c]) - to_f32<T>(centre[prm.v0 + c]);
                        orow[c] = (w > 0.f) ? gi * (xc - s / w) : 0.f;
                    } else {
                        part[c] = s;
                    }
                }
            }
        }
        if (half == 0 && ns > 1) {
            part[prm.nv] = w;
            part[prm.nv + 1] = mn;
        }
    }
}

// Combines the column splits of a gradient pass: one thread per (row, coordinate).  The partials of a row are nv sums of centred
// coordinates and the mass — both relative to 2^m of their split — and m (plan_merge_kernel's format): brought to the largest m, added,
// divided, and put through the epilogue of xk_grad_kernel.
template <typename T>
__global__ void __launch_bounds__(kBlock)
xk_grad_merge_kernel(XkGradParams<T> prm, int N, int D, long rows, SplitInfo sp) {
    const long id = (long)blockIdx.x * kBlock + threadIdx.x;
    const int nv = prm.nv;
    if (id >= rows * nv) return;
    const long row = id / nv;
    const int c = (int)(id - row * nv);
    const float* part = sp.workspace + row * (nv + 2);
    float mx = kMinusHuge;
    for (int k = 0; k < sp.n_splits; ++k) mx = fmaxf(mx, part[k * sp.split_stride + nv + 1]);
    float s = 0.f, w = 0.f;
    for (int k = 0; k < sp.n_splits; ++k) {
        const float rs = fast_exp2(part[k * sp.split_stride + nv + 1] - mx);
        s = __builtin_fmaf(part[k * sp.split_stride + c], rs, s);
        w = __builtin_fmaf(part[k * sp.split_stride + nv], rs, w);
    }
    const long i = row % N;
    const long crow = row - i + (i / kXkRows) * kXkRows;      // the first row of the row block, within the batch item
    const float xc = to_f32<T>(prm.x[row * D + prm.v0 + c]) - to_f32<T>(prm.x[crow * D + prm.v0 + c]);
    prm.gx[row * D + prm.v0 + c] = (w > 0.f) ? prm.g[row] * (xc - s / w) : 0.f;
}

}  // namespace glhip
