// glhip_softmin_xk.h — the K-chunked matrix-core reductions for clouds of dimension 17 <= D <= 4095, p = 2: soft-min forward (incl.
// the fused Sinkhorn half-step) and gaussian kernel product, float32 / bfloat16 clouds, dense / batched / block-sparse launches.
//
// The exponent of a pair is the same short dot product as in glhip_softmin_xd.h — the scalar item ([H1,H2,H3,1,1,1] against
// [1,1,1,n1,n2,n3]) followed by six K slots per coordinate on bf16 x 3 (three on f16 x 2, GLHIP_FLAG_F16X2), pieces and slot order
// of glhip_klayout.h — but D is a RUN-TIME argument and neither side's operands are resident for the whole of D: at D = 128 a point
// is 49 chained MFMAs = 98 records of 16 bytes.  Instead a workgroup owns a block of 256 rows x 128 columns of exponents at a time
// and sweeps the K dimension in STAGES of 6 MFMAs (96 slots = 12 records per point); the 32 x 32 exponent blocks live in the
// MFMA's C operand (float32) from the first stage to the last.
//
//   workgroup = 8 wavefronts as 4 (rows) x 2 (columns); a wavefront owns 2 row tiles x 2 column groups of 32 = four accumulators
//   (64 VGPRs) and reads 2 + 2 records per K chunk for its 4 MFMAs: ONE ds_read_b128 per v_mfma_f32_32x32x16 (LDS sets the pace
//   from two on).
//   stage: all 512 threads split the (up to) 384 points of the block into pieces for the 12 records of the stage — a work item is
//   one point x one GROUP of 3 records = 24 slots = 4 coordinates (8 on f16 x 2): every coordinate is loaded and split once —
//   barrier, 6 K chunks of MFMAs, barrier.  The rows are re-split for every column tile (the price of staging on the fly: 384
//   points split per 32768 pairs and stage); a second resident workgroup per CU overlaps its MFMAs with this one's VALU work.
//   (xk_exponent_blocks below: the one stage loop of this kernel, xk_plan_kernel and argmin_xk_kernel.)
//   LDS: 12 point groups x 12 records x 33 (32 + 1 pad: the 3-record groups of a point land on different banks) x 16 B = 74.25 KiB
//   + 4.5 KiB of indices / scalars = 78.75 KiB: two workgroups per CU (157.5 of 160 KiB), 4 wavefronts per SIMD (<= 128 VGPRs).
//
// The scalar item comes first (slots 0..5), coordinate d takes slots 6 + kPer d ...; in 24-slot groups, with the scalar item
// counted as item 0 (bf16 x 3: one six-slot item; f16 x 2: two three-slot items), group g holds items 4 g .. 4 g + 3
// (coordinates 4 g - 1 .. 4 g + 2), resp. items 8 g .. 8 g + 7 (coordinates 8 g - 2 .. 8 g + 5).  NM = ceil((6 + kPer D) / 16)
// MFMAs per block; ceil(2 NM / 3) groups are packed (slots past the last coordinate are zero).
//
// Points are centred on the first row of the row block before they are split; |xt|^2, |yt|^2 are float32 FMA chains (four
// interleaved chains per point, summed pairwise).  Soft-min: the x-side scalar is 0 and r_i = -s/2 |xt_i|^2 joins after the reduction,
// as in glhip_softmin_xd.h; gaussian: n = r_i.  The running maximum is EXPLICIT: after the last stage of a column tile a wavefront
// takes the maximum of its 2 x 32 x 32 exponents per row and rescales the row's sum only when the maximum grew (there is no
// speculative pass to redo: the epilogue is 16 max + 16 sub + 16 exp + 16 add per block against NM >= 7 MFMAs).  -inf duals give
// -inf exponents (weight 0); padded columns carry -1e30 (f16 x 2: the floor -5e5, and a row that never left the floor has an empty
// sum), exactly as xd_fwd_kernel.
//
// Error of an exponent, run-time D (restating glhip_softmin_xd.h): per coordinate the two dropped products are <= 2^-25 |a y|
// each (bf16 x 3; f16 x 2: the dropped lo lo <= 2^-22 |a y|), so the dropped terms sum to <= 2^-24 sum_d |a_d y_d| <= 2^-24 s |xt| |yt|
// (Cauchy-Schwarz), whatever D is; the float32 accumulation in the MFMA chain adds <= NM + 3 roundings of the partial sums, each
// <= 2^-24 max(|H_j|, s |xt| |yt|) — products inside one MFMA are summed before they are rounded, so the chain is ~D / 2.7
// roundings long (bf16 x 3), not 6 D.  With xt, yt at most one diameter long and |H_j| ~ s/2 diam^2 that is
// ~2^-24 (NM + 5) s diam^2 worst case and ~sqrt(NM) 2^-24 s diam^2 typically; in units of a potential (x eps ln 2 / log2 e):
// ~sqrt(D / 2.7) 2^-24 diam^2, against the test bound 4e-7 D + 2e-6 max|f| with diam^2 <= D.
//
// Cost model: NM MFMAs of 32 cycles per 1024 pairs per SIMD (25 at D = 64, 49 at D = 128) against ~128 D issue cycles for the
// one-thread-per-row kernel of glhip_generic.h; on top, the splitting: ~20 VALU instructions per coordinate and point, 384 points
// per 32768 pairs.  Measured (profiles/r08_anyd.txt): 4.9-5.05x the generic kernel at D = 32 ... 256, not the modelled ~10x; at D = 64
// the matrix pipe is 14 % busy, the VALU 43 %, and the wavefronts wait for 70 % of their cycles — the barriers of the staging, the
// latency of the D-strided loads of the split loop and bank conflicts on its LDS writes, not either pipe.
#pragma once

#include "glhip_softmin_xd.h"

namespace glhip {

constexpr int kXkMinD = 17, kXkMaxD = 4095;
constexpr int kXkRT = 2, kXkCG = 2;                      // row tiles x column groups of a wavefront
constexpr int kXkWR = 4, kXkWC = 2;                      // wavefronts of a workgroup: rows x columns
constexpr int kXkNW = kXkWR * kXkWC;
constexpr int kXkThreads = kXkNW * 64;
constexpr int kXkRows = kXkWR * kXkRT * 32;              // 256
constexpr int kXkCols = kXkWC * kXkCG * 32;              // 128
constexpr int kXkPts = kXkRows + kXkCols;
constexpr int kXkStageChunks = 6;                        // MFMAs (K chunks of 16 slots) per stage
constexpr int kXkStageRecs = 2 * kXkStageChunks;         // records per point and stage
constexpr int kXkStageGroups = kXkStageRecs / 3;         // 24-slot groups per point and stage
constexpr int kXkRecStride = 33;                         // records between consecutive records of a point group (32 points + 1 pad)
constexpr int kXkBufRecs = (kXkPts / 32) * kXkStageRecs * kXkRecStride;

// chained MFMAs of one exponent block and 24-slot groups to pack (host and device)
__host__ __device__ inline int xk_num_mfma(int D, int layout) { return (6 + (layout == XL_F16X2 ? 3 : 6) * D + 15) / 16; }
__host__ __device__ inline int xk_num_groups(int D, int layout) { return (2 * xk_num_mfma(D, layout) + 2) / 3; }

// Half a 24-slot group (records 3 g .. 3 g + 2 of a point) from the values of its items, as six packed dwords: slots 12 HALF ..
// 12 HALF + 11.  bf16 x 3: two six-slot items per half, v[q] = value of item 4 g + 2 HALF + q; f16 x 2: four three-slot items,
// item 8 g + 4 HALF + q.  `first` (g == 0, HALF == 0): the leading six slots are the scalar item of `scalar` instead (v[0], resp.
// v[0] and v[1], are not used).
template <bool XSIDE, int L, int HALF>
__device__ __forceinline__ void xk_pack_half(bool first, float scalar, const float (&v)[L == XL_F16X2 ? 4 : 2], uint32_t (&w)[6]) {
    uint32_t h[12];
    if constexpr (L == XL_F16X2) {
        uint32_t sc[3] = {0u, 0u, 0u};
        if (HALF == 0) split3_h(scalar * (1.0f / kH2Kappa), sc);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t p[2];
            split2_h(v[q], p);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int slot = 3 * q + t;
                uint32_t hv = p[xd_piece_at<XSIDE, L>(t)];
                if (HALF == 0 && slot < 6) {      // [k,k,k,n1,n2,n3] | [H1,H2,H3,k,k,k]
                    const bool one = XSIDE ? slot < 3 : slot >= 3;
                    const uint32_t hs = one ? kF16Kappa : sc[XSIDE ? slot - 3 : slot];
                    hv = first ? hs : hv;
                }
                h[slot] = hv;
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint32_t p[3];
            split3_rn((HALF == 0 && q == 0 && first) ? scalar : v[q], p);
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                uint32_t hv = p[xd_piece_at<XSIDE, L>(t)];
                if (HALF == 0 && q == 0) {        // [1,1,1,n1,n2,n3] | [H1,H2,H3,1,1,1]
                    const bool one = XSIDE ? t < 3 : t >= 3;
                    const uint32_t hs = one ? kBf16One : p[XSIDE ? t - 3 : t];
                    hv = first ? hs : hv;
                }
                h[6 * q + t] = hv;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = h[2 * k] | (h[2 * k + 1] << 16);
}

// LDS of a workgroup
struct XkLds {
    uint4 buf[kXkBufRecs];        // [point group: 8 of rows, 4 of columns][record of the stage][33]
    int idx[kXkPts];              // global point index of a slot (rows: clamped to the last row of the block; columns: -1 = padding)
    float n2row[kXkRows];         // |xt_i|^2
    float scal[kXkPts];           // scalar of a slot: n_i (rows: 0 | r_i), H_j (columns)
    float v[kXkCols];             // gaussian product: weights of the column tile
};

// |p - c|^2 of `count` slots starting at slot0 (count a multiple of 16): four threads per point, interleaved float32 FMA chains
template <typename T>
__device__ __forceinline__ void xk_norms(const T* __restrict__ pts, const T* __restrict__ centre, int D, const int* idx, int slot0, int count,
                                         float* out, int tid) {
    for (int t = tid; t < count * 4; t += kXkThreads) {
        const int s = t >> 2, sub = t & 3;
        const int i = idx[slot0 + s];
        float n2 = 0.f;
        if (i >= 0) {
            const T* p = pts + (long)i * D;
            for (int d = sub; d < D; d += 4) {
                const float w = to_f32<T>(p[d]) - to_f32<T>(centre[d]);
                n2 = __builtin_fmaf(w, w, n2);
            }
        }
        n2 += __shfl_xor(n2, 1, 64);
        n2 += __shfl_xor(n2, 2, 64);
        if (sub == 0) out[s] = n2;
    }
}

// The exponent blocks of one column tile: zeroes a wavefront's 2 x 2 accumulators and sweeps the K dimension in stages.  The ONE stage
// loop of the D > 16 kernels (xk_fwd_kernel, xk_plan_kernel, argmin_xk_kernel); the caller has written lds.idx and lds.scal of the
// nr32 row slots and of the ncg * 32 column slots of the tile (no barrier needed after: the first stage starts with one).
//   split     all 512 threads; a work item is (point, 24-slot group of the stage), the groups of a point on neighbouring lanes.  The
//             coordinates of the group — kItems of them, less the kLead items the scalar item takes in group 0 — are loaded, centred,
//             scaled (xscale for rows, yscale for columns; argmin passes 1), split by xk_pack_half and written as three records.
//             SCHED puts a sched_barrier between the two half groups of f16 x 2: eight coordinates in flight at once cost xk_fwd_kernel
//             its 128-VGPR budget; the other kernels have no such budget and leave it out.
//   multiply  wavefronts with wave_on; K chunk c of the stage = records 2 c (lane half 0) and 2 c + 1 (half 1): 2 + 2 ds_read_b128 for
//             the 4 MFMAs of a chunk, mfma(Y, X, acc) — lane (half, i) ends up with row i for the columns 8 (r / 4) + 4 half + r % 4.
// Keep this a __forceinline__ function called from a __global__ body.  Moving a whole kernel BODY into a device function behind thin
// __global__ wrappers was tried for xk_plan_kernel: +30 VGPRs at NCH = 1 and 112-180 bytes of scratch per lane at NCH = 2.
// CENTRED = false (the weight half of xk_bilinear_kernel, glhip_plan_bilinear_xk.h): the points are taken as they are and `centre` is not read.
template <typename T, int L, bool SCHED, bool CENTRED = true>
__device__ __forceinline__ void xk_exponent_blocks(XkLds& lds, const T* __restrict__ xb, const T* __restrict__ yb, const T* __restrict__ centre,
                                                   int D, int NM, int NG, int nr32, int ncg, float xscale, float yscale, bool wave_on, int wr,
                                                   int wc, int half, int l31, int tid, f32x16 (&acc)[kXkRT][kXkCG]) {
    constexpr bool H2 = (L == XL_F16X2);
    constexpr int kItems = H2 ? 8 : 4;                        // items (coordinates) of a 24-slot group
    constexpr int kLead = H2 ? 2 : 1;                         // items taken by the scalar item
#pragma unroll
    for (int rt = 0; rt < kXkRT; ++rt)
#pragma unroll
        for (int cg = 0; cg < kXkCG; ++cg)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[rt][cg][k] = 0.f;

    const int npts = nr32 + ncg * 32;
    for (int g0 = 0; g0 < NG; g0 += kXkStageGroups) {
        __syncthreads();                                      // the previous stage is consumed (first stage: the scalars are written)
        // ---- split ----
        for (int t = tid; t < npts * kXkStageGroups; t += kXkThreads) {
            const int pt = t / kXkStageGroups, gi = t % kXkStageGroups;
            const int g = g0 + gi;
            if (g >= NG) continue;
            const bool isrow = pt < nr32;
            const int slot = isrow ? pt : kXkRows + (pt - nr32);
            const int i = lds.idx[slot];
            const T* p = (isrow ? xb : yb) + (long)max(i, 0) * D;
            const float scale = isrow ? xscale : yscale;
            const int d0 = kItems * g - kLead;
            const float sc = lds.scal[slot];
            uint32_t w[2][6];
            auto half_group = [&](auto hsel) {                // items d0 + kItems / 2 * HALF ... of the point -> six dwords
                constexpr int HALF = decltype(hsel)::value;
                float val[kItems / 2];
#pragma unroll
                for (int q = 0; q < kItems / 2; ++q) {
                    const int d = d0 + HALF * (kItems / 2) + q;
                    if constexpr (CENTRED) val[q] = (d >= 0 && d < D && i >= 0) ? (to_f32<T>(p[d]) - to_f32<T>(centre[d])) * scale : 0.f;
                    else val[q] = (d >= 0 && d < D && i >= 0) ? to_f32<T>(p[d]) * scale : 0.f;
                }
                if (isrow) xk_pack_half<true, L, HALF>(g == 0, sc, val, w[HALF]);
                else xk_pack_half<false, L, HALF>(g == 0, sc, val, w[HALF]);
            };
            half_group(std::integral_constant<int, 0>{});
            if (SCHED && H2) __builtin_amdgcn_sched_barrier(0);
            half_group(std::integral_constant<int, 1>{});
            const uint4 rec[3] = {uint4{w[0][0], w[0][1], w[0][2], w[0][3]}, uint4{w[0][4], w[0][5], w[1][0], w[1][1]},
                                  uint4{w[1][2], w[1][3], w[1][4], w[1][5]}};
            uint4* dst = &lds.buf[((slot >> 5) * kXkStageRecs + 3 * gi) * kXkRecStride + (slot & 31)];
#pragma unroll
            for (int r = 0; r < 3; ++r) dst[r * kXkRecStride] = rec[r];
        }
        __syncthreads();
        // ---- multiply ----
        if (wave_on) {
            const int nch = min(kXkStageChunks, NM - (g0 / kXkStageGroups) * kXkStageChunks);
            const uint4* rbase = &lds.buf[((wr * kXkRT) * kXkStageRecs + half) * kXkRecStride + l31];
            const uint4* cbase = &lds.buf[((kXkRows / 32 + wc * kXkCG) * kXkStageRecs + half) * kXkRecStride + l31];
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
}

template <int MODE, typename T, bool SPARSE, int L>
__global__ void __launch_bounds__(kXkThreads, 4)
xk_fwd_kernel(SoftminParams<T> prm, Ranges rg, int N, int M, int D, SplitInfo sp) {
    constexpr bool H2 = (L == XL_F16X2);
    constexpr float kFloor = H2 ? kH2Floor : kMinusHuge;      // the running maximum of a row that has seen no mass yet
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
    const float xscale = H2 ? __builtin_sqrtf(prm.s2) : prm.s2;
    const float yscale = H2 ? __builtin_sqrtf(prm.s2) : 1.0f;
    const T* xb = prm.x + (long)b * N * D;
    const T* yb = prm.y + (long)b * M * D;

    int row_begin, row_end, q_begin, q_end;
    block_extent<SPARSE>(rg, N, kXkRows, row_begin, row_end, q_begin, q_end, bx);

    for (int row0 = row_begin; row0 < row_end; row0 += kXkRows) {
        const T* centre = xb + (long)row0 * D;
        const int nrows = min(kXkRows, row_end - row0);
        const int nr32 = (nrows + 31) & ~31;                  // row slots that are packed
        __syncthreads();                                      // the previous pass is done with the LDS
        if (tid < kXkRows) lds.idx[tid] = min(row0 + tid, row_end - 1);
        __syncthreads();
        xk_norms<T>(xb, centre, D, lds.idx, 0, kXkRows, lds.n2row, tid);
        __syncthreads();
        if (tid < kXkRows) {
            float nrow = (MODE == XD_SOFTMIN) ? 0.f : -0.5f * prm.s2 * lds.n2row[tid];
            if (H2) nrow = __builtin_fmaxf(nrow, kH2Floor);
            lds.scal[tid] = nrow;
        }

        const int wave_row0 = row0 + wr * (kXkRT * 32);
        const bool wave_rows = wave_row0 < row_end;
        float m[kXkRT], ssum[kXkRT];
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) { m[rt] = kFloor; ssum[rt] = 0.f; }

        // one tile: n real columns in the slots kXkRows .. kXkRows + n - 1; `col` = this thread's column (tid < kXkCols), -1 = padding
        auto tile_body = [&](int n, int col) {
            const int ncg = (n + 31) >> 5;                    // column groups that are packed and multiplied
            __syncthreads();                                  // the previous tile (and the row scalars) are settled
            if (tid < kXkCols) lds.idx[kXkRows + tid] = col;
            __syncthreads();
            xk_norms<T>(yb, centre, D, lds.idx, kXkRows, ncg * 32, &lds.scal[kXkRows], tid);
            __syncthreads();
            if (tid < ncg * 32) {                             // |yt|^2 -> H_j
                float H = kNegBig, vj = 0.f;
                if (col >= 0) {
                    const float n2 = lds.scal[kXkRows + tid];
                    if (MODE == XD_SOFTMIN) {
                        H = __builtin_fmaf(-0.5f * prm.s2, n2, dual_entry(prm, (long)b * M + col) * kLog2e);
                    } else {
                        H = -0.5f * prm.s2 * n2;
                        vj = prm.h[(long)b * M + col];
                    }
                }
                if (H2) H = __builtin_fmaxf(H, kH2Floor);
                lds.scal[kXkRows + tid] = H;
                if (MODE == XD_GAUSS) lds.v[tid] = vj;
            }

            const bool wave_on = wave_rows && wc * kXkCG < ncg;
            f32x16 acc[kXkRT][kXkCG];
            xk_exponent_blocks<T, L, true>(lds, xb, yb, centre, D, NM, NG, nr32, ncg, xscale, yscale, wave_on, wr, wc, half, l31, tid, acc);
            if (!wave_on) return;

            // ---- epilogue: the exponents of this wavefront's 2 x 2 blocks join the row sums (column groups >= ncg were not packed) ----
#pragma unroll
            for (int rt = 0; rt < kXkRT; ++rt) {
                if (MODE == XD_GAUSS) {
#pragma unroll
                    for (int cg = 0; cg < kXkCG; ++cg)
                        if (wc * kXkCG + cg < ncg) ssum[rt] += xd_weighted_sum(acc[rt][cg], &lds.v[(wc * kXkCG + cg) * 32 + half * 4]);
                } else {
                    float um = kFloor;
#pragma unroll
                    for (int cg = 0; cg < kXkCG; ++cg)
                        if (wc * kXkCG + cg < ncg) um = fmaxf(um, max16(acc[rt][cg]));
                    um = fmaxf(um, __shfl_xor(um, 32, 64));
                    if (um > m[rt]) {                         // lazy: rescale only when the maximum grew
                        ssum[rt] *= fast_exp2(m[rt] - um);
                        m[rt] = um;
                    }
#pragma unroll
                    for (int cg = 0; cg < kXkCG; ++cg)
                        if (wc * kXkCG + cg < ncg) ssum[rt] += sum_exp2_16(acc[rt][cg], m[rt]);
                }
            }
        };

        if (SPARSE) {
            // the concatenation of the column intervals of the row block, gathered into tiles when the clusters are small
            // (SplitInfo::gather), as xd_fwd_kernel
            TileCursor cur;
            cur.q = q_begin + split;
            cur.j0 = cur.je = 0;
            open_interval<true, true>(rg, M, q_end, split, ns, cur);
            const int pieces = sp.gather ? kXkCols : 1;
            while (cur.q < q_end) {
                int gcols[1], n = 0;
                const TileCursor nxt = gather_tile<1, kXkThreads, kXkCols>(rg, M, q_end, split, ns, cur, tid, gcols, n, pieces);
                tile_body(n, (tid < n) ? gcols[0] : -1);
                cur = nxt;
            }
        } else {
            int js, je;
            column_interval<false>(rg, M, 0, split, ns, js, je);
            for (int j0 = js; j0 < je; j0 += kXkCols) {
                const int n = min(kXkCols, je - j0);
                tile_body(n, (tid < n) ? j0 + tid : -1);
            }
        }

        // ---- the two column halves of the workgroup meet in LDS (the tile buffer is free now): [wc][row] of (m, s) ----
        __syncthreads();
        float* mrg = reinterpret_cast<float*>(lds.buf);
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) {
            float s = ssum[rt] + __shfl_xor(ssum[rt], 32, 64);      // the lane halves hold the two 16-column halves of every block
            // XL_F16X2: a row still at the floor has seen padded / massless columns only (2^0 each): its sum is empty
            if (H2 && MODE == XD_SOFTMIN && m[rt] <= kH2Floor * 0.98f) s = 0.f;
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
                if (MODE == XD_GAUSS) {
                    s += s2;
                } else {
                    const float mn = fmaxf(mt, m2);
                    s = s * fast_exp2(mt - mn) + s2 * fast_exp2(m2 - mn);
                    mt = mn;
                }
            }
            const long idx = (long)b * N + row0 + tid;
            if (MODE == XD_GAUSS) {
                if (ns == 1) prm.out[idx] = s;
                else sp.workspace[split * sp.split_stride + idx] = s;
            } else {
                const float mtot = __builtin_fmaf(-0.5f * prm.s2, lds.n2row[tid], mt);      // r_i + m
                if (ns == 1) {
                    prm.out[idx] = finish_value(prm, idx, mtot + fast_log2(s));
                } else {
                    float* dst = sp.workspace + split * sp.split_stride + idx * 2;
                    dst[0] = mtot;
                    dst[1] = s;
                }
            }
        }
    }
}

}  // namespace glhip
