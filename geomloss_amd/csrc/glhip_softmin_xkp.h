// glhip_softmin_xkp.h — the Sinkhorn iteration on PRE-PACKED operands for clouds of dimension 17 <= D <= 4095, p = 2: up to four dense
// soft-min half-steps in one launch (glhip_sinkhorn_iter4 / glhip_sinkhorn_anneal), float32 / bfloat16 clouds, batched or not.
//
// Why a second kernel next to glhip_softmin_xk.h.  xk_fwd_kernel splits every float32 coordinate of its rows and columns into bf16
// pieces on the VALU for every column tile, with the temperature baked into the pieces, and owns 256 rows: a loop on two clouds of a few
// thousand points launches it 4 (n_eps + 2) times on 8 row blocks each and spends its time splitting the same points again.  Nothing
// about the pieces changes between those reductions but the temperature, and the temperature need not be in the pieces:
//     u_ij = s (xt_i . yt_j) + H_j + r_i,     s = log2(e) / eps,   H_j = log2(e) h_j - s |yt_j|^2 / 2,   r_i = -s |xt_i|^2 / 2,
// so the matrix cores compute the plain dot product of the centred points and ONE FMA per pair makes it an exponent.
//
// Pack kernel (xkp_pack_kernel), once per iter4 call and once per whole anneal call.  Both clouds of a batch item are centred on one
// point, x[b, 0, :] — every centred point is then at most one diameter of the union long, the assumption of the error bound in
// glhip_softmin_xk.h, which carries over: the dropped products and the float32 accumulation are those of that kernel, the scale by s
// moved behind them.  A coordinate is the three bf16 pieces of split3_rn in the six K slots of glhip_klayout.h (xd_piece_at: rows
// [a1,a1,a2,a1,a3,a2], columns [y1,y2,y1,y3,y1,y2]); there is no scalar item and no scale.  A STAGE is 8 coordinates = 48 slots = 3 chained
// v_mfma_f32_32x32x16_bf16 = 6 records of 16 bytes per point, NS = ceil(D / 8) stages, NM = ceil(6 D / 16) MFMAs per 32 x 32 block (the
// last stage has 1 .. 3 of them; slots past the last coordinate are zero).  Records are written in the order the reducing kernel
// consumes them,
//     [batch item][group of 32 points][stage][record 0..5][32 points],
// so that one stage of one point group is one linear block of 3 KiB, and lane l of a wavefront finds its operand of MFMA c of the stage
// at record 64 c + l of that block.  Every cloud is packed in BOTH roles (x and y are rows in two of the four problems and columns in
// the other two); points past the end of the last group are zero.  |xt|^2, |yt|^2: float32 FMA chains, four interleaved per point
// summed pairwise as in xk_norms, stored once per point.
//
// Reducing kernel (xkp_fwd_multi_kernel).  grid = (row blocks of 128, B, splits x problems) as xd_fwd_multi_kernel; problem slots past
// `count` have N = 0.  A workgroup is 4 wavefronts as 2 (rows) x 2 (columns) on a tile of 128 rows x 128 columns, 2 x 2 blocks of
// 32 x 32 per wavefront = 64 accumulator VGPRs.  It walks the flat sequence (column tile, stage): the stage's records of its 4 row
// groups and of the tile's column groups come in by LDS-DMA (glds16, 1 KiB per wavefront instruction, no staging registers) into one
// of two buffers of 8 groups x 3 KiB = 24 KiB while the other is multiplied — ONE barrier per stage, no VALU work on operands, and a
// chunk is 2 + 2 contiguous ds_read_b128 for 4 MFMAs.  After the last stage of a tile the dot products become exponents (16 FMAs per
// block against H_j, which 128 threads wrote to LDS at the tile's first stage from the stored norm, the log-weight and the potential)
// and join the rows' sums under the explicit running maximum of xk_fwd_kernel: 16 max + 16 sub + 16 exp2 + 16 add per block, the sum
// rescaled only when the maximum grew.  -inf duals weigh exactly 0, padded columns carry -1e30, a row that saw no mass keeps the huge
// finite value of the other kernels.  The two column halves meet in LDS; r_i, the fused half-step (finish_value) or the split partial
// (max, sum) of SoftminFwdOp come last.  Column splits are whole tiles' worth of groups of 32; merge_multi_kernel merges them.
//
// LDS: 2 x 24 KiB + 1 KiB of H_j + 2 KiB of (max, sum) = 51 KiB: three workgroups per CU, 3 wavefronts per SIMD (<= 168 VGPRs).  At
// N = M = 2048 with four problems the launch is 16 row blocks x 4 splits x 4 = 256 workgroups.  Resources as the compiler reports them
// (the translation unit prints them with every build): DESIGN.md §4.
//
// Version 147: the body takes the metric as a template parameter.  P = 2 is everything above; P = 1 (GLHIP_FLAG_XK_ITER_DIST) keeps the
// operands, the grid and the stage loop and swaps the epilogue for the distance one of glhip_dist_xkp.h (S_j and N_j in LDS, near-pair
// repair, clamp, square root, one FMA per pair).  Every P = 1 line sits under `if constexpr`: the P = 2 report above did not move.
#pragma once

#include "glhip_dist_xkp.h"
#include "glhip_softmin_xk.h"

namespace glhip {

constexpr int kXkpWaves = 4, kXkpThreads = kXkpWaves * 64;
constexpr int kXkpRows = 128, kXkpCols = 128;             // the tile: 2 x 2 wavefronts of 2 x 2 blocks
constexpr int kXkpStageDims = 8;                          // coordinates per stage
constexpr int kXkpStageChunks = 3;                        // MFMAs per block and stage
constexpr int kXkpStageRecs = 2 * kXkpStageChunks * 32;   // records of one stage of one group of 32 points (3 KiB)
constexpr int kXkpGroups = (kXkpRows + kXkpCols) / 32;    // point groups of a stage buffer: 4 of rows, then 4 of columns

__host__ __device__ inline int xkp_num_stages(int D) { return (D + kXkpStageDims - 1) / kXkpStageDims; }
__host__ __device__ inline int xkp_num_mfma(int D) { return (6 * D + 15) / 16; }
// records of one cloud in one role, per batch item
__host__ __device__ inline long xkp_cloud_recs(int n, int D) { return (long)((n + 31) / 32) * xkp_num_stages(D) * kXkpStageRecs; }

// Where a call keeps its operands in the workspace: the two clouds in both roles, their norms, then the split partials.  Every part is
// rounded up to 256 bytes.  Plain arithmetic: the sizing entry point and the launcher read the same numbers.
struct XkpLayout {
    size_t xr, xc, yr, yc, n2x, n2y, partials;      // byte offsets; `partials`: the end of the operands
    XkpLayout(int B, int N, int M, int D) {
        const size_t bx = align256((size_t)B * xkp_cloud_recs(N, D) * 16), by = align256((size_t)B * xkp_cloud_recs(M, D) * 16);
        xr = 0; xc = bx; yr = 2 * bx; yc = 2 * bx + by;
        n2x = 2 * bx + 2 * by;
        n2y = n2x + align256((size_t)B * N * sizeof(float));
        partials = n2y + align256((size_t)B * M * sizeof(float));
    }
};

// What a call is sized for behind the operands: (max, sum) per row, split and problem for as many splits as choose_splits can take
// (512 columns per split, 32 at most), on the wider cloud — non-decreasing in N and M; a launch caps its splits at what it is given.
inline size_t xkp_partial_bytes(int B, int N, int M) {
    const int n = N > M ? N : M;
    const int ns = n / 512 < 32 ? n / 512 : 32;
    return ns < 2 ? 0 : align256((size_t)ns * B * n * 2 * sizeof(float) * 4);
}

struct XkpOperands {
    const uint4* rrec[4];     // packed rows of each problem, [B][groups][NS][6][32]
    const uint4* crec[4];     // packed columns
    const float* rn2[4];      // |xt_i|^2 of its rows, (B, N[k])
    const float* cn2[4];      // |yt_j|^2 of its columns, (B, M[k])
    float guard;              // P = 1: the near-pair rule of glhip_dist_xkp.h (GLHIP_DIST_GUARD)
};

// Both clouds of a call as records, in both roles, and their squared norms.  grid = (blocks of 256 points of the longer cloud, B,
// 2 NS): blockIdx.z = 2 stage + cloud.  A thread owns one point and one stage: 8 coordinates -> 6 + 6 records.
template <typename T>
__global__ void __launch_bounds__(kBlock)
xkp_pack_kernel(const T* __restrict__ x, const T* __restrict__ y, int N, int M, int D, uint4* __restrict__ xr, uint4* __restrict__ xc,
                uint4* __restrict__ yr, uint4* __restrict__ yc, float* __restrict__ n2x, float* __restrict__ n2y) {
    const int cloud = blockIdx.z & 1, s = blockIdx.z >> 1, b = blockIdx.y;
    const int n = cloud ? M : N;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ((n + 31) & ~31)) return;
    const int NS = xkp_num_stages(D);
    const T* centre = x + (long)b * N * D;
    const T* p = (cloud ? y : x) + ((long)b * n + min(i, n - 1)) * D;
    uint32_t h[2][6 * kXkpStageDims];      // the 48 slots of the stage, row role and column role
#pragma unroll
    for (int q = 0; q < kXkpStageDims; ++q) {
        const int d = s * kXkpStageDims + q;
        const float v = (i < n && d < D) ? to_f32<T>(p[d]) - to_f32<T>(centre[d]) : 0.f;
        uint32_t pc[3];
        split3_rn(v, pc);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            h[0][6 * q + t] = pc[xd_piece_at<true, XL_BF16X3>(t)];
            h[1][6 * q + t] = pc[xd_piece_at<false, XL_BF16X3>(t)];
        }
    }
    const long off = (long)b * xkp_cloud_recs(n, D) + ((long)(i >> 5) * NS + s) * kXkpStageRecs + (i & 31);
    uint4* dst[2] = {(cloud ? yr : xr) + off, (cloud ? yc : xc) + off};
#pragma unroll
    for (int role = 0; role < 2; ++role)
#pragma unroll
        for (int r = 0; r < 2 * kXkpStageChunks; ++r) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = h[role][8 * r + 2 * k] | (h[role][8 * r + 2 * k + 1] << 16);
            dst[role][r * 32] = uint4{w[0], w[1], w[2], w[3]};
        }
    if (s == 0 && i < n) {      // the norm: four interleaved FMA chains, summed pairwise
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d0 = 0; d0 < D; d0 += 4)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (d0 + k < D) {
                    const float w = to_f32<T>(p[d0 + k]) - to_f32<T>(centre[d0 + k]);
                    c[k] = __builtin_fmaf(w, w, c[k]);
                }
        (cloud ? n2y : n2x)[(long)b * n + i] = (c[0] + c[1]) + (c[2] + c[3]);
    }
}

// P = 2: the dot-product epilogue described above.  P = 1: the distance epilogue of glhip_dist_xkp.h (Hs[2 ..] holds N_j of the tile).
template <typename T, int P = 2>
__global__ void __launch_bounds__(kXkpThreads, 3)
xkp_fwd_multi_kernel(SoftminMulti<T> m, XkpOperands ops, int D, SplitInfo sp) {
    __shared__ uint4 stageBuf[2][kXkpGroups * kXkpStageRecs];
    __shared__ __attribute__((aligned(16))) float Hs[P == 1 ? 4 : 2][kXkpCols];
    __shared__ float mrg[2][kXkpRows][2];

    const int ns = sp.n_splits;
    const int k = blockIdx.z / ns;
    const int split = blockIdx.z - k * ns;
    const int N = m.N[k], M = m.M[k];
    const int row0 = blockIdx.x * kXkpRows;
    if (row0 >= N) return;
    const int b = blockIdx.y;
    const SoftminParams<T>& prm = m.p[k];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    const int NS = xkp_num_stages(D), NM = xkp_num_mfma(D);
    const float s2 = prm.s2;

    const uint4* rrec = ops.rrec[k] + (long)b * xkp_cloud_recs(N, D) + (long)(row0 >> 5) * NS * kXkpStageRecs;
    const uint4* crec = ops.crec[k] + (long)b * xkp_cloud_recs(M, D);
    const int nrg = min(kXkpRows / 32, (N - row0 + 31) >> 5);      // row groups of this block

    // this split's columns: whole groups of 32, like the packed layout
    const int len = (((M + ns - 1) / ns) + 31) & ~31;
    const int js = (int)min((long)M, (long)split * len);
    const int je = (int)min((long)M, (long)js + len);
    const int ntiles = (je - js + kXkpCols - 1) / kXkpCols;
    const int total = ntiles * NS;

    // step q = (tile, stage): the records of the stage, 3 runs of 64 per point group, straight into LDS
    auto stage = [&](int q) {
        const int t = q / NS, s = q - t * NS;
        const int j0 = js + t * kXkpCols;
        const int ncg = (min(kXkpCols, je - j0) + 31) >> 5;
        const int nch = min(kXkpStageChunks, NM - s * kXkpStageChunks);
        uint4* dst = stageBuf[q & 1];
        for (int c = wave; c < kXkpGroups * kXkpStageChunks; c += kXkpWaves) {
            const int g = c / kXkpStageChunks, ch = c - g * kXkpStageChunks;
            if (ch >= nch) continue;
            const uint4* src;
            if (g < kXkpRows / 32) {
                if (g >= nrg) continue;
                src = rrec + ((long)g * NS + s) * kXkpStageRecs;
            } else {
                if (g - kXkpRows / 32 >= ncg) continue;
                src = crec + ((long)((j0 >> 5) + g - kXkpRows / 32) * NS + s) * kXkpStageRecs;
            }
            glds16(src + ch * 64 + lane, dst + g * kXkpStageRecs + ch * 64);
        }
    };

    const bool rows_on = wr * 2 < nrg;
    f32x16 acc[2][2];
    float mx[2], ssum[2];
    // P = 1: n_i of this lane's rows and their near-pair thresholds; -inf for a row past the cloud: its group may not even be staged, and
    // nothing its accumulators hold is ever below it
    [[maybe_unused]] float rn[2], thr[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        if constexpr (P == 1) {
            const int row = row0 + wr * 64 + rt * 32 + l31;
            rn[rt] = ops.rn2[k][(long)b * N + min(row, N - 1)];
            thr[rt] = (row < N && ops.guard > 0.f) ? fmaxf(ops.guard * rn[rt], 4.f * kXkpDistClamp2) : -__builtin_inff();
        }
        mx[rt] = kMinusHuge;
        ssum[rt] = 0.f;
#pragma unroll
        for (int cg = 0; cg < 2; ++cg)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rt][cg][e] = 0.f;
    }

    if (total > 0) stage(0);
    int t = 0, s = 0;
    for (int q = 0; q < total; ++q) {
        const int j0 = js + t * kXkpCols;
        const int n = min(kXkpCols, je - j0);
        const int ncg = (n + 31) >> 5;
        if (s == 0 && tid < kXkpCols) {      // H_j of the tile; read after the last stage's barrier, rewritten two tiles on
            if constexpr (P == 1) {
                xkp_dist_columns<T>(prm, ops.cn2[k], (long)b * M + j0 + tid, tid < n, &Hs[t & 1][tid], &Hs[2 + (t & 1)][tid]);
            } else {
                float H = kNegBig;
                if (tid < n) {
                    const long col = (long)b * M + j0 + tid;
                    H = __builtin_fmaf(-0.5f * s2, ops.cn2[k][col], dual_entry(prm, col) * kLog2e);
                }
                Hs[t & 1][tid] = H;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's share of step q has landed ...
        __syncthreads();                                      // ... and so has everybody's; step q - 1 is consumed
        if (q + 1 < total) stage(q + 1);
        const bool wave_on = rows_on && wc * 2 < ncg;
        if (wave_on) {
            const int nch = min(kXkpStageChunks, NM - s * kXkpStageChunks);
            const uint4* rb = &stageBuf[q & 1][(wr * 2) * kXkpStageRecs + lane];
            const uint4* cb = &stageBuf[q & 1][(kXkpRows / 32 + wc * 2) * kXkpStageRecs + lane];
#pragma unroll
            for (int c = 0; c < kXkpStageChunks; ++c) {
                if (c < nch) {
                    uint4 X[2], Y[2];
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) X[rt] = rb[rt * kXkpStageRecs + c * 64];
#pragma unroll
                    for (int cg = 0; cg < 2; ++cg) Y[cg] = cb[cg * kXkpStageRecs + c * 64];
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                        for (int cg = 0; cg < 2; ++cg) acc[rt][cg] = mfma_x32(Y[cg], X[rt], acc[rt][cg]);
                }
            }
            if (s == NS - 1) {
                // ---- epilogue: lane (half, i) holds row i of a block against the columns 8 (e / 4) + 4 half + e % 4 ----
                [[maybe_unused]] f32x16 H[2];
                if constexpr (P == 2) {
#pragma unroll
                    for (int cg = 0; cg < 2; ++cg)
#pragma unroll
                        for (int g4 = 0; g4 < 4; ++g4) {
                            const float4 v = *reinterpret_cast<const float4*>(&Hs[t & 1][(wc * 2 + cg) * 32 + g4 * 8 + half * 4]);
                            H[cg][4 * g4] = v.x; H[cg][4 * g4 + 1] = v.y; H[cg][4 * g4 + 2] = v.z; H[cg][4 * g4 + 3] = v.w;
                        }
                }
                const bool cg1 = wc * 2 + 1 < ncg;      // (the wavefront's second column group may lie past the tile)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    if constexpr (P == 1) {
                        xkp_dist_exponents<T>(acc[rt], &Hs[t & 1][wc * 64], &Hs[2 + (t & 1)][wc * 64], rn[rt], thr[rt], s2, cg1,
                                              prm.x + (long)b * N * D, prm.y + (long)b * M * D, row0 + wr * 64 + rt * 32, N, j0 + wc * 64, je,
                                              half, D);
                    } else {
#pragma unroll
                        for (int cg = 0; cg < 2; ++cg)
#pragma unroll
                            for (int e = 0; e < 16; ++e) acc[rt][cg][e] = __builtin_fmaf(s2, acc[rt][cg][e], H[cg][e]);
                    }
                    float um = fmaxf(kMinusHuge, max16(acc[rt][0]));
                    if (cg1) um = fmaxf(um, max16(acc[rt][1]));
                    um = fmaxf(um, __shfl_xor(um, 32, 64));
                    if (um > mx[rt]) {                  // lazy: rescale only when the maximum grew
                        ssum[rt] *= fast_exp2(mx[rt] - um);
                        mx[rt] = um;
                    }
                    ssum[rt] += sum_exp2_16(acc[rt][0], mx[rt]);
                    if (cg1) ssum[rt] += sum_exp2_16(acc[rt][1], mx[rt]);
#pragma unroll
                    for (int cg = 0; cg < 2; ++cg)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[rt][cg][e] = 0.f;
                }
            }
        }
        if (++s == NS) { s = 0; ++t; }
    }

    // ---- the two column halves of the workgroup meet: [wc][row] of (max, sum) ----
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const float sum = ssum[rt] + __shfl_xor(ssum[rt], 32, 64);      // the lane halves hold the two 16-column halves of every block
        if (half == 0) {
            const int r = wr * 64 + rt * 32 + l31;
            mrg[wc][r][0] = mx[rt];
            mrg[wc][r][1] = sum;
        }
    }
    __syncthreads();
    if (tid < min(kXkpRows, N - row0)) {
        const float m0 = mrg[0][tid][0], m1 = mrg[1][tid][0];
        const float mn = fmaxf(m0, m1);
        const float sum = mrg[0][tid][1] * fast_exp2(m0 - mn) + mrg[1][tid][1] * fast_exp2(m1 - mn);
        const long idx = (long)b * N + row0 + tid;
        const float mtot = P == 1 ? mn : __builtin_fmaf(-0.5f * s2, ops.rn2[k][idx], mn);      // r_i + max (P = 1: no row constant)
        if (ns == 1) {
            prm.out[idx] = finish_value(prm, idx, mtot + fast_log2(sum));
        } else {
            float* dst = sp.workspace + k * m.ws_stride + split * ((long)gridDim.y * N * 2) + idx * 2;
            dst[0] = mtot;
            dst[1] = sum;
        }
    }
}

// ---- what glhip_api.hip calls (glhip_api_iter4_xk.hip) ----

// Packs the clouds of a call into `ws` (XkpLayout); false, and nothing queued, where `bytes` does not hold them.
bool xkp_pack(const void* x, const void* y, int B, int N, int M, int D, int in_dtype, void* ws, size_t bytes, hipStream_t st);
// The problems of `m` (rows / columns of problem k: x / y, y / x, x / x, y / y) on the operands xkp_pack left in `ws`: one launch, and
// the merge of its column splits where the rest of the workspace holds some.
// p = 2: the dot-product epilogue; p = 1: the distance epilogue (glhip_dist_xkp.h), `m` built with p = 1.
void xkp_reduce(SoftminMulti<float>& m, int B, int N, int M, int D, int p, void* ws, size_t bytes, bool allow_split, hipStream_t st);
void xkp_reduce(SoftminMulti<bf16_t>& m, int B, int N, int M, int D, int p, void* ws, size_t bytes, bool allow_split, hipStream_t st);

}  // namespace glhip
