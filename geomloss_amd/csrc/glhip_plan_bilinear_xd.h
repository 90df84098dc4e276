// glhip_plan_bilinear_xd.h — the bilinear plan reduction on RESIDENT, PRE-PACKED operands for clouds of dimension 1 <= D <= 16 and
// 1 <= K <= 32 features (GLHIP_FLAG_XD_BILINEAR), p = 2, float32 / bfloat16 clouds, float32 features, dense and batched launches:
//
//     w_ij   = exp(h_j - |x_i - y_j|^2 / (2 eps) + fwd_i / eps),      pi_ij = w_ij / sum_j w_ij,      tau_ij = <rowfeat_i, colfeat_j>
//     out[i][:] = sum_j pi_ij tau_ij (y_j - x_i)                      wsum[i] = sum_j pi_ij tau_ij
//
// Why a second family.  xk_bilinear_kernel (glhip_plan_bilinear_xk.h) stages both chains on the fly, twice per tile of 128 columns with
// three barriers each, holds a 2 x 2 arrangement of tau blocks in 256 VGPRs and spends a pass of 32 coordinates on D <= 16.  What bounds
// D <= 16 and K <= 32 is small enough to pack ONCE per call and to keep the whole row side in registers, so the reducing kernel only
// copies, multiplies and folds.
//
// Shape: the geometry of plan_apply_kernel (glhip_plan_apply.h).  Eight wavefronts of 32 rows share one column tile; a row lives in one
// wavefront, which works on ONE 32 x 32 block at a time: exponent block (NM chained MFMAs), tau block (NMK), product on the VALU, six
// MFMAs against the coordinate chunk, fold into 16 running registers.  No 2 x 2 arrangement, no column halves of the workgroup to merge:
// only the two lane halves (__shfl_xor 32) and the column splits, which go through plan_merge_kernel / plan_merge_store with W counted as
// one more sum.  No float atomics: bit-identical run to run.
//
// Resident row operands (4 (NM + NMK) VGPRs for the whole column sweep), packed by xd_bilinear_pack_rows_kernel / _pack_feat_kernel:
//   exponent chain  the 6-slot bf16 x 3 records of glhip_klayout.h, NM = ceil(6 (D + 1) / 16) = 1 .. 7 v_mfma_f32_32x32x16_bf16, around
//                   ONE centre per launch (launch_centre), all of s = log2(e) / eps on the rows, scalar item [1,1,1,c1,c2,c3] with
//                   C_i = r_i - LSE2_i as in plan_apply_kernel (fwd_i = +inf: kNegBig, a row without mass).
//   weight chain    the same six products per feature over rowfeat, NO scalar item, uncentred, unit scale: slot 6 k + t of feature k.
//                   K is padded to a bucket: K <= 5 / 8 / 16 / 32 -> NMK = 2 / 3 / 6 / 12 MFMAs (padding slots are zero on both sides).
// The kernel is templated on (NM, NMK) alone — 7 x 4 = 28 instantiations; D and the cloud's dtype are known to the packing kernels only.
//
// Column side, packed once per call, group-major so that a tile is ONE contiguous run: per group of 32 columns
//   [NM x 64 exponent records][NMK x 64 colfeat records][256 records of coordinate pieces]        = NM + NMK + 4 KiB
//   exponent records  [H1,H2,H3,1,1,1] with H_j = log2(e) h_j - s/2 |yt_j|^2; h_j = -inf stays -inf and the padded columns of the last
//                     group carry -inf too: their exponent is -inf whatever the (finite) C_i, their weight exactly 0, no test by index.
//   coordinates       PRE-PACKED (the other option, staging them on the fly with plan_store_pieces as plan_apply_kernel does, costs
//                     that kernel two more barriers per tile, an LDS atomic per item and D + 8 staging registers: the resource report
//                     below has no room for them at two workgroups per CU).  (y_j - centre) as two f16 pieces in the A-operand layout
//                     of plan_chunk_mfma — one chunk of 32 feature rows holds all D <= 16 coordinates, rows D .. 31 are zero — under ONE
//                     power-of-two scale per group of 32 columns (plan_scale_exponent of the group's largest |coordinate|: it lands in
//                     [2^14, 2^15), a piece that falls into the f16 subnormals is off by 2^-39 of it, far below the float32 rounding of
//                     y_j - centre itself).  The inverse scale (times 2^-13) is one float per group, read as a wavefront-uniform load.
// Tiles move by LDS-DMA (glds16, 1 KiB per wavefront instruction) into two buffers, ONE barrier per tile, as arg_xd_kernel does.
//
// Numerics: the contract of xk_bilinear_kernel.  Two running maxima per row — m over the exponents for the mass (unsplit fp32 weights),
// mq over u + log2 |tau| for the signed sums, u - mq capped at kBilinearMaxLift; q_ij = tau_ij 2^13 2^(u_ij - mq_i) through
// plan_split_weights and plan_chunk_mfma; W_i summed on the VALU from the unsplit products (no spare feature row is spent on it: 16
// adds per block buy W at fp32 accuracy, independent of the coordinate scale); a pair without mass contributes 0 by a select, whatever
// finite tau it holds; T_c = S_c - (x_i - centre)_c W is formed before anything is written ((x_i - centre) is kept aside, one float per
// row and coordinate); the signed sums are brought to the scale of the mass (2^(mq - m), capped) before the division or the partial;
// a row without mass writes 0 in both outputs.  GLHIP_FLAG_F16X2 is accepted and ignored (bf16 x 3 exponents only).
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage, printed by every build of glhip_api_plan_bilinear_xd.hip; read with
// tools/kernel_resources.py).  The aim — two workgroups per CU — is REACHED wherever the resident operands are at most 40 registers:
// __launch_bounds__(512, 4), 128 VGPRs, two tile buffers of <= 36 KiB, for NM + NMK <= kXdBilinearLight = 10, i.e. every D with K <= 8 and
// D <= 9 with K <= 16.  Beyond (K > 16, or D >= 10 with K > 8) the budget goes to the 4 (NM + NMK) = 44 ... 76 operand registers:
// __launch_bounds__(512, 2), one workgroup per CU, two buffers of <= 60 KiB.  Every instantiation: 0 bytes of scratch.
// VGPRs / waves per SIMD / LDS bytes (columns per tile = LDS / (2 KiB (NM + NMK + 4)) x 32):
//     NMK \ NM        1              2              3              4              5              6              7
//      2 (K <= 5)   100 4  71680   103 4  65536   108 4  73728   112 4  61440   116 4  67584   120 4  73728   124 4  53248
//      3 (K <= 8)   103 4  65536   108 4  73728   112 4  61440   116 4  67584   120 4  73728   124 4  53248   128 4  57344
//      6 (K <= 16)  116 4  67584   120 4  73728   124 4  53248   128 4  57344   132 2 122880   135 2  98304   140 2 104448
//     12 (K <= 32)  141 2 104448   144 2 110592   148 2 116736   152 2 122880   156 2  86016   160 2  90112   164 2  94208
//   xd_bilinear_pack_rows_kernel<D, T> / xd_bilinear_pack_cols_kernel<D, T>: 13 ... 79 / 16 ... 76 VGPRs (the latter 32 KiB of LDS),
//   xd_bilinear_pack_feat_kernel: 14; plan_merge_kernel<XdBilinearParams>: as for the other parameter structs; no scratch anywhere.
// Timings: profiles/plan_bilinear_xd.txt.
#pragma once

#include "glhip_plan_apply.h"
#include "glhip_plan_bilinear_xk.h"

namespace glhip {

constexpr int kXdBilinearMaxK = 32;
constexpr int kXdBilinearThreads = 8 * 64;
constexpr int kXdBilinearRows = 8 * 32;                    // rows per workgroup: one row tile per wavefront
constexpr int kXdBilinearLight = 10;                       // NM + NMK up to which an instantiation is built for 128 VGPRs
constexpr int xd_bilinear_num_mfma(int D) { return (6 * (D + 1) + 15) / 16; }
constexpr int xd_bilinear_num_mfma_k(int K) { return K <= 5 ? 2 : K <= 8 ? 3 : K <= 16 ? 6 : 12; }
constexpr int xd_bilinear_waves(int NM, int NMK) { return NM + NMK <= kXdBilinearLight ? 4 : 2; }      // wavefronts per SIMD
constexpr long xd_bilinear_slots(int NM, int NMK) { return 256 * (xd_bilinear_waves(NM, NMK) / 2); }   // resident workgroups
constexpr int xd_bilinear_group_recs(int NM, int NMK) { return 64 * (NM + NMK + 4); }                  // 16-byte records per column group
constexpr int xd_bilinear_groups(int NM, int NMK) {        // column groups per tile buffer: 36 / 60 KiB, at most 256 columns
    const int g = (xd_bilinear_waves(NM, NMK) == 4 ? 36 : 60) / (NM + NMK + 4);
    return g < 1 ? 1 : (g > 8 ? 8 : g);
}
static_assert(xd_bilinear_num_mfma(16) == XdShape<16>::NM && xd_bilinear_num_mfma(1) == XdShape<1>::NM, "glhip_klayout.h");
static_assert(6 * kXdBilinearMaxK <= 16 * xd_bilinear_num_mfma_k(kXdBilinearMaxK) && 6 * 5 <= 16 * xd_bilinear_num_mfma_k(5) &&
              6 * 8 <= 16 * xd_bilinear_num_mfma_k(8) && 6 * 16 <= 16 * xd_bilinear_num_mfma_k(16), "six slots per feature fit every bucket");

struct XdBilinearParams {
    const uint4* xrec;   // packed rows, [B][ceil(N / 32)][2 NM][32]
    long xstride;        // records per batch item
    const uint4* rrec;   // packed row features, [B][ceil(N / 32)][2 NMK][32]
    long rstride;
    const uint4* yrec;   // packed columns, [B][ceil(M / 32)][xd_bilinear_group_recs]
    long ystride;
    const float* yinv;   // [B][ceil(M / 32)]: 2^-13 / scale of the group's coordinate pieces
    const float* xc;     // (B,N,D): x_i - centre
    float* out;          // (B,N,D)
    float* wsum;         // (B,N) or NULL
    int nv;              // the merge: D + 1, W counts as the last sum
};

// The end of plan_merge_kernel: D coordinates and W of a row, merged sum s and mass w relative to the same 2^mx — divided.
__device__ __forceinline__ void plan_merge_store(const XdBilinearParams& prm, int, int D, long row, int c, float s, float w, float) {
    const float q = (w > 0.f) ? s / w : 0.f;
    if (c < D) prm.out[row * D + c] = q;
    else if (prm.wsum) prm.wsum[row] = q;
}

// The rows of a call as x-side exponent records (scalar item C_i, coordinates times s), and x_i - centre.  Rows i >= N of the last group
// are zero points (their results are not stored).
template <int D, typename T>
__global__ void __launch_bounds__(kBlock)
xd_bilinear_pack_rows_kernel(const T* __restrict__ x, const float* __restrict__ fwd, int N, float s2, float out_scale, XdPacked pk,
                             float* __restrict__ xc) {
    using S = XdShape<D>;
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ((N + 31) & ~31)) return;
    float centre[D], a[D], cst = kNegBig;
    launch_centre<D, T>(x, b, N, centre);
#pragma unroll
    for (int d = 0; d < D; ++d) a[d] = 0.f;
    if (i < N) {
        float xi[D], n2 = 0.f;
        load_point<D, T>(x, (long)b * N + i, xi);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float xt = xi[d] - centre[d];
            n2 = __builtin_fmaf(xt, xt, n2);
            a[d] = xt * s2;
            xc[((long)b * N + i) * D + d] = xt;
        }
        // C_i = r_i - LSE2_i as in plan_apply_kernel: fwd_i = +inf is a row without mass, a huge fwd_i stays finite against the -inf columns
        const float fw = fwd[(long)b * N + i];
        cst = (fw == __builtin_inff()) ? kNegBig : __builtin_fminf(-0.5f * s2 * n2 - fw / out_scale, -kNegBig);
    }
    uint4* base = pk.rec + b * pk.stride + (long)(i >> 5) * S::kGroupRecs + (i & 31);
#pragma unroll
    for (int r = 0; r < S::NBP; ++r) base[r * 32] = xd_record_of<D, true>(r, cst, a);
}

// Record blockIdx.y (K slots 8 r .. 8 r + 7) of the weight chain of every point: six slots per feature, no scalar item, zero beyond K and
// for the points that pad the last group.  `off`: where the records of a point's group begin inside its run of `group_recs`.
template <bool XSIDE>
__global__ void __launch_bounds__(kBlock)
xd_bilinear_pack_feat_kernel(const float* __restrict__ feat, int P, int K, uint4* __restrict__ rec, long stride, int group_recs, int off) {
    const int b = blockIdx.z, r = blockIdx.y;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= ((P + 31) & ~31)) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (j < P) {
        const float* f = feat + ((long)b * P + j) * K;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int slot = 8 * r + k, ft = slot / 6;
            uint32_t h = 0u;
            if (ft < K) {
                uint32_t p[3];
                split3_rn(f[ft], p);
                const int piece = xd_piece_at<XSIDE, XL_BF16X3>(slot - 6 * ft);
                h = piece == 0 ? p[0] : (piece == 1 ? p[1] : p[2]);
            }
            w[k >> 1] |= (k & 1) ? (h << 16) : h;
        }
    }
    rec[b * stride + (long)(j >> 5) * group_recs + off + r * 32 + (j & 31)] = uint4{w[0], w[1], w[2], w[3]};
}

// The columns of a call: exponent records at the head of their group's run, the coordinate pieces `coord_off` records into it (built in
// LDS in the A-operand layout, copied out in whole records), and the group's inverse scale.  One workgroup = 8 groups of 32 columns.
template <int D, typename T>
__global__ void __launch_bounds__(kBlock)
xd_bilinear_pack_cols_kernel(const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ h, int N, int M, float s2,
                             XdPacked pk, int group_recs, int coord_off, float* __restrict__ yinv) {
    using S = XdShape<D>;
    __shared__ uint4 q[(kBlock / 32) * 256];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int j = blockIdx.x * kBlock + tid;
    const int groups = (M + 31) >> 5;
    for (int k = tid; k < (kBlock / 32) * 256; k += kBlock) q[k] = uint4{0u, 0u, 0u, 0u};
    float centre[D], yt[D], H = -__builtin_inff();
    launch_centre<D, T>(x, b, N, centre);
    uint32_t mx = 0u;
#pragma unroll
    for (int d = 0; d < D; ++d) yt[d] = 0.f;
    if (j < M) {
        float yj[D], n2 = 0.f;
        load_point<D, T>(y, (long)b * M + j, yj);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            yt[d] = yj[d] - centre[d];
            n2 = __builtin_fmaf(yt[d], yt[d], n2);
            mx = max(mx, __float_as_uint(yt[d]) & 0x7FFFFFFFu);
        }
        H = __builtin_fmaf(-0.5f * s2, n2, h[(long)b * M + j] * kLog2e);
    }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));      // the group's 32 lanes
    const uint32_t se = plan_scale_exponent(mx);
    const float sc = __uint_as_float(se << 23);
    const bool in_group = (j >> 5) < groups;
    if (in_group && (j & 31) == 0) yinv[(long)b * groups + (j >> 5)] = __uint_as_float((254u - (uint32_t)kWqShift - se) << 23);
    __syncthreads();      // q is zero
    {   // column jj of a group: instruction jj / 16, lane half (jj / 4) % 2, f16 number 4 ((jj / 8) % 2) + jj % 4 of the record of coordinate d
        const int g = tid >> 5, jj = tid & 31;
        unsigned short* qs = reinterpret_cast<unsigned short*>(&q[g * 256 + (jj >> 4) * 64 + ((jj >> 2) & 1) * 32]) + 4 * ((jj >> 3) & 1) + (jj & 3);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float v = yt[d] * sc;
            const _Float16 hi = (_Float16)v;
            const _Float16 lo = (_Float16)(v - (float)hi);
            qs[d * 8] = __builtin_bit_cast(unsigned short, hi);
            qs[(128 + d) * 8] = __builtin_bit_cast(unsigned short, lo);
        }
    }
    __syncthreads();
    for (int k = tid; k < (kBlock / 32) * 256; k += kBlock) {
        const int G = blockIdx.x * (kBlock / 32) + (k >> 8);
        if (G < groups) pk.rec[b * pk.stride + (long)G * group_recs + coord_off + (k & 255)] = q[k];
    }
    if (in_group) {
        uint4* base = pk.rec + b * pk.stride + (long)(j >> 5) * group_recs + (j & 31);
#pragma unroll
        for (int r = 0; r < S::NBP; ++r) base[r * 32] = xd_record_of<D, false>(r, H, yt);
    }
}

template <int NM, int NMK>
__global__ void __launch_bounds__(kXdBilinearThreads, xd_bilinear_waves(NM, NMK))
xd_bilinear_kernel(XdBilinearParams prm, int N, int M, int D, SplitInfo sp) {
    constexpr int GR = xd_bilinear_group_recs(NM, NMK), kG = xd_bilinear_groups(NM, NMK), kTileD = 32 * kG;
    __shared__ uint4 tileBuf[2 * kG * GR];

    int bx, b, split;
    workgroup_coords(sp, bx, b, split);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int ns = sp.n_splits;

    const int row0 = bx * kXdBilinearRows;
    const int row_end = min(N, row0 + kXdBilinearRows);
    const int wave_row0 = row0 + wave * 32;
    const bool wave_active = wave_row0 < row_end;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // both x-side operands of this wavefront's 32 rows, resident for the whole sweep (a tile past the last group repeats the last one)
    uint4 X[NM], R[NMK];
    {
        const int G = min(wave_row0 >> 5, (N - 1) >> 5);
        const uint4* xs = prm.xrec + b * prm.xstride + (long)G * (64 * NM) + lane;
        const uint4* rs = prm.rrec + b * prm.rstride + (long)G * (64 * NMK) + lane;
#pragma unroll
        for (int mm = 0; mm < NM; ++mm) X[mm] = xs[mm * 64];
#pragma unroll
        for (int mm = 0; mm < NMK; ++mm) R[mm] = rs[mm * 64];
    }
    f32x16 pacc[1] = {zero16};                                // running sums S (centred coordinates), relative to 2^mq
    float mass4[4] = {0.f, 0.f, 0.f, 0.f}, w4[4] = {0.f, 0.f, 0.f, 0.f};      // the mass (2^m) and W (2^mq), times 2^kWqShift
    float m = kMinusHuge, mq = kMinusHuge;

    // this split's columns: whole groups of 32, like the packed layout
    const int groups = (M + 31) >> 5;
    const int len = (((M + ns - 1) / ns) + 31) & ~31;
    const int js = (int)min((long)M, (long)split * len);
    const int je = (int)min((long)M, (long)js + len);
    const float* inv = prm.yinv + (long)b * groups;
    auto stage = [&](int j0, int buf) {
        const int nGs = (min(kTileD, je - j0) + 31) >> 5;
        const uint4* src = prm.yrec + b * prm.ystride + (long)(j0 >> 5) * GR;
        for (int c = wave; c < nGs * (GR / 64); c += 8) glds16(src + c * 64 + lane, &tileBuf[buf * (kG * GR) + c * 64]);
    };
    if (js < je) stage(js, 0);

    int t = 0;
    for (int j0 = js; j0 < je; j0 += kTileD, ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's share of tile t has landed ...
        __syncthreads();                                      // ... and so has everybody's; tile t - 1 is consumed
        if (j0 + kTileD < je) stage(j0 + kTileD, (t + 1) & 1);
        if (!wave_active) continue;
        const uint4* tile = tileBuf + (t & 1) * (kG * GR);
        const int nG = (min(kTileD, je - j0) + 31) >> 5;
        for (int G = 0; G < nG; ++G) {
            const uint4* g = &tile[G * GR];
            const float ginv = inv[(j0 >> 5) + G];
            f32x16 u = xd_block<NM, 2 * NM>(g, lane, X, zero16);
            const f32x16 tb = xd_block<NMK, 2 * NMK>(g + 64 * NM, lane, R, zero16);
            float bm = kMinusHuge, bq = kMinusHuge;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                bm = fmaxf(bm, u[r]);
                bq = fmaxf(bq, u[r] + fast_log2(__builtin_fabsf(tb[r])));      // tau == 0 or no mass: -inf
            }
            bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
            bq = fmaxf(bq, __shfl_xor(bq, 32, 64));
            if (__any(bm > m)) {                              // plan_rescale for the mass alone
                const float mn = fmaxf(m, bm);
                const float rs = fast_exp2(m - mn);
#pragma unroll
                for (int k = 0; k < 4; ++k) mass4[k] *= rs;
                m = mn;
            }
            plan_rescale(bq, mq, pacc, w4);
            Pack16h whi[2], wlo[2];
#pragma unroll
            for (int k = 0; k < 16; k += 2) {
                f32x2_t qq;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    mass4[(k & 3) + e] += fast_exp2(u[k + e] - m) * (float)(1 << kWqShift);
                    const float ex = fast_exp2(__builtin_fminf(u[k + e] - mq, kBilinearMaxLift)) * (float)(1 << kWqShift);
                    qq[e] = (ex > 0.f) ? tb[k + e] * ex : 0.f;      // no weight: exactly 0, whatever tau holds
                    w4[(k & 3) + e] += qq[e];
                }
                plan_split_weights(qq, k, whi, wlo);
            }
            const f32x16 tt = plan_chunk_mfma(g + 64 * (NM + NMK) + lane, whi, wlo);
#pragma unroll
            for (int r = 0; r < 16; ++r) pacc[0][r] = __builtin_fmaf(tt[r], ginv, pacc[0][r]);
        }
    }
    if (!wave_active) return;

    // ---- the two lane halves meet (they hold the two 16-column halves of every block); T = S - (x_i - centre) W, to the scale of the mass ----
    float mass = (mass4[0] + mass4[1]) + (mass4[2] + mass4[3]);
    float ws = (w4[0] + w4[1]) + (w4[2] + w4[3]);
    mass += __shfl_xor(mass, 32, 64);
    ws += __shfl_xor(ws, 32, 64);
    mass *= 1.0f / (float)(1 << kWqShift);                    // relative to 2^m
    ws *= 1.0f / (float)(1 << kWqShift);                      // relative to 2^mq
    const int i = wave_row0 + l31;
    if (i >= row_end) return;
    const float lift = fast_exp2(__builtin_fminf(mq - m, 126.f));
    const long idx = (long)b * N + i;
    float* part = sp.workspace + split * sp.split_stride + idx * (D + 3);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = reg_feature(r, half);
        if (c < D) {
            const float s = __builtin_fmaf(-prm.xc[idx * D + c], ws, pacc[0][r]) * lift;
            if (ns > 1) part[c] = s;
            else prm.out[idx * D + c] = (mass > 0.f) ? s / mass : 0.f;
        }
    }
    if (half == 0) {
        const float W = ws * lift;
        if (ns > 1) {
            part[D] = W;
            part[D + 1] = mass;
            part[D + 2] = m;
        } else if (prm.wsum) {
            prm.wsum[idx] = (mass > 0.f) ? W / mass : 0.f;
        }
    }
}

}  // namespace glhip
