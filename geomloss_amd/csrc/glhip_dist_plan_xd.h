// glhip_dist_plan_xd.h — the plan of a p = 1 soft-min applied to a feature matrix on RESIDENT, PRE-PACKED operands for clouds of dimension
// 1 <= D <= 16 (GLHIP_FLAG_XD_PLAN_P1), float32 / bfloat16 clouds, float32 features of any width, dense and batched launches:
//
//     out[i][v]  = sum_j w_ij feat[j][v] / sum_j w_ij,      w_ij = 2^( S_j - dist_ij ),   S_j = log2(e) h_j,
//     softmin[i] = -eps ln 2 log2 sum_j w_ij                (optional)
// with dist_ij = sqrt(max(d2_ij, clamp2)), d2 = t^2 |x_i - y_j|^2, t = log2(e) / eps, clamp2 = 1e-8 t^2: the contract of
// xk_dist_plan_kernel (glhip_dist_plan_xk.h), which serves the same entry point for every D up to 4095.
//
// Why a second family.  Below D = 17 xk_dist_plan_kernel still runs the K-chunked chain: tiles of 128 columns staged on the fly with
// several barriers each, 95-111 KiB of LDS and 206-246 VGPRs, one workgroup per CU — to feed the one to seven MFMAs a block needs.  What
// bounds D <= 16 is small enough to pack ONCE per call (the clouds) or once per pass (the features), so the reducing kernel only copies,
// multiplies and folds.
//
// Shape: the geometry of xd_bilinear_kernel (glhip_plan_bilinear_xd.h) and arg_xd_kernel (glhip_arg_xd.h).  Eight wavefronts of 32 rows
// share one column tile; a row lives in one wavefront, which works on ONE 32 x 32 block at a time: distance block (NM chained MFMAs),
// near pairs, sqrt, weights on the VALU, six MFMAs per feature chunk, fold.  No column halves of the workgroup to merge: only the two lane
// halves (__shfl_xor 32) and the column splits, which go through plan_merge_kernel / plan_merge_store; the partial of a row is
// (sums[nv], Z, m).  No float atomics: bit-identical run to run.
//
// Rows (xd_dist_plan_pack_rows_kernel, once per call): the x-side bf16 x 3 records of the distance layout (glhip_dist_xd.h) — scalar item
// [1,1,1,n1,n2,n3], coordinates -2 t (x_i - c) — around ONE centre per launch (launch_centre); n_i = t^2 |x_i - c|^2 is kept aside, one
// float per row, for the near-pair threshold.  4 NM VGPRs for the whole column sweep, NM = ceil(6 (D + 1) / 16) = 1 .. 7.
//
// Columns (xd_dist_plan_pack_cols_kernel, once per call), group-major, so that a tile is one contiguous run of each array: per group of 32
// columns the NM x 64 y-side records ([N1,N2,N3,1,1,1], pieces of t (y_j - c)) and 32 floats S_j = log2(e) h_j.  Columns with h = -inf
// keep -inf and the padded columns of the last group carry -inf too: u = -inf whatever the distance, their weight is exactly 0 and no
// tile needs a test by index.
//
// Features: PRE-PACKED, once per pass (xd_dist_plan_pack_feat_kernel), as two f16 pieces in the A-operand layout of plan_chunk_mfma — 4
// KiB per group and chunk of 32 features — under ONE power-of-two scale per feature column and GROUP of 32 columns (plan_scale_exponent of
// the group's largest |f| among the columns that carry mass; the features of a column without mass are packed as 0, as
// plan_live_features does, so that a huge one sets no scale); the inverse scales (times 2^-13), 32 floats per group and chunk, travel
// with the tile.  The other option — staging them on the fly as plan_apply_kernel and xk_dist_plan_kernel do — costs those kernels two
// more barriers per tile, an LDS atomic per item and 4-16 staging registers held across the MFMA loop: the one-chunk instantiations
// below have no room for them at two workgroups per CU, and one barrier per tile is what the LDS-DMA buys.  The price is one small
// kernel per pass that reads feat once and writes 128 bytes per column and chunk, a few per cent of a pass at the sizes where a pass
// matters; a thread owns one (group, feature) item, so the scale needs no atomics and no second sweep.
//
// Tiles move by LDS-DMA (glds16 for the records, glds4 for S_j and the inverse scales: 1 KiB / 256 bytes per wavefront instruction, no
// staging registers) into two buffers, ONE barrier per tile, as arg_xd_kernel does.
//
// Per block: NM chained v_mfma_f32_32x32x16_bf16 give d2 (bf16 x 3 only: a squared distance needs all 24 bits).  Pairs with
// d2 < max(guard n_i, 4 clamp2) are re-evaluated on explicit differences of the caller's ORIGINAL points, re-read from global memory — not
// of centred float32 copies: x - c is rounded at the scale of the cloud, and a near pair needs the bits below that.  The path is rare, so D
// and the cloud's dtype are run-time values there (xk_dist_exact_d2) and the kernel is templated on (NM, chunks per pass) alone; D and T
// are known to the packing kernels only.  GLHIP_DIST_GUARD applies as elsewhere.  Then v_med3 against clamp2, v_sqrt_f32, u = S_j - dist;
// the lazy running row maximum (plan_rescale); weights relative to it times 2^13 in two f16 pieces (plan_split_weights) — the largest
// weight of a row is 2^13 exactly, so a one-hot plan row returns its features bit for bit; six v_mfma_f32_32x32x16_f16 per chunk into a
// fresh accumulator (plan_chunk_mfma), folded into the running sums with the inverse scale; Z from the unsplit fp32 weights on the VALU.
// Rows without mass write out = 0 and softmin = +inf, never NaN.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage, printed by every build of glhip_api_plan_p1_xd.hip; read with
// tools/kernel_resources.py).  NCH = chunks of 32 features per pass: 1, 2 or 4.  A pass of <= 32 features runs the one-chunk
// instantiation, which reaches the aim — two workgroups per CU: __launch_bounds__(512, 4), 128 VGPRs, two tile buffers of <= 36 KiB —
// for EVERY NM, D = 16 included; two and four chunks are built for 256 VGPRs, one workgroup per CU, two buffers of <= 60 KiB.  Every
// instantiation: 0 bytes of scratch, so every dimension ships the widest pass, 128 features.
// VGPRs / waves per SIMD / LDS bytes (columns per tile = 32 x min(8, budget / (NM + 4 NCH) KiB)):
//     NCH \ NM            1             2             3             4             5             6             7
//      1 (V <= 32)   108 4  75776  112 4  76800  117 4  74752  117 4  67584  125 4  75776  120 4  63488  124 4  69632
//      2 (V <= 64)   136 2 115200  142 2 127488  147 2 116736  150 2 126976  155 2 109568  159 2 117760  163 2 125952
//      4 (V <= 128)  187 2 108544  189 2 114688  196 2 120832  199 2 126976  204 2  88576  208 2  92672  212 2  96768
//   xd_dist_plan_pack_rows_kernel<D, T> / _pack_cols_kernel<D, T>: 13 ... 126 / 11 ... 115 VGPRs; xd_dist_plan_pack_feat_kernel: 47;
//   plan_merge_kernel<XdDistPlanParams>: as for the other parameter structs; no scratch anywhere.
// Timings: profiles/plan_apply_p1_xd.txt.
#pragma once

#include "glhip_dist_xk.h"
#include "glhip_plan_apply.h"

namespace glhip {

constexpr int kXdDistPlanThreads = 8 * 64;
constexpr int kXdDistPlanRows = 8 * 32;                    // rows per workgroup: one row tile per wavefront
constexpr int kXdDistPlanMaxChunks = 4;                    // chunks of 32 features per pass: no instantiation spills (table above)
constexpr int xd_dist_plan_num_mfma(int D) { return (6 * (D + 1) + 15) / 16; }
constexpr int xd_dist_plan_inst_chunks(int nch) { return nch <= 1 ? 1 : (nch == 2 ? 2 : 4); }           // the instantiation that carries nch chunks
constexpr int xd_dist_plan_waves(int, int NCH) { return NCH == 1 ? 4 : 2; }                             // wavefronts per SIMD
constexpr long xd_dist_plan_slots(int NM, int NCH) { return 256 * (xd_dist_plan_waves(NM, NCH) / 2); }  // resident workgroups
constexpr int xd_dist_plan_groups(int NM, int NCH) {       // column groups per tile buffer: 36 / 60 KiB of records, at most 256 columns
    const int g = (xd_dist_plan_waves(NM, NCH) == 4 ? 36 : 60) / (NM + 4 * NCH);
    return g < 1 ? 1 : (g > 8 ? 8 : g);
}
static_assert(xd_dist_plan_num_mfma(16) == XdShape<16>::NM && xd_dist_plan_num_mfma(1) == XdShape<1>::NM, "glhip_klayout.h");

struct XdDistPlanParams {
    const uint4* xrec;    // packed rows, [B][ceil(N / 32)][2 NM][32]
    long xstride;         // records per batch item
    const float* nrow;    // (B,N): n_i = t^2 |x_i - centre|^2
    const uint4* yrec;    // packed columns, [B][ceil(M / 32)][2 NM][32]
    long ystride;
    const float* ys;      // [B][32 ceil(M / 32)]: S_j = log2(e) h_j, -inf for the padded columns
    const uint4* qrec;    // the features of this pass, [B][ceil(M / 32)][NCH][piece][instruction][64]
    long qstride;
    const float* qinv;    // [B][ceil(M / 32)][32 NCH]: 2^-13 / scale of the group's pieces, per feature
    const void* x;        // (B,N,D), (B,M,D): the caller's points, for the near pairs
    const void* y;
    float* out;           // (B,N,V)
    float* softmin;       // (B,N), written on the pass with v0 == 0; NULL: not wanted
    float t;              // coordinate scale log2(e) / eps
    float clamp2;         // 1e-8 t^2
    float guard;          // near pairs: d2 < max(guard n_i, 4 clamp2)
    float out_scale;      // -eps ln 2: softmin = out_scale (m + log2 Z)
    int bf16;             // the dtype of x, y
    int V;                // feature columns of feat / out
    int v0;               // first feature of this pass
    int nv;               // features of this pass, <= 32 NCH
};

// The soft-min of a row from its sum z relative to 2^m; z == 0 (no mass): +inf
__device__ __forceinline__ float xd_dist_plan_softmin(const XdDistPlanParams& prm, float z, float m) {
    return (z > 0.f) ? prm.out_scale * (m + fast_log2(z)) : __builtin_inff();
}

// The end of plan_merge_kernel (glhip_plan_apply.h): the merged sum s of feature c and the row sum w, both relative to 2^mx — divided.
__device__ __forceinline__ void plan_merge_store(const XdDistPlanParams& prm, int, int, long row, int c, float s, float w, float mx) {
    prm.out[row * prm.V + prm.v0 + c] = (w > 0.f) ? s / w : 0.f;
    if (c == 0 && prm.v0 == 0 && prm.softmin) prm.softmin[row] = xd_dist_plan_softmin(prm, w, mx);
}

// t^2 |x_i - y_j|^2 of global row i and global column j on explicit differences of the caller's points (D and the dtype at run time)
__device__ __forceinline__ float xd_dist_plan_exact_d2(const XdDistPlanParams& prm, long i, long j, int D) {
    if (prm.bf16) return xk_dist_exact_d2<bf16_t>(static_cast<const bf16_t*>(prm.x) + i * D, static_cast<const bf16_t*>(prm.y) + j * D, D, prm.t);
    return xk_dist_exact_d2<float>(static_cast<const float*>(prm.x) + i * D, static_cast<const float*>(prm.y) + j * D, D, prm.t);
}

// The rows of a call as x-side distance records (scalar item n_i, coordinates -2 t (x_i - centre)), and n_i.  Rows i >= N of the last
// group are zero points (their results are not stored).
template <int D, typename T>
__global__ void __launch_bounds__(kBlock)
xd_dist_plan_pack_rows_kernel(const T* __restrict__ x, int N, float t, XdPacked pk, float* __restrict__ nrow) {
    using S = XdShape<D>;
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ((N + 31) & ~31)) return;
    float centre[D], a[D], n = 0.f;
    launch_centre<D, T>(x, b, N, centre);
#pragma unroll
    for (int d = 0; d < D; ++d) a[d] = 0.f;
    if (i < N) {
        float xi[D];
        load_point<D, T>(x, (long)b * N + i, xi);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float xs = (xi[d] - centre[d]) * t;
            n = __builtin_fmaf(xs, xs, n);
            a[d] = -2.f * xs;
        }
        nrow[(long)b * N + i] = n;
    }
    uint4* base = pk.rec + b * pk.stride + (long)(i >> 5) * S::kGroupRecs + (i & 31);
#pragma unroll
    for (int r = 0; r < S::NBP; ++r) base[r * 32] = xd_record_of<D, true>(r, n, a);
}

// The columns of a call: y-side distance records (scalar item N_j, coordinates t (y_j - centre)) and S_j.  Columns j >= M of the last group:
// the centre itself, S = -inf.
template <int D, typename T>
__global__ void __launch_bounds__(kBlock)
xd_dist_plan_pack_cols_kernel(const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ h, int N, int M, float t, XdPacked pk,
                              float* __restrict__ ys) {
    using S = XdShape<D>;
    const int b = blockIdx.y;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int mpad = (M + 31) & ~31;
    if (j >= mpad) return;
    float centre[D], yt[D], n2 = 0.f, sj = -__builtin_inff();
    launch_centre<D, T>(x, b, N, centre);
#pragma unroll
    for (int d = 0; d < D; ++d) yt[d] = 0.f;
    if (j < M) {
        float yj[D];
        load_point<D, T>(y, (long)b * M + j, yj);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            yt[d] = (yj[d] - centre[d]) * t;
            n2 = __builtin_fmaf(yt[d], yt[d], n2);
        }
        sj = h[(long)b * M + j] * kLog2e;
    }
    ys[(long)b * mpad + j] = sj;
    uint4* base = pk.rec + b * pk.stride + (long)(j >> 5) * S::kGroupRecs + (j & 31);
#pragma unroll
    for (int r = 0; r < S::NBP; ++r) base[r * 32] = xd_record_of<D, false>(r, n2, yt);
}

// The features v0 .. v0 + nv - 1 of a pass as A operands of plan_chunk_mfma: one thread per (column group G, feature c of the VC = 32 NCH
// the pass carries) reads the 32 values of its item (coalesced along c), zeroes those of the columns without mass (S_j = -inf: h_j = -inf
// or padding) and of the features beyond nv, takes the item's power-of-two scale and writes its eight records — column jj of a group is
// instruction jj / 16, lane half (jj / 4) % 2, f16 number 4 ((jj / 8) % 2) + jj % 4 of the record of feature c — and the inverse scale.
__global__ void __launch_bounds__(kBlock)
xd_dist_plan_pack_feat_kernel(const float* __restrict__ feat, const float* __restrict__ ys, int M, int V, int v0, int nv, int VC,
                              uint4* __restrict__ qrec, long qstride, float* __restrict__ qinv) {
    const int b = blockIdx.y;
    const int groups = (M + 31) >> 5;
    const long id = (long)blockIdx.x * kBlock + threadIdx.x;
    if (id >= (long)groups * VC) return;
    const int G = (int)(id / VC), c = (int)(id - (long)G * VC);
    const float* sg = ys + ((long)b * groups + G) * 32;
    float f[32];
    uint32_t mx = 0u;
#pragma unroll
    for (int jj = 0; jj < 32; ++jj) {
        const int j = G * 32 + jj;
        float v = 0.f;
        if (c < nv && j < M && sg[jj] != -__builtin_inff()) v = feat[((long)b * M + j) * V + v0 + c];
        f[jj] = v;
        mx = max(mx, __float_as_uint(v) & 0x7FFFFFFFu);
    }
    const uint32_t se = plan_scale_exponent(mx);
    const float sc = __uint_as_float(se << 23);
    qinv[((long)b * groups + G) * VC + c] = __uint_as_float((254u - (uint32_t)kWqShift - se) << 23);
    uint4* base = qrec + b * qstride + (long)G * (8 * VC) + (c >> 5) * 256 + (c & 31);
#pragma unroll
    for (int I = 0; I < 2; ++I) {
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
            Pack16h hi, lo;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float v = f[16 * I + 8 * (k >> 2) + 4 * hq + (k & 3)] * sc;
                const _Float16 vh = (_Float16)v;
                hi.v[k] = vh;
                lo.v[k] = (_Float16)(v - (float)vh);
            }
            base[I * 64 + hq * 32] = hi.u;
            base[128 + I * 64 + hq * 32] = lo.u;
        }
    }
}

template <int NM, int NCH>
__global__ void __launch_bounds__(kXdDistPlanThreads, xd_dist_plan_waves(NM, NCH))
xd_dist_plan_kernel(XdDistPlanParams prm, int N, int M, int D, SplitInfo sp) {
    constexpr int kG = xd_dist_plan_groups(NM, NCH), kTileD = 32 * kG, VC = 32 * NCH;
    constexpr int kYRecs = kG * 64 * NM, kQRecs = kG * 256 * NCH;      // records per tile buffer
    constexpr int kSF = (kG * 32 + 63) & ~63, kIF = (kG * VC + 63) & ~63;      // floats per tile buffer, in whole LDS-DMA instructions
    static_assert(NCH == 1 || NCH == 2 || NCH == 4, "1, 2 or 4 chunks of 32 features per pass");
    __shared__ uint4 tileY[2 * kYRecs];
    __shared__ uint4 tileQ[2 * kQRecs];
    __shared__ __attribute__((aligned(16))) float tileS[2 * kSF];
    __shared__ __attribute__((aligned(16))) float tileI[2 * kIF];

    int bx, b, split;
    workgroup_coords(sp, bx, b, split);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int ns = sp.n_splits;

    const int row0 = bx * kXdDistPlanRows;
    const int row_end = min(N, row0 + kXdDistPlanRows);
    const int wave_row0 = row0 + wave * 32;
    const bool wave_active = wave_row0 < row_end;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // the x-side records of this wavefront's 32 rows, resident for the whole sweep (a tile past the last group repeats the last one), and
    // the near-pair threshold of the lane's row (a lane past the last row repeats it: in bounds, never stored)
    uint4 X[NM];
    {
        const int G = min(wave_row0 >> 5, (N - 1) >> 5);
        const uint4* xs = prm.xrec + b * prm.xstride + (long)G * (64 * NM) + lane;
#pragma unroll
        for (int mm = 0; mm < NM; ++mm) X[mm] = xs[mm * 64];
    }
    const long row_lane = (long)b * N + min(wave_row0 + l31, N - 1);
    const float thr = fmaxf(prm.guard * prm.nrow[row_lane], 4.f * prm.clamp2);
    f32x16 pacc[NCH];                                         // running sums, relative to 2^m
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) pacc[ch] = zero16;
    float mass4[4] = {0.f, 0.f, 0.f, 0.f};                    // Z times 2^kWqShift
    float m = kMinusHuge;                                     // the running maximum of u (both lane halves of a row hold the same value)

    // this split's columns: whole groups of 32, like the packed layout
    const int groups = (M + 31) >> 5;
    const int len = (((M + ns - 1) / ns) + 31) & ~31;
    const int js = (int)min((long)M, (long)split * len);
    const int je = (int)min((long)M, (long)js + len);
    const float* ysb = prm.ys + (long)b * groups * 32;
    const float* qib = prm.qinv + (long)b * groups * VC;
    auto stage = [&](int j0, int buf) {
        const int nGs = (min(kTileD, je - j0) + 31) >> 5;
        const int g0 = j0 >> 5;
        const uint4* ysrc = prm.yrec + b * prm.ystride + (long)g0 * (64 * NM);
        const uint4* qsrc = prm.qrec + b * prm.qstride + (long)g0 * (256 * NCH);
        for (int c = wave; c < nGs * NM; c += 8) glds16(ysrc + c * 64 + lane, &tileY[buf * kYRecs + c * 64]);
        for (int c = wave; c < nGs * 4 * NCH; c += 8) glds16(qsrc + c * 64 + lane, &tileQ[buf * kQRecs + c * 64]);
        // (a last instruction that reaches past the tile's floats repeats the array's last one: inside the arrays and inside the buffer)
        for (int c = wave; c < (nGs * 32 + 63) >> 6; c += 8)
            glds4(ysb + min((long)g0 * 32 + c * 64 + lane, (long)groups * 32 - 1), &tileS[buf * kSF + c * 64]);
        for (int c = wave; c < (nGs * VC + 63) >> 6; c += 8)
            glds4(qib + min((long)g0 * VC + c * 64 + lane, (long)groups * VC - 1), &tileI[buf * kIF + c * 64]);
    };
    if (js < je) stage(js, 0);

    int tl = 0;
    for (int j0 = js; j0 < je; j0 += kTileD, ++tl) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's share of tile tl has landed ...
        __syncthreads();                                      // ... and so has everybody's; tile tl - 1 is consumed
        if (j0 + kTileD < je) stage(j0 + kTileD, (tl + 1) & 1);
        if (!wave_active) continue;
        const int buf = tl & 1;
        const int nG = (min(kTileD, je - j0) + 31) >> 5;
        for (int G = 0; G < nG; ++G) {
            f32x16 d2 = xd_block<NM, 2 * NM>(&tileY[buf * kYRecs + G * (64 * NM)], lane, X, zero16);
            // ---- near pairs: the owner patches its d2 with the exact value, from the caller's points (padded columns are never re-read)
            if (prm.guard > 0.f && __any(min16(d2) < thr)) {
                uint32_t near = 0u;
#pragma unroll
                for (int k = 15; k >= 0; --k) near = (near << 1) | (d2[k] < thr ? 1u : 0u);
                const int col0 = j0 + G * 32;
                while (near != 0u) {
                    const int k = __builtin_ctz(near);
                    near &= near - 1u;
                    const int j = col0 + reg_column(k, half);
                    if (j < M) {
                        const float e = fmaxf(xd_dist_plan_exact_d2(prm, row_lane, (long)b * M + j, D), prm.clamp2);
#pragma unroll
                        for (int kk = 0; kk < 16; ++kk) d2[kk] = (kk == k) ? e : d2[kk];
                    }
                }
            }
            // ---- u = S_j - dist in place: four broadcast 16-byte reads of the dual values
            const float* sg = &tileS[buf * kSF + G * 32 + half * 4];
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
            plan_rescale(bm, m, pacc, mass4);                 // lazy: only when the maximum grew
            // ---- weights: Z from the unsplit fp32 weights, two f16 pieces for the product
            Pack16h whi[2], wlo[2];
#pragma unroll
            for (int k = 0; k < 16; k += 2) {
                const f32x2_t w = {fast_exp2(d2[k] - m) * (float)(1 << kWqShift), fast_exp2(d2[k + 1] - m) * (float)(1 << kWqShift)};
                mass4[k & 3] += w[0];
                mass4[(k & 3) + 1] += w[1];
                plan_split_weights(w, k, whi, wlo);
            }
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const f32x16 tt = plan_chunk_mfma(&tileQ[buf * kQRecs + G * (256 * NCH) + ch * 256 + lane], whi, wlo);
                // register r <-> feature reg_feature(r, half) of the chunk: four broadcast 16-byte reads of the inverse scales
                const float* ig = &tileI[buf * kIF + G * VC + ch * 32 + half * 4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 i4 = *reinterpret_cast<const float4*>(ig + q * 8);
                    pacc[ch][4 * q + 0] = __builtin_fmaf(tt[4 * q + 0], i4.x, pacc[ch][4 * q + 0]);
                    pacc[ch][4 * q + 1] = __builtin_fmaf(tt[4 * q + 1], i4.y, pacc[ch][4 * q + 1]);
                    pacc[ch][4 * q + 2] = __builtin_fmaf(tt[4 * q + 2], i4.z, pacc[ch][4 * q + 2]);
                    pacc[ch][4 * q + 3] = __builtin_fmaf(tt[4 * q + 3], i4.w, pacc[ch][4 * q + 3]);
                }
            }
        }
    }
    if (!wave_active) return;

    // ---- the two lane halves meet (they hold the two 16-column halves of every block, and the same m) ----
    float z = (mass4[0] + mass4[1]) + (mass4[2] + mass4[3]);
    z += __shfl_xor(z, 32, 64);
    z *= 1.0f / (float)(1 << kWqShift);                       // relative to 2^m
    const int i = wave_row0 + l31;
    if (i >= row_end) return;
    const long idx = (long)b * N + i;
    float* orow = prm.out + idx * prm.V + prm.v0;
    float* part = sp.workspace + split * sp.split_stride + idx * (prm.nv + 2);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * ch + reg_feature(r, half);
            if (c < prm.nv) {
                if (ns > 1) part[c] = pacc[ch][r];
                else orow[c] = (z > 0.f) ? pacc[ch][r] / z : 0.f;      // a division: exact where the quotient is
            }
        }
    }
    if (half == 0) {
        if (ns > 1) {
            part[prm.nv] = z;
            part[prm.nv + 1] = m;
        } else if (prm.softmin && prm.v0 == 0) {
            prm.softmin[idx] = xd_dist_plan_softmin(prm, z, m);
        }
    }
}

}  // namespace glhip
