// glhip_plan_apply.h — the transport plan of a p = 2 soft-min applied to a feature matrix on the matrix cores, 1 <= D <= 16:
//
//     out[i][v] = sum_j w_ij feat[j][v] / sum_j w_ij,      w_ij = 2^( [a_i,1].[yt_j,H_j] + C_i ),  C_i = r_i - LSE2_i  (glhip_wsum_t32.h)
//
// wsum_t32q_kernel (glhip_wsum_t32.h) already feeds the plan weights of a transposed 32 x 32 exponent block, as they sit in the
// registers, to a second MFMA as its B operand, against an A operand of per-column components staged in LDS — and uses D + 1 <= 17 of
// the 32 MFMA rows, for (y_j, 1).  Here all 32 rows are the caller's features, in chunks of 32 (the last one zero-padded):
//     out[c][i] = sum_j F[c][j] W[j][i],    A = F (feature c = MFMA row, from LDS),  B = W (row i = MFMA column, in registers).
// Lane (half h, i) holds the weights of row i for the 16 columns col(h, r) = 8 (r / 4) + 4 h + r % 4; registers 0..7 are the K slots
// 8 h .. 8 h + 7 of a first instruction, 8..15 of a second one, and the A operand is staged in that same K order: column jj of a group
// is register r = 4 (jj / 8) + jj % 4 of lane half (jj / 4) % 2.  All 16 result registers of a lane are live: register r of lane (h, i)
// is feature c = (r & 3) + 8 (r >> 2) + 4 h of the chunk.
//
// Pieces.  Weights and features are split into TWO f16 pieces each (hi + lo, round to nearest, subnormal pieces kept: 22 significant
// bits) and three products are kept — lo hi, hi lo, hi hi; the dropped lo lo is <= 2^-24 |w f|.  Six v_mfma_f32_32x32x16_f16 per chunk
// and 32 x 32 block, smallest products first (the MFMA truncates the rounding of its accumulation: the early, small partial sums keep
// that bias relative to themselves).  Three bf16 pieces per side would need no scaling at all but six products = twelve MFMAs for the
// same accuracy: 384 matrix-pipe cycles per block next to the ~230 of a whole forward block; weights in two bf16 pieces miss the
// 1e-6 of the model (tools/plan_apply_model.py; this split: <= 2e-7 of sum_j w |f| in the worst column).  f16 has five exponent bits:
//   * weights are taken relative to the running maximum m of their row's exponents and carry 2^13 (kWqShift): w' = 2^13 2^(u - m) <= 8192
//     whatever fwd is worth, the largest weight of a row is 2^13 exactly, and a low piece or a small weight that falls into the f16
//     subnormals is off by 2^-25 of w' units = 2^-38 of the row's largest weight.  A new maximum rescales the running sums;
//   * features get a power-of-two scale per feature column AND LDS tile, computed by the workgroup that stages the tile (one
//     ds_max_u32 per thread and item on the |f| bit patterns, no pre-pass over feat, no host round trip, no workspace): the largest
//     |f| of the tile's 128 (64) columns lands in [2^14, 2^15).  Columns of any magnitude sit next to each other, and a column
//     whose entries span many orders of magnitude along j is rescaled tile by tile.  The inverse scale (times 2^-13) multiplies
//     the block result on its way into the running sums.  The features of a column without mass (h_j = -inf) are staged as 0: they weigh
//     nothing, and a huge one would otherwise set the scale of its tile (plan_live_features, in the tiles that have such a column).
//
// Accumulation: the discipline of wsum_t32q_kernel — a fresh accumulator per 32-column block, folded into the running sums with one
// VALU instruction per register (here v_fma_f32 with the tile's inverse scale, round to nearest); chained through 31 250 blocks the
// MFMA's truncation would grow to 1e-3.  The mass sum_j w_ij is summed from the unsplit fp32 weights on the VALU (16 adds per
// block): no feature slot is spent on it.
//
// Chunks per pass.  The 16 exponentials and the piece conversions of a block (~50 VALU instructions) are shared by the NCH = 1, 2
// or 4 feature chunks a wavefront carries (16 accumulator registers each); wider feature matrices take further passes (launches) of up
// to 128 features.  Eight wavefronts x 32 rows = 256 rows per workgroup share the staged tile.  Features are staged on the fly:
// a thread reads one feature of four consecutive columns (coalesced along V), and after the tile's scales are known writes the two
// pieces as two 8-byte LDS stores.  Three barriers per tile; with two or four chunks the global loads of tile t + 1 are issued before
// the MFMA loop of tile t (PlanShape::kPrefetch).
//   registers / LDS over all D, both layouts, fp32 and bf16 clouds (gfx950, tools/kernel_resources.py, profiles/plan_apply.txt);
//   LDS = 16 NBP bytes of exponent records + 128 NCH bytes of feature pieces per column, tiles of 128 columns (64 for NCH = 4):
//     NCH = 1: 124-177 VGPRs (<= 128 for D <= 3 with fp32 clouds: 4 wavefronts per SIMD; 2-3 otherwise), 20.4-44.4 KiB of LDS
//     NCH = 2: 219-250 VGPRs (2 wavefronts per SIMD), 36.8-52.8 KiB      (D <= 11)
//     NCH = 4: 252-256 VGPRs (2 wavefronts per SIMD), 35.5-37.5 KiB      (D <= 4)
//     scratch: 0 bytes, except the two one-chunk bf16 x 3 instantiations that sit on the 128-VGPR budget with fp32 clouds: D = 2 spills 20
//     bytes per lane, D = 3 8 bytes (the dual value of the next tile's column, held across the MFMA loop); measured cost of the mask of
//     columns without mass: 1.3 % of a pass at NCH = 1, 3.6 % at NCH = 2, 4.3 % at NCH = 4 (profiles/hostile_duals.txt)
//
// Column splits: the SplitLaunch plumbing (glhip_mapreduce.h); the partial of a row is (sums[nv], mass, m), nv = the features of the pass,
// sums and mass relative to 2^m.  The merge brings the splits to the largest m, adds and divides.  Its width is a RUN-TIME
// argument (plan_merge_kernel below, one thread per row and feature) — one merge for every chunk count and any V, instead of one
// MergeOp instantiation per width.
//
// Shared pieces (profiles/xk_plan_pieces.txt).  The plan half exists in five __global__ bodies: plan_apply_kernel here, xk_plan_kernel
// (glhip_plan_apply_xk.h), xk_dist_grad_kernel (glhip_dist_grad_xk.h), xk_dist_plan_kernel (glhip_dist_plan_xk.h) and xk_bilinear_kernel
// (glhip_plan_bilinear_xk.h).  What they share as __device__ __forceinline__ pieces is defined
// here — plan_store_pieces (scale, split and store of one staged feature item), plan_rescale (the lazy rescale; this kernel keeps its
// inline text: the helper costs the four-chunk instantiations 2 VGPRs), plan_split_weights, plan_chunk_mfma (the six MFMAs of a chunk) —
// next to the register maps reg_column / reg_feature of glhip_klayout.h.  The staging loops, the fold of a fresh accumulator into the running
// sums and the meeting of the column halves stay in each body: as pieces they moved registers in one kernel or another.
#pragma once

#include "glhip_softmin_xd.h"
#include "glhip_wsum_t32.h"

namespace glhip {

template <typename T>
struct PlanParams {
    const T* x;           // (B,N,D)
    const T* y;           // (B,M,D)
    const float* h;       // (B,M)
    const float* fwd;     // (B,N): the saved soft-min
    const float* feat;    // (B,M,V)
    float* out;           // (B,N,V)
    float* mass;          // (B,N) or NULL
    float s2;             // log2(e) / eps
    float out_scale;      // -eps ln 2: LSE2_i = fwd_i / out_scale
    int V;                // feature columns of feat / out
    int v0;               // first feature of this pass
    int nv;               // features of this pass, <= 32 NCH
};

constexpr int kPlanNW = 8;                       // wavefronts per workgroup, 32 rows each
constexpr int kPlanRows = kPlanNW * 32;
constexpr int kPlanMaxChunks = 4;                // feature chunks per pass

template <int D, int NCH, int L>
struct PlanShape {
    static constexpr int NM = XdShape<D, L>::NM;
    static constexpr int NBP = 2 * NM;
    static constexpr int kTile = NCH == 4 ? 64 : 128;        // columns per LDS tile
    static constexpr int kQRecs = NCH * 4 * 64;              // 16-byte feature records per column group: [chunk][piece][instruction][lane]
    // One chunk: the loads of a tile are issued when it is staged, which leaves D <= 3 within 128 VGPRs — 4 wavefronts per SIMD, two
    // workgroups per CU, one staging while the other multiplies; with the prefetch below and one workgroup per CU a pass measured
    // 30 % slower.  Two and four chunks: the loads are issued one tile ahead, right before the MFMA loop of the tile in LDS (D + 1 +
    // 4 NCH .. 16 more live registers), on a budget of 256 VGPRs = one workgroup per CU (V = 128: 22 % faster than without).
    static constexpr bool kPrefetch = NCH > 1;
    static constexpr int kWaves = (NCH == 1 && D <= 3) ? 4 : 2;      // wavefronts per SIMD the register budget is set for (fp32 clouds)
    // bf16 clouds: 2 everywhere (D = 2 spills 8 bytes at 128 VGPRs)
    template <typename T> static constexpr int waves() { return sizeof(T) == 2 ? 2 : kWaves; }
    // chunks per pass that fit 256 VGPRs without scratch next to the x-side operands of NM chained MFMAs and the prefetch registers:
    // four up to D = 4, two up to D = 11, one beyond
    static constexpr int kMaxChunks = D <= 4 ? 4 : (D <= 11 ? 2 : 1);
};

// The power-of-two scale of a feature column within a tile, from the bit pattern of its largest |f|: the scaled maximum lies in
// [2^14, 2^15).  Returned as biased exponents of the scale (se) — the inverse, times 2^-kWqShift, has 254 - kWqShift - se.
__device__ __forceinline__ uint32_t plan_scale_exponent(uint32_t max_bits) {
    const int e = (int)(max_bits >> 23);                     // biased exponent of the maximum (0: zero or subnormal)
    const int se = 127 + 14 - (e - 127);
    return (uint32_t)min(max(se, 1), 254 - kWqShift - 1);
}

// ---- The pieces of the plan half.  plan_apply_kernel below, xk_plan_kernel (glhip_plan_apply_xk.h), xk_dist_grad_kernel
// (glhip_dist_grad_xk.h) and xk_dist_plan_kernel (glhip_dist_plan_xk.h) are four __global__ bodies that call them (plan_rescale: the
// latter three); each is __device__ __forceinline__ and holds no barrier. ----

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// Feature c of four consecutive columns — K slots s0 .. s0 + 3 of one lane half and one instruction — under the power-of-two scale sc,
// in two f16 pieces: the high one at qb, the low one a piece further ([piece][instruction][lane]: 128 records = 256 uint2 per piece)
__device__ __forceinline__ void plan_store_pieces(const float (&f)[4], float sc, uint2* qb) {
    const f32x2_t v01 = {f[0] * sc, f[1] * sc}, v23 = {f[2] * sc, f[3] * sc};
    const f16x2_t h01 = __builtin_convertvector(v01, f16x2_t), h23 = __builtin_convertvector(v23, f16x2_t);
    const f16x2_t l01 = __builtin_convertvector(v01 - __builtin_convertvector(h01, f32x2_t), f16x2_t);
    const f16x2_t l23 = __builtin_convertvector(v23 - __builtin_convertvector(h23, f32x2_t), f16x2_t);
    qb[0] = uint2{__builtin_bit_cast(uint32_t, h01), __builtin_bit_cast(uint32_t, h23)};
    qb[256] = uint2{__builtin_bit_cast(uint32_t, l01), __builtin_bit_cast(uint32_t, l23)};
}

// The features of a column without mass (h_j = -inf) are staged as 0, whatever finite value they hold: their weight is 0, and left in, a
// large one would set the power-of-two scale of its tile and push the features of the columns that do carry mass below the f16 pieces.
// A staged item of four consecutive columns t .. t + 3 (t a multiple of 4), from the tile's mask of columns with mass: bit c of
// live[c / 32], as the wavefronts that hold the dual values of the tile's columns published it (the halves of their `__ballot`).
__device__ __forceinline__ void plan_live_features(float (&f)[4], const uint32_t* live, int t) {
    const uint32_t bits = live[t >> 5] >> (t & 31);
#pragma unroll
    for (int q = 0; q < 4; ++q) f[q] = ((bits >> q) & 1u) ? f[q] : 0.f;
}

// A block whose row maximum bm (the same in both lane halves of a row) passes the running maximum m of some row of the wavefront
// brings the running sums and every four-register scalar to the new maximum: factor exactly 1 for the rows that keep theirs.
template <int NCH, class... Scal4>
__device__ __forceinline__ void plan_rescale(float bm, float& m, f32x16 (&acc)[NCH], Scal4&... scal4) {
    if (!__any(bm > m)) return;
    const float mn = fmaxf(m, bm);
    const float rs = fast_exp2(m - mn);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ch][r] *= rs;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) ((scal4[k] *= rs), ...);
    m = mn;
}

// Two weights into their two f16 pieces, K slots k and k + 1 of the B operands: one v_cvt_pk_f16_f32 per two high pieces, both read
// back from it (wsum_t32q_kernel)
__device__ __forceinline__ void plan_split_weights(f32x2_t w, int k, Pack16h (&whi)[2], Pack16h (&wlo)[2]) {
    const f16x2_t hh = __builtin_convertvector(w, f16x2_t);
    const f32x2_t back = __builtin_convertvector(hh, f32x2_t);
    const f16x2_t ll = __builtin_convertvector(w - back, f16x2_t);
    whi[k >> 3].v[k & 7] = hh[0];
    whi[k >> 3].v[(k & 7) + 1] = hh[1];
    wlo[k >> 3].v[k & 7] = ll[0];
    wlo[k >> 3].v[(k & 7) + 1] = ll[1];
}

// One chunk of 32 features times the weights of a 32-column block, into a fresh accumulator: six v_mfma_f32_32x32x16_f16.  qg: this
// lane's records of the chunk (piece p, instruction I: qg[p * 128 + I * 64]).  The fold into the running sums stays with the caller.
__device__ __forceinline__ f32x16 plan_chunk_mfma(const uint4* qg, const Pack16h (&whi)[2], const Pack16h (&wlo)[2]) {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    Pack16h qh0, qh1, ql0, ql1;
    qh0.u = qg[0]; qh1.u = qg[64]; ql0.u = qg[128]; ql1.u = qg[192];
    // smallest products first: lo hi, hi lo, hi hi
    f32x16 t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ql0.v, whi[0].v, zero16, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ql1.v, whi[1].v, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh0.v, wlo[0].v, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh1.v, wlo[1].v, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh0.v, whi[0].v, t, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(qh1.v, whi[1].v, t, 0, 0, 0);
}

template <int D, typename T, int NCH, int L>
__global__ void __launch_bounds__(kPlanNW * 64, (PlanShape<D, NCH, L>::template waves<T>()))
plan_apply_kernel(PlanParams<T> prm, int N, int M, SplitInfo sp) {
    using S = PlanShape<D, NCH, L>;
    constexpr int NM = S::NM, NBP = S::NBP, kTileD = S::kTile, kGroups = kTileD / 32;
    constexpr int kThreads = kPlanNW * 64;
    constexpr int VC = 32 * NCH;
    constexpr int kItems = (kTileD / 4) * VC / kThreads;      // (column quad, feature) items per thread and tile: 2, 4, 4
    static_assert(kTileD <= kThreads, "one column per thread");
    static_assert(NCH == 1 || NCH == 2 || NCH == 4, "1, 2 or 4 chunks of 32 features per pass");
    static_assert(kItems * kThreads == (kTileD / 4) * VC, "whole items per thread");
    __shared__ uint4 tile[kTileD * NBP];                 // exponent records: [column group of 32][K block][column]
    __shared__ uint4 tileQ[kGroups * S::kQRecs];         // feature A operands: [group][chunk][piece][instruction][lane = 32 h + c] x 8 f16
    __shared__ uint32_t tileMax[2][VC];                  // largest |f| bit pattern per feature, tiles of even / odd index
    __shared__ __attribute__((aligned(16))) float tileInv[VC];      // 2^-13 / scale of the current tile, per feature
    __shared__ uint32_t tileLive[4];                     // the current tile's columns with mass (h_j > -inf), one bit each

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int bx, b, split;
    workgroup_coords(sp, bx, b, split);
    const int ns = sp.n_splits;
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const int rec0 = half * 32 + l31;
    const float xscale = (L == XL_F16X2) ? __builtin_sqrtf(prm.s2) : prm.s2;      // f16 x 2: sqrt(s) on both sides (glhip_softmin_xd.h)
    const Ranges none{nullptr, nullptr, nullptr, nullptr};

    int row_begin, row_end, q_begin, q_end;
    block_extent<false>(none, N, kPlanRows, row_begin, row_end, q_begin, q_end, bx);
    if (row_begin >= row_end) return;
    const int row0 = row_begin;

    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (tid < 2 * VC) tileMax[tid / VC][tid % VC] = 0u;

    float centre[D];
    load_point<D, T>(prm.x, (long)b * N + row0, centre);

    const int wave_row0 = row0 + wave * 32;
    const bool wave_active = wave_row0 < row_end;
    uint4 X[NM];
    f32x16 acc[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) acc[ch] = zero16;
    float mass4[4] = {0.f, 0.f, 0.f, 0.f};
    float m = kMinusHuge;      // running maximum of the row's exponents (both lane halves of a row hold the same value)
    {
        const int i = min(wave_row0 + l31, row_end - 1);
        float xi[D];
        load_point<D, T>(prm.x, (long)b * N + i, xi);
        float a[D], n2 = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float xt = xi[d] - centre[d];
            n2 = __builtin_fmaf(xt, xt, n2);
            a[d] = xt * xscale;
        }
        // C_i = r_i - LSE2_i, r_i = -s/2 |xt_i|^2, LSE2_i = fwd_i / out_scale.  fwd_i = +inf is a row
        // without mass (every h_j = -inf): all its weights are zero
        const float fw = prm.fwd[(long)b * N + i];
        float cst = (fw == __builtin_inff()) ? kNegBig : -0.5f * prm.s2 * n2 - fw / prm.out_scale;
        if (L == XL_F16X2) cst = __builtin_fminf(__builtin_fmaxf(cst, kH2Floor), -kH2Floor);
#pragma unroll
        for (int mm = 0; mm < NM; ++mm)     // scalar item [1,1,1,c1,c2,c3], then the slots of every coordinate (xd_record_of)
            X[mm] = select_u4(half != 0, xd_record_of<D, true, L>(2 * mm + 1, cst, a), xd_record_of<D, true, L>(2 * mm, cst, a));
    }

    int js, je;
    column_interval<false>(none, M, 0, split, ns, js, je);
    // The global loads of a tile: this thread's column (point and dual value) and its feature items.  kPrefetch: issued one tile
    // ahead, right before the MFMA loop of the tile in LDS, so that they land while it runs.
    float yreg[D], hreg = 0.f;
    float fv[kItems][4];
    auto load_tile = [&](int j0) {
        const int n = min(kTileD, je - j0);
#pragma unroll
        for (int d = 0; d < D; ++d) yreg[d] = 0.f;
        if (tid < n) load_point<D, T>(prm.y, (long)b * M + j0 + tid, yreg);
        // features: item (column quad cq, feature c of the pass) — c runs fastest, so the four loads of a wavefront are contiguous runs
        // of feat rows
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int it = tid + k * kThreads;
            const int cq = it / VC, c = it - cq * VC;
            const int t = cq << 2;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float f = 0.f;
                if (t + q < n && c < prm.nv) f = prm.feat[((long)b * M + j0 + t + q) * prm.V + prm.v0 + c];
                fv[k][q] = f;
            }
        }
    };
    // The dual value of this thread's column is always loaded one tile ahead: the wavefronts that hold them publish, before the first barrier
    // of a tile, which of its columns carry mass (h_j > -inf).
    auto load_h = [&](int j0) {
        if (tid < min(kTileD, je - j0)) hreg = prm.h[(long)b * M + j0 + tid];
    };
    if (js < je) load_h(js);
    if (S::kPrefetch && js < je) load_tile(js);
    int parity = 0;
    for (int j0 = js; j0 < je; j0 += kTileD, parity ^= 1) {
        const int n = min(kTileD, je - j0);
        const int npad = (n + 31) & ~31;
        {   // the tile's columns with mass, for the staging of its features (read between the next two barriers; the previous tile's mask
            // was last read before the second barrier of its iteration)
            const unsigned long long live = __ballot(tid < n && hreg != -__builtin_inff());
            if (lane == 0 && wave < 2) {
                tileLive[2 * wave] = (uint32_t)live;
                tileLive[2 * wave + 1] = (uint32_t)(live >> 32);
            }
        }
        __syncthreads();      // the previous tile is consumed (and, the first time, tileMax is zero)
        if (!S::kPrefetch) load_tile(j0);
        if (tid < npad) {     // (kTileD <= 128 columns: one per thread)
            const int t = tid;
            // padded columns: H = -inf, not the kNegBig of the other kernels — the forward counts ITS padded columns (H = -1e30) into a row
            // whose real columns all carry h = -inf and returns fwd_i ~ 7e27 for it: C_i = +1e30 here, which must meet nothing finite
            float yt[D], H = -__builtin_inff();
#pragma unroll
            for (int d = 0; d < D; ++d) yt[d] = 0.f;
            if (t < n) {
                float n2 = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    yt[d] = yreg[d] - centre[d];
                    n2 = __builtin_fmaf(yt[d], yt[d], n2);
                }
                H = __builtin_fmaf(-0.5f * prm.s2, n2, hreg * kLog2e);
            }
            if (L == XL_F16X2) {
#pragma unroll
                for (int d = 0; d < D; ++d) yt[d] *= xscale;
                // (-inf stays -inf — it survives the f16 pieces and the MFMA, and meets only finite row constants: columns without
                // mass and padded columns weigh exactly 0 in this layout too, whatever fwd_i is)
                H = (H == -__builtin_inff()) ? H : __builtin_fmaxf(H, kH2Floor);
            }
            uint4* base = &tile[(t >> 5) * (32 * NBP) + (t & 31)];
#pragma unroll
            for (int r = 0; r < NBP; ++r) base[r * 32] = xd_record_of<D, false, L>(r, H, yt);
        }
        // (nearly every tile: all n columns carry mass, and the features stay as they were loaded)
        const bool voids = __popc(tileLive[0]) + __popc(tileLive[1]) + __popc(tileLive[2]) + __popc(tileLive[3]) != n;
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int it = tid + k * kThreads;
            const int cq = it / VC, c = it - cq * VC;
            uint32_t mx = 0u;
            if (voids) plan_live_features(fv[k], tileLive, cq << 2);
#pragma unroll
            for (int q = 0; q < 4; ++q) mx = max(mx, __float_as_uint(fv[k][q]) & 0x7FFFFFFFu);
            if ((cq << 2) < npad && mx) atomicMax(&tileMax[parity][c], mx);
        }
        __syncthreads();      // the tile's maxima are complete
        if (tid < VC) {
            const uint32_t se = plan_scale_exponent(tileMax[parity][tid]);
            tileInv[tid] = __uint_as_float((254u - (uint32_t)kWqShift - se) << 23);
            tileMax[parity ^ 1][tid] = 0u;      // for the next tile: last read before the barrier above of the previous tile
        }
        // columns 4 cq .. 4 cq + 3 of a group are K slots s0 .. s0 + 3 of one lane half and one instruction
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int it = tid + k * kThreads;
            const int cq = it / VC, c = it - cq * VC;
            const int t = cq << 2;
            if (t < npad) {
                const float sc = __uint_as_float(plan_scale_exponent(tileMax[parity][c]) << 23);
                const int jj = t & 31;
                const int r = (jj >> 3) << 2, hq = (jj >> 2) & 1;
                uint2* qb = reinterpret_cast<uint2*>(&tileQ[(t >> 5) * S::kQRecs + (c >> 5) * (4 * 64) + (r >> 3) * 64 + hq * 32 + (c & 31)]) + ((r & 7) >> 2);
                plan_store_pieces(fv[k], sc, qb);
            }
        }
        __syncthreads();
        if (j0 + kTileD < je) load_h(j0 + kTileD);
        if (S::kPrefetch && j0 + kTileD < je) load_tile(j0 + kTileD);
        if (!wave_active) continue;

        for (int G = 0; G < npad / 32; ++G) {
            const f32x16 u = xd_block<NM, NBP, L>(&tile[G * (32 * NBP)], rec0, X, zero16);
            // weights relative to the running maximum of the row: w' = 2^13 2^(u - m) <= 8192 whatever fwd is worth, and the largest
            // weight of a row is 2^13 EXACTLY (u - m = 0 on the VALU) — a one-hot plan row returns its features bit for bit.  A new
            // maximum rescales the running sums (factor exactly 1 for the rows of the wavefront that keep theirs)
            float bm = max16(u);
            bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
            if (__any(bm > m)) {
                const float mn = fmaxf(m, bm);
                const float rs = fast_exp2(m - mn);
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[ch][r] *= rs;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) mass4[k] *= rs;
                m = mn;
            }
            Pack16h whi[2], wlo[2];
#pragma unroll
            for (int k = 0; k < 16; k += 2) {
                const f32x2_t w = {fast_exp2(u[k] - m) * (float)(1 << kWqShift), fast_exp2(u[k + 1] - m) * (float)(1 << kWqShift)};
                mass4[k & 3] += w[0];
                mass4[(k & 3) + 1] += w[1];
                plan_split_weights(w, k, whi, wlo);
            }
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const f32x16 t = plan_chunk_mfma(&tileQ[G * S::kQRecs + ch * (4 * 64) + lane], whi, wlo);
                // register r <-> feature reg_feature(r, half) of the chunk: four broadcast 16-byte reads of the inverse scales
                const float* ig = &tileInv[ch * 32 + half * 4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 i4 = *reinterpret_cast<const float4*>(ig + q * 8);
                    acc[ch][4 * q + 0] = __builtin_fmaf(t[4 * q + 0], i4.x, acc[ch][4 * q + 0]);
                    acc[ch][4 * q + 1] = __builtin_fmaf(t[4 * q + 1], i4.y, acc[ch][4 * q + 1]);
                    acc[ch][4 * q + 2] = __builtin_fmaf(t[4 * q + 2], i4.z, acc[ch][4 * q + 2]);
                    acc[ch][4 * q + 3] = __builtin_fmaf(t[4 * q + 3], i4.w, acc[ch][4 * q + 3]);
                }
            }
        }
    }

    if (wave_active) {
        float mass = (mass4[0] + mass4[1]) + (mass4[2] + mass4[3]);
        mass += __shfl_xor(mass, 32, 64);      // the two 16-column halves
        mass *= 1.0f / (float)(1 << kWqShift);      // relative to 2^m
        const int i = wave_row0 + l31;
        if (i < row_end) {
            const long idx = (long)b * N + i;
            float* orow = prm.out + idx * prm.V + prm.v0;
            float* part = sp.workspace + split * sp.split_stride + idx * (prm.nv + 2);
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = 32 * ch + reg_feature(r, half);
                    if (c < prm.nv) {
                        if (ns == 1) orow[c] = (mass > 0.f) ? acc[ch][r] / mass : 0.f;      // a division: exact where the quotient is
                        else part[c] = acc[ch][r];
                    }
                }
            }
            if (half == 0) {
                if (ns > 1) {
                    part[prm.nv] = mass;
                    part[prm.nv + 1] = m;
                } else if (prm.mass && prm.v0 == 0) {
                    prm.mass[idx] = mass * fast_exp2(m);
                }
            }
        }
    }
}

// The plan's end of plan_merge_kernel: entry c of the pass in row `row` from the merged sum s and mass w, both relative to 2^mx — divided.
template <typename T>
__device__ __forceinline__ void plan_merge_store(const PlanParams<T>& prm, int, int, long row, int c, float s, float w, float mx) {
    prm.out[row * prm.V + prm.v0 + c] = (w > 0.f) ? s / w : 0.f;
    if (c == 0 && prm.v0 == 0 && prm.mass) prm.mass[row] = w * fast_exp2(mx);
}

// Combines the column splits of a pass of plan_apply_kernel or of xk_plan_kernel (glhip_plan_apply_xk.h) on the parameter struct P: one
// thread per (row, feature).  The partials of a row are nv sums, the mass — both relative to 2^m of their split — and m: the splits are
// brought to the largest m (factor exactly 1 for the split that holds it) and added; plan_merge_store(prm, N, D, ...), overloaded next
// to each parameter struct, puts the sums through the epilogue of its kernel.
template <class P>
__global__ void __launch_bounds__(kBlock)
plan_merge_kernel(P prm, int N, int D, long rows, SplitInfo sp) {
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
    plan_merge_store(prm, N, D, row, c, s, w, mx);
}

}  // namespace glhip
