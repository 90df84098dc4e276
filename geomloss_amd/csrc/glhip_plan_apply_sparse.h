// glhip_plan_apply_sparse.h — the transport plan of a p = 2 soft-min applied to a feature matrix on the caller's block-sparse ranges,
// 1 <= D <= 16, B = 1 (the KeOps convention of include/glhip.h):
//
//     out[i][v] = sum_{j in kept(i)} w_ij feat[j][v] / sum_{j in kept(i)} w_ij,      kept(i) = the columns of the intervals of row i's block
//
// The exponent half, the plan half and the numerics are those of plan_apply_kernel (glhip_plan_apply.h), through the same __device__
// pieces: weights relative to the running row maximum times 2^13, two f16 pieces per side and three products = six
// v_mfma_f32_32x32x16_f16 per chunk and 32 x 32 block, a fresh accumulator per block folded in by v_fma, a power-of-two scale per tile
// and feature, features of columns with h = -inf staged as 0.  What is this kernel's own is the work split and the staging:
//
// Rows.  One workgroup per entry of the row-chunk table (build_row_chunks_kernel, glhip_mapreduce.h: chunks of at most kPlanRows = 256
// rows of ONE row block), eight wavefronts of 32 rows; wavefronts beyond the chunk's rows stage and idle.  The centre of the expansion
// is the chunk's first row: with cluster-sorted clouds the offsets are a few cluster diameters long, which is what keeps the f16 x 2
// layout in range.  Columns are staged on the fly for that reason: a pre-packed record would carry one centre.
// Should the table overflow (overlapping row blocks; chunks[0] < 0) a workgroup owns a whole row block and takes it 256 rows at a time.
//
// Columns.  The workgroup walks the CSR slice of its row block, split s of ns taking the intervals q = s (mod ns).  Voxel clusters are
// short (45 points at N = 1e5, 450 at 1e6) next to a tile of 128 (64) columns, and a tile is what three barriers and six MFMAs per chunk
// and block are paid for: so a tile GATHERS consecutive intervals until it is full (gather_tile, glhip_softmin_x32.h; SplitInfo::gather,
// decided per launch on the host), or takes one piece of one interval (long intervals: the linear path, the tiles of the dense kernel).
// Either way the tile's columns go through a per-tile index list in LDS, tileCol[2][kTile], -1 in its padding slots: the thread of slot t
// loads point and dual value of column tileCol[t], and a feature item reads its four columns with one ds_read_b128.  Padding slots get
// H = -inf and zero features and never raise a feature scale, exactly as the padding of the dense kernel's last tile.  The list of tile
// t + 1 is written between the first two barriers of tile t into the other half of tileCol (last read before the second barrier of tile
// t - 1) and read after the third, where the dense kernel issues its prefetch: no barrier is added, and the loads of the next tile are
// prefetched where plan_apply_kernel prefetches them (PlanShape::kPrefetch; the dual value always one tile ahead).
//
// Chunks per pass: PlanShape::kMaxChunks (up to 128 features for D <= 4, 64 for D <= 11, 32 beyond), except where the list's four column
// indices per feature item push a four-chunk instantiation into scratch that the dense kernel does not use: D = 2, 3 on the bf16 x 3
// layout (20 bytes per lane) and D = 4 on f16 x 2 (24 bytes) run two chunks per pass instead — V = 128 is two passes there
// (plan_sparse_max_chunks).  The next tile's loads are prefetched where the dense kernel prefetches.
//   registers / LDS / scratch of the shipped instantiations, fp32 and bf16 clouds, both layouts (gfx950, the compiler's resource remarks
//   of this unit; per instantiation: profiles/plan_apply_sparse.txt).  LDS is the dense kernel's plus the list, 1 KiB (0.5 at NCH = 4):
//     NCH = 1: 124-180 VGPRs (<= 128 for D <= 3 with fp32 clouds: 4 wavefronts per SIMD; 2-3 otherwise), 21.4-45.4 KiB of LDS
//     NCH = 2: 194-234 VGPRs (2 wavefronts per SIMD), 37.8-53.8 KiB      (D <= 11)
//     NCH = 4: 253-256 VGPRs (2 wavefronts per SIMD), 36.0-38.0 KiB      (D <= 4, less the three above)
//     scratch: 0 bytes, except the two one-chunk bf16 x 3 instantiations on the 128-VGPR budget with fp32 clouds, D = 2 and D = 3: 8 bytes
//     per lane each (plan_apply_kernel: 20 and 8)
//
// Column splits: a launch whose chunks fill the chip takes none (plan_sparse_splits, glhip_api_plan_sparse.hip); a small one takes the
// rule of every block-sparse launch (choose_splits).  Partials (sums[nv], mass, m) per row and split as in the dense kernel, merged by
// plan_merge_kernel over ALL rows: plan_sparse_fill_kernel first writes the neutral partial (0, 0, -huge) everywhere — or, unsplit,
// zeroes the pass's columns of out and mass — so that rows outside every range come back as 0 and nothing stale is read.  No float
// atomics: results are bit-identical run to run.
#pragma once

#include "glhip_plan_apply.h"

namespace glhip {

// What a launch leaves for the rows no workgroup owns.  Unsplit: zeros in the nv columns of the pass and (first pass) in mass.  Split:
// the neutral partial in every split, which plan_merge_kernel turns into those zeros.
template <typename T>
__global__ void __launch_bounds__(kBlock)
plan_sparse_fill_kernel(PlanParams<T> prm, long rows, SplitInfo sp) {
    const long id = (long)blockIdx.x * kBlock + threadIdx.x;
    const int nv = prm.nv;
    if (sp.n_splits == 1) {
        if (id >= rows * nv) return;
        const long row = id / nv;
        const int c = (int)(id - row * nv);
        prm.out[row * prm.V + prm.v0 + c] = 0.f;
        if (c == 0 && prm.v0 == 0 && prm.mass) prm.mass[row] = 0.f;
        return;
    }
    const int w = nv + 2;
    if (id >= rows * w * sp.n_splits) return;
    const long k = id / (rows * w), e = id - k * (rows * w);
    sp.workspace[k * sp.split_stride + e] = (e % w == nv + 1) ? kMinusHuge : 0.f;
}

// chunks per pass of plan_apply_sparse_kernel: see "Chunks per pass" above
template <int D, int L>
constexpr int plan_sparse_max_chunks() {
    return ((L == XL_BF16X3 && (D == 2 || D == 3)) || (L == XL_F16X2 && D == 4)) ? 2 : PlanShape<D, 1, L>::kMaxChunks;
}

template <int D, typename T, int NCH, int L>
__global__ void __launch_bounds__(kPlanNW * 64, (PlanShape<D, NCH, L>::template waves<T>()))
plan_apply_sparse_kernel(PlanParams<T> prm, Ranges rg, int N, int M, SplitInfo sp) {
    using S = PlanShape<D, NCH, L>;
    constexpr int NM = S::NM, NBP = S::NBP, kTileD = S::kTile, kGroups = kTileD / 32;
    constexpr int kThreads = kPlanNW * 64;
    constexpr int VC = 32 * NCH;
    constexpr int kItems = (kTileD / 4) * VC / kThreads;      // (column quad, feature) items per thread and tile: 2, 4, 4
    static_assert(kTileD <= kThreads, "one column per thread");
    static_assert(kItems * kThreads == (kTileD / 4) * VC, "whole items per thread");
    __shared__ uint4 tile[kTileD * NBP];                 // exponent records: [column group of 32][K block][column]
    __shared__ uint4 tileQ[kGroups * S::kQRecs];         // feature A operands: [group][chunk][piece][instruction][lane = 32 h + c] x 8 f16
    __shared__ uint32_t tileMax[2][VC];                  // largest |f| bit pattern per feature, tiles of even / odd index
    __shared__ __attribute__((aligned(16))) float tileInv[VC];      // 2^-13 / scale of the current tile, per feature
    __shared__ uint32_t tileLive[4];                     // the current tile's columns with mass (h_j > -inf), one bit each
    __shared__ __attribute__((aligned(16))) int tileCol[2][kTileD];      // the columns of the tiles of even / odd index, -1: padding

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = blockIdx.x, split = blockIdx.z;
    const int ns = sp.n_splits;
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const int rec0 = half * 32 + l31;
    const float xscale = (L == XL_F16X2) ? __builtin_sqrtf(prm.s2) : prm.s2;      // f16 x 2: sqrt(s) on both sides (glhip_softmin_xd.h)
    const int pieces = sp.gather ? kTileD : 1;           // interval pieces a tile may hold

    int block_begin, block_end, q_begin, q_end;
    block_extent<true>(rg, N, kPlanRows, block_begin, block_end, q_begin, q_end, bx);
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // (one pass per workgroup with a chunk table; without one, the row block 256 rows at a time)
    for (int row0 = block_begin; row0 < block_end; row0 += kPlanRows) {
        const int row_end = min(block_end, row0 + kPlanRows);
        if (tid < 2 * VC) tileMax[tid / VC][tid % VC] = 0u;

        float centre[D];
        load_point<D, T>(prm.x, (long)row0, centre);

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
            load_point<D, T>(prm.x, (long)i, xi);
            float a[D], n2 = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float xt = xi[d] - centre[d];
                n2 = __builtin_fmaf(xt, xt, n2);
                a[d] = xt * xscale;
            }
            // C_i = r_i - LSE2_i as in plan_apply_kernel; fwd_i = +inf is a row without mass: all its weights are zero
            const float fw = prm.fwd[i];
            float cst = (fw == __builtin_inff()) ? kNegBig : -0.5f * prm.s2 * n2 - fw / prm.out_scale;
            if (L == XL_F16X2) cst = __builtin_fminf(__builtin_fmaxf(cst, kH2Floor), -kH2Floor);
#pragma unroll
            for (int mm = 0; mm < NM; ++mm)
                X[mm] = select_u4(half != 0, xd_record_of<D, true, L>(2 * mm + 1, cst, a), xd_record_of<D, true, L>(2 * mm, cst, a));
        }

        // The global loads of a tile through its column list: this thread's column (point and dual value) and its feature items.
        float yreg[D], hreg = 0.f;
        float fv[kItems][4];
        auto load_tile = [&](const int* cols, int n) {
#pragma unroll
            for (int d = 0; d < D; ++d) yreg[d] = 0.f;
            if (tid < n) load_point<D, T>(prm.y, (long)cols[tid], yreg);
            // item (column quad cq, feature c of the pass) — c runs fastest: the loads of a wavefront are contiguous runs of feat rows
#pragma unroll
            for (int k = 0; k < kItems; ++k) {
                const int it = tid + k * kThreads;
                const int cq = it / VC, c = it - cq * VC;
                const int t = cq << 2;
                const int4 j4 = *reinterpret_cast<const int4*>(cols + t);
                const int jq[4] = {j4.x, j4.y, j4.z, j4.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float f = 0.f;
                    if (t + q < n && c < prm.nv) f = prm.feat[(long)jq[q] * prm.V + prm.v0 + c];
                    fv[k][q] = f;
                }
            }
        };
        auto load_h = [&](const int* cols, int n) {
            if (tid < n) hreg = prm.h[cols[tid]];
        };

        // the walk over the slice: `cur` is where the next tile starts, n / n_next the real columns of the current / next tile
        TileCursor cur;
        cur.q = q_begin + split;
        cur.j0 = cur.je = 0;
        open_interval<true, true>(rg, M, q_end, split, ns, cur);
        int gcol[1], n = 0, n_next = 0;
        cur = gather_tile<1, kThreads, kTileD>(rg, M, q_end, split, ns, cur, tid, gcol, n, pieces);
        __syncthreads();      // the previous pass of this workgroup is through with the lists, the tiles and tileMax
        if (tid < kTileD) tileCol[0][tid] = gcol[0];
        __syncthreads();
        if (n > 0) load_h(tileCol[0], n);
        if (S::kPrefetch && n > 0) load_tile(tileCol[0], n);
        for (int parity = 0; n > 0; n = n_next, parity ^= 1) {
            const int npad = (n + 31) & ~31;
            {   // the tile's columns with mass, for the staging of its features
                const unsigned long long live = __ballot(tid < n && hreg != -__builtin_inff());
                if (lane == 0 && wave < 2) {
                    tileLive[2 * wave] = (uint32_t)live;
                    tileLive[2 * wave + 1] = (uint32_t)(live >> 32);
                }
            }
            __syncthreads();      // the previous tile is consumed
            // the list of the next tile, into the half the tile before this one has left
            cur = gather_tile<1, kThreads, kTileD>(rg, M, q_end, split, ns, cur, tid, gcol, n_next, pieces);
            if (tid < kTileD) tileCol[parity ^ 1][tid] = gcol[0];
            if (!S::kPrefetch) load_tile(tileCol[parity], n);
            if (tid < npad) {
                const int t = tid;
                // padding: H = -inf, which meets nothing finite (plan_apply_kernel)
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
                    H = (H == -__builtin_inff()) ? H : __builtin_fmaxf(H, kH2Floor);
                }
                uint4* base = &tile[(t >> 5) * (32 * NBP) + (t & 31)];
#pragma unroll
                for (int r = 0; r < NBP; ++r) base[r * 32] = xd_record_of<D, false, L>(r, H, yt);
            }
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
                tileMax[parity ^ 1][tid] = 0u;
            }
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
            if (n_next > 0) load_h(tileCol[parity ^ 1], n_next);
            if (S::kPrefetch && n_next > 0) load_tile(tileCol[parity ^ 1], n_next);
            if (!wave_active) continue;

            for (int G = 0; G < npad / 32; ++G) {
                const f32x16 u = xd_block<NM, NBP, L>(&tile[G * (32 * NBP)], rec0, X, zero16);
                float bm = max16(u);
                bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
                if (__any(bm > m)) {      // (inline as in plan_apply_kernel: plan_rescale costs the four-chunk instantiations registers)
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
                const long idx = i;
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
                        prm.mass[idx] = mass * fast_exp2(m);      // (an empty slice: 0 x 2^-huge = 0)
                    }
                }
            }
        }
    }
}

}  // namespace glhip
