// glhip_argmin_xk.h — the arg-reduction of the library: for every row the column of the smallest dual-shifted cost,
//   index_i = argmin_j [ |x_i - y_j|^2 / 2 - g_j ],   value_i = that minimum,
// p = 2, clouds of dimension 1 <= D <= 4095, float32 / bfloat16, dense and batched launches.  Replaces KeOps'
// generic_argmin("SqDist(x,y)") of the reference's K-means recipe (g = 0) and gives the hard correspondences of a transport plan
// (g = dual potential + eps log weight).
//
// It is the staging and the MFMA chain of xk_fwd_kernel (glhip_softmin_xk.h: xk_exponent_blocks, called with scales of 1) with another
// epilogue: the same 256 rows x 128 columns per workgroup, 8 wavefronts as 4 x 2, stages of 6 K chunks, points centred on the first
// row of the row block, split into bf16 x 3 pieces on the fly.  The bf16 x 3 layout only: it has no range precondition.  s = 1, row scalar 0, column scalar
// H_j = g_j - |yt_j|^2 / 2: the exponent block u_ij = H_j + xt_i . yt_j is largest where the cost |xt_i|^2 / 2 - u_ij is smallest.
// kXkMinD = 17 is where the soft-min dispatch hands over to this family, not a limit of the packing: xk_num_mfma / xk_num_groups
// count the scalar item plus D coordinates from D = 1 (one MFMA, one group), and slots past the last coordinate are zero.
//
// Epilogue: a lane (half, l31) holds, for row l31 of a row tile, the 16 columns 8 (k / 4) + 4 half + k % 4 of each of its column
// groups.  It walks them in ascending column order with a strict compare — 1 compare + 2 selects per pair instead of the soft-min's
// max + sub + exp + add — and keeps (best u, best column) per row tile.  Then the two lane halves meet (__shfl_xor 32), the two
// column halves of the workgroup meet in LDS, and the column splits meet in argmin_merge_kernel over (u, index) partials.
//
// Semantics:
//   * ties go to the smallest column index: every merge compares (u, -index) lexicographically.  u_ij does not depend on the tile or
//     the split a column falls into (the centre is the row block's), so neither does the result; exact duplicates among the columns
//     produce bit-identical u and the first copy wins.
//   * padded columns never win: the last tile of a split looks up lds.idx and skips slots < 0, whatever their scalar is.
//   * g_j = -inf gives u = -inf, which never beats the initial -inf: such a column cannot be chosen.  A row without an admissible
//     column (M == 0, or every g_j = -inf) gets index -1 and value +inf.  NaN exponents never win either.
//   * value_i = |xt_i|^2 / 2 - u_max in float32: the exponent error of glhip_softmin_xk.h with s = 1, <= (NM + 5) 2^-24 (diam^2 + max |g|).
#pragma once

#include "glhip_softmin_xk.h"

namespace glhip {

template <typename T>
struct ArgminParams {
    const T* x;          // (B,N,D)
    const T* y;          // (B,M,D)
    const float* g;      // (B,M) or NULL (= 0)
    int32_t* index;      // (B,N)
    float* value;        // (B,N) or NULL
};

// (u, -index) lexicographic: does (u2, i2) beat (u1, i1)?  An empty result is (-inf, -1) and is beaten by any u > -inf only.
__device__ __forceinline__ bool argmin_beats(float u2, int i2, float u1, int i1) { return u2 > u1 || (u2 == u1 && i2 < i1); }

template <typename T>
__global__ void __launch_bounds__(kXkThreads, 4)
argmin_xk_kernel(ArgminParams<T> prm, int N, int M, int D, SplitInfo sp) {
    constexpr int L = XL_BF16X3;
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
    const T* xb = prm.x + (long)b * N * D;
    const T* yb = prm.y + (long)b * M * D;
    const Ranges none{nullptr, nullptr, nullptr, nullptr};

    int row_begin, row_end, q_begin, q_end;
    block_extent<false>(none, N, kXkRows, row_begin, row_end, q_begin, q_end, bx);

    for (int row0 = row_begin; row0 < row_end; row0 += kXkRows) {
        const T* centre = xb + (long)row0 * D;
        const int nrows = min(kXkRows, row_end - row0);
        const int nr32 = (nrows + 31) & ~31;                  // row slots that are packed
        __syncthreads();                                      // the previous pass is done with the LDS
        if (tid < kXkRows) lds.idx[tid] = min(row0 + tid, row_end - 1);
        __syncthreads();
        xk_norms<T>(xb, centre, D, lds.idx, 0, kXkRows, lds.n2row, tid);
        __syncthreads();
        if (tid < kXkRows) lds.scal[tid] = 0.f;               // the row scalar: |xt_i|^2 / 2 joins after the reduction

        const int wave_row0 = row0 + wr * (kXkRT * 32);
        const bool wave_rows = wave_row0 < row_end;
        float bu[kXkRT];                                      // best exponent of the row so far ...
        int bi[kXkRT];                                        // ... and its column (-1: none yet)
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) { bu[rt] = -__builtin_inff(); bi[rt] = -1; }
        const int lanecol = wc * (kXkCG * 32) + 4 * half;     // tile slot of this lane's element (cg = 0, k = 0)

        // one tile: the n real columns j0 .. j0 + n - 1 in the slots kXkRows .. kXkRows + n - 1; `col` = this thread's column (tid < kXkCols), -1 = padding
        auto tile_body = [&](int n, int col, int j0) {
            const int ncg = (n + 31) >> 5;                    // column groups that are packed and multiplied
            __syncthreads();                                  // the previous tile (and the row scalars) are settled
            if (tid < kXkCols) lds.idx[kXkRows + tid] = col;
            __syncthreads();
            xk_norms<T>(yb, centre, D, lds.idx, kXkRows, ncg * 32, &lds.scal[kXkRows], tid);
            __syncthreads();
            if (tid < ncg * 32) {                             // |yt|^2 -> H_j
                float H = kNegBig;
                if (col >= 0) {
                    const float gj = prm.g ? prm.g[(long)b * M + col] : 0.f;
                    H = __builtin_fmaf(-0.5f, lds.scal[kXkRows + tid], gj);
                }
                lds.scal[kXkRows + tid] = H;
            }

            const bool wave_on = wave_rows && wc * kXkCG < ncg;
            f32x16 acc[kXkRT][kXkCG];
            xk_exponent_blocks<T, L, false>(lds, xb, yb, centre, D, NM, NG, nr32, ncg, 1.0f, 1.0f, wave_on, wr, wc, half, l31, tid, acc);
            if (!wave_on) return;

            // ---- epilogue: the best exponent of this wavefront's 2 x 2 blocks per row, columns in ascending order, strict compare
            // (column groups >= ncg were not packed).  `code` = tile slot of an element relative to lanecol.  A partial tile — the last
            // of a split — checks every slot's index: padding is excluded by index, not by its scalar.
            auto scan = [&](auto partial_tag) {
                constexpr bool PARTIAL = decltype(partial_tag)::value;
#pragma unroll
                for (int rt = 0; rt < kXkRT; ++rt) {
                    float lu = bu[rt];
                    int lc = -1;
#pragma unroll
                    for (int cg = 0; cg < kXkCG; ++cg) {
                        if (wc * kXkCG + cg < ncg) {
#pragma unroll
                            for (int k = 0; k < 16; ++k) {
                                const int code = cg * 32 + 8 * (k / 4) + (k % 4);
                                const float u = acc[rt][cg][k];
                                bool take = u > lu;
                                if (PARTIAL) take = take && lds.idx[kXkRows + lanecol + code] >= 0;
                                lu = take ? u : lu;
                                lc = take ? code : lc;
                            }
                        }
                    }
                    if (lc >= 0) {
                        bu[rt] = lu;
                        bi[rt] = j0 + lanecol + lc;
                    }
                }
            };
            if (n < kXkCols) scan(std::true_type{});
            else scan(std::false_type{});
        };

        {
            int js, je;
            column_interval<false>(none, M, 0, split, ns, js, je);
            for (int j0 = js; j0 < je; j0 += kXkCols) {
                const int n = min(kXkCols, je - j0);
                tile_body(n, (tid < n) ? j0 + tid : -1, j0);
            }
        }

        // ---- the two lane halves meet, then the two column halves of the workgroup in LDS (the tile buffer is free now): [wc][row] of (u, index) ----
        __syncthreads();
        float* mrg = reinterpret_cast<float*>(lds.buf);
        int* mrgi = reinterpret_cast<int*>(lds.buf);
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) {
            float u = bu[rt];
            int i = bi[rt];
            const float uo = __shfl_xor(u, 32, 64);
            const int io = __shfl_xor(i, 32, 64);
            if (argmin_beats(uo, io, u, i)) { u = uo; i = io; }
            if (half == 0) {
                const int r = wr * (kXkRT * 32) + rt * 32 + l31;
                mrg[(wc * kXkRows + r) * 2] = u;
                mrgi[(wc * kXkRows + r) * 2 + 1] = i;
            }
        }
        __syncthreads();
        if (tid < nrows) {
            float u = mrg[tid * 2];
            int i = mrgi[tid * 2 + 1];
#pragma unroll
            for (int w = 1; w < kXkWC; ++w) {
                const float u2 = mrg[(w * kXkRows + tid) * 2];
                const int i2 = mrgi[(w * kXkRows + tid) * 2 + 1];
                if (argmin_beats(u2, i2, u, i)) { u = u2; i = i2; }
            }
            const long row = (long)b * N + row0 + tid;
            const float hn = 0.5f * lds.n2row[tid];
            if (ns == 1) {
                prm.index[row] = i;
                if (prm.value) prm.value[row] = hn - u;
            } else {
                float* dst = sp.workspace + split * sp.split_stride + row * 2;
                dst[0] = u;
                reinterpret_cast<int*>(dst)[1] = i;
                if (split == 0 && prm.value) prm.value[row] = hn;      // |xt_i|^2 / 2 is the same in every split: the merge subtracts u_max
            }
        }
    }
}

// Combines the column splits of every row: one thread per row over the (u, index) partials, in split order.
static __global__ void __launch_bounds__(kBlock)
argmin_merge_kernel(int32_t* __restrict__ index, float* __restrict__ value, long rows, SplitInfo sp) {
    const long row = (long)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    float u = -__builtin_inff();
    int i = -1;
    for (int s = 0; s < sp.n_splits; ++s) {
        const float* src = sp.workspace + s * sp.split_stride + row * 2;
        const float u2 = src[0];
        const int i2 = reinterpret_cast<const int*>(src)[1];
        if (argmin_beats(u2, i2, u, i)) { u = u2; i = i2; }
    }
    index[row] = i;
    if (value) value[row] = value[row] - u;
}

}  // namespace glhip
