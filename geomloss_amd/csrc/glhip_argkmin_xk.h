// glhip_argkmin_xk.h — the top-k arg-reduction: for every row the k columns of the smallest dual-shifted cost, best first,
//   index_i[r] = column of the (r+1)-th smallest  c_ij = |x_i - y_j|^2 / 2 - g_j,   value_i[r] = that cost,      0 <= r < k <= kArgkminMaxK,
// p = 2, clouds of dimension 1 <= D <= 4095, float32 / bfloat16, dense and batched launches.  KeOps' argKmin / Kmin_argKmin of SqDist
// (g = 0: k nearest neighbours) and the k heaviest entries of every row of a transport plan (g = dual potential + eps log weight).
//
// Staging, norms, the MFMA chain (xk_exponent_blocks with scales of 1) and H_j = g_j - |yt_j|^2 / 2 are those of argmin_xk_kernel
// (glhip_argmin_xk.h), statement for statement: the exponent u_ij = H_j + xt_i . yt_j is the same float32 number, so k = 1 is argmin
// bit for bit.  New are the epilogue and the merges.
//
// Epilogue.  A lane (half, l31) owns row l31 of each of its kXkRT row tiles and sees 32 exponents of it per column tile (2 column
// groups x 16), in ascending column order.  Per row tile it keeps a list of CAP (u, column), best first, in registers
// (glhip_topk_list.h: every subscript static).
//   fast path  the maximum of the 32 exponents (v_max chain; NaN drops out) against the list's last entry, one ballot, one
//              wavefront-uniform branch: 33 VALU instructions per row tile and column tile where argmin's scan spends 96.  Once a list
//              has warmed up this is all a tile costs.
//   slow path  some lane has a candidate: every lane builds the 32-bit set of its elements that beat its last entry (a partial tile
//              drops padded slots here, by index), and the wavefront loops while any set is non-empty: lowest bit -> element by a
//              select tree (31 v_cndmask: a run-time subscript into the accumulators would send them to scratch), topk_push (strict
//              compare: the earlier column stays ahead on a tie; lanes without a candidate push -inf, a no-op).  The loop runs as often
//              as the busiest lane has candidates; a list takes about CAP ln(columns of the lane / CAP) pushes in all.
// Merges, all by the lexicographic rule (u descending, index ascending: topk_insert_lex): the two lane halves by ds_bpermute, the
// two column halves of the workgroup in LDS (the tile buffer is free by then: 2 x CAP x 256 pairs = 64 KiB at CAP = 16 of its
// 74.25), the column splits in argkmin_merge_kernel over partials of 2 k floats per row and split.  u_ij does not depend on tile or
// split (the centre is the row block's), so neither does the result.
//
// Semantics: rank r of a call with k is rank r of a call with any larger k; exact duplicates among the columns give bit-identical u
// and come in ascending index order; g_j = -inf, NaN exponents and padded slots never enter a list; ranks a row has no admissible
// column for are (-1, +inf); value = |xt_i|^2 / 2 - u, the accuracy of argmin per entry.
//
// Capacities and resources.  Three capacities are compiled, 4 / 8 / 16, and a launch takes the smallest that holds k.  The compiler's
// remarks (-Rpass-analysis=kernel-resource-usage, gfx950, printed by every build of glhip_api_argkmin.hip), float32 and bfloat16 alike:
//     CAP   launch bounds   VGPRs   scratch   LDS       waves / SIMD   workgroups / CU   resident slots
//      4    (512, 4)         128     0 B      80640 B        4               2           kXkSlots
//      8    (512, 2)         199     0 B      80640 B        2               1           kXkTopkSlots
//     16    (512, 2)         256     0 B      80640 B        2               1           kXkTopkSlots
//   argkmin_merge_kernel<4 / 8 / 16>: 17 / 25 / 56 VGPRs, 0 B of scratch.
// argmin_xk_kernel has 123 VGPRs under (512, 4) with two registers of state per row tile, and the lists are live across the whole
// stage loop.  CAP = 4 (16 registers) just fits that budget, with the lean select of argkmin_pick and the opaque shuffle address of the
// half merge; under the same bounds CAP = 6 / 8 spill 40 / 104 bytes per lane (CAP = 16: 440, with the select tree).  So k <= 4 runs like argmin, two workgroups
// per CU, and k <= 8 / k <= 16 run one workgroup per CU in ONE pass.  That costs real time — this family waits on its staging barriers
// most of the time, and without a second resident workgroup nothing fills those waits (measured, profiles/argkmin.txt: k = 16 takes
// 2.7 / 2.0 / 1.6 x argmin's time at D = 32 / 64 / 128, k <= 4 1.06 / 1.02 / 1.01 x) —
// but less than the alternative, ceil(k / 4) passes of the CAP = 4 kernel with a floor per row (2 / 4 times argmin for k = 8 / 16),
// wherever the MFMA chain is long enough to matter (D >= 32).  At low D, where staging is everything, the passes would win (D = 3,
// k = 8: 3.8 x argmin in one pass against 2 x): see DESIGN.md §9.
#pragma once

#include "glhip_softmin_xk.h"
#include "glhip_topk_list.h"

namespace glhip {

constexpr int kArgkminMaxK = 16;       // the largest list: what glhip_argkmin_max_k() reports
// wavefronts per SIMD a capacity's registers allow: 4 = two workgroups per CU like argmin (kXkSlots), 2 = one (kXkTopkSlots, glhip_split_policy.h)
constexpr int argkmin_occ(int cap) { return cap <= 4 ? 4 : 2; }

template <typename T>
struct ArgkminParams {
    const T* x;          // (B,N,D)
    const T* y;          // (B,M,D)
    const float* g;      // (B,M) or NULL (= 0)
    int32_t* index;      // (B,N,k)
    float* value;        // (B,N,k) or NULL
    int k;               // 1 <= k <= CAP of the launch
};

// Element e = 16 cg + r of a lane's 2 x 16 exponents of a row tile, e a run-time number: selects over static subscripts.  LEAN: a chain
// of 31 compares and selects on one register (the kernels with a 128-VGPR budget); else a tree of 31 selects on 16.
template <bool LEAN>
__device__ __forceinline__ float argkmin_pick(const f32x16 (&a)[kXkCG], int e) {
    static_assert(kXkCG == 2, "the candidate set of a row tile is one 32-bit word");
    if constexpr (LEAN) {
        float u = a[0][0];
#pragma unroll
        for (int i = 1; i < 32; ++i) u = (e == i) ? a[i >> 4][i & 15] : u;
        return u;
    } else {
        float t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = (e & 16) ? a[1][i] : a[0][i];
#pragma unroll
        for (int w = 8; w >= 1; w >>= 1) {
#pragma unroll
            for (int i = 0; i < w; ++i) t[i] = (e & w) ? t[i + w] : t[i];
        }
        return t[0];
    }
}

// CAP: entries per list; OCC: wavefronts per SIMD the register budget is set for (4: two workgroups per CU, 2: one)
template <typename T, int CAP, int OCC>
__global__ void __launch_bounds__(kXkThreads, OCC)
argkmin_xk_kernel(ArgkminParams<T> prm, int N, int M, int D, SplitInfo sp) {
    constexpr int L = XL_BF16X3;
    static_assert(2 * kXkWC * CAP * kXkRows * sizeof(float) <= sizeof(XkLds::buf), "the workgroup merge is one round in the tile buffer");
    __shared__ XkLds lds;

    int bx, b, split;
    workgroup_coords(sp, bx, b, split);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / kXkWC, wc = wave % kXkWC;
    const int half = lane >> 5, l31 = lane & 31;
    const int ns = sp.n_splits;
    const int k = prm.k;
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
        float lu[kXkRT][CAP];                                 // the best exponents of the row so far, descending ...
        int li[kXkRT][CAP];                                   // ... and their columns (-1: none yet)
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) topk_clear<CAP>(lu[rt], li[rt]);
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

            // ---- epilogue (see the header): element e = 16 cg + r of a row tile sits in tile slot lanecol + 32 cg + 8 (r / 4) + r % 4,
            // ascending in e.  Column groups >= ncg were not packed.  A partial tile — the last of a split — excludes padding by index.
            auto scan = [&](auto partial_tag) {
                constexpr bool PARTIAL = decltype(partial_tag)::value;
#pragma unroll
                for (int rt = 0; rt < kXkRT; ++rt) {
                    const float last = lu[rt][CAP - 1];
                    float mx = -__builtin_inff();
#pragma unroll
                    for (int cg = 0; cg < kXkCG; ++cg) {
                        if (wc * kXkCG + cg < ncg) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc[rt][cg][r]);
                        }
                    }
                    if (__ballot(mx > last) == 0) continue;
                    unsigned todo = 0;
#pragma unroll
                    for (int cg = 0; cg < kXkCG; ++cg) {
                        if (wc * kXkCG + cg < ncg) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                bool take = acc[rt][cg][r] > last;
                                if (PARTIAL) take = take && lds.idx[kXkRows + lanecol + cg * 32 + 8 * (r / 4) + (r % 4)] >= 0;
                                todo |= take ? (1u << (cg * 16 + r)) : 0u;
                            }
                        }
                    }
                    while (__ballot(todo != 0) != 0) {
                        const int e = todo ? __builtin_ctz(todo) : 0;
                        const float u = todo ? argkmin_pick<(OCC >= 4)>(acc[rt], e) : -__builtin_inff();
                        const int code = (e >> 4) * 32 + ((e & 15) >> 2) * 8 + (e & 3);
                        topk_push<CAP>(lu[rt], li[rt], u, j0 + lanecol + code);
                        todo &= todo - 1;
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

        // ---- the two lane halves meet, then the two column halves of the workgroup in LDS (the tile buffer is free now):
        // pair [(wc CAP + entry) 256 + row] of (u, index) ----
        __syncthreads();
        float* mrg = reinterpret_cast<float*>(lds.buf);
        int* mrgi = reinterpret_cast<int*>(lds.buf);
        // the other lane half's byte address for ds_bpermute, from a lane id the compiler cannot see through: __shfl_xor's own address
        // arithmetic is hoisted above the tile loop and costs the 128-VGPR kernel a register it does not have (8 bytes of scratch)
        int other = threadIdx.x;
        asm volatile("" : "+v"(other));
        other = ((other ^ 32) & 63) << 2;
#pragma unroll
        for (int rt = 0; rt < kXkRT; ++rt) {
            float ou[CAP];
            int oi[CAP];
#pragma unroll
            for (int e = 0; e < CAP; ++e) {
                ou[e] = __int_as_float(__builtin_amdgcn_ds_bpermute(other, __float_as_int(lu[rt][e])));
                oi[e] = __builtin_amdgcn_ds_bpermute(other, li[rt][e]);
            }
            topk_merge<CAP>(lu[rt], li[rt], ou, oi);
            if (half == 0) {
                const int r = wr * (kXkRT * 32) + rt * 32 + l31;
#pragma unroll
                for (int e = 0; e < CAP; ++e) {
                    mrg[((wc * CAP + e) * kXkRows + r) * 2] = lu[rt][e];
                    mrgi[((wc * CAP + e) * kXkRows + r) * 2 + 1] = li[rt][e];
                }
            }
        }
        __syncthreads();
        if (tid < nrows) {
            float u[CAP];
            int i[CAP];
#pragma unroll
            for (int e = 0; e < CAP; ++e) {
                u[e] = mrg[(e * kXkRows + tid) * 2];
                i[e] = mrgi[(e * kXkRows + tid) * 2 + 1];
            }
#pragma unroll
            for (int w = 1; w < kXkWC; ++w) {
#pragma unroll
                for (int e = 0; e < CAP; ++e)
                    topk_insert_lex<CAP>(u, i, mrg[((w * CAP + e) * kXkRows + tid) * 2], mrgi[((w * CAP + e) * kXkRows + tid) * 2 + 1]);
            }
            const long row = (long)b * N + row0 + tid;
            const float hn = 0.5f * lds.n2row[tid];
            if (ns == 1) {
#pragma unroll
                for (int e = 0; e < CAP; ++e) {
                    if (e < k) {
                        prm.index[row * k + e] = i[e];
                        if (prm.value) prm.value[row * k + e] = hn - u[e];
                    }
                }
            } else {
                float* dst = sp.workspace + split * sp.split_stride + row * (2 * k);
#pragma unroll
                for (int e = 0; e < CAP; ++e) {
                    if (e < k) {
                        dst[2 * e] = u[e];
                        reinterpret_cast<int*>(dst)[2 * e + 1] = i[e];
                    }
                }
                if (split == 0 && prm.value) prm.value[row * k] = hn;      // |xt_i|^2 / 2 is the same in every split: the merge subtracts the exponents
            }
        }
    }
}

// Combines the column splits of every row: one thread per row over the k (u, index) partials of every split, in split order.
template <int CAP>
__global__ void __launch_bounds__(kBlock)
argkmin_merge_kernel(int32_t* __restrict__ index, float* __restrict__ value, long rows, int k, SplitInfo sp) {
    const long row = (long)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    float u[CAP];
    int i[CAP];
    topk_clear<CAP>(u, i);
    for (int s = 0; s < sp.n_splits; ++s) {
        const float* src = sp.workspace + s * sp.split_stride + row * (2 * k);
#pragma unroll
        for (int e = 0; e < CAP; ++e)
            if (e < k) topk_insert_lex<CAP>(u, i, src[2 * e], reinterpret_cast<const int*>(src)[2 * e + 1]);
    }
    const float hn = value ? value[row * k] : 0.f;
#pragma unroll
    for (int e = 0; e < CAP; ++e) {
        if (e < k) {
            index[row * k + e] = i[e];
            if (value) value[row * k + e] = hn - u[e];
        }
    }
}

}  // namespace glhip
