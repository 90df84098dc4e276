// glhip_argkmin_xk.h — the top-k arg-reduction: for every row the k columns of the smallest dual-shifted cost, best first,
//   index_i[r] = column of the (r+1)-th smallest  c_ij = |x_i - y_j|^2 / 2 - g_j,   value_i[r] = that cost,      0 <= r < k <= kArgkminMaxK,
// in one pass up to k = kArgkminCap = 16 and in ceil(k / 16) floored passes beyond (below),
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
//   floored (k > 16):
//      4    (512, 4)         128     0 B      80640 B        4               2           kXkSlots
//      8    (512, 2)         197     0 B      80640 B        2               1           kXkTopkSlots
//     16    (512, 2)         256     0 B      80640 B        2               1           kXkTopkSlots
//   argkmin_merge_kernel<4 / 8 / 16>: 18 / 26 / 56 VGPRs, 0 B of scratch.
// argmin_xk_kernel has 123 VGPRs under (512, 4) with two registers of state per row tile, and the lists are live across the whole
// stage loop.  CAP = 4 (16 registers) just fits that budget, with the lean select of argkmin_pick and the opaque shuffle address of the
// half merge; under the same bounds CAP = 6 / 8 spill 40 / 104 bytes per lane (CAP = 16: 440, with the select tree).  So k <= 4 runs like argmin, two workgroups
// per CU, and k <= 8 / k <= 16 run one workgroup per CU in ONE pass.  That costs real time — this family waits on its staging barriers
// most of the time, and without a second resident workgroup nothing fills those waits (measured, profiles/argkmin.txt: k = 16 takes
// 2.7 / 2.0 / 1.6 x argmin's time at D = 32 / 64 / 128, k <= 4 1.06 / 1.02 / 1.01 x) —
// but less than the alternative, ceil(k / 4) passes of the CAP = 4 kernel with a floor per row (2 / 4 times argmin for k = 8 / 16),
// wherever the MFMA chain is long enough to matter (D >= 32).  At low D, where staging is everything, the passes would win (D = 3,
// k = 8: 3.8 x argmin in one pass against 2 x): see DESIGN.md §9.
//
// Floored passes (FLOOR; k > 16).  Pass t writes the ranks r0 = 16 t .. r0 + kc - 1 of a row stride k and admits a candidate (u, j) of
// row i only strictly behind the row's floor (fu, fj) in the order of the lists: u < fu, or u == fu and j > fj.  The floor is the raw
// (u, index) of the last rank the pass before wrote, one pair of 32-bit words per row at the head of the workspace — never recomputed
// from `value` — (+inf, -1) before the first pass (argkmin_floor_fill_kernel) and (-inf, INT_MAX) once a rank is missing, so that the
// later ranks of the row stay (-1, +inf).  u_ij is the same float32 number in every pass: the union of the passes is exact for any k,
// the first pass returns the bits of the k = 16 call, and a tie group that straddles a pass boundary continues in ascending index order.
// Full passes run on CAP = 16 (no scratch, as the table says: no need to fall back to ceil(k / 8) passes of CAP = 8), the last one on
// the smallest capacity that holds the remainder (k = 20 = 16 + 4: at argmin's occupancy).
//   Where the floor lives: nowhere across the stage loop.  CAP = 16 and CAP = 4 have no register to spare and the workgroup no 2 KiB of
//   LDS (2 x 80640 B is what lets two CAP = 4 workgroups share a CU).  The fast path is untouched: one max chain, one ballot, one branch.
//   Only the slow path needs the floor — it ANDs the lexicographic test into the `todo` set next to `> last` and PARTIAL — so it
//   fetches the lane's pair there with one 8-byte global load (scalar base + lane offset; the rows of a wavefront are one 256-byte
//   line of the L1 / L2), from a lane id the compiler cannot see through, else the address is hoisted above the tile loop (12 bytes of
//   scratch per lane at CAP = 4).  The two registers are dead before the push loop.  In passes >= 1 the at most r0 columns a row has
//   emitted lie ahead of its floor with exponents above its list's last entry: they send their tile through the slow path, where the
//   test drops them — at most r0 tiles per row.
//   Who writes the floor: the last merge of a row — this kernel without splits (every row has one workgroup, which has left the tile
//   loop by then), argkmin_merge_kernel with splits (the main kernel only reads) — so stream order between the passes is all the
//   synchronisation there is.  The partial of a pass is 2 kc floats per row and split.
#pragma once

#include "glhip_softmin_xk.h"
#include "glhip_topk_list.h"

namespace glhip {

constexpr int kArgkminCap = 16;        // the largest list: the most ranks one pass writes
constexpr int kArgkminMaxK = 128;      // what glhip_argkmin_max_k() reports: eight floored passes (a larger k is the same loop; the cap bounds the time of a call)
// wavefronts per SIMD a capacity's registers allow: 4 = two workgroups per CU like argmin (kXkSlots), 2 = one (kXkTopkSlots, glhip_split_policy.h)
constexpr int argkmin_occ(int cap) { return cap <= 4 ? 4 : 2; }

template <typename T>
struct ArgkminParams {
    const T* x;          // (B,N,D)
    const T* y;          // (B,M,D)
    const float* g;      // (B,M) or NULL (= 0)
    int32_t* index;      // (B,N,k)
    float* value;        // (B,N,k) or NULL
    int k;               // ranks per row of index / value: their row stride (plain kernel: 1 <= k <= CAP, all written by the launch)
    // a floored pass (FLOOR; see the header) writes the kc <= CAP ranks r0 .. r0 + kc - 1 and admits only what lies behind the row's floor
    int r0, kc;
    int32_t* floor;      // (B N, 2): bits of u and index of the last rank the row has been given so far; (+inf, -1) before the first pass
};

// the floor of a row whose last rank is missing: nothing lies behind it
constexpr int kArgkminFloorNoneU = (int)0xff800000u, kArgkminFloorNoneI = 0x7fffffff;

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

// The next pass's floor of a row from the list its last merge wrote ranks r0 .. r0 + kc - 1 from: the raw (u, index) of entry kc - 1, or the
// floor nothing lies behind where that rank is missing (so every later rank of the row stays missing).
template <int CAP>
__device__ __forceinline__ void topk_store_floor(int32_t* floor, const float (&u)[CAP], const int (&i)[CAP], int kc) {
    float fu = u[0];
    int fi = i[0];
#pragma unroll
    for (int e = 1; e < CAP; ++e) {
        fu = (e < kc) ? u[e] : fu;
        fi = (e < kc) ? i[e] : fi;
    }
    floor[0] = fi < 0 ? kArgkminFloorNoneU : __float_as_int(fu);
    floor[1] = fi < 0 ? kArgkminFloorNoneI : fi;
}

// CAP: entries per list; OCC: wavefronts per SIMD the register budget is set for (4: two workgroups per CU, 2: one); FLOOR: a floored pass
template <typename T, int CAP, int OCC, bool FLOOR = false>
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
    const int r0 = FLOOR ? prm.r0 : 0, kc = FLOOR ? prm.kc : k;      // the ranks this launch writes
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
                    // the floor of the lane's row, fetched here and dead before the push loop: (fu, column of the floor - column of element 0)
                    float fu = 0.f;
                    int fd = 0;
                    if constexpr (FLOOR) {
                        // (the row from a thread id the compiler cannot see through: a loop-invariant address would be hoisted above the tile
                        // loop and live across it, in registers the 128-VGPR kernel does not have; scalar base + 32-bit lane offset)
                        int t = threadIdx.x;
                        asm volatile("" : "+v"(t));
                        const unsigned rowl = (unsigned)min(row0 + ((t >> 7) * kXkRT + rt) * 32 + (t & 31), row_end - 1) - (unsigned)row0;
                        static_assert(kXkWC == 2 && kXkThreads == 512, "wr = tid >> 7");
                        const int2 f = reinterpret_cast<const int2*>(prm.floor + 2 * ((long)b * N + row0))[rowl];
                        fu = __int_as_float(f.x);
                        fd = f.y - (j0 + lanecol);
                    }
                    unsigned todo = 0;
#pragma unroll
                    for (int cg = 0; cg < kXkCG; ++cg) {
                        if (wc * kXkCG + cg < ncg) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                bool take = acc[rt][cg][r] > last;
                                if (FLOOR) take = take && (acc[rt][cg][r] < fu || (acc[rt][cg][r] == fu && cg * 32 + 8 * (r / 4) + (r % 4) > fd));
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
                    if (e < kc) {
                        prm.index[row * k + r0 + e] = i[e];
                        if (prm.value) prm.value[row * k + r0 + e] = hn - u[e];
                    }
                }
                if constexpr (FLOOR) topk_store_floor<CAP>(prm.floor + 2 * row, u, i, kc);
            } else {
                float* dst = sp.workspace + split * sp.split_stride + row * (2 * kc);
#pragma unroll
                for (int e = 0; e < CAP; ++e) {
                    if (e < kc) {
                        dst[2 * e] = u[e];
                        reinterpret_cast<int*>(dst)[2 * e + 1] = i[e];
                    }
                }
                if (split == 0 && prm.value) prm.value[row * k + r0] = hn;      // |xt_i|^2 / 2 is the same in every split: the merge subtracts the exponents
            }
        }
    }
}

// Combines the column splits of every row: one thread per row over the kc (u, index) partials of every split, in split order; writes
// the ranks r0 .. r0 + kc - 1 of the row's k and, for a floored pass (floor != NULL), the row's next floor.
template <int CAP>
__global__ void __launch_bounds__(kBlock)
argkmin_merge_kernel(int32_t* __restrict__ index, float* __restrict__ value, long rows, int k, int r0, int kc, int32_t* __restrict__ floor,
                     SplitInfo sp) {
    const long row = (long)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    float u[CAP];
    int i[CAP];
    topk_clear<CAP>(u, i);
    for (int s = 0; s < sp.n_splits; ++s) {
        const float* src = sp.workspace + s * sp.split_stride + row * (2 * kc);
#pragma unroll
        for (int e = 0; e < CAP; ++e)
            if (e < kc) topk_insert_lex<CAP>(u, i, src[2 * e], reinterpret_cast<const int*>(src)[2 * e + 1]);
    }
    const float hn = value ? value[row * k + r0] : 0.f;
#pragma unroll
    for (int e = 0; e < CAP; ++e) {
        if (e < kc) {
            index[row * k + r0 + e] = i[e];
            if (value) value[row * k + r0 + e] = hn - u[e];
        }
    }
    if (floor) topk_store_floor<CAP>(floor + 2 * row, u, i, kc);
}

// (+inf, -1) for every row: what the first pass of a k > kArgkminCap call runs behind, everything
static __global__ void __launch_bounds__(kBlock) argkmin_floor_fill_kernel(int32_t* __restrict__ floor, long rows) {
    const long row = (long)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    floor[2 * row] = 0x7f800000;
    floor[2 * row + 1] = -1;
}

}  // namespace glhip
