// glhip_softmin_list.h — the sweep of the sorted p = 2 launch on the f16 x 2 layout (D <= 3): list-driven, no LDS tile, no barrier.
//
// The pruning it applies is the second level of glhip_softmin_x32.h (P2) word for word: the seed, the float32 test with kP2Slack on
// the keep side, thr = max(term rule, t2 of the tile), the lazy maximum with its exact redo, the floor rule.  What differs is the data
// path around the exponentials:
//   * one wavefront = one row tile of 32 rows, and wavefronts never wait for each other.  A workgroup is still 4 wavefronts = one
//     chunk of 128 rows (grid, SplitInfo, Ranges and the chunk table are those of the staged kernel); a chunk with fewer than 4 row
//     tiles (the cloud's last rows) leaves wavefronts idle instead of sharing a tile between them.
//   * operands come straight from the group-major packed columns (PackedCols, GROUPED: [group of 32][K block][column] — lane l of
//     the MFMA reads record l of the group): one coalesced 16-byte load per lane and group, scalar base + lane offset.
//   * batch = up to 64 consecutive groups of one piece (pieces are whole blocks of 256 sorted columns; the cloud's last group is
//     neutral-padded by the pack kernel).  Lane g reads the record of group g and forms ub; ONE ballot is the keep set of 2048 columns.
//     The records of the next batch are asked for before the current one is swept.
//   * the kept groups are walked in ascending order on the scalar unit (s_ff1 on the ballot), through a ring of four operands in
//     registers: three loads are in flight ahead of the MFMA that consumes the fourth.  The ring restarts at every ballot; the
//     prefetches past a ballot's last kept group re-read the batch's first group (a valid address, a cache hit, never consumed).
//   * lazy maximum: batch = one ballot.  The speculative sums run with the running maximum folded into the x operand; when a lane's
//     batch sum is not below kSumThr the batch is redone group by group with exact maxima (operands loaded again), the maximum is
//     set, and thr is recomputed for the batches that follow.  A batch tested under an older, lower thr kept a superset of what the
//     newer thr keeps: the exactness argument of glhip_softmin_x32.h holds unchanged.
//   * the order of summation is a function of the records alone: equal bits on a repeated call.
//   * every group index that forms an address is clamped to [0, n_groups - 1].
// Which sweep takes the launch is read from Level2::list_takes, written once per launch in front of both sweeps, before anything else.
// Precondition (the launcher's): pre-packed GROUPED columns, no gathered tiles (SplitInfo::gather == 0).
#pragma once

#include "glhip_list_cursor.h"
#include "glhip_softmin_x32.h"

namespace glhip {

// ub of one group for a wavefront whose row box is (wlo, whi): the expression of the staged test (glhip_softmin_x32.h), the three
// squared gaps added as its two shuffles add them, (0 + 1) + (2 + 3) with part 3 = 0, and never contracted into the products
__device__ __forceinline__ float list_group_ub(const float4& ra, const float4& rb, const float (&wlo)[3], const float (&whi)[3], float s2) {
    float d2;
    {
#pragma clang fp contract(off)
        const float g0 = fmaxf(fmaxf(ra.x - whi[0], wlo[0] - ra.y), 0.f);
        const float g1 = fmaxf(fmaxf(ra.z - whi[1], wlo[1] - ra.w), 0.f);
        const float g2 = fmaxf(fmaxf(rb.x - whi[2], wlo[2] - rb.y), 0.f);
        const float s01 = g0 * g0 + g1 * g1;
        const float s23 = g2 * g2 + 0.f;
        d2 = s01 + s23;
    }
    const float hm2 = rb.z * kLog2e, q = 0.5f * s2 * d2;
    return (hm2 - q) + kP2Slack * (fminf(__builtin_fabsf(hm2), 3.0e38f) + q);
}

// One operand of the ring: 16 bytes per lane at (wave-uniform base) + (lane offset), issued where it stands.  The compiler does not
// count this load: list_wait3 / list_drain do, and name the registers so that no reader moves above them.
__device__ __forceinline__ void list_issue(u32x4& dst, const uint4* base, uint32_t lane_off) {
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(dst) : "v"(lane_off), "s"(base) : "memory");
}
__device__ __forceinline__ void list_wait3(u32x4& a) {      // all but the three youngest loads have landed
    asm volatile("s_waitcnt vmcnt(3)" : "+v"(a) : : "memory");
}
__device__ __forceinline__ void list_drain(u32x4& a0, u32x4& a1, u32x4& a2, u32x4& a3) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "memory");
}

template <int D, typename T>
__global__ void __launch_bounds__(256, 6)
softmin_fwd_list_p2_kernel(SoftminParams<T> prm, Ranges rg, int N, int M, SplitInfo sp, PackedCols pk, Level2 l2) {
    if (*l2.list_takes == 0) return;      // the staged kernel's launch (the int: list_decide, glhip_prune.hip)
    constexpr int L = XL_F16X2;
    constexpr int kRowsPerBlock = 128;
    int bx, b, split;
    workgroup_coords(sp, bx, b, split);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ns = sp.n_splits;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    int row_begin, row_end, q_begin, q_end;
    block_extent<true>(rg, N, kRowsPerBlock, row_begin, row_end, q_begin, q_end, bx);
    if (row_begin >= row_end) return;
    const int home = l2.home[(rg.chunks && rg.chunks[0] >= 0) ? rg.chunks[1 + 3 * bx] : bx];      // (workgroup-uniform) -1: first level only
    const int glast = l2.n_groups - 1;

    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float centre[D];
    launch_centre<D, T>(static_cast<const T*>(l2.centre_x), b, N, centre);
    // lane l reads record l of a group: K block `half`, column l31
    const uint4* cols0 = pk.rec + b * pk.stride;      // (wave-uniform: the ring's scalar base)
    const uint4* cols = cols0 + lane;
    const uint32_t lane_off = lane * 16u;
    auto operand = [&](int g) -> u32x4 {
        return *reinterpret_cast<const u32x4*>(cols + (long)list_clamp(g, glast) * 64);
    };
    auto as_u4 = [](const u32x4& v) { return uint4{v.x, v.y, v.z, v.w}; };

    const int wslot = (wave + bx) & 3;      // (the rotation of the staged kernel: the empty slots of partial chunks fall on different SIMDs)
    for (int row0 = row_begin; row0 < row_end; row0 += kRowsPerBlock) {
        const int wave_row0 = row0 + wslot * 32;
        if (wave_row0 >= row_end) continue;
        const long irow = (long)b * N + min(wave_row0 + l31, row_end - 1);
        float xi[D];
        load_point<D, T>(prm.x, irow, xi);
        uint4 X;      // record `half` of [k,k,k,n1,n2,n3 | a_hi,a_hi,a_lo per coordinate], n = 0 for now
        float n2 = 0.f;
        {
            float a[D];
            const float q = __builtin_sqrtf(prm.s2);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float xt = xi[d] - centre[d];
                a[d] = xt * q;
                n2 = __builtin_fmaf(xt, xt, n2);
            }
            X = select_u4(half != 0, xd_record_of<D, true, L>(1, 0.f, a), xd_record_of<D, true, L>(0, 0.f, a));
        }
        float m = kH2Floor, ssum = 0.f;
        bool first_group = true;
        float thr = -INFINITY;
        float wlo[3] = {0.f, 0.f, 0.f}, whi[3] = {0.f, 0.f, 0.f};      // the wavefront's row box, wave-uniform
        if (home >= 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                wlo[d] = wave_min_uniform(xi[d]);
                whi[d] = wave_max_uniform(xi[d]);
            }
        }
        auto row_threshold = [&]() {      // from the running maxima as they stand
            const float rowoff = 0.5f * prm.s2 * n2;      // m - rowoff: the running maximum as a full exponent
            const float full = m - rowoff;
            const float low = __builtin_isfinite(full) ? full - kP2Slack * (__builtin_fabsf(m) + rowoff) : -INFINITY;
            return wave_min_uniform(low) - l2.L2;
        };
        auto set_max = [&](float mx) { X = select_u4(half == 0, xd_with_n<L>(X, -mx), X); };
        auto plain_x = [&]() { return select_u4(half == 0, xd_with_n<L>(X, 0.f), X); };

        if (home >= 0) {      // seed: exact row maxima over the home block (MFMA + max, no exponentials; n = 0 so far)
            const int hj0 = home * kHomeCols, hg = (min(kHomeCols, M - hj0) + 31) >> 5;
            float um = kH2Floor;
            for (int G = 0; G < hg; ++G) um = fmaxf(um, max16(mfma_h32(as_u4(operand((hj0 >> 5) + G)), X, zero16)));
            um = fmaxf(um, __shfl_xor(um, 32, 64));
            m = um;
            set_max(um);
            first_group = false;
            thr = fmaxf(row_threshold(), l2.t2[wave_row0 >> 5]);
        }

        ListCursor cur = list_begin(rg.redranges_j, q_begin, q_end, split, ns);
        // the records of a batch's groups, one per lane
        float4 ra = float4{0.f, 0.f, 0.f, 0.f}, rb = ra;
        auto fetch_records = [&](const ListCursor& c) {
            const float4* r = reinterpret_cast<const float4*>(l2.groups + list_clamp((c.j0 >> 5) + lane, glast));
            ra = r[0];
            rb = r[1];
        };
        if (home >= 0 && cur.q < q_end) fetch_records(cur);

        while (cur.q < q_end) {
            int g0, ng;
            const ListCursor nxt = list_next(rg.redranges_j, q_end, ns, cur, g0, ng);
            cur = nxt;
            unsigned long long keep = list_lanes(ng);      // lanes past the piece's end keep nothing
            if (home >= 0) {
                const float ub = list_group_ub(ra, rb, wlo, whi, prm.s2);
                keep &= __ballot(__float_as_int(rb.w) != 0 || !(ub < thr));
                if (nxt.q < q_end) fetch_records(nxt);
            }
            if (first_group) {      // a slab without a seed: exact maximum over the first 32 columns
                const f32x16 u = mfma_h32(as_u4(operand(g0)), X, zero16);
                float um = max16(u);
                um = fmaxf(um, __shfl_xor(um, 32, 64));
                um = fmaxf(um, kH2Floor);
                m = um;
                ssum = sum_exp2_16(u, um);
                set_max(um);
                first_group = false;
                keep &= keep - 1ull;
            }
            int n = __builtin_popcountll(keep);
            if (n == 0) continue;

            unsigned long long todo = keep;
            auto pop = [&]() { return list_pop(todo, g0, glast); };
            // The ring.  hipcc sinks a plain load to the block of its first use — behind the early exits below every operand would
            // be loaded where it is consumed, and waited for at once — so these loads are issued by hand and counted by hand: the
            // loads of one batch return in order, three are in flight when the fourth is awaited, and the ring is drained before
            // its registers are free again (a load still in flight would land in whatever they hold by then).
            float stmp = 0.f;
            u32x4 a0, a1, a2, a3;
            list_issue(a0, cols0 + (long)pop() * 64, lane_off);
            list_issue(a1, cols0 + (long)pop() * 64, lane_off);
            list_issue(a2, cols0 + (long)pop() * 64, lane_off);
            while (true) {
                list_issue(a3, cols0 + (long)pop() * 64, lane_off);
                list_wait3(a0);
                stmp += sum_exp2_16(mfma_h32(as_u4(a0), X, zero16));
                if (--n == 0) break;
                list_issue(a0, cols0 + (long)pop() * 64, lane_off);
                list_wait3(a1);
                stmp += sum_exp2_16(mfma_h32(as_u4(a1), X, zero16));
                if (--n == 0) break;
                list_issue(a1, cols0 + (long)pop() * 64, lane_off);
                list_wait3(a2);
                stmp += sum_exp2_16(mfma_h32(as_u4(a2), X, zero16));
                if (--n == 0) break;
                list_issue(a2, cols0 + (long)pop() * 64, lane_off);
                list_wait3(a3);
                stmp += sum_exp2_16(mfma_h32(as_u4(a3), X, zero16));
                if (--n == 0) break;
            }
            list_drain(a0, a1, a2, a3);
            if (__any(!(stmp < kSumThr))) {
                // a term far above the lazy max arrived (or inf / NaN): redo the batch with exact per-group maxima
                const uint4 xp = plain_x();
                for (todo = keep; todo; todo &= todo - 1ull) {
                    const f32x16 u = mfma_h32(as_u4(operand(g0 + __builtin_ctzll(todo))), xp, zero16);
                    float um = max16(u);
                    um = fmaxf(um, __shfl_xor(um, 32, 64));
                    const float mnew = fmaxf(m, um);
                    ssum = ssum * fast_exp2(m - mnew) + sum_exp2_16(u, mnew);
                    m = mnew;
                }
                set_max(m);
                if (home >= 0) thr = fmaxf(row_threshold(), l2.t2[wave_row0 >> 5]);
            } else {
                ssum += stmp;
            }
        }

        float sfin = ssum + __shfl_xor(ssum, 32, 64);      // both halves carry the same max
        if (m <= kH2Floor * 0.98f) sfin = 0.f;              // a row still at the floor has seen no mass
        const int i = wave_row0 + l31;
        if (half == 0 && i < row_end) {
            const float mtot = __builtin_fmaf(-0.5f * prm.s2, n2, m);      // r_i + m
            if (ns == 1) {
                prm.out[(long)b * N + i] = finish_value(prm, (long)b * N + i, mtot + fast_log2(sfin));
            } else {
                float* dst = sp.workspace + split * sp.split_stride + ((long)b * N + i) * 2;
                dst[0] = mtot;
                dst[1] = sfin;
            }
        }
    }
}

}  // namespace glhip
