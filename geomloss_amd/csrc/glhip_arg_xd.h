// glhip_arg_xd.h — the arg-reductions on RESIDENT, PRE-PACKED operands for clouds of dimension 1 <= D <= 16 (GLHIP_FLAG_XD_ARG): for
// every row the k columns of the smallest dual-shifted cost, best first,
//   index_i[r] = column of the (r+1)-th smallest  c_ij = |x_i - y_j|^2 / 2 - g_j,   value_i[r] = that cost,      0 <= r < k,
// p = 2, float32 / bfloat16, dense and batched launches; k = 1 serves glhip_argmin, every k up to kArgkminMaxK glhip_argkmin.
//
// Why a second family.  The K-chunked chain of glhip_argmin_xk.h / glhip_argkmin_xk.h stages on the fly with three barriers per tile of
// 128 columns and takes D at run time: below D = 17 it feeds one to seven MFMAs per block with staging that costs far more than they
// do.  Here BOTH operands are packed once per call and the reducing kernel only copies, multiplies and filters.
//
// Operands: the 6-slot bf16 x 3 layout of glhip_klayout.h (scalar item first, six slots per coordinate, NM = ceil(6 (D + 1) / 16) =
// 1 .. 7 chained v_mfma_f32_32x32x16_bf16), both sides in the group-major order of XdPacked — [batch][group of 32 points][NBP = 2 NM
// records][32 points] — around ONE centre per launch (launch_centre), scales of 1:
//   columns  xd_pack_kernel<XD_ARG> (glhip_softmin_xd.h): scalar item [H1,H2,H3,1,1,1] with H_j = g_j - |yt_j|^2 / 2.  g_j = -inf stays
//            -inf, and the padded columns of the last group carry H = -inf too: their exponent is -inf whatever the row, and -inf never
//            enters a list (strict compare), so that no tile needs a test by index.
//   rows     arg_xd_pack_rows_kernel: scalar item [1,1,1,0,0,0]; |xt_i|^2 / 2 is kept aside (one float per row) for
//            value = |xt_i|^2 / 2 - u.  A group of 32 rows is NM runs of 64 records: lane l of a wavefront loads its operand of MFMA m with
//            one 16-byte read at [64 m + l], coalesced.
// The packed records are free of the cloud's dtype and of D (only NM is left of it), so the reducing kernel is templated on NM and the
// list capacity alone: 7 x 4 = 28 instantiations, where D x T x CAP would be 128.  A floored pass (k > 16) is the SAME kernel with a
// non-NULL floor pointer — the floor is read on the slow path only, behind a wavefront-uniform branch — which halves the count again.
// The packing kernels are the only ones that know D and T (16 x 2 each side, a few dozen instructions each).
//
// Reducing kernel (arg_xd_kernel): the geometry of the pre-packed xd_fwd_body.  Two LDS tile buffers of kTile = XdShape::kTilePre
// columns (1152 / 576 / 384 / 288 / 224 / 192 / 160 for NM = 1 .. 7: at most 36 KiB each), filled by LDS-DMA (glds16: 1 KiB per wavefront
// instruction, no staging registers) while the other one is consumed, ONE barrier per tile.  8 wavefronts; every wavefront sweeps all
// the columns of the tile against its own RT row tiles of 32 rows, whose x-side records stay in registers for the whole column sweep
// (4 NM RT VGPRs).  So a row lives in one wavefront: there are no column halves of the workgroup to merge, only the two lane halves
// (__shfl_xor 32) and the column splits.  Column splits are whole groups of 32 (as the packed layout), through launch_plan_pass /
// plan_splits like the other arg kernels; their partials have the format of argkmin_merge_kernel (kc pairs (u, index) per row and
// split, |xt_i|^2 / 2 parked in value[row k + r0]), which merges them — CAP = 1 included, so glhip_argmin needs no merge of its own.
//
// Epilogue: the filter of glhip_argkmin_xk.h, per 32 x 32 block (16 exponents of a lane's row, ascending columns), for every capacity,
// k = 1 included — the VALU is the bound here, not the staging:
//   fast path  max chain over the 16 exponents (NaN drops out) against the list's last entry, one ballot, one wavefront-uniform branch;
//   slow path  the 16-bit set of elements that beat the last entry (a floored pass ANDs in "strictly behind the row's floor", the
//              lexicographic test of glhip_argkmin_xk.h on the same floor words at the head of the workspace), then lowest bit ->
//              element by a select tree (15 v_cndmask) -> topk_push (glhip_topk_list.h, static subscripts), while any lane has one.
// u_ij = H_j + xt_i . yt_j does not depend on tile, split or capacity, so inside this family: ties go to the smallest index,
// duplicates come in ascending index order, rank r of a call with k is rank r of a call with any larger k, k = 1 of glhip_argkmin is
// glhip_argmin bit for bit, and the result does not depend on the column splits.  Against the xk family the centre differs (one per
// launch here, one per row block there): values differ by rounding, indices agree where float64 separates the candidates.
//
// Row tiles per wavefront and resources.  __launch_bounds__(512, 4): 4 waves per SIMD, 128 VGPRs, two workgroups per CU (2 x 72 KiB of
// LDS).  RT = 2 (512 rows per workgroup) where lists and operands fit that budget — capacities 1 and 4 up to NM = 5 —, RT = 1 (256
// rows) for capacities 8 and 16, whose lists alone are 16 / 32 registers per row tile, and for NM = 6 / 7, whose operands are 24 / 28
// per row tile (RT = 2 there: 48 / 48 / 64 bytes of scratch per lane at (NM, CAP) = (6, 4) / (7, 1) / (7, 4)).  So k = 8 / 16 keep two
// workgroups per CU: the occupancy penalty the xk family pays there (one workgroup per CU) is gone; they pay half the reuse of an LDS
// read instead.  The compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950, printed by every build of
// glhip_api_arg_xd.hip), VGPRs per instantiation; scratch 0 bytes and 4 waves per SIMD for every one; LDS 73728 bytes, 71680 at NM = 5 / 7:
//     CAP \ NM     1     2     3     4     5     6     7
//      1          67    79    92   103   116    76    80
//      4          79    91   104   115   127    82    86
//      8          69    73    78    81    86    90    94
//     16          92    96   101   104   109   113   117
//   arg_xd_pack_rows_kernel<D, T>: 12 ... 103 VGPRs, xd_pack_kernel<XD_ARG, D, T> alike; argkmin_merge_kernel<1 / 4 / 8 / 16>: 10 / 18 / 26 / 56;
//   no scratch anywhere.  Timings: profiles/arg_xd.txt.
#pragma once

#include "glhip_softmin_xd.h"
#include "glhip_argkmin_xk.h"

namespace glhip {

constexpr int kArgXdWaves = 8;
constexpr int kArgXdThreads = kArgXdWaves * 64;
constexpr long kArgXdSlots = 256 * 2;      // resident workgroups: two per CU
constexpr int arg_xd_num_mfma(int D) { return (6 * (D + 1) + 15) / 16; }
constexpr int arg_xd_rt(int cap, int NM) { return (cap <= 4 && NM <= 5) ? 2 : 1; }                  // row tiles per wavefront
constexpr int arg_xd_rows(int cap, int NM) { return kArgXdWaves * 32 * arg_xd_rt(cap, NM); }        // rows per workgroup
constexpr int arg_xd_cap(int k) { return k <= 1 ? 1 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }
constexpr int arg_xd_tile(int NM) { return (2304 / (2 * NM)) / 32 * 32; }        // XdShape::kTilePre
static_assert(arg_xd_num_mfma(16) == XdShape<16>::NM && arg_xd_num_mfma(1) == XdShape<1>::NM && arg_xd_tile(XdShape<9>::NM) == XdShape<9>::kTilePre,
              "glhip_klayout.h");

struct ArgXdParams {
    const uint4* xrec;   // packed rows, [B][ceil(N / 32)][2 NM][32]
    long xstride;        // records per batch item
    const uint4* yrec;   // packed columns, [B][ceil(M / 32)][2 NM][32]
    long ystride;
    const float* hn;     // (B,N): |xt_i|^2 / 2
    int32_t* index;      // (B,N,k)
    float* value;        // (B,N,k) or NULL
    int k;               // ranks per row of index / value: their row stride
    int r0, kc;          // the launch writes the ranks r0 .. r0 + kc - 1, kc <= CAP
    int32_t* floor;      // NULL: a plain launch; else (B N, 2), the floors of a floored pass (glhip_argkmin_xk.h)
};

// The rows of a call as x-side records, and |xt_i|^2 / 2.  Rows i >= N of the last group are zero points (their results are not stored).
template <int D, typename T>
__global__ void __launch_bounds__(kBlock)
arg_xd_pack_rows_kernel(const T* __restrict__ x, int N, XdPacked pk, float* __restrict__ hn) {
    using S = XdShape<D>;
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ((N + 31) & ~31)) return;
    float centre[D], xt[D], n2 = 0.f;
    launch_centre<D, T>(x, b, N, centre);
#pragma unroll
    for (int d = 0; d < D; ++d) xt[d] = 0.f;
    if (i < N) {
        float xi[D];
        load_point<D, T>(x, (long)b * N + i, xi);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            xt[d] = xi[d] - centre[d];
            n2 = __builtin_fmaf(xt[d], xt[d], n2);
        }
        hn[(long)b * N + i] = 0.5f * n2;
    }
    uint4* base = pk.rec + b * pk.stride + (long)(i >> 5) * S::kGroupRecs + (i & 31);
#pragma unroll
    for (int r = 0; r < S::NBP; ++r) base[r * 32] = xd_record_of<D, true>(r, 0.f, xt);
}

// element e of the 16 exponents of a block, e a run-time number: a tree of 15 selects over static subscripts
__device__ __forceinline__ float arg_xd_pick(const f32x16& a, int e) {
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = (e & 8) ? a[i + 8] : a[i];
#pragma unroll
    for (int w = 4; w >= 1; w >>= 1) {
#pragma unroll
        for (int i = 0; i < w; ++i) t[i] = (e & w) ? t[i + w] : t[i];
    }
    return t[0];
}

template <int NM, int CAP>
__global__ void __launch_bounds__(kArgXdThreads, 4)
arg_xd_kernel(ArgXdParams prm, int N, int M, SplitInfo sp) {
    constexpr int NBP = 2 * NM, kTileD = arg_xd_tile(NM), RT = arg_xd_rt(CAP, NM), kRows = arg_xd_rows(CAP, NM);
    __shared__ uint4 tileBuf[2 * kTileD * NBP];

    int bx, b, split;
    workgroup_coords(sp, bx, b, split);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int rec0 = half * 32 + l31;       // K block `half` of MFMA 0; MFMA m: + 64 m
    const int ns = sp.n_splits;
    const int k = prm.k, r0 = prm.r0, kc = prm.kc;
    const bool floored = prm.floor != nullptr;

    const int row0 = bx * kRows;
    const int row_end = min(N, row0 + kRows);
    const int wave_row0 = row0 + wave * (RT * 32);
    const bool wave_active = wave_row0 < row_end;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // the x-side records of this wavefront's row tiles, resident for the whole sweep (a tile past the last group repeats the last one)
    uint4 X[RT][NM];
    float lu[RT][CAP];
    int li[RT][CAP];
    const int last_group = (N - 1) >> 5;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int G = min((wave_row0 >> 5) + rt, last_group);
        const uint4* src = prm.xrec + b * prm.xstride + (long)G * (32 * NBP) + lane;
#pragma unroll
        for (int m = 0; m < NM; ++m) X[rt][m] = src[m * 64];
        topk_clear<CAP>(lu[rt], li[rt]);
    }

    // this split's columns: whole groups of 32, like the packed layout
    const int len = (((M + ns - 1) / ns) + 31) & ~31;
    const int js = (int)min((long)M, (long)split * len);
    const int je = (int)min((long)M, (long)js + len);
    auto stage = [&](int j0, int buf) {
        const int nGs = (min(kTileD, je - j0) + 31) >> 5;
        const uint4* src = prm.yrec + b * prm.ystride + (long)(j0 >> 5) * (32 * NBP);
        for (int c = wave; c < nGs * NM; c += kArgXdWaves) glds16(src + c * 64 + lane, &tileBuf[buf * (kTileD * NBP) + c * 64]);
    };
    if (js < je) stage(js, 0);

    int t = 0;
    for (int j0 = js; j0 < je; j0 += kTileD, ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's share of tile t has landed ...
        __syncthreads();                                      // ... and so has everybody's; tile t - 1 is consumed
        if (j0 + kTileD < je) stage(j0 + kTileD, (t + 1) & 1);
        if (!wave_active) continue;
        const uint4* tile = tileBuf + (t & 1) * (kTileD * NBP);
        const int nG = (min(kTileD, je - j0) + 31) >> 5;
        for (int G = 0; G < nG; ++G) {
            const uint4* g = &tile[G * (32 * NBP)];
            const int col0 = j0 + G * 32 + 4 * half;          // column of this lane's element 0; element e: + 8 (e / 4) + e % 4
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const f32x16 u = xd_block<NM, NBP>(g, rec0, X[rt], zero16);
                const float last = lu[rt][CAP - 1];
                float mx = u[0];
#pragma unroll
                for (int e = 1; e < 16; ++e) mx = fmaxf(mx, u[e]);
                if (__ballot(mx > last) == 0) continue;
                // ---- slow path: some lane has a candidate ----
                float fu = __builtin_inff();
                int fd = -1;
                if (floored) {      // (fu, column of the floor - column of element 0) of the lane's row
                    const int i = min(wave_row0 + rt * 32 + l31, row_end - 1);
                    const int2 f = reinterpret_cast<const int2*>(prm.floor)[(long)b * N + i];
                    fu = __int_as_float(f.x);
                    fd = f.y - col0;
                }
                unsigned todo = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    bool take = u[e] > last;
                    take = take && (!floored || u[e] < fu || (u[e] == fu && 8 * (e / 4) + (e % 4) > fd));
                    todo |= take ? (1u << e) : 0u;
                }
                while (__ballot(todo != 0) != 0) {
                    const int e = todo ? __builtin_ctz(todo) : 0;
                    const float ue = todo ? arg_xd_pick(u, e) : -__builtin_inff();
                    topk_push<CAP>(lu[rt], li[rt], ue, col0 + 8 * (e >> 2) + (e & 3));
                    todo &= todo - 1;
                }
            }
        }
    }
    if (!wave_active) return;

    // ---- the two lane halves meet (they hold the two 16-column halves of every block); lane half 0 writes the row ----
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float ou[CAP];
        int oi[CAP];
#pragma unroll
        for (int e = 0; e < CAP; ++e) {
            ou[e] = __shfl_xor(lu[rt][e], 32, 64);
            oi[e] = __shfl_xor(li[rt][e], 32, 64);
        }
        topk_merge<CAP>(lu[rt], li[rt], ou, oi);
        const int i = wave_row0 + rt * 32 + l31;
        if (half != 0 || i >= row_end) continue;
        const long row = (long)b * N + i;
        const float hn = prm.hn[row];
        if (ns == 1) {
#pragma unroll
            for (int e = 0; e < CAP; ++e) {
                if (e < kc) {
                    prm.index[row * k + r0 + e] = li[rt][e];
                    if (prm.value) prm.value[row * k + r0 + e] = hn - lu[rt][e];
                }
            }
            if (floored) topk_store_floor<CAP>(prm.floor + 2 * row, lu[rt], li[rt], kc);
        } else {      // the partial of argkmin_merge_kernel, which also writes the next floor
            float* dst = sp.workspace + split * sp.split_stride + row * (2 * kc);
#pragma unroll
            for (int e = 0; e < CAP; ++e) {
                if (e < kc) {
                    dst[2 * e] = lu[rt][e];
                    reinterpret_cast<int*>(dst)[2 * e + 1] = li[rt][e];
                }
            }
            if (split == 0 && prm.value) prm.value[row * k + r0] = hn;
        }
    }
}

// A call without columns: every rank is missing
static __global__ void __launch_bounds__(kBlock) arg_xd_none_kernel(int32_t* __restrict__ index, float* __restrict__ value, long n) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    index[i] = -1;
    if (value) value[i] = __builtin_inff();
}

}  // namespace glhip
