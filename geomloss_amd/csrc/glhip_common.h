// glhip_common.h — shared device helpers for the gfx950 map-reduce kernels.
// Written for CDNA4 only: 64-lane wavefronts, 256-thread workgroups, LDS-staged
// column tiles.  No CUDA compatibility layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glhip.h"

namespace glhip {

constexpr int kBlock = 256;   // threads per workgroup = 4 wavefronts, one per SIMD
constexpr int kTile = 1024;   // column records staged in LDS per tile (16 KiB of float4)
constexpr int kChunk = 8;     // column records consumed per inner-loop step
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kNegBig = -1.0e30f;   // "minus infinity" that survives (a - a)

// The base-2 log-sum-exp on which a gradient kernel centres the exponents of a row, from the saved forward value.  A row without mass
// (every h_j = -inf) comes back from the forward as +inf or as about kNegBig * out_scale (its neutral padding was all it saw): centred on
// that, the padding of the gradient sweep would weigh 2^(kNegBig - kNegBig).  Such a row is centred on -kNegBig instead, so that each
// of its weights is 2^(-huge) = 0, and its gradient is 0 (`row_gradient_scale`).  NaN passes through.
__device__ __forceinline__ float centring_lse2(float fwd, float out_scale) {
    const float lse2 = fwd / out_scale;
    return (lse2 <= 0.5f * kNegBig) ? -kNegBig : lse2;
}
// grad_out_i for a row with mass, 0 for a row without: g_i (x_i - sum_j P_ij y_j / mass_i) has no second term there, and the result is 0
__device__ __forceinline__ float row_gradient_scale(float gi, float mass) { return (mass > 0.f) ? gi : 0.f; }

// bf16 is carried as raw uint16_t: widening to fp32 is a 16-bit shift.
struct bf16_t { uint16_t bits; };

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<bf16_t>(bf16_t v) {
    return __uint_as_float(static_cast<uint32_t>(v.bits) << 16);
}

// raw transcendental instructions (v_exp_f32 = 2^x, v_log_f32 = log2, v_rsq_f32, v_sqrt_f32)
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float fast_log2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float fast_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// Column-interval description handed to every kernel (KeOps "ranges" convention, see glhip.h).
struct Ranges {
    const int32_t* ranges_i;
    const int32_t* slices_i;
    const int32_t* redranges_j;
    // optional row-chunk table built by build_row_chunks_kernel (glhip_mapreduce.h): chunks[0] = number of chunks T, then
    // T triplets (row block k, first row, end row).  NULL: one workgroup per row block (the KeOps granularity).
    const int32_t* chunks;
};

// Second, in-kernel level of the exact pruning of sorted p = 2 launches (glhip_autosort.h; the test itself: glhip_softmin_x32.h).
struct GroupBox {           // one aligned group of 32 sorted columns, as four 8-byte parts: the test reads one part per lane
    float lohi[3][2];       // box corners, (lo, hi) per coordinate (0, 0 beyond D)
    float lse;              // log sum exp of the group's dual values, rounded up (>= the largest of them; -inf: all -inf)
    int special;            // a non-finite coordinate or a NaN dual value: never skipped, left out of every sum
};
constexpr int kHomeCols = 256;      // columns of a slab's home block (= kPruneColBlock)
struct Level2 {
    const GroupBox* groups = nullptr;   // ceil(M / 32) records
    const int32_t* home = nullptr;      // per row block (slab): the column block that attains Mlb, -1: no second level for this slab
    const void* centre_x = nullptr;     // the caller's UNSORTED rows (N, D): launch_centre reads them, so the sorted launch expands its
                                        // exponents around the very centre of the dense launch of the same call
    int n_groups = 0;
    float L2 = 0.f;                     // L of the bound, in log2 units
    const float* t2 = nullptr;          // per tile of 32 sorted rows: the threshold of the mass rule, in log2 units (prune_tiles_kernel); read
                                        // only by slabs with a home block
    int32_t* list_takes = nullptr;      // f16 x 2: one int, written once per launch (list_decide) and read by both sweeps —
                                        // nonzero: the list-driven sweep takes the launch, 0: the staged one
};
// Which sweep takes the sorted p = 2 launch on the f16 x 2 layout, once per launch (glhip_prune.hip: one wavefront, behind prune_ranges
// on the same stream): list_takes_launch (glhip_list_cursor.h) on the emitted intervals and home blocks -> *out (Level2::list_takes);
// keep_pct: the rule's threshold.
void list_decide(const int32_t* slices_i, const int32_t* red, const int32_t* home, int n_slabs, int M, int keep_pct, int32_t* out,
                 hipStream_t st);

// One LDS record per column point: D coordinates (already centred / scaled) + one scalar.
template <int D> struct alignas(16) Rec { float c[4]; };            // D = 2, 3
template <> struct alignas(8) Rec<1> { float c[2]; };

template <int D> __device__ __forceinline__ float& rec_tail(Rec<D>& r) { return r.c[D]; }
template <int D> __device__ __forceinline__ float rec_tail(const Rec<D>& r) { return r.c[D]; }

template <int D, typename T>
__device__ __forceinline__ void load_point(const T* __restrict__ p, long idx, float (&o)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] = to_f32<T>(p[idx * D + d]);
}

// The one centre of a launch whose columns are packed once for all row blocks (pre-packed records, glhip_softmin_x32.h /
// glhip_wsum_x32.h): the mean of 8 rows spread evenly over batch item b.  The float32 error of an exponent assembled on the matrix
// cores grows with |x - c| |y - c|, so the centre should sit in the middle of the cloud whatever the order of the
// points: a single row (round 2: the first one) is a CORNER of the cloud as soon as the caller's points are sorted — a grid, a
// voxel-sorted scan — and costs 2-4 x the error of a central point.  Every kernel of a launch must compute the same bits: fixed
// order of additions, a power-of-two count.
template <int D, typename T>
__device__ __forceinline__ void launch_centre(const T* __restrict__ x, int b, int N, float (&c)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {       // rows (2k + 1) N / 16: the middles of 8 equal runs (N < 8: some rows twice — still a row mean)
        float p[D];
        load_point<D, T>(x, (long)b * N + (((long)(2 * k + 1) * N) >> 4), p);
#pragma unroll
        for (int d = 0; d < D; ++d) c[d] += p[d];
    }
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] *= 0.125f;
}

}  // namespace glhip
