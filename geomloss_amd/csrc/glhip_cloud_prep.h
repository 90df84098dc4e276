// glhip_cloud_prep.h — what the two translation units that sort a cloud share (glhip_cluster.hip: voxel clusters; glhip_compact_sort.hip:
// the compact order): the bounding box of a cloud, one workgroup at a time, and the size of rocPRIM's radix-sort scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace glhip {

// min / max for ints, fminf / fmaxf for floats (a NaN coordinate loses to every number)
__device__ __forceinline__ int box_min(int a, int b) { return min(a, b); }
__device__ __forceinline__ int box_max(int a, int b) { return max(a, b); }
__device__ __forceinline__ float box_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float box_max(float a, float b) { return fmaxf(a, b); }

// the box of no point
template <typename V> struct BoxEmpty;
template <> struct BoxEmpty<int> { static constexpr int lo = INT_MAX, hi = INT_MIN; };
template <> struct BoxEmpty<float> { static constexpr float lo = INFINITY, hi = -INFINITY; };

// The box of the points that a workgroup of 256 threads meets on its grid-stride walk over n points of D <= 3 coordinates V (int,
// float).  load(i, d): coordinate d of point i; commit(d, lo, hi): called by thread d < D of a workgroup that met a point, with the
// workgroup's extent on axis d.
// one commit — a pair of atomics — per axis and WORKGROUP: 4096 wavefronts hammering the same 6 words took 0.29 ms at 1e6 points
template <typename V, class Load, class Commit>
__device__ __forceinline__ void workgroup_box(int n, int D, Load load, Commit commit) {
    V lo[3] = {BoxEmpty<V>::lo, BoxEmpty<V>::lo, BoxEmpty<V>::lo}, hi[3] = {BoxEmpty<V>::hi, BoxEmpty<V>::hi, BoxEmpty<V>::hi};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        for (int d = 0; d < D; ++d) {
            const V v = load(i, d);
            lo[d] = box_min(lo[d], v);
            hi[d] = box_max(hi[d], v);
        }
    }
    for (int d = 0; d < D; ++d) {
        for (int off = 32; off > 0; off >>= 1) {
            lo[d] = box_min(lo[d], __shfl_xor(lo[d], off, 64));
            hi[d] = box_max(hi[d], __shfl_xor(hi[d], off, 64));
        }
    }
    __shared__ V wlo[4][3], whi[4][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int d = 0; d < D; ++d) { wlo[wave][d] = lo[d]; whi[wave][d] = hi[d]; }
    }
    __syncthreads();
    if (threadIdx.x < D) {
        const int d = threadIdx.x;
        V l = wlo[0][d], h = whi[0][d];
        for (int w = 1; w < 4; ++w) { l = box_min(l, wlo[w][d]); h = box_max(h, whi[w][d]); }
        if (l <= h) commit(d, l, h);
    }
}

// scratch of a radix sort of n (uint64 key, int32 value) pairs on the key bits [0, end_bit)
static inline size_t radix_sort_temp_bytes(int n, unsigned end_bit) {
    size_t bytes = 0;
    uint64_t* k = nullptr;
    int32_t* v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)n, 0u, end_bit, (hipStream_t)0) != hipSuccess || bytes == 0)
        bytes = (size_t)n * 16 + (1 << 20);   // no device to ask (build box): a bound rocPRIM's merge/onesweep paths stay under
    (void)hipGetLastError();
    return bytes;
}

}  // namespace glhip
