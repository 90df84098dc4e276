// glhip_cluster.hip — the cluster pyramid of the two-scale ("multiscale") backends, on the device:
//   glhip_grid_cluster   voxel labels -> cluster-sorted cloud, per-cluster row ranges, weighted centroids, cluster weights
//   glhip_block_ranges   cluster-cluster keep rule -> CSR lists of merged column intervals, both orientations
// The reference does this with pykeops.torch.cluster.{grid_cluster, cluster_ranges_centroids, sort_clusters, from_matrix}
// (torch ops; _legacy/sinkhorn_samples.py:453-530, _legacy/kernel_samples.py:214-256); geomloss_amd/cluster.py restates those
// helpers with torch tensor ops (dozens of small launches, two host round trips each, and 1.2 s of lazily loaded torch code
// objects on the first call).  Here: a handful of launches on the caller's stream, no host round trip inside the library,
// deterministic results (fixed-order float64 sums, no atomics on floating-point data).
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <climits>
#include <cstdint>

#include "glhip_autosort.h"
#include "glhip_perm_index.h"
#include "glhip_balance.h"
#include "glhip_common.h"
#include "glhip_error.h"
#include "glhip_prune_words.h"

using namespace glhip;

namespace {

constexpr int kAxisBits = 21;                       // voxel coordinates (relative to the cloud's minimum) per axis
constexpr int kAxisMax = (1 << kAxisBits) - 1;

struct ClusterHead {        // first bytes of the workspace
    int qmin[3];
    int qmax[3];
    int overflow;           // a voxel coordinate did not fit kAxisBits
    int pad;
};

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

template <typename T>
__device__ __forceinline__ int voxel_of(const T* __restrict__ x, long idx, float pre_div, float voxel) {
    // two IEEE divisions, as torch evaluates floor((x / blur) / size)
    return (int)floorf((to_f32<T>(x[idx]) / pre_div) / voxel);
}

// the workspace head in its start state (one launch; three hipMemsetAsync calls were four fill kernels)
__global__ void head_init_kernel(ClusterHead* head) {
    const int t = threadIdx.x;
    if (t < 3) head->qmin[t] = INT_MAX;
    else if (t < 6) head->qmax[t - 3] = INT_MIN;
    else if (t == 6) head->overflow = 0;
    else if (t == 7) head->pad = 0;
}

template <typename T>
__global__ void __launch_bounds__(256) bounds_kernel(const T* __restrict__ x, int N, int D, float pre_div, float voxel, ClusterHead* head) {
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
        for (int d = 0; d < D; ++d) {
            const int q = voxel_of<T>(x, i * D + d, pre_div, voxel);
            lo[d] = min(lo[d], q);
            hi[d] = max(hi[d], q);
        }
    }
    for (int d = 0; d < D; ++d) {
        for (int off = 32; off > 0; off >>= 1) {
            lo[d] = min(lo[d], __shfl_xor(lo[d], off, 64));
            hi[d] = max(hi[d], __shfl_xor(hi[d], off, 64));
        }
    }
    // one pair of atomics per axis and WORKGROUP: 4096 wavefronts hammering the same 6 words took 0.29 ms at 1e6 points
    __shared__ int wlo[4][3], whi[4][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int d = 0; d < D; ++d) { wlo[wave][d] = lo[d]; whi[wave][d] = hi[d]; }
    }
    __syncthreads();
    if (threadIdx.x < D) {
        const int d = threadIdx.x;
        int l = wlo[0][d], h = whi[0][d];
        for (int w = 1; w < 4; ++w) { l = min(l, wlo[w][d]); h = max(h, whi[w][d]); }
        if (l <= h) {
            atomicMin(&head->qmin[d], l);
            atomicMax(&head->qmax[d], h);
        }
    }
}

// key = voxel coordinates packed most-significant-axis first: sorting the keys sorts the voxels lexicographically, which is
// the order of the labels pykeops' grid_cluster hands out
template <typename T>
__global__ void __launch_bounds__(256) keys_kernel(const T* __restrict__ x, int N, int D, float pre_div, float voxel, ClusterHead* head,
                                                   uint64_t* __restrict__ keys, int32_t* __restrict__ idx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    uint64_t key = 0;
    for (int d = 0; d < D; ++d) {
        const long q = (long)voxel_of<T>(x, i * D + d, pre_div, voxel) - head->qmin[d];
        if (q > kAxisMax) head->overflow = 1;
        key = (key << kAxisBits) | (uint64_t)(q & kAxisMax);
    }
    keys[i] = key;
    idx[i] = (int32_t)i;
}

__global__ void __launch_bounds__(256) flags_kernel(const uint64_t* __restrict__ keys, int N, int32_t* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < N) flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// labels (inclusive scan of the flags) -> [start, end) of every cluster, and the cluster count
__global__ void __launch_bounds__(256) ranges_kernel(const int32_t* __restrict__ incl, int N, int32_t* __restrict__ ranges, int32_t* n_clusters,
                                                     const ClusterHead* __restrict__ head) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int c = incl[i] - 1;
    if (i == 0 || incl[i - 1] != incl[i]) {
        ranges[2 * c] = (int32_t)i;
        if (c > 0) ranges[2 * (c - 1) + 1] = (int32_t)i;
    }
    if (i == N - 1) {
        ranges[2 * c + 1] = N;
        n_clusters[0] = c + 1;
        n_clusters[1] = head->overflow;     // the overflow flag of keys_kernel travels with the cluster count
        for (int d = 0; d < 3; ++d) {       // ... and so do the voxel bounds of the cloud: its bounding box, to one voxel
            n_clusters[2 + d] = head->qmin[d] == INT_MAX ? 0 : head->qmin[d];
            n_clusters[5 + d] = head->qmax[d] == INT_MIN ? 0 : head->qmax[d];
        }
    }
}

__device__ __forceinline__ double shfl_xor_f64(double v, int off) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, off, 64);
    hi = __shfl_xor(hi, off, 64);
    return __hiloint2double(hi, lo);
}

// one wavefront per cluster: weight and weighted centroid of (x / pre_div) in float64, in a fixed order
template <typename T>
__global__ void __launch_bounds__(256) centroids_kernel(const T* __restrict__ x, const float* __restrict__ w, const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ ranges, const int32_t* __restrict__ n_clusters, int D,
                                                        float pre_div, float* __restrict__ centroids, float* __restrict__ weights_c) {
    const int lane = threadIdx.x & 63;
    const int n_waves = gridDim.x * 4;
    const int C = n_clusters[0];
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < C; c += n_waves) {
        const int r0 = ranges[2 * c], r1 = ranges[2 * c + 1];
        double sw = 0.0, sx[3] = {0.0, 0.0, 0.0};
        for (int p = r0 + lane; p < r1; p += 64) {
            const long j = perm[p];
            const double wj = w ? (double)w[j] : 1.0;
            sw += wj;
            for (int d = 0; d < D; ++d) sx[d] += wj * (double)(to_f32<T>(x[j * D + d]) / pre_div);
        }
        for (int off = 32; off > 0; off >>= 1) {
            sw += shfl_xor_f64(sw, off);
            for (int d = 0; d < D; ++d) sx[d] += shfl_xor_f64(sx[d], off);
        }
        if (lane == 0) {
            const double den = sw > 1e-9 ? sw : 1e-9;     // cluster_ranges_centroids' min_weight
            for (int d = 0; d < D; ++d) centroids[(long)c * D + d] = (float)(sx[d] / den);
            weights_c[c] = (float)sw;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) gather_kernel(const T* __restrict__ x, const float* __restrict__ w, const int32_t* __restrict__ perm,
                                                     int N, int D, T* __restrict__ x_sorted, float* __restrict__ w_sorted) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const long j = perm[p];
    for (int d = 0; d < D; ++d) x_sorted[p * D + d] = x[j * D + d];
    if (w_sorted) w_sorted[p] = w ? w[j] : 1.0f;
}

size_t sort_temp_bytes(int N) {
    size_t bytes = 0;
    uint64_t* k = nullptr;
    int32_t* v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)N, 0u, (unsigned)(3 * kAxisBits), (hipStream_t)0) != hipSuccess || bytes == 0)
        bytes = (size_t)N * 16 + (1 << 20);   // no device to ask (build box): a bound rocPRIM's merge/onesweep paths stay under
    (void)hipGetLastError();
    return bytes;
}

size_t scan_temp_bytes(int N) {
    size_t bytes = 0;
    int32_t* v = nullptr;
    if (rocprim::inclusive_scan(nullptr, bytes, v, v, (size_t)N, rocprim::plus<int32_t>(), (hipStream_t)0) != hipSuccess || bytes == 0)
        bytes = (size_t)N * 4 + (1 << 20);
    (void)hipGetLastError();
    return bytes;
}

template <typename T>
int grid_cluster_typed(const void* x_, const float* w, int N, int D, float pre_div, float voxel, int32_t* perm, void* x_sorted,
                       float* w_sorted, int32_t* ranges, float* centroids, float* weights_c, int32_t* n_clusters, void* workspace,
                       size_t workspace_bytes, hipStream_t st) {
    const T* x = static_cast<const T*>(x_);
    char* ws = static_cast<char*>(workspace);
    ClusterHead* head = reinterpret_cast<ClusterHead*>(ws);
    size_t off = align256(sizeof(ClusterHead));
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(ws + off); off += align256((size_t)N * 8);
    uint64_t* keys_out = reinterpret_cast<uint64_t*>(ws + off); off += align256((size_t)N * 8);
    int32_t* idx_in = reinterpret_cast<int32_t*>(ws + off); off += align256((size_t)N * 4);
    int32_t* flags = reinterpret_cast<int32_t*>(ws + off); off += align256((size_t)N * 4);
    size_t temp_sort = sort_temp_bytes(N), temp_scan = scan_temp_bytes(N);
    const size_t temp = temp_sort > temp_scan ? temp_sort : temp_scan;
    if (off + temp > workspace_bytes)
        return fail(GLHIP_EINVAL, "glhip_grid_cluster: workspace of %zu bytes, need %zu (glhip_cluster_workspace_bytes)", workspace_bytes, off + temp);
    void* tmp = ws + off;

    const int blocks = (N + 255) / 256;
    hipLaunchKernelGGL(head_init_kernel, dim3(1), dim3(64), 0, st, head);
    hipLaunchKernelGGL((bounds_kernel<T>), dim3(blocks < 512 ? blocks : 512), dim3(256), 0, st, x, N, D, pre_div, voxel, head);
    hipLaunchKernelGGL((keys_kernel<T>), dim3(blocks), dim3(256), 0, st, x, N, D, pre_div, voxel, head, keys_in, idx_in);
    // rocPRIM's radix sort is stable: equal keys (one voxel) keep the order of their indices, as torch.sort(stable=True) does
    if (rocprim::radix_sort_pairs(tmp, temp_sort, keys_in, keys_out, idx_in, perm, (size_t)N, 0u, (unsigned)(D * kAxisBits), st) != hipSuccess)
        return fail(GLHIP_ELAUNCH, "glhip_grid_cluster: radix sort failed: %s", hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(flags_kernel, dim3(blocks), dim3(256), 0, st, keys_out, N, flags);
    int32_t* incl = idx_in;   // the unsorted indices are no longer needed
    if (rocprim::inclusive_scan(tmp, temp_scan, flags, incl, (size_t)N, rocprim::plus<int32_t>(), st) != hipSuccess)
        return fail(GLHIP_ELAUNCH, "glhip_grid_cluster: scan failed: %s", hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(ranges_kernel, dim3(blocks), dim3(256), 0, st, incl, N, ranges, n_clusters, head);
    // one wavefront per cluster, the count known on the device only: a wavefront per 4 points covers the fine grids of small clouds
    // in one round (a cluster loop of 7 rounds cost 50 us at N = 1e4), surplus wavefronts leave at once
    const int blocks_c = (N + 15) / 16;
    hipLaunchKernelGGL((centroids_kernel<T>), dim3(blocks_c < 2048 ? blocks_c : 2048), dim3(256), 0, st, x, w, perm, ranges, n_clusters, D, pre_div,
                       centroids, weights_c);
    if (x_sorted)
        hipLaunchKernelGGL((gather_kernel<T>), dim3(blocks), dim3(256), 0, st, x, w, perm, N, D, static_cast<T*>(x_sorted), w_sorted);
    return check_launch("glhip_grid_cluster");
}

// ---- compact order of a cloud (glhip_autosort.h): bounding box -> voxel edge -> boustrophedon path keys -> radix sort -> gather ----

struct SortHead {           // first bytes of the sort scratch
    unsigned lo[3], hi[3];  // bounding box, as order-preserving unsigned images of the floats
    float voxel;
    int qmin[3], ext[3];
};

__device__ __forceinline__ unsigned ordered_of(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

__global__ void sort_head_init_kernel(SortHead* head) {
    const int t = threadIdx.x;
    if (t < 3) { head->lo[t] = 0xFFFFFFFFu; head->hi[t] = 0u; }
}

template <typename T>
__global__ void __launch_bounds__(256) bbox_kernel(const T* __restrict__ x, int n, int D, SortHead* head) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        for (int d = 0; d < D; ++d) {
            const float v = to_f32<T>(x[i * D + d]);
            lo[d] = fminf(lo[d], v);
            hi[d] = fmaxf(hi[d], v);
        }
    }
    for (int d = 0; d < D; ++d) {
        for (int off = 32; off > 0; off >>= 1) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], off, 64));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off, 64));
        }
    }
    __shared__ float wlo[4][3], whi[4][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int d = 0; d < D; ++d) { wlo[wave][d] = lo[d]; whi[wave][d] = hi[d]; }
    }
    __syncthreads();
    if (threadIdx.x < D) {
        const int d = threadIdx.x;
        float l = wlo[0][d], h = whi[0][d];
        for (int w = 1; w < 4; ++w) { l = fminf(l, wlo[w][d]); h = fmaxf(h, whi[w][d]); }
        if (l <= h) {
            atomicMin(&head->lo[d], ordered_of(l));
            atomicMax(&head->hi[d], ordered_of(h));
        }
    }
}

// voxel edge that puts ~rows_per_voxel points in an occupied voxel (hip.py:_voxel_for), and the voxel grid of the cloud
__global__ void voxel_kernel(SortHead* head, int n, int D, int rows_per_voxel) {
    if (threadIdx.x != 0) return;
    float lo[3], ext[3], emax = 0.f;
    for (int d = 0; d < D; ++d) {
        lo[d] = float_of(head->lo[d]);
        ext[d] = float_of(head->hi[d]) - lo[d];
        emax = fmaxf(emax, ext[d]);
    }
    float vol = 1.f;
    int live = 0;
    for (int d = 0; d < D; ++d)
        if (ext[d] > 1e-6f * fmaxf(emax, 1e-30f)) { vol *= ext[d]; ++live; }
    float voxel = powf(vol * (float)rows_per_voxel / (float)n, 1.0f / (float)(live > 0 ? live : 1));
    voxel = fmaxf(fmaxf(voxel, emax / (float)(1 << 20)), 1e-30f);       // never more than 2^20 voxels along an axis
    head->voxel = voxel;
    for (int d = 0; d < 3; ++d) {
        head->qmin[d] = d < D ? (int)floorf(lo[d] / voxel) : 0;
        head->ext[d] = d < D ? (int)floorf((lo[d] + ext[d]) / voxel) - head->qmin[d] + 1 : 1;
    }
}

// sort key = index of the point's voxel along a boustrophedon path through the voxel grid (the scan direction of an axis flips each
// time the path index of the axes before it advances): voxels that follow each other in the order are face neighbours in space, so
// ANY run of consecutive rows of the sorted cloud is spatially compact (hip.py:_serpentine did this on the cluster list).
// sub > 1 (the sorted p = 2 launches): a minor key orders the points INSIDE a voxel by sub-voxel of edge voxel / sub, along the same
// kind of path, so that a run of ~rows_per_voxel / sub^D consecutive points (a 32-row wavefront tile, a group of 32 columns) has a
// sub-voxel's box instead of the whole voxel's; the voxel order itself, which the slab x block bound sees, is unchanged.
// With sub > 1 this path order is not the final one: balance_kernel reorders the points inside every whole aligned block of
// kBalanceBlock positions into median-cut cells (glhip_autosort.h: balanced cells); the path decides which points share a block,
// and it alone orders the last n mod kBalanceBlock points.
template <typename T>
__global__ void __launch_bounds__(256) path_keys_kernel(const T* __restrict__ x, int n, int D, const SortHead* __restrict__ head, int sub,
                                                        uint64_t* __restrict__ keys, int32_t* __restrict__ idx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float voxel = head->voxel;
    uint64_t path = 0, minor = 0, cells = 1;
    for (int d = 0; d < D; ++d) {
        const int e = head->ext[d];
        const float f = to_f32<T>(x[i * D + d]) / voxel, fl = floorf(f);
        int q = (int)fl - head->qmin[d];
        q = q < 0 ? 0 : (q >= e ? e - 1 : q);
        const int c = (path & 1) ? e - 1 - q : q;
        path = path * (uint64_t)e + (uint64_t)c;
        if (sub > 1) {
            int r = (int)((f - fl) * (float)sub);
            r = r > 0 ? (r >= sub ? sub - 1 : r) : 0;      // (NaN: 0)
            minor = minor * (uint64_t)sub + (uint64_t)((minor & 1) ? sub - 1 - r : r);
            cells *= (uint64_t)sub;
        }
    }
    keys[i] = path * cells + minor;      // path < 2^60 (at most 2^20 voxels along an axis), cells <= 9
    idx[i] = (int32_t)i;
}

// The balancing pass of the sorted p = 2 call (glhip_autosort.h: balanced cells; the rules: glhip_balance.h).  One workgroup per whole
// aligned block of kBalanceBlock positions of `perm`, one point per thread, in place: the block's points and indices go to LDS, five
// levels sort every segment (1024, 512, ..., 64 positions) by (coordinate on the segment's longest axis, incoming position), and the
// indices come back in the new order.  The sort is a bitonic network on the words of balance_word, one word per thread in a register:
// partners less than a wavefront apart meet in registers (lane_xor), the others through LDS.  The levels above the last stop their
// last merge after its first step: it already splits the segment into its lower and upper half, which is all the next level reads
// of it (balance_step_runs: 155 of the 185 steps of five full sorts run, 14 of the 20 through LDS).  The words of a segment are
// distinct, so the order is a function of the block's points alone.
static_assert(kBalanceBlock == 1024 && kBalanceLeaf == 32, "one point per thread of a 1024-thread workgroup; segments down to one wavefront");

// The value of lane (lane ^ j) of the wavefront, j a power of two below 64 that is a constant where this is inlined: a DPP move inside
// rows of 16 lanes (j = 1, 2: quad_perm; 8: a row rotated by 8; 4: half-row mirror, lane ^ 7, then the quads reversed, lane ^ 3), a
// swap of 16-lane rows (j = 16) or of the halves (j = 32) of two copies.  All VALU: the network's 141 shuffle steps and the 90
// extent steps of a block take no LDS cycles (__shfl_xor is a ds_bpermute: 462 of them per wavefront and block).
template <int CTRL>
__device__ __forceinline__ unsigned dpp_move(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ unsigned lane_xor(unsigned v, int j, int lane) {
    switch (j) {
        case 1: return dpp_move<0xB1>(v);                       // quad_perm:[1,0,3,2]
        case 2: return dpp_move<0x4E>(v);                       // quad_perm:[2,3,0,1]
        case 4: return dpp_move<0x1B>(dpp_move<0x141>(v));      // row_half_mirror, quad_perm:[3,2,1,0]
        case 8: return dpp_move<0x128>(v);                      // row_ror:8
        case 16: {      // r[0]: rows 0, 0, 2, 2 of v; r[1]: rows 1, 1, 3, 3
            const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
            return (lane & 16) ? r[0] : r[1];
        }
        case 32: {      // r[0]: the lower half twice; r[1]: the upper half twice
            const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
            return (lane & 32) ? r[0] : r[1];
        }
        default: return (unsigned)__shfl_xor((int)v, j, 64);
    }
}
__device__ __forceinline__ float lane_xor(float v, int j, int lane) { return __uint_as_float(lane_xor(__float_as_uint(v), j, lane)); }

template <typename T>
__global__ void __launch_bounds__(kBalanceBlock) balance_kernel(const T* __restrict__ z, int D, int32_t* __restrict__ perm) {
    __shared__ float pts[3][kBalanceBlock];
    __shared__ int32_t src[kBalanceBlock];
    __shared__ unsigned long long words[kBalanceBlock];
    __shared__ float wlo[kBalanceBlock / 64][3], whi[kBalanceBlock / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long base = (long)blockIdx.x * kBalanceBlock;
    {
        const int32_t j = perm[base + tid];
        src[tid] = j;
        for (int d = 0; d < 3; ++d) pts[d][tid] = d < D ? to_f32<T>(z[(long)j * D + d]) : 0.f;
    }
    __syncthreads();
    int p = tid;      // the incoming position of the point that sits at position tid now
    constexpr int kBalanceBits = 10, kBalanceLevels = 5;      // 1024 = 2^10 positions; segments of 1024 >> 0, ..., 1024 >> 4 = 64
#pragma unroll
    for (int lv = 0; lv < kBalanceLevels; ++lv) {
        const int seg = kBalanceBlock >> lv;
        // the extents of this thread's segment: per wavefront by shuffle, then over the segment's wavefronts
        float lo[3], hi[3];      // (an axis beyond D: no finite value, it loses to every other)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = INFINITY;
            hi[d] = -INFINITY;
            if (d < D) balance_extent_add(pts[d][p], lo[d], hi[d]);
#pragma unroll
            for (int ob = 5; ob >= 0; --ob) {
                lo[d] = fminf(lo[d], lane_xor(lo[d], 1 << ob, lane));
                hi[d] = fmaxf(hi[d], lane_xor(hi[d], 1 << ob, lane));
            }
            if (lane == 0) { wlo[wave][d] = lo[d]; whi[wave][d] = hi[d]; }
        }
        __syncthreads();
        const int waves = seg >> 6, w0 = wave & ~(waves - 1);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            for (int w = w0; w < w0 + waves; ++w) {
                lo[d] = fminf(lo[d], wlo[w][d]);
                hi[d] = fmaxf(hi[d], whi[w][d]);
            }
        }
        const int axis = balance_axis(lo, hi, 3);
        unsigned long long v = balance_word(balance_key(pts[axis][p]), (unsigned)p);
        // (counted loops that unroll: seg, k and j are constants in every step, so the partner and the direction cost no arithmetic)
#pragma unroll
        for (int kb = 1; kb <= kBalanceBits - lv; ++kb) {
            const int k = 1 << kb;
#pragma unroll
            for (int jb = kb - 1; jb >= 0; --jb) {
                const int j = 1 << jb;
                if (!balance_step_runs(j, k, seg, 2 * kBalanceLeaf)) break;      // a level above the last: the halves as sets
                unsigned long long o;
                if (j >= 64) {      // (uniform over the workgroup)
                    __syncthreads();      // every read of the step before is done (and, first, every read of wlo / whi)
                    words[tid] = v;
                    __syncthreads();
                    o = words[tid ^ j];
                } else {
                    const unsigned ol = lane_xor((unsigned)v, j, lane), oh = lane_xor((unsigned)(v >> 32), j, lane);
                    o = ((unsigned long long)oh << 32) | ol;
                }
                v = (balance_keeps_min(tid, j, k, seg) == (o < v)) ? o : v;
            }
        }
        p = (int)(unsigned)v;
        __syncthreads();      // wlo / whi and words are free for the next level
    }
    perm[base + tid] = src[p];
}

// kHinted: `perm` came from outside the call (a hinted permutation, glhip_perm_index.h): every entry is clamped into [0, n).  Without
// it the three kernels are what they were.
template <typename T, bool kHinted>
__global__ void __launch_bounds__(256) gather_points_kernel(const T* __restrict__ x, const int32_t* __restrict__ perm, int n, int D, T* __restrict__ xs) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const long j = kHinted ? perm_index(perm[p], n) : perm[p];
    for (int d = 0; d < D; ++d) xs[p * D + d] = x[j * D + d];
}

template <bool kHinted>
__global__ void __launch_bounds__(256) gather_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ perm, float* __restrict__ dst, int n) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < n) dst[k] = src[kHinted ? perm_index(perm[k], n) : perm[k]];
}
template <bool kHinted>
__global__ void __launch_bounds__(256) scatter_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ perm, float* __restrict__ dst, int n, int width) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const long j = kHinted ? perm_index(perm[k], n) : perm[k];
    for (int d = 0; d < width; ++d) dst[j * width + d] = src[k * width + d];
}

// "every slab of kSortSlab rows x all columns, in kSortColChunks column intervals" as KeOps-style ranges
__global__ void __launch_bounds__(256) slab_ranges_kernel(int N, int M, int C, int32_t* __restrict__ ranges_i, int32_t* __restrict__ slices_i,
                                                          int32_t* __restrict__ red) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= C) return;
    ranges_i[2 * k] = k * kSortSlab;
    ranges_i[2 * k + 1] = min(N, (k + 1) * kSortSlab);
    slices_i[k] = (k + 1) * kSortColChunks;
    const int step = (((M + kSortColChunks - 1) / kSortColChunks) + 31) / 32 * 32;
    for (int c = 0; c < kSortColChunks; ++c) {
        red[2 * (k * kSortColChunks + c)] = min(M, c * step);
        red[2 * (k * kSortColChunks + c) + 1] = min(M, (c + 1) * step);
    }
}

// ---- exact block pruning of the sorted p = 2 launch (glhip_autosort.h: the bound and why it is exact) ------------------------------

struct ColBlock {           // one block of kPruneColBlock sorted columns
    float lo[3];
    float hmax;             // largest dual value of the block (-inf: all -inf)
    float hi[3];
    float lse;              // log sum exp of the block's dual values, rounded up; NaN marks a SPECIAL block (a non-finite coordinate or a
                            // NaN dual value): kept by every slab, left out of Mlb and of every sum
};
// lse in float32, rounded up.  The sum of up to 256 terms e^(h - hmax) in [0, 1] is a tree of float32 adds 8 deep over expf values good to
// 2 ulp: under 1e-6 relative, so under 1e-6 in the logarithm; logf of a value in [1, 256] is good to 2 ulp of 5.6: 1e-6; the final add
// rounds by 2^-24 |lse|.  The block's value is formed from the eight rounded-up group values in the same way, once more.  Slack
// 2^-20 (|lse| + 8): 16 ulp of the value plus 7.6e-6, several times the sum of those.
constexpr float kPruneLseSlack = 9.5367431640625e-7f;      // 2^-20
__device__ __forceinline__ float lse_up(float v) { return v + kPruneLseSlack * (__builtin_fabsf(v) + 8.f); }

static_assert(kHomeCols == kPruneColBlock && kPruneColBlock % 64 == 0 && sizeof(GroupBox) == 32, "block / group records");

// one wavefront per column block; in step k lanes 0-31 take the block's group 2 k of 32 columns and lanes 32-63 group 2 k + 1: the
// same pass writes the record of every group (the second level of the bound, glhip_softmin_x32.h) and the block's own
template <typename T>
__global__ void __launch_bounds__(256) prune_blocks_kernel(const T* __restrict__ ys, const float* __restrict__ h, const float* __restrict__ pot,
                                                           float pot_scale, int M, int D, int nT, ColBlock* __restrict__ out,
                                                           GroupBox* __restrict__ groups) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= nT) return;
    float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float bhm = -INFINITY;
    float gls[kPruneColBlock / 64];      // the values of this half's groups
    int bbad = 0;
    const int j0 = t * kPruneColBlock, j1 = min(M, j0 + kPruneColBlock);
#pragma unroll
    for (int k = 0; k < kPruneColBlock / 64; ++k) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        float hm = -INFINITY, hv = -INFINITY;
        int bad = 0;
        const int j = j0 + 64 * k + lane;
        if (j < j1) {
            for (int d = 0; d < D; ++d) {
                const float v = to_f32<T>(ys[(long)j * D + d]);
                bad |= !__builtin_isfinite(v);
                lo[d] = v;
                hi[d] = v;
            }
            hv = pot ? __builtin_fmaf(pot[j], pot_scale, h[j]) : h[j];     // as the half-step forms it (glhip_softmin_ops.h)
            bad |= __builtin_isnan(hv);
            hm = fmaxf(hm, hv);      // (drops a NaN: the mark carries it)
        }
        for (int off = 16; off > 0; off >>= 1) {
            for (int d = 0; d < D; ++d) {
                lo[d] = fminf(lo[d], __shfl_xor(lo[d], off, 64));
                hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off, 64));
            }
            hm = fmaxf(hm, __shfl_xor(hm, off, 64));
            bad |= __shfl_xor(bad, off, 64);
        }
        // the group's log sum exp around its maximum (a NaN or -inf value adds nothing; hm = +-inf stands for itself)
        float se = (__builtin_isfinite(hm) && hv > -INFINITY) ? expf(hv - hm) : 0.f;
        for (int off = 16; off > 0; off >>= 1) se += __shfl_xor(se, off, 64);
        const float gl = __builtin_isfinite(hm) ? lse_up(hm + logf(se)) : hm;
        gls[k] = gl;
        const int g0 = j0 + 64 * k + (lane & 32);      // first column of this half's group
        if ((lane & 31) == 0 && g0 < j1) {
            GroupBox b;
            for (int d = 0; d < 3; ++d) {
                b.lohi[d][0] = d < D ? lo[d] : 0.f;
                b.lohi[d][1] = d < D ? hi[d] : 0.f;
            }
            b.lse = gl;
            b.special = bad;
            groups[g0 >> 5] = b;
        }
        for (int d = 0; d < D; ++d) {
            blo[d] = fminf(blo[d], lo[d]);
            bhi[d] = fmaxf(bhi[d], hi[d]);
        }
        bhm = fmaxf(bhm, hm);
        bbad |= bad;
    }
    for (int d = 0; d < D; ++d) {
        blo[d] = fminf(blo[d], __shfl_xor(blo[d], 32, 64));
        bhi[d] = fmaxf(bhi[d], __shfl_xor(bhi[d], 32, 64));
    }
    bhm = fmaxf(bhm, __shfl_xor(bhm, 32, 64));
    bbad |= __shfl_xor(bbad, 32, 64);
    float gm = -INFINITY;
#pragma unroll
    for (int k = 0; k < kPruneColBlock / 64; ++k) gm = fmaxf(gm, gls[k]);
    gm = fmaxf(gm, __shfl_xor(gm, 32, 64));
    float blse = gm;
    if (__builtin_isfinite(gm)) {
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < kPruneColBlock / 64; ++k) se += expf(gls[k] - gm);      // (an empty or all -inf group: e^-inf = 0)
        se += __shfl_xor(se, 32, 64);
        blse = lse_up(gm + logf(se));
    }
    if (lane == 0) {
        ColBlock b;
        for (int d = 0; d < 3; ++d) {
            b.lo[d] = d < D ? blo[d] : 0.f;
            b.hi[d] = d < D ? bhi[d] : 0.f;
        }
        b.hmax = bhm;
        b.lse = bbad ? NAN : blse;
        out[t] = b;
    }
}

// squared distances between two boxes, smallest and largest, in float64 (exact float32 corners in, 1e-16 relative error out)
__device__ __forceinline__ void box_d2(const double (&rlo)[3], const double (&rhi)[3], const ColBlock& b, int D, double& dmin2, double& dmax2) {
    dmin2 = 0.0;
    dmax2 = 0.0;
    for (int d = 0; d < D; ++d) {
        const double blo = b.lo[d], bhi = b.hi[d];
        const double gap = fmax(fmax(blo - rhi[d], rlo[d] - bhi), 0.0);
        const double far = fmax(bhi - rlo[d], rhi[d] - blo);
        dmin2 = fma(gap, gap, dmin2);
        dmax2 = fma(far, far, dmax2);
    }
}

// inclusive scan of one int per thread over a 256-thread workgroup (MAX: maximum, else sum); `buf` holds 256 ints of LDS
template <bool MAX>
__device__ __forceinline__ int block_scan256(int v, int* buf) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int o = t >= off ? buf[t - off] : (MAX ? INT_MIN : 0);
        __syncthreads();
        v = MAX ? max(v, o) : v + o;
        buf[t] = v;
        __syncthreads();
    }
    return v;
}

// The bucket of a key for a histogram that starts at `lo`: -1 below it (the underflow bucket, always dropped), kPruneBuckets above its
// range (never dropped).  A NaN key counts as above the range.
__device__ __forceinline__ int prune_bucket(double key, double lo) {
    const double d = (key - lo) * (1.0 / kPruneBucketNats);
    if (d < 0.0) return -1;
    return d < (double)kPruneBuckets ? (int)d : kPruneBuckets;
}
// The first bucket that is kept: buckets are dropped from the bottom while the dropped mass (the underflow bucket first) stays within the
// budget.  The underflow bucket alone cannot exceed it: every key in it has a mass below e^-L = 2^-26 e^-1 / M, and it holds at most
// ceil(M / 256) blocks (first level, budget 2^-26 e^-1) or ceil(M / 32) groups (second level, budget 2^-26 (1 - 2 / e) > 2^-26 e^-1 / 16)
// — so bucket 0 is always a valid answer.
__device__ __forceinline__ int prune_first_kept(const double* hist, double under, double budget) {
    double s = under;
    int b = 0;
    for (; b < kPruneBuckets; ++b) {
        if (s + hist[b] > budget) break;
        s += hist[b];
    }
    return b;
}

// One workgroup per slab of kSortSlab sorted rows: its box, Mlb, then the kept blocks as column intervals in its S slots of `red`
// (unused slots: empty intervals, which the kernels skip).  A piece starts at a kept block that opens a run (the gap to the previous
// kept block is >= g blocks) or that sits on the piece grid (a multiple of PB).  g = 1 unless the slab has more than kPruneRuns runs;
// then g is the smallest gap length that leaves at most kPruneRuns runs (gaps shorter than g are closed).
// kept(t) is evaluated once per block, into a bit set in LDS (up to 64 x kPruneMaskWords = 65536 blocks; beyond that every walk evaluates it
// again, as all of them did before).  For g = 1 — all but a handful of slabs — runs are counted and pieces written from
// the 64-bit words (glhip_prune_words.h): one prefix sum over the workgroup instead of two per 256 blocks (~1100 barriers per slab at M = 1e6).
// A slab with more runs (one in seven at M = 1e6 with balanced cells) takes its gap lengths from the same words into a list in LDS,
// finds g on the list and writes its pieces from the words too; only a slab whose bit set or whose gap list does not fit walks the blocks.
constexpr int kPruneMaskWords = 1024;      // 65536 blocks = 16.7e6 columns: 8 KB
constexpr int kPruneGaps = 2048;           // gap lengths of a slab with more than kPruneRuns runs: 8 KB
template <typename T>
__global__ void __launch_bounds__(256) prune_slabs_kernel(const T* __restrict__ xs, int N, int M, int D, const ColBlock* __restrict__ blocks,
                                                          int nT, int PB, int S, double inv2eps, double L, int32_t* __restrict__ ranges_i,
                                                          int32_t* __restrict__ slices_i, int32_t* __restrict__ red, int32_t* __restrict__ home,
                                                          double* __restrict__ mlb_out, double* __restrict__ t1_out) {
    __shared__ int buf[256];
    __shared__ double hist[kPruneBuckets + 1];      // (the last entry: the underflow bucket)
    __shared__ int first_kept;
    __shared__ unsigned long long mask[kPruneMaskWords];
    __shared__ int32_t gaps[kPruneGaps];
    __shared__ float wlo[4][3], whi[4][3];
    __shared__ double wm[4];
    __shared__ int wb[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = k * kSortSlab, r1 = min(N, r0 + kSortSlab);
    if (tid == 0) {
        ranges_i[2 * k] = r0;
        ranges_i[2 * k + 1] = r1;
        slices_i[k] = (k + 1) * S;
    }
    // the slab's box
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    if (r0 + tid < r1) {
        for (int d = 0; d < D; ++d) {
            const float v = to_f32<T>(xs[(long)(r0 + tid) * D + d]);
            bad |= !__builtin_isfinite(v);
            lo[d] = v;
            hi[d] = v;
        }
    }
    for (int d = 0; d < D; ++d) {
        for (int off = 32; off > 0; off >>= 1) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], off, 64));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off, 64));
        }
        if (lane == 0) { wlo[wave][d] = lo[d]; whi[wave][d] = hi[d]; }
    }
    bad = __syncthreads_or(bad);
    double rlo[3] = {0.0, 0.0, 0.0}, rhi[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < D; ++d) {
        rlo[d] = fminf(fminf(wlo[0][d], wlo[1][d]), fminf(wlo[2][d], wlo[3][d]));
        rhi[d] = fmaxf(fmaxf(whi[0][d], whi[1][d]), fmaxf(whi[2][d], whi[3][d]));
    }
    // Mlb: a lower bound on the largest exponent of every row of the slab
    // ... and the block that attains it: the slab's home block (the first of them)
    double mlb = -INFINITY;
    int best = -1;
    if (!bad) {
        for (int t = tid; t < nT; t += 256) {
            const ColBlock b = blocks[t];
            if (__builtin_isnan(b.lse)) continue;
            double dmin2, dmax2;
            box_d2(rlo, rhi, b, D, dmin2, dmax2);
            const double v = (double)b.hmax - dmax2 * inv2eps;
            if (v > mlb) { mlb = v; best = t; }      // (t ascends: the first block of a tie stays)
        }
        auto take = [&](double v, int t) {
            if (t >= 0 && (v > mlb || (v == mlb && (best < 0 || t < best)))) { mlb = v; best = t; }
        };
        for (int off = 32; off > 0; off >>= 1) {
            const double v = __shfl_xor(mlb, off, 64);
            const int t = __shfl_xor(best, off, 64);
            take(v, t);
        }
        if (lane == 0) { wm[wave] = mlb; wb[wave] = best; }
        __syncthreads();
        mlb = -INFINITY;
        best = -1;
        for (int w = 0; w < 4; ++w) take(wm[w], wb[w]);
    }
    const bool keep_all = bad || !__builtin_isfinite(mlb);
    // The mass rule (glhip_autosort.h): a histogram of the keys k(T) = lse(T) - dmin(R,T)^2 / (2 eps) above the classic threshold Mlb - L,
    // every bucket holding the mass e^(k(T) - Mlb) of its blocks
    const double lo_key = mlb - L;
    auto block_key = [&](const ColBlock& b) {
        double dmin2, dmax2;
        box_d2(rlo, rhi, b, D, dmin2, dmax2);
        return (double)b.lse - dmin2 * inv2eps;
    };
    for (int q = tid; q <= kPruneBuckets; q += 256) hist[q] = 0.0;
    __syncthreads();
    if (!keep_all) {
        for (int t = tid; t < nT; t += 256) {
            const ColBlock b = blocks[t];
            if (__builtin_isnan(b.lse)) continue;
            const double key = block_key(b);
            const int q = prune_bucket(key, lo_key);
            if (q >= kPruneBuckets) continue;      // above the range: never added, so no exp for it
            const double mass = exp(key - mlb);
            if (mass > 0.0) atomicAdd(&hist[q < 0 ? kPruneBuckets : q], mass);
        }
    }
    __syncthreads();
    if (tid == 0) {
        first_kept = keep_all ? 0 : prune_first_kept(hist, hist[kPruneBuckets], kPruneBudget1);
        mlb_out[k] = mlb;
        t1_out[k] = keep_all ? -INFINITY : lo_key + first_kept * kPruneBucketNats;
    }
    __syncthreads();
    const int fk = first_kept;
    auto kept = [&](int t) {
        if (keep_all) return true;
        const ColBlock b = blocks[t];
        if (__builtin_isnan(b.lse)) return true;
        return prune_bucket(block_key(b), lo_key) >= fk;
    };
    // No second level where it has nothing to win: a slab without a bound, and a slab whose bound keeps every block (large eps: the
    // finer test would pass nearly every group as well, and costs ~2 % of the sweep)
    const int nW = (nT + 63) >> 6;
    const bool masked = nW <= kPruneMaskWords;
    {
        int all = 1;
        if (masked) {      // one word per wavefront and step
            for (int w = wave; w < nW; w += 4) {
                const int t = 64 * w + lane;
                const unsigned long long m = __ballot(t < nT && kept(t));
                if (lane == 0) mask[w] = m;
                all &= m == (nT - 64 * w >= 64 ? ~0ull : (1ull << (nT - 64 * w)) - 1ull);
            }
        } else if (!keep_all) {
            for (int t = tid; t < nT && all; t += 256) all = kept(t) ? 1 : 0;
        }
        all = __syncthreads_and(all);      // (also: the bit set is written)
        if (tid == 0) home[k] = (keep_all || all) ? -1 : best;
    }
    auto kept_at = [&](int t) { return masked ? ((mask[t >> 6] >> (t & 63)) & 1ull) != 0 : kept(t); };
    // one walk over the blocks: the number of runs for gap length g, and (EMIT) the pieces written out
    int32_t* slots = red + 2 * (long)k * S;
    auto walk = [&](int g, bool emit) {
        int carry = -1, runs = 0, pieces = 0;
        for (int c0 = 0; c0 < nT; c0 += 256) {
            const int t = c0 + tid;
            const bool kp = t < nT && kept_at(t);
            block_scan256<true>(kp ? t : -1, buf);      // buf[t]: the last kept block of the chunk up to t
            const int prev = max(carry, tid > 0 ? buf[tid - 1] : -1);
            const int last = buf[255];
            const bool run = kp && (prev < 0 || t - prev - 1 >= g);
            const bool start = run || (kp && t % PB == 0);
            runs += __syncthreads_count(run);             // (also: every read of buf is done before the next scan writes it)
            carry = max(carry, last);
            if (emit) {
                const int idx = pieces + block_scan256<false>(start ? 1 : 0, buf) - 1;
                if (start && idx < S) {
                    slots[2 * idx] = t * kPruneColBlock;
                    if (idx > 0) slots[2 * idx - 1] = min(M, (run ? prev + 1 : t) * kPruneColBlock);
                }
                pieces += __syncthreads_count(start);
            }
        }
        if (emit) {
            const int n = min(pieces, S);
            if (tid == 0 && n > 0) slots[2 * n - 1] = min(M, (carry + 1) * kPruneColBlock);
            for (int q = n + tid; q < S; q += 256) {
                slots[2 * q] = 0;
                slots[2 * q + 1] = 0;
            }
        }
        return runs;
    };
    // g = 1 on the bit set (glhip_prune_words.h): thread i owns the words [i wpt, (i + 1) wpt)
    const int wpt = (nW + 255) / 256, w0 = min(nW, tid * wpt), w1 = min(nW, w0 + wpt);
    int runs1 = 0;
    if (masked) {
        // the pieces for gap length gw from the words: nstart of them start in this thread's words
        auto emit_words = [&](int gw, int nstart) {
            const int base = block_scan256<false>(nstart, buf) - nstart;
            const int n = min(buf[255], S);
            prune_emit_words(mask, w0, w1, base, PB, S, kPruneColBlock, M, slots, gw);
            if (tid == 0 && n > 0) prune_emit_last(mask, nW, n, kPruneColBlock, M, slots);
            for (int q = n + tid; q < S; q += 256) {
                slots[2 * q] = 0;
                slots[2 * q + 1] = 0;
            }
        };
        int nrun, nstart;
        prune_count_words(mask, w0, w1, PB, nrun, nstart);
        const int run0 = block_scan256<false>(nrun, buf) - nrun;      // the runs that start before this thread's words
        runs1 = buf[255];
        __syncthreads();
        if (runs1 <= kPruneRuns) {      // (workgroup-uniform)
            emit_words(1, nstart);
            return;
        }
        // More runs than kPruneRuns: the gap in front of every run but the first, from the words as well, g by bisection over the
        // gap lengths (one count over the workgroup per step and 256 gaps; the walk pays two scans per step and 256 BLOCKS), and the
        // pieces from the words again.  A slab with more gaps than the list holds keeps the walk below.
        if (runs1 - 1 <= kPruneGaps) {
            const int n_gaps = runs1 - 1;
            prune_gap_lengths(mask, w0, w1, run0, kPruneGaps, gaps);
            __syncthreads();
            int lo_g = 0, hi_g = nT;      // (prune_gap_select, glhip_prune_words.h)
            while (hi_g - lo_g > 1) {
                const int mid = lo_g + (hi_g - lo_g) / 2;
                int c = 0;
                for (int q0 = 0; q0 < n_gaps; q0 += 256) c += __syncthreads_count(q0 + tid < n_gaps && gaps[q0 + tid] >= mid);
                if (1 + c > kPruneRuns) lo_g = mid; else hi_g = mid;
            }
            prune_count_words(mask, w0, w1, PB, nrun, nstart, hi_g);
            emit_words(hi_g, nstart);
            return;
        }
    }
    int g = 1;
    if ((masked ? runs1 : walk(1, false)) > kPruneRuns) {
        int lo_g = 1, hi_g = nT;   // walk(nT) has one run
        while (hi_g - lo_g > 1) {
            const int mid = lo_g + (hi_g - lo_g) / 2;
            if (walk(mid, false) > kPruneRuns) lo_g = mid; else hi_g = mid;
        }
        g = hi_g;
    }
    walk(g, true);
}

// The mass rule of the second level (glhip_autosort.h).  One workgroup per slab with a home block, after prune_slabs_kernel: for each of
// the slab's 8 tiles W of 32 rows, the seed ms(W) — the smallest over the tile's rows of the row's exact largest exponent over the home
// block, float64 from the points themselves — then one histogram per tile of the keys k(W, G) = lse(G) - dmin(W,G)^2 / (2 eps) of the
// groups G inside the slab's emitted intervals, starting at ms(W) - L, and from it the threshold t2(W): written in log2 units, the
// reducing kernel's, as a float32 rounded toward minus infinity.  Thread = row for the seeds, thread = (group, tile) for the histograms.
static_assert(kPruneRuns + kPruneGrid <= 256 && kSortSlab == 256, "one thread per interval slot / per row");
template <typename T>
__global__ void __launch_bounds__(256) prune_tiles_kernel(const T* __restrict__ xs, const T* __restrict__ ys, const float* __restrict__ h,
                                                          const float* __restrict__ pot, float pot_scale, int N, int M, int D,
                                                          const GroupBox* __restrict__ groups, const int32_t* __restrict__ red, int S,
                                                          const int32_t* __restrict__ home, double inv2eps, double L, float* __restrict__ t2) {
    constexpr int kTiles = kSortSlab / 32;
    __shared__ int buf[256];
    __shared__ int first_group[256];
    __shared__ double hy[kPruneColBlock][3], hh[kPruneColBlock];
    __shared__ float tlo[kTiles][3], thi[kTiles][3];
    __shared__ double ms[kTiles];
    __shared__ double hist[kTiles][kPruneBuckets + 1];      // (the last entry: the underflow bucket)
    const int k = blockIdx.x, tid = threadIdx.x, w = tid >> 5;
    const int hb = home[k];
    if (hb < 0) return;      // no second level for this slab: nobody reads its thresholds
    const int r0 = k * kSortSlab, r1 = min(N, r0 + kSortSlab);
    // the home block's columns
    {
        const int j = hb * kPruneColBlock + tid;
        const bool real = j < M;
        for (int d = 0; d < 3; ++d) hy[tid][d] = (real && d < D) ? (double)to_f32<T>(ys[(long)j * D + d]) : 0.0;
        hh[tid] = real ? (double)(pot ? __builtin_fmaf(pot[j], pot_scale, h[j]) : h[j]) : -INFINITY;
    }
    for (int q = tid; q < kTiles * (kPruneBuckets + 1); q += 256) (&hist[0][0])[q] = 0.0;
    // this thread's row, its tile's box and seed
    const bool row = r0 + tid < r1;
    float x[3] = {0.f, 0.f, 0.f};
    if (row)
        for (int d = 0; d < D; ++d) x[d] = to_f32<T>(xs[(long)(r0 + tid) * D + d]);
    for (int d = 0; d < 3; ++d) {
        float lo = row ? x[d] : INFINITY, hi = row ? x[d] : -INFINITY;
        for (int off = 16; off > 0; off >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, off, 64));
            hi = fmaxf(hi, __shfl_xor(hi, off, 64));
        }
        if ((tid & 31) == 0) { tlo[w][d] = lo; thi[w][d] = hi; }
    }
    __syncthreads();
    {
        double seed = -INFINITY;
        const double xd[3] = {(double)x[0], (double)x[1], (double)x[2]};
        for (int j = 0; j < kPruneColBlock; ++j) {
            double d2 = 0.0;
            for (int d = 0; d < 3; ++d) {
                const double t = xd[d] - hy[j][d];
                d2 = fma(t, t, d2);
            }
            seed = fmax(seed, hh[j] - d2 * inv2eps);      // (a padding column: -inf)
        }
        // the tile's smallest seed; a seed that is not finite (none should be: the home block attains a finite Mlb) turns the rule off
        int ok = !row || __builtin_isfinite(seed);
        double v = row ? seed : INFINITY;
        for (int off = 16; off > 0; off >>= 1) {
            v = fmin(v, __shfl_xor(v, off, 64));
            ok &= __shfl_xor(ok, off, 64);
        }
        if ((tid & 31) == 0) ms[w] = (ok && r0 + 32 * w < r1) ? v : NAN;      // NaN: no rows, or no finite seed
    }
    // the groups of the emitted intervals, numbered through: first_group[q] = groups before interval q
    const int32_t* slots = red + 2 * (long)k * S;
    int j0 = 0, ng = 0;
    if (tid < S) {
        j0 = slots[2 * tid];
        ng = (max(slots[2 * tid + 1], j0) - j0 + 31) >> 5;      // (intervals start on multiples of kPruneColBlock)
    }
    const int incl = block_scan256<false>(ng, buf);
    first_group[tid] = incl - ng;
    const int total = buf[255];
    __syncthreads();
    // The groups go through in chunks of 256: thread = group to find the chunk's group numbers, then thread = (group, tile) pair with
    // the tile in the low bits, 32 groups per pass.  A wavefront's adds of one instruction so go to the 8 histograms, 8 groups each,
    // not to the few buckets that 64 neighbouring groups share in ONE histogram; a thread keeps one tile's box, seed and underflow
    // sum in registers, not eight, and the loop over tiles with the inlined exp is gone.
    const int c = tid & (kTiles - 1), sub = tid / kTiles;
    const double m = ms[c], lo_key = m - L;
    double tl[3], th[3];
    for (int d = 0; d < 3; ++d) {
        tl[d] = (double)tlo[c][d];
        th[d] = (double)thi[c][d];
    }
    double under = 0.0;
    for (int f0 = 0; f0 < total; f0 += 256) {
        const int f = f0 + tid;
        int g = 0;
        if (f < total) {
            int q = 0;      // the last slot with first_group <= f (empty slots share their successor's value and are passed over)
            for (int step = 128; step > 0; step >>= 1)
                if (q + step < 256 && first_group[q + step] <= f) q += step;
            g = (slots[2 * q] >> 5) + (f - first_group[q]);
        }
        __syncthreads();      // every read of the chunk before is done (and, first, of the scan)
        buf[tid] = g;
        __syncthreads();
        if (!(m == m)) continue;      // (the barriers above are passed by every thread)
        const int cnt = min(256, total - f0);
        for (int s = sub; s < cnt; s += 2 * (256 / kTiles)) {      // two records in flight
            const int s1 = s + 256 / kTiles;
            const GroupBox b0 = groups[buf[s]], b1 = groups[buf[min(s1, cnt - 1)]];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const GroupBox& b = u ? b1 : b0;
                if ((u && s1 >= cnt) || b.special) continue;
                double dmin2 = 0.0;
                for (int d = 0; d < 3; ++d) {
                    const double gap = fmax(fmax((double)b.lohi[d][0] - th[d], tl[d] - (double)b.lohi[d][1]), 0.0);
                    dmin2 = fma(gap, gap, dmin2);
                }
                const double key = (double)b.lse - dmin2 * inv2eps;
                const int bk = prune_bucket(key, lo_key);
                if (bk >= kPruneBuckets) continue;
                const double mass = exp(key - m);
                if (bk < 0) under += mass;
                else if (mass > 0.0) atomicAdd(&hist[c][bk], mass);
            }
        }
    }
    if (under > 0.0) atomicAdd(&hist[c][kPruneBuckets], under);
    __syncthreads();
    if (tid < kTiles && r0 + 32 * tid < r1) {
        const double m = ms[tid];
        float out = -INFINITY;
        if (m == m) {
            const int fk = prune_first_kept(hist[tid], hist[tid][kPruneBuckets], kPruneBudget2);
            const double v = (m - L + fk * kPruneBucketNats) * 1.4426950408889634;
            out = (float)v;
            if ((double)out > v) out = nextafterf(out, -INFINITY);
        }
        t2[(r0 >> 5) + tid] = out;
    }
}

size_t sort64_temp_bytes(int n) {
    size_t bytes = 0;
    uint64_t* k = nullptr;
    int32_t* v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)n, 0u, 64u, (hipStream_t)0) != hipSuccess || bytes == 0)
        bytes = (size_t)n * 16 + (1 << 20);
    (void)hipGetLastError();
    return bytes;
}

template <typename T>
int compact_sort_typed(const void* z_, int n, int D, int rows_per_voxel, int sub, int32_t* perm, void* z_sorted, void* scratch,
                       size_t scratch_bytes, hipStream_t st, bool hinted) {
    const T* z = static_cast<const T*>(z_);
    const int blocks = (n + 255) / 256;
    if (hinted) {      // `perm` holds the order already (glhip_perm_index.h): no box, no keys, no sort, no balancing — the gather alone
        hipLaunchKernelGGL((gather_points_kernel<T, true>), dim3(blocks), dim3(256), 0, st, z, perm, n, D, static_cast<T*>(z_sorted));
        return GLHIP_OK;
    }
    char* ws = static_cast<char*>(scratch);
    SortHead* head = reinterpret_cast<SortHead*>(ws);
    size_t off = align256(sizeof(SortHead));
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(ws + off); off += align256((size_t)n * 8);
    uint64_t* keys_out = reinterpret_cast<uint64_t*>(ws + off); off += align256((size_t)n * 8);
    int32_t* idx_in = reinterpret_cast<int32_t*>(ws + off); off += align256((size_t)n * 4);
    size_t temp = sort64_temp_bytes(n);
    if (off + temp > scratch_bytes) return fail(GLHIP_EINVAL, "compact_sort: scratch of %zu bytes, need %zu", scratch_bytes, off + temp);
    hipLaunchKernelGGL(sort_head_init_kernel, dim3(1), dim3(64), 0, st, head);
    hipLaunchKernelGGL((bbox_kernel<T>), dim3(blocks < 512 ? blocks : 512), dim3(256), 0, st, z, n, D, head);
    hipLaunchKernelGGL(voxel_kernel, dim3(1), dim3(64), 0, st, head, n, D, rows_per_voxel);
    hipLaunchKernelGGL((path_keys_kernel<T>), dim3(blocks), dim3(256), 0, st, z, n, D, head, sub, keys_in, idx_in);
    if (rocprim::radix_sort_pairs(ws + off, temp, keys_in, keys_out, idx_in, perm, (size_t)n, 0u, 64u, st) != hipSuccess)
        return fail(GLHIP_ELAUNCH, "compact_sort: radix sort failed: %s", hipGetErrorString(hipGetLastError()));
    // the sorted p = 2 call: balanced cells inside every whole block of kBalanceBlock positions; the partial last block keeps the path order
    if (sub > 1 && n >= kBalanceBlock)
        hipLaunchKernelGGL((balance_kernel<T>), dim3(n / kBalanceBlock), dim3(kBalanceBlock), 0, st, z, D, perm);
    hipLaunchKernelGGL((gather_points_kernel<T, false>), dim3(blocks), dim3(256), 0, st, z, perm, n, D, static_cast<T*>(z_sorted));
    return GLHIP_OK;
}

}  // namespace

namespace glhip {

size_t compact_sort_scratch_bytes(int n) {
    return align256(sizeof(SortHead)) + 2 * align256((size_t)n * 8) + align256((size_t)n * 4) + align256(sort64_temp_bytes(n));
}

int compact_sort(const void* z, int n, int D, int in_dtype, int rows_per_voxel, int32_t* perm, void* z_sorted, void* scratch,
                 size_t scratch_bytes, hipStream_t st, int sub, bool hinted) {
    return in_dtype == GLHIP_F32 ? compact_sort_typed<float>(z, n, D, rows_per_voxel, sub, perm, z_sorted, scratch, scratch_bytes, st, hinted)
                                 : compact_sort_typed<bf16_t>(z, n, D, rows_per_voxel, sub, perm, z_sorted, scratch, scratch_bytes, st, hinted);
}

void gather_f32(const float* src, const int32_t* perm, float* dst, int n, hipStream_t st, bool hinted) {
    if (hinted) hipLaunchKernelGGL(gather_f32_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, st, src, perm, dst, n);
    else hipLaunchKernelGGL(gather_f32_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, st, src, perm, dst, n);
}

void scatter_f32(const float* src, const int32_t* perm, float* dst, int n, hipStream_t st, int width, bool hinted) {
    if (hinted) hipLaunchKernelGGL(scatter_f32_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, st, src, perm, dst, n, width);
    else hipLaunchKernelGGL(scatter_f32_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, st, src, perm, dst, n, width);
}

void slab_ranges(int N, int M, int32_t* ranges_i, int32_t* slices_i, int32_t* red, hipStream_t st) {
    const int C = (N + kSortSlab - 1) / kSortSlab;
    hipLaunchKernelGGL(slab_ranges_kernel, dim3((C + 255) / 256), dim3(256), 0, st, N, M, C, ranges_i, slices_i, red);
}

size_t prune_blocks_bytes(int M) { return (size_t)prune_plan(M).nT * sizeof(ColBlock); }
size_t prune_groups_bytes(int M) { return (size_t)((M + 31) / 32) * sizeof(GroupBox); }

void prune_ranges(const void* xs, const void* ys, const float* h, const float* pot, float pot_scale, int N, int M, int D, int in_dtype,
                  float eps, int32_t* ranges_i, int32_t* slices_i, int32_t* red, void* blocks_, void* groups_, int32_t* home, float* t2,
                  double* mlb, double* t1, hipStream_t st) {
    const PrunePlan pp = prune_plan(M);
    const int C = (N + kSortSlab - 1) / kSortSlab;
    ColBlock* blocks = static_cast<ColBlock*>(blocks_);
    GroupBox* groups = static_cast<GroupBox*>(groups_);
    const double inv2eps = 0.5 / (double)eps;
    const double L = prune_L(M);
    if (in_dtype == GLHIP_F32) {
        hipLaunchKernelGGL(prune_blocks_kernel<float>, dim3((pp.nT + 3) / 4), dim3(256), 0, st, static_cast<const float*>(ys), h, pot, pot_scale, M, D,
                           pp.nT, blocks, groups);
        hipLaunchKernelGGL(prune_slabs_kernel<float>, dim3(C), dim3(256), 0, st, static_cast<const float*>(xs), N, M, D, blocks, pp.nT, pp.PB, pp.S,
                           inv2eps, L, ranges_i, slices_i, red, home, mlb, t1);
        hipLaunchKernelGGL(prune_tiles_kernel<float>, dim3(C), dim3(256), 0, st, static_cast<const float*>(xs), static_cast<const float*>(ys), h, pot,
                           pot_scale, N, M, D, groups, red, pp.S, home, inv2eps, L, t2);
    } else {
        hipLaunchKernelGGL(prune_blocks_kernel<bf16_t>, dim3((pp.nT + 3) / 4), dim3(256), 0, st, static_cast<const bf16_t*>(ys), h, pot, pot_scale, M,
                           D, pp.nT, blocks, groups);
        hipLaunchKernelGGL(prune_slabs_kernel<bf16_t>, dim3(C), dim3(256), 0, st, static_cast<const bf16_t*>(xs), N, M, D, blocks, pp.nT, pp.PB,
                           pp.S, inv2eps, L, ranges_i, slices_i, red, home, mlb, t1);
        hipLaunchKernelGGL(prune_tiles_kernel<bf16_t>, dim3(C), dim3(256), 0, st, static_cast<const bf16_t*>(xs), static_cast<const bf16_t*>(ys), h,
                           pot, pot_scale, N, M, D, groups, red, pp.S, home, inv2eps, L, t2);
    }
}

}  // namespace glhip

namespace {

// ---- keep rule -> merged column intervals ------------------------------------------------------------------------------

struct KeepRule {
    int kind;              // GLHIP_KEEP_DUAL_SLACK | GLHIP_KEEP_WITHIN
    const float* rows;     // (Cr, D) centroids of the row clusters
    const float* cols;     // (Cc, D)
    const float* f;        // (Cr) dual values of the rows   (dual slack only)
    const float* g;        // (Cc)
    int D, p;
    float thr;
};

__device__ __forceinline__ bool keep_pair(const KeepRule& k, int i, int j) {
    float d2 = 0.f;
    if (k.D <= 3) {      // branch-free: the loads of several calls can be in flight together (runs_kernel)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int dd = d < k.D ? d : 0;
            const float t = k.rows[(long)i * k.D + dd] - k.cols[(long)j * k.D + dd];
            d2 = d < k.D ? __builtin_fmaf(t, t, d2) : d2;
        }
    } else {
        for (int d = 0; d < k.D; ++d) {
            const float t = k.rows[(long)i * k.D + d] - k.cols[(long)j * k.D + d];
            d2 = __builtin_fmaf(t, t, d2);
        }
    }
    if (k.kind == GLHIP_KEEP_WITHIN) return d2 <= k.thr;                       // kernel_samples.py:244-252
    const float C = (k.p == 2) ? 0.5f * d2 : sqrtf(fmaxf(d2, 1e-8f));          // cost_routines, sinkhorn_samples.py:26-29
    return k.f[i] + k.g[j] > C - k.thr;                                        // sinkhorn_samples.py:512-514
}

// One wavefront per row cluster.  A "run" is a maximal sequence of kept column clusters that are adjacent in memory
// (range end == next range start): it becomes ONE column interval (same pair set as one interval per cluster, longer
// tiles for the kernels).  Every run has one start and one stop and they alternate along the row, so the k-th start and the
// k-th stop belong to the same run: ranks are plain prefix counts.
// FILL = false: counts[i] = number of runs.  FILL = true: writes the runs at offset slices[i-1] of `red`.
template <bool FILL>
__global__ void __launch_bounds__(256) runs_kernel(KeepRule rule, int Cr, int Cc, const int32_t* __restrict__ ranges_cols,
                                                   int32_t* __restrict__ counts, const int32_t* __restrict__ slices,
                                                   int32_t* __restrict__ red, long long capacity, int32_t* overflow) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= Cr) return;
    const int base = FILL ? (i == 0 ? 0 : slices[i - 1]) : 0;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int n_starts = 0, n_stops = 0;
    int prev_keep = 0, prev_end = -1;     // column c0 - 1 (wave-uniform)
    // four 64-column steps per round: the loads behind their keep tests are independent and in flight together (a wavefront per
    // row cluster is a latency-bound walk: 27-47 us per launch over ~2000 x 2000 clusters with one step per round)
    constexpr int U = 4;
    for (int c0 = 0; c0 < Cc; c0 += 64 * U) {
        int k[U + 1], cs[U + 1], ce[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + 64 * u + lane, cc = min(c, Cc - 1);      // unconditional loads, masked afterwards
            const int kk = keep_pair(rule, i, cc) ? 1 : 0, s0 = ranges_cols[2 * cc], e0 = ranges_cols[2 * cc + 1];
            k[u] = c < Cc ? kk : 0;
            cs[u] = c < Cc ? s0 : -2;
            ce[u] = c < Cc ? e0 : -3;
        }
        {   // lane 0 of the next round, for the right neighbour of the last lane
            const int c = c0 + 64 * U, cc = min(c, Cc - 1);
            const int kk = keep_pair(rule, i, cc) ? 1 : 0, s0 = ranges_cols[2 * cc];
            k[U] = c < Cc ? kk : 0;
            cs[U] = c < Cc ? s0 : -4;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + 64 * u >= Cc) break;      // wave-uniform
            int kl = __shfl_up(k[u], 1, 64), el = __shfl_up(ce[u], 1, 64);
            if (lane == 0) { kl = prev_keep; el = prev_end; }
            int kr = __shfl_down(k[u], 1, 64), sr = __shfl_down(cs[u], 1, 64);
            const int kn = __shfl(k[u + 1], 0, 64), sn = __shfl(cs[u + 1], 0, 64);     // first column of the next step
            if (lane == 63) { kr = kn; sr = sn; }
            const bool start = k[u] && !(kl && el == cs[u]);
            const bool stop = k[u] && !(kr && sr == ce[u]);
            const unsigned long long ms = __ballot(start), me = __ballot(stop);
            if (FILL) {
                if (start) {
                    const int slot = base + n_starts + __popcll(ms & below);
                    if (slot < capacity) red[2 * slot] = cs[u]; else *overflow = 1;
                }
                if (stop) {
                    const int slot = base + n_stops + __popcll(me & below);
                    if (slot < capacity) red[2 * slot + 1] = ce[u]; else *overflow = 1;
                }
            }
            n_starts += __popcll(ms);
            n_stops += __popcll(me);
            prev_keep = __shfl(k[u], 63, 64);
            prev_end = __shfl(ce[u], 63, 64);
        }
    }
    if (!FILL && lane == 0) counts[i] = n_starts;
}

// Pairs of POINTS a keep rule retains, without building its intervals: a wavefront per (row cluster, slab of 256 column clusters)
// adds (rows of the cluster) x (columns of the kept column clusters).  Round 5: a fixed number of workgroups walks the items and
// adds its total with ONE atomic — with one workgroup per 4 row clusters the ~500 same-address atomics of a launch (each a trip to
// memory: the 8 L2s do not share lines) cost 40 us of a 45 us launch, a 2-D grid with 3000 of them 57 us.
constexpr int kKeptBlocks = 512, kKeptWaves = 16;      // ~15 ns per atomic against ~1 us per item of a wavefront's walk: 2000 x 2000 clusters -> 2 items each

__global__ void kept_zero_kernel(unsigned long long* kept) {
    if (threadIdx.x < 3) kept[threadIdx.x] = 0;
}

// Small fills and copies as kernels of this library: the FIRST hipMemsetAsync / hipMemcpyAsync of a process loads the runtime's own
// blit kernels — 110 ms inside the first glhip_block_ranges call of a two-scale loss (round 6, tools/first_call.py)
__global__ void fill_i32_kernel(int32_t* dst, int n, int32_t v) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = v;
}
__global__ void gather2_i32_kernel(int32_t* dst, const int32_t* a, const int32_t* b) {
    if (threadIdx.x == 0) { dst[0] = *a; dst[1] = *b; }
}

__global__ void __launch_bounds__(64 * kKeptWaves) kept_pairs_kernel(KeepRule rule, int Cr, int Cc, const int32_t* __restrict__ ranges_rows,
                                                                    const int32_t* __restrict__ ranges_cols, unsigned long long* __restrict__ kept) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_slabs = (Cc + 255) / 256;
    const long n_items = (long)Cr * n_slabs;
    unsigned long long acc = 0;
    for (long item = (long)blockIdx.x * kKeptWaves + wave; item < n_items; item += (long)gridDim.x * kKeptWaves) {
        const int i = (int)(item / n_slabs), c0 = (int)(item - (long)i * n_slabs) * 256;
        long long cols = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + 64 * u + lane, cc = min(c, Cc - 1);      // unconditional loads, masked afterwards
            const int len = ranges_cols[2 * cc + 1] - ranges_cols[2 * cc];
            cols += (keep_pair(rule, i, cc) && c < Cc) ? len : 0;
        }
        acc += (unsigned long long)cols * (unsigned long long)(ranges_rows[2 * i + 1] - ranges_rows[2 * i]);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    __shared__ unsigned long long part[kKeptWaves];
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kKeptWaves; ++w) t += part[w];
        if (t) atomicAdd(kept, t);
    }
    if (blockIdx.x == 0 && wave < 2) {      // the sums of squared cluster sizes, rows (wavefront 0) and columns (wavefront 1), once
        const int32_t* rg = wave == 0 ? ranges_rows : ranges_cols;
        const int C = wave == 0 ? Cr : Cc;
        unsigned long long sq = 0;
        for (int c = lane; c < C; c += 64) {
            const unsigned long long m = (unsigned long long)(rg[2 * c + 1] - rg[2 * c]);
            sq += m * m;
        }
        for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
        if (lane == 0) kept[1 + wave] = sq;
    }
}

// inclusive scan of `counts` (n <= a few 1e5) by a single workgroup -> CSR end offsets
__global__ void __launch_bounds__(1024) slices_kernel(const int32_t* __restrict__ counts, int n, int32_t* __restrict__ slices) {
    __shared__ int scan[1024];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int k = base + tid;
        scan[tid] = k < n ? counts[k] : 0;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int v = (tid >= off) ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        if (k < n) slices[k] = carry + scan[tid];
        __syncthreads();
        if (tid == 1023) carry += scan[1023];
        __syncthreads();
    }
}

}  // namespace

extern "C" {

size_t glhip_cluster_workspace_bytes(int N, int D) {
    if (N <= 0 || D < 1 || D > 3) return 0;
    const size_t ts = sort_temp_bytes(N), tc = scan_temp_bytes(N);
    return align256(sizeof(ClusterHead)) + 2 * align256((size_t)N * 8) + 2 * align256((size_t)N * 4) + align256(ts > tc ? ts : tc);
}

int glhip_grid_cluster(const void* x, const float* weights, int N, int D, int in_dtype, float pre_div, float voxel, int32_t* perm,
                       void* x_sorted, float* w_sorted, int32_t* ranges, float* centroids, float* weights_c, int32_t* n_clusters,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 0 || D < 1 || D > 3) return fail(N < 0 ? GLHIP_EINVAL : GLHIP_EUNSUPPORTED, "glhip_grid_cluster: bad sizes N=%d D=%d (D <= 3)", N, D);
    if (in_dtype != GLHIP_F32 && in_dtype != GLHIP_BF16) return fail(GLHIP_EINVAL, "glhip_grid_cluster: bad in_dtype %d", in_dtype);
    if (!(voxel > 0.f) || !(pre_div > 0.f)) return fail(GLHIP_EINVAL, "glhip_grid_cluster: voxel and pre_div must be > 0");
    if (!n_clusters) return fail(GLHIP_EINVAL, "glhip_grid_cluster: NULL n_clusters");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (N == 0) {
        hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(64), 0, st, n_clusters, 8, 0);
        return GLHIP_OK;
    }
    if (!x || !perm || !ranges || !centroids || !weights_c || !workspace)
        return fail(GLHIP_EINVAL, "glhip_grid_cluster: NULL pointer");
    return in_dtype == GLHIP_F32
               ? grid_cluster_typed<float>(x, weights, N, D, pre_div, voxel, perm, x_sorted, w_sorted, ranges, centroids, weights_c, n_clusters, workspace, workspace_bytes, st)
               : grid_cluster_typed<bf16_t>(x, weights, N, D, pre_div, voxel, perm, x_sorted, w_sorted, ranges, centroids, weights_c, n_clusters, workspace, workspace_bytes, st);
}

namespace {
int check_block_ranges(const char* fn, int kind, const float* rows, const float* cols, const float* f, const float* g, int Cr, int Cc, int D,
                       int p, const int32_t* ranges_rows, const int32_t* ranges_cols, const int32_t* slices_rows, const int32_t* slices_cols) {
    if (kind != GLHIP_KEEP_DUAL_SLACK && kind != GLHIP_KEEP_WITHIN) return fail(GLHIP_EINVAL, "%s: bad kind %d", fn, kind);
    if (Cr < 0 || Cc < 0 || D < 1) return fail(GLHIP_EINVAL, "%s: bad sizes", fn);
    if (kind == GLHIP_KEEP_DUAL_SLACK && p != 1 && p != 2) return fail(GLHIP_EUNSUPPORTED, "%s: p must be 1 or 2", fn);
    if (Cr == 0 || Cc == 0) return GLHIP_OK;
    if (!rows || !cols || !ranges_rows || !ranges_cols || !slices_rows || !slices_cols || (kind == GLHIP_KEEP_DUAL_SLACK && (!f || !g)))
        return fail(GLHIP_EINVAL, "%s: NULL pointer", fn);
    return GLHIP_OK;
}
}  // namespace

int glhip_block_ranges_count(int kind, const float* rows, const float* cols, const float* f, const float* g, int Cr, int Cc, int D, int p,
                             float thr, const int32_t* ranges_rows, const int32_t* ranges_cols, int32_t* slices_rows,
                             int32_t* slices_cols, int32_t* totals, void* stream) {
    const int rc = check_block_ranges("glhip_block_ranges_count", kind, rows, cols, f, g, Cr, Cc, D, p, ranges_rows, ranges_cols, slices_rows, slices_cols);
    if (rc) return rc;
    if (!totals) return fail(GLHIP_EINVAL, "glhip_block_ranges_count: NULL totals");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (Cr == 0 || Cc == 0) {
        hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(64), 0, st, totals, 2, 0);
        return GLHIP_OK;
    }
    const KeepRule fwd{kind, rows, cols, f, g, D, p, thr}, bwd{kind, cols, rows, g, f, D, p, thr};
    hipLaunchKernelGGL((runs_kernel<false>), dim3((Cr + 3) / 4), dim3(256), 0, st, fwd, Cr, Cc, ranges_cols, slices_rows, nullptr, nullptr, 0LL, nullptr);
    hipLaunchKernelGGL(slices_kernel, dim3(1), dim3(1024), 0, st, slices_rows, Cr, slices_rows);
    hipLaunchKernelGGL((runs_kernel<false>), dim3((Cc + 3) / 4), dim3(256), 0, st, bwd, Cc, Cr, ranges_rows, slices_cols, nullptr, nullptr, 0LL, nullptr);
    hipLaunchKernelGGL(slices_kernel, dim3(1), dim3(1024), 0, st, slices_cols, Cc, slices_cols);
    hipLaunchKernelGGL(gather2_i32_kernel, dim3(1), dim3(64), 0, st, totals, slices_rows + (Cr - 1), slices_cols + (Cc - 1));
    return check_launch("glhip_block_ranges_count");
}

int glhip_block_ranges(int kind, const float* rows, const float* cols, const float* f, const float* g, int Cr, int Cc, int D, int p,
                       float thr, const int32_t* ranges_rows, const int32_t* ranges_cols, int32_t* slices_rows, int32_t* red_cols,
                       int32_t* slices_cols, int32_t* red_rows, long long capacity, int32_t* status, void* stream) {
    // slices_cols == red_rows == NULL: the row-major pattern only (a caller whose pattern is symmetric — the debiasing terms of a
    // Sinkhorn divergence: rows = cols, f = g — uses it for both orientations: two launches of the rule and one scan less)
    const bool both = slices_cols != nullptr || red_rows != nullptr;
    const int rc = check_block_ranges("glhip_block_ranges", kind, rows, cols, f, g, Cr, Cc, D, p, ranges_rows, ranges_cols, slices_rows,
                                      both ? slices_cols : slices_rows);
    if (rc) return rc;
    if (capacity < 0) return fail(GLHIP_EINVAL, "glhip_block_ranges: capacity < 0");
    if (Cr == 0 || Cc == 0) return GLHIP_OK;
    if (!red_cols || (both && !red_rows) || !status) return fail(GLHIP_EINVAL, "glhip_block_ranges: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(64), 0, st, status, 1, 0);
    const KeepRule fwd{kind, rows, cols, f, g, D, p, thr}, bwd{kind, cols, rows, g, f, D, p, thr};
    // the CSR offsets double as the count buffers of the first pass
    hipLaunchKernelGGL((runs_kernel<false>), dim3((Cr + 3) / 4), dim3(256), 0, st, fwd, Cr, Cc, ranges_cols, slices_rows, nullptr, nullptr, 0LL, status);
    hipLaunchKernelGGL(slices_kernel, dim3(1), dim3(1024), 0, st, slices_rows, Cr, slices_rows);
    hipLaunchKernelGGL((runs_kernel<true>), dim3((Cr + 3) / 4), dim3(256), 0, st, fwd, Cr, Cc, ranges_cols, nullptr, slices_rows, red_cols, capacity, status);
    if (both) {
        hipLaunchKernelGGL((runs_kernel<false>), dim3((Cc + 3) / 4), dim3(256), 0, st, bwd, Cc, Cr, ranges_rows, slices_cols, nullptr, nullptr, 0LL, status);
        hipLaunchKernelGGL(slices_kernel, dim3(1), dim3(1024), 0, st, slices_cols, Cc, slices_cols);
        hipLaunchKernelGGL((runs_kernel<true>), dim3((Cc + 3) / 4), dim3(256), 0, st, bwd, Cc, Cr, ranges_rows, nullptr, slices_cols, red_rows, capacity, status);
    }
    return check_launch("glhip_block_ranges");
}

int glhip_block_ranges_kept_pairs(int kind, const float* rows, const float* cols, const float* f, const float* g, int Cr, int Cc, int D,
                                  int p, float thr, const int32_t* ranges_rows, const int32_t* ranges_cols, long long* kept, void* stream) {
    if (kind != GLHIP_KEEP_DUAL_SLACK && kind != GLHIP_KEEP_WITHIN) return fail(GLHIP_EINVAL, "glhip_block_ranges_kept_pairs: bad kind %d", kind);
    if (Cr < 0 || Cc < 0 || D < 1) return fail(GLHIP_EINVAL, "glhip_block_ranges_kept_pairs: bad sizes");
    if (kind == GLHIP_KEEP_DUAL_SLACK && p != 1 && p != 2) return fail(GLHIP_EUNSUPPORTED, "glhip_block_ranges_kept_pairs: p must be 1 or 2");
    if (!kept) return fail(GLHIP_EINVAL, "glhip_block_ranges_kept_pairs: NULL kept");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kept_zero_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long*>(kept));      // (a 24-byte hipMemsetAsync is two fill kernels)
    if (Cr == 0 || Cc == 0) return GLHIP_OK;
    if (!rows || !cols || !ranges_rows || !ranges_cols || (kind == GLHIP_KEEP_DUAL_SLACK && (!f || !g)))
        return fail(GLHIP_EINVAL, "glhip_block_ranges_kept_pairs: NULL pointer");
    const KeepRule rule{kind, rows, cols, f, g, D, p, thr};
    const long items = (long)Cr * ((Cc + 255) / 256);
    const long want = (items + kKeptWaves - 1) / kKeptWaves;
    hipLaunchKernelGGL(kept_pairs_kernel, dim3(want < kKeptBlocks ? (unsigned)want : kKeptBlocks), dim3(64 * kKeptWaves), 0, st, rule, Cr, Cc, ranges_rows, ranges_cols,
                       reinterpret_cast<unsigned long long*>(kept));
    return check_launch("glhip_block_ranges_kept_pairs");
}

}  // extern "C"
