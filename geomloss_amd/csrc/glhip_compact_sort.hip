// glhip_compact_sort.hip — the compact order of a cloud, for the launches that sort their clouds behind the ABI (the autosorted p = 1 /
// laplacian / energy calls and the sorted p = 2 call):
//   compact_sort              bounding box -> voxel edge -> boustrophedon path keys -> rocPRIM radix sort (-> balanced cells) -> gather
//   gather_f32 / scatter_f32  vectors into and out of that order
//   slab_ranges               "every slab of rows x all columns" as ranges
// Declared in glhip_autosort.h, which also holds the reasoning (why the launches sort, the order, balanced cells, reused permutations);
// the rules of the balancing pass: glhip_balance.h; the clamp of a hinted permutation: glhip_perm_index.h.
#include <cmath>
#include <cstdint>

#include "glhip_autosort.h"
#include "glhip_balance.h"
#include "glhip_cloud_prep.h"
#include "glhip_common.h"
#include "glhip_error.h"
#include "glhip_perm_index.h"

using namespace glhip;

namespace {

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
    workgroup_box<float>(
        n, D, [&](long i, int d) { return to_f32<T>(x[i * D + d]); },
        [&](int d, float l, float h) {
            atomicMin(&head->lo[d], ordered_of(l));
            atomicMax(&head->hi[d], ordered_of(h));
        });
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
    size_t temp = radix_sort_temp_bytes(n, 64u);
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

template <bool kHinted>
void gather_f32_typed(const float* src, const int32_t* perm, float* dst, int n, hipStream_t st) {
    hipLaunchKernelGGL(gather_f32_kernel<kHinted>, dim3((n + 255) / 256), dim3(256), 0, st, src, perm, dst, n);
}

template <bool kHinted>
void scatter_f32_typed(const float* src, const int32_t* perm, float* dst, int n, hipStream_t st, int width) {
    hipLaunchKernelGGL(scatter_f32_kernel<kHinted>, dim3((n + 255) / 256), dim3(256), 0, st, src, perm, dst, n, width);
}

}  // namespace

namespace glhip {

size_t compact_sort_scratch_bytes(int n) {
    return align256(sizeof(SortHead)) + 2 * align256((size_t)n * 8) + align256((size_t)n * 4) + align256(radix_sort_temp_bytes(n, 64u));
}

int compact_sort(const void* z, int n, int D, int in_dtype, int rows_per_voxel, int32_t* perm, void* z_sorted, void* scratch,
                 size_t scratch_bytes, hipStream_t st, int sub, bool hinted) {
    return in_dtype == GLHIP_F32 ? compact_sort_typed<float>(z, n, D, rows_per_voxel, sub, perm, z_sorted, scratch, scratch_bytes, st, hinted)
                                 : compact_sort_typed<bf16_t>(z, n, D, rows_per_voxel, sub, perm, z_sorted, scratch, scratch_bytes, st, hinted);
}

void gather_f32(const float* src, const int32_t* perm, float* dst, int n, hipStream_t st, bool hinted) {
    if (hinted) gather_f32_typed<true>(src, perm, dst, n, st);
    else gather_f32_typed<false>(src, perm, dst, n, st);
}

void scatter_f32(const float* src, const int32_t* perm, float* dst, int n, hipStream_t st, int width, bool hinted) {
    if (hinted) scatter_f32_typed<true>(src, perm, dst, n, st, width);
    else scatter_f32_typed<false>(src, perm, dst, n, st, width);
}

void slab_ranges(int N, int M, int32_t* ranges_i, int32_t* slices_i, int32_t* red, hipStream_t st) {
    const int C = (N + kSortSlab - 1) / kSortSlab;
    hipLaunchKernelGGL(slab_ranges_kernel, dim3((C + 255) / 256), dim3(256), 0, st, N, M, C, ranges_i, slices_i, red);
}

}  // namespace glhip
