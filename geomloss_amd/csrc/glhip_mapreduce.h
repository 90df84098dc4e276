// glhip_mapreduce.h — the tiling skeleton shared by the low-dimensional (D <= 3) reductions
//   out_i = REDUCE_j F(x_i, y_j, s_j).
//
// Work decomposition (CDNA4):
//   * one workgroup = 256 threads = 4 wavefronts; each thread owns R rows i, held in VGPRs;
//     rows are assigned lane-contiguously (row = base + r*256 + tid) so x loads / out stores coalesce.
//   * the column cloud is streamed through LDS in tiles of kTile records of 16 B
//     ({y_0, y_1, y_2, s_j}); every lane of a wavefront reads the same record at the same time,
//     i.e. one conflict-free broadcast ds_read_b128 per column and per R rows.
//   * grid = (row blocks) x (batch) x (column splits).  A workgroup that owns all the columns of its
//     rows writes the final result; otherwise it writes a per-row partial state to the caller's
//     workspace and `merge_kernel` combines the splits.  Column splits exist for load balance: one
//     workgroup working through 1e6 columns runs for ~the whole kernel, so without them the last
//     partially filled round of workgroups leaves most CUs idle (measured: 4.2 of 7 resident waves/SIMD).
//   * dense mode: grid.x tiles the rows.  Block-sparse mode: grid.x = row block k of the KeOps-style
//     ranges; split s of a row block takes the column intervals q = s (mod n_splits) of its CSR slice.
//   * coordinates are re-centred on the first row of the workgroup's row pass before any product is
//     formed, so the expanded form  -|x-y|^2/2 = x.y - |x|^2/2 - |y|^2/2  is evaluated on offsets that
//     are at most one cloud diameter long (and much shorter when the rows are cluster-sorted).
//
// An `Op` supplies: Params, RowState, kRows (R), kDim (D), kPartial and the device functions
//   load_centre / init_rows / make_record / neutral_record / consume / finish_rows /
//   store_partial / merge_row.
#pragma once

#include <type_traits>

#include "glhip_common.h"
#include "glhip_split_policy.h"

namespace glhip {

struct SplitInfo {
    int n_splits;       // 1 = no split
    float* workspace;   // [n_splits][B*N][kPartial] floats
    long split_stride;  // floats between consecutive splits = B*N*kPartial
    int xcd_grid_x;     // > 0: 1-D XCD-aware grid (see workgroup_coords); value = number of row blocks per batch item
    int xcd_blocks;     // XCD-aware grid: row blocks x batch items (workgroups per column split)
    int gather = 0;     // block-sparse forward kernel: tiles gather several short column intervals (glhip_softmin_x32.h: gather_tile)
    int share = 0;      // block-sparse forward kernel, 4 wavefronts: the chunk table was built in share mode (build_row_chunks_kernel)
};

// Logical (row block, batch item, column split) of this workgroup.  Plain mode: the 3-D grid.  XCD-aware mode
// (dense kernels with n_splits == 8): a 1-D grid whose linear id is split-major modulo 8.  The dispatcher places
// workgroup b on XCD b % 8 (observed behaviour, used for speed only), so XCD k only ever streams the k-th eighth
// of the column cloud: at M = 1e6 that is 2 MB of points + dual values, resident in the XCD's 4 MB L2 instead of
// being re-fetched through the fabric by every row block.
__device__ __forceinline__ void workgroup_coords(const SplitInfo& sp, int& bx, int& by, int& bz) {
    if (sp.xcd_grid_x > 0) {
        // linear id = ((phase * blocks + block) * 8 + xcd): XCD k runs split k of every row block first, then split
        // k + 8, ... — at any time its L2 holds one split's columns, however many splits there are
        const int lid = blockIdx.x;
        const int xcd = lid & 7;
        const int t = lid >> 3;
        const int phase = t / sp.xcd_blocks;
        const int block = t - phase * sp.xcd_blocks;
        bz = phase * 8 + xcd;
        bx = block % sp.xcd_grid_x;
        by = block / sp.xcd_grid_x;
    } else {
        bx = blockIdx.x;
        by = blockIdx.y;
        bz = blockIdx.z;
    }
}

// rows [row_begin,row_end) and CSR slice [q_begin,q_end) of workgroup blockIdx.x
template <bool SPARSE>
__device__ __forceinline__ void block_extent(const Ranges& rg, int N, int rows_per_pass, int& row_begin,
                                             int& row_end, int& q_begin, int& q_end, int bx = blockIdx.x) {
    if (SPARSE) {
        int k = bx;
        const int T = rg.chunks ? rg.chunks[0] : 0;
        if (rg.chunks && T >= 0) {   // row blocks cut into chunks of at most `rows_per_pass` rows: workgroup bx owns chunk bx
            if (bx >= T) { row_begin = row_end = q_begin = q_end = 0; return; }
            k = rg.chunks[1 + 3 * bx];
            row_begin = rg.chunks[2 + 3 * bx];
            row_end = rg.chunks[3 + 3 * bx];
        } else if (rg.chunks) {      // the table overflowed (T = -n_ranges): one workgroup per row block, the KeOps granularity
            if (bx >= -T) { row_begin = row_end = q_begin = q_end = 0; return; }
            row_begin = rg.ranges_i[2 * k];
            row_end = rg.ranges_i[2 * k + 1];
        } else {
            row_begin = rg.ranges_i[2 * k];
            row_end = rg.ranges_i[2 * k + 1];
        }
        q_begin = (k == 0) ? 0 : rg.slices_i[k - 1];
        q_end = rg.slices_i[k];
    } else {
        row_begin = bx * rows_per_pass;
        row_end = min(N, row_begin + rows_per_pass);
        q_begin = 0;
        q_end = 1;
    }
}

// column interval q as seen by split `s` of `ns`
template <bool SPARSE>
__device__ __forceinline__ void column_interval(const Ranges& rg, int M, int q, int s, int ns, int& js, int& je) {
    if (SPARSE) {
        js = rg.redranges_j[2 * q];
        je = rg.redranges_j[2 * q + 1];
    } else {
        const int len = (((M + ns - 1) / ns) + kChunk - 1) & ~(kChunk - 1);
        js = min(M, s * len);
        je = min(M, js + len);
    }
}

// Row-chunk table of a block-sparse launch.  The KeOps convention gives one workgroup per row block (cluster); voxel clusters
// of real clouds are very uneven (a sphere sampled at 1e6 points: 1 ... 19 566 rows per cluster), so the workgroup of the
// biggest cluster runs long after the chip has drained.  This single-workgroup kernel cuts every row block into chunks of
// `rows` rows (the row tile of the kernel that follows) with a block-wide prefix sum over the clusters, so that the grid of
// the reduction is one workgroup per chunk: chunks[0] = T, chunks[1 + 3c ...] = (row block, first row, end row).  The host
// only knows the bound T <= n_ranges + N / rows (valid for disjoint row blocks) and launches that many workgroups; the surplus
// exits at once.  chunks[0] < 0 = "table too small, ignore it" (see the end of the kernel).
static __global__ void __launch_bounds__(1024)
build_row_chunks_kernel(const int32_t* __restrict__ ranges_i, int n_ranges, int rows, int32_t* __restrict__ chunks, int capacity,
                        int share = 0) {
    __shared__ int scan[1024];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_ranges; base += 1024) {
        const int k = base + tid;
        int r0 = 0, r1 = 0;
        if (k < n_ranges) { r0 = ranges_i[2 * k]; r1 = ranges_i[2 * k + 1]; }
        int cnt = (r1 > r0) ? (r1 - r0 + rows - 1) / rows : 0;
        // share (rows = 128 = 4 row tiles of 32; glhip_softmin_x32.h): a row block of nt > 4 row tiles gets W = nt / 4 chunks of exactly
        // 4 tiles; of the rl = nt mod 4 tiles left over, min(rl, W) are reduced on the side by the workgroups of the first chunks
        // (one each) and belong to no chunk; the others (W < rl: blocks of 5 - 7, 11 row tiles) form a trailing partial chunk
        int full = cnt, skip = 0;      // chunks of `rows` rows; share: rows of the carried tiles, between the last full chunk and the trailing one
        if (share && cnt > 1) {
            const int nt = (r1 - r0 + 31) >> 5, W = nt >> 2, rl = nt - 4 * W, e = rl < W ? rl : W;
            full = W;
            skip = 32 * e;
            cnt = W + (rl > e ? 1 : 0);
        }
        scan[tid] = cnt;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {   // inclusive Hillis-Steele scan
            const int v = (tid >= off) ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int first = carry + scan[tid] - cnt;
        for (int c = 0; c < cnt; ++c) {
            const int slot = first + c;
            if (slot < capacity) {
                chunks[1 + 3 * slot] = k;
                chunks[2 + 3 * slot] = r0 + c * rows + (c < full ? 0 : skip);
                chunks[3 + 3 * slot] = c < full ? min(r1, r0 + (c + 1) * rows) : r1;
            }
        }
        __syncthreads();
        if (tid == 1023) carry += scan[1023];
        __syncthreads();
    }
    // The host sizes the table for DISJOINT row blocks inside [0, N) (n_ranges + N / rows chunks always suffice then).  Overlapping
    // or out-of-range blocks can need more: instead of dropping the surplus chunks, tell the reduction to ignore the table and run
    // one workgroup per row block (the grid, >= n_ranges workgroups, covers that too).
    if (tid == 0) chunks[0] = (carry <= capacity) ? carry : -n_ranges;
}

template <class Op, bool SPARSE>
__global__ void __launch_bounds__(kBlock)
mapreduce_kernel(typename Op::Params prm, Ranges rg, int N, int M, SplitInfo sp) {
    constexpr int D = Op::kDim;
    constexpr int R = Op::kRows;
    constexpr int kRowsPerPass = kBlock * R;
    __shared__ Rec<D> tile[kTile];

    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int split = blockIdx.z;
    const int ns = sp.n_splits;

    int row_begin, row_end, q_begin, q_end;
    block_extent<SPARSE>(rg, N, kRowsPerPass, row_begin, row_end, q_begin, q_end);

    for (int row0 = row_begin; row0 < row_end; row0 += kRowsPerPass) {
        float centre[D];
        Op::load_centre(prm, b, N, row0, centre);   // wave-uniform (scalar loads)

        typename Op::RowState st;
        Op::init_rows(prm, b, N, row0, row_end, tid, centre, st);

        for (int q = q_begin + (SPARSE ? split : 0); q < q_end; q += (SPARSE ? ns : 1)) {
            int js, je;
            column_interval<SPARSE>(rg, M, q, split, ns, js, je);
            for (int j0 = js; j0 < je; j0 += kTile) {
                const int n = min(kTile, je - j0);
                const int npad = (n + kChunk - 1) & ~(kChunk - 1);
                __syncthreads();   // previous tile fully consumed
                for (int t = tid; t < npad; t += kBlock) {
                    tile[t] = (t < n) ? Op::make_record(prm, b, M, j0 + t, centre) : Op::neutral_record();
                }
                __syncthreads();
                for (int jj = 0; jj < npad; jj += kChunk) Op::consume(st, &tile[jj]);
            }
        }
        if (ns == 1) {
            Op::finish_rows(prm, b, N, row0, row_end, tid, centre, st);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = row0 + r * kBlock + tid;
                if (i < row_end)
                    Op::store_partial(st, r, sp.workspace + split * sp.split_stride +
                                                 ((long)b * N + i) * Op::kPartial);
            }
        }
    }
}

// Combines the column splits of every row: one thread per row.
template <class Op, bool SPARSE>
__global__ void __launch_bounds__(kBlock)
merge_kernel(typename Op::Params prm, Ranges rg, int N, SplitInfo sp) {
    constexpr int D = Op::kDim;
    constexpr int kRowsPerPass = kBlock * Op::kRows;
    const int b = blockIdx.y;
    int row_begin, row_end, q_begin, q_end;
    block_extent<SPARSE>(rg, N, kRowsPerPass, row_begin, row_end, q_begin, q_end);
    for (int row0 = row_begin; row0 < row_end; row0 += kRowsPerPass) {
        float centre[D];
        Op::load_centre(prm, b, N, row0, centre);
        for (int i = row0 + threadIdx.x; i < min(row_end, row0 + kRowsPerPass); i += kBlock) {
            Op::merge_row(prm, b, N, i, centre, sp.workspace + ((long)b * N + i) * Op::kPartial, sp.n_splits,
                          sp.split_stride);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------

// (the split rules and the arithmetic of a split workspace: glhip_split_policy.h)

// Space reserved at the front of the caller's workspace for the row-chunk table of a block-sparse launch.
struct ChunkBuf {
    int32_t* buf = nullptr;
    long capacity = 0;      // chunks the table can hold
};

// Queues build_row_chunks_kernel for a reduction whose workgroups take `rows` rows and returns the ranges to hand to it
// together with its grid.x; without a reserved table (no workspace) the launch keeps one workgroup per row block.
static inline Ranges with_row_chunks(const Ranges& rg, int n_ranges, int N, int rows, const ChunkBuf& cb, hipStream_t stream,
                                     unsigned& grid_x, int share = 0) {
    grid_x = (unsigned)n_ranges;
    const long bound = (long)n_ranges + N / rows;
    if (!cb.buf || cb.capacity < bound || n_ranges <= 0) return rg;
    hipLaunchKernelGGL(build_row_chunks_kernel, dim3(1), dim3(1024), 0, stream, rg.ranges_i, n_ranges, rows, cb.buf, (int)bound, share);
    Ranges out = rg;
    out.chunks = cb.buf;
    grid_x = (unsigned)bound;
    return out;
}

// The column-split mechanics of a row-tiled reduction launch (this file's kernel and the matrix-core kernels of glhip_launch.h): the HIP
// half of glhip_split_policy.h's SplitGeom — row-chunk table, SplitInfo, grid, main launch, merge launch.  No policy lives here or in a
// launcher: between construction and launch() the launcher builds a SplitPlan from this geometry (one plan function per policy,
// glhip_split_policy.h) and hands it to apply().  launch() hands the main kernel's launch to a callable
// main(std::integral_constant<bool, SPARSE>, grid, ranges), then queues merge_kernel<MergeOp, SPARSE> when the columns are split.
struct SplitLaunch : SplitGeom {
    Ranges rg;                  // the caller's ranges: what the merge kernel reads
    Ranges rgc;                 // what the main kernel reads: block-sparse launches with a row-chunk table get it here
    unsigned chunk_grid = 0;    // block-sparse launches: grid.x (one workgroup per row chunk, or per row block without a table)
    SplitInfo sp;

    // `rows`: rows per workgroup of the main kernel; `partial`: floats per row and split (MergeOp::kPartial)
    SplitLaunch(const Ranges& ranges, int n_ranges_, int B_, int N_, int M_, int rows, int partial, void* workspace, size_t bytes_,
                const ChunkBuf& cb, hipStream_t stream, int share = 0)
        : SplitGeom(n_ranges_, B_, N_, M_, rows, partial, workspace != nullptr, bytes_), rg(ranges),
          sp{1, static_cast<float*>(workspace), (long)B_ * N_ * partial, 0, 0} {
        rgc = n_ranges > 0 ? with_row_chunks(rg, n_ranges, N, rows, cb, stream, chunk_grid, share) : rg;
    }

    // takes the plan: its splits, its bits, the XCD-aware 1-D grid (workgroup_coords) where it says so
    void apply(const SplitPlan& p) {
        sp.n_splits = p.n_splits;
        sp.gather = p.gather;
        sp.share = p.share;
        if (p.xcd) { sp.xcd_grid_x = gx; sp.xcd_blocks = gx * B; }
    }
    // where the plan's pre-packed columns go
    template <class R> R* packed(const SplitPlan& p, size_t behind = 0) const {
        return reinterpret_cast<R*>(reinterpret_cast<char*>(sp.workspace) + p.packed_offset + behind);
    }

    template <class MergeOp, class F>
    void launch(F&& main, const typename MergeOp::Params& mprm, hipStream_t stream) const {
        if (n_ranges > 0) launch_sparse<MergeOp>(main, mprm, stream);
        else launch_dense<MergeOp>(main, mprm, stream);
    }
    // (launchers whose kernels exist in one mode only call these directly: the other mode is not instantiated)
    template <class MergeOp, class F>
    void launch_sparse(F&& main, const typename MergeOp::Params& mprm, hipStream_t stream) const {
        main(std::true_type{}, dim3(chunk_grid, 1, sp.n_splits), rgc);
        if (sp.n_splits > 1) hipLaunchKernelGGL((merge_kernel<MergeOp, true>), dim3(n_ranges, 1, 1), dim3(kBlock), 0, stream, mprm, rg, N, sp);
    }
    template <class MergeOp, class F>
    void launch_dense(F&& main, const typename MergeOp::Params& mprm, hipStream_t stream) const {
        constexpr int kMergeRows = kBlock * MergeOp::kRows;
        main(std::false_type{}, sp.xcd_grid_x > 0 ? dim3((unsigned)((long)gx * B * sp.n_splits), 1, 1) : dim3(gx, B, sp.n_splits), rg);
        if (sp.n_splits > 1)
            hipLaunchKernelGGL((merge_kernel<MergeOp, false>), dim3((N + kMergeRows - 1) / kMergeRows, B, 1), dim3(kBlock), 0, stream, mprm, rg, N, sp);
    }
};

template <class Op>
static inline void launch_mapreduce(const typename Op::Params& prm, const Ranges& rg, int n_ranges, int B, int N,
                                    int M, void* workspace, size_t workspace_bytes, bool allow_split,
                                    hipStream_t stream, const ChunkBuf& cb = ChunkBuf()) {
    SplitLaunch sl(rg, n_ranges, B, N, M, kBlock * Op::kRows, Op::kPartial, workspace, workspace_bytes, cb, stream);
    sl.apply(plan_rule(sl, allow_split));
    sl.launch<Op>([&](auto sparse, dim3 grid, const Ranges& r) {
        hipLaunchKernelGGL((mapreduce_kernel<Op, decltype(sparse)::value>), grid, dim3(kBlock), 0, stream, prm, r, N, M, sl.sp);
    }, prm, stream);
}

}  // namespace glhip
