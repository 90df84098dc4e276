// glhip_prune.hip — the exact pruning of the sorted p = 2 call: what is kept of every slab of sorted rows, on the device:
//   prune_ranges   column-block and group records -> per slab: Mlb, t1, home block, reference blocks, kept blocks as column intervals
//                  -> per tile: t2
// Declared in glhip_autosort.h, which also holds the reasoning (the bound and why it is exact, the second level, the mass rule and its
// budgets); the kept blocks of a slab as 64-bit words: glhip_prune_words.h; the second level's test itself: glhip_softmin_x32.h.
#include <climits>
#include <cmath>
#include <cstdint>

#include "glhip_autosort.h"
#include "glhip_common.h"
#include "glhip_list_cursor.h"
#include "glhip_prune_words.h"

using namespace glhip;

namespace {

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
// a record lowered by `times` its own slack, in float64: never above the true log sum exp for times = 2 (a group's record) and
// times = 4 (a block's: rounded up twice) — the sum reference of glhip_autosort.h.  -inf stays -inf.
__device__ __forceinline__ double lse_dn(float v, double times) {
    return (double)v - times * (double)kPruneLseSlack * ((double)__builtin_fabsf(v) + 8.0);
}
// the cell of a block's score on the grid its slab's reference list is ranked on (kPruneRefCells: not on it); the score of a block
// whose dual values are all -inf is -inf
__device__ __forceinline__ int prune_ref_cell(double score, double mlb) {
    const double q = (mlb + kPruneRefTop - score) * (double)kPruneRefCellsPerNat;
    if (!(q < (double)kPruneRefCells)) return kPruneRefCells;
    return q > 0.0 ? (int)q : 0;
}

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
// ceil(M / 256) blocks (first level, budget 0.132 x 2^-26 > 2^-26 e^-1 / 256) or ceil(M / 32) groups (second level, budget 2^-26 / 2 > 2^-26 e^-1 / 32)
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
                                                          double* __restrict__ mlb_out, double* __restrict__ t1_out, int32_t* __restrict__ refs_out) {
    __shared__ int buf[256];
    __shared__ double hist[kPruneBuckets + 1];      // (the last entry: the underflow bucket)
    __shared__ int first_kept;
    __shared__ int cells[kPruneRefCells];           // blocks per cell of the score grid: the reference list (the sum reference)
    __shared__ int ref_cells, ref_n, ref_l[kPruneRefBlocks];
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
    for (int q = tid; q < kPruneRefCells; q += 256) cells[q] = 0;
    if (tid == 0) ref_n = 0;
    __syncthreads();
    // The same pass sums e^(s(T) - Mlb) of the scores s(T) = lse_dn(T) - dmaxpen(R, T) for Slb(R), the lower bound of every row's SUM
    // that the budget refers to (terms below e^-40: left out), and counts the blocks per cell of the score grid
    double ssum = 0.0;
    if (!keep_all) {
        for (int t = tid; t < nT; t += 256) {
            const ColBlock b = blocks[t];
            if (__builtin_isnan(b.lse)) continue;
            double dmin2, dmax2;
            box_d2(rlo, rhi, b, D, dmin2, dmax2);
            const double score = lse_dn(b.lse, 4.0) - dmax2 * inv2eps;
            if (score - mlb > -40.0) ssum += exp(score - mlb);
            const int cell = prune_ref_cell(score, mlb);
            if (cell < kPruneRefCells) atomicAdd(&cells[cell], 1);
            const double key = (double)b.lse - dmin2 * inv2eps;
            const int q = prune_bucket(key, lo_key);
            if (q >= kPruneBuckets) continue;      // above the range: never added, so no exp for it
            const double mass = exp(key - mlb);
            if (mass > 0.0) atomicAdd(&hist[q < 0 ? kPruneBuckets : q], mass);
        }
    }
    for (int off = 32; off > 0; off >>= 1) ssum += __shfl_xor(ssum, off, 64);
    __syncthreads();      // (also: every read of wm above is done)
    if (lane == 0) wm[wave] = ssum;
    __syncthreads();
    if (tid == 0) {
        // the masses stay relative to Mlb and the budget is multiplied by e^(Slb - Mlb): the same comparison
        const double sum = (wm[0] + wm[1]) + (wm[2] + wm[3]);
        double slb = mlb;
        if (!keep_all && sum > 0.0 && __builtin_isfinite(sum)) slb = fmax(mlb, mlb + log(sum) - kPruneSumSlack);
        first_kept = keep_all ? 0 : prune_first_kept(hist, hist[kPruneBuckets], kPruneBudget1 * exp(slb - mlb));
        mlb_out[k] = mlb;
        t1_out[k] = keep_all ? -INFINITY : lo_key + first_kept * kPruneBucketNats;
        // whole cells from the top while at most kPruneRefBlocks - 1 blocks are in: one place stays for the home block
        int nc = 0;
        for (int n = 0; nc < kPruneRefCells && n + cells[nc] <= kPruneRefBlocks - 1; ++nc) n += cells[nc];
        ref_cells = nc;
    }
    __syncthreads();
    const int fk = first_kept, rc = ref_cells;
    // a block of the reference list: on the kept cells of the score grid, or the home block
    auto ref_take = [&](int t, const ColBlock& b, double dmax2) {
        if (t != best && prune_ref_cell(lse_dn(b.lse, 4.0) - dmax2 * inv2eps, mlb) >= rc) return;
        const int i = atomicAdd(&ref_n, 1);
        if (i < kPruneRefBlocks) ref_l[i] = t;
    };
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
                bool kp = t < nT;
                if (kp && !keep_all) {      // (kept(t), and the reference list from the same distances)
                    const ColBlock b = blocks[t];
                    if (!__builtin_isnan(b.lse)) {
                        double dmin2, dmax2;
                        box_d2(rlo, rhi, b, D, dmin2, dmax2);
                        kp = prune_bucket((double)b.lse - dmin2 * inv2eps, lo_key) >= fk;
                        ref_take(t, b, dmax2);
                    }
                }
                const unsigned long long m = __ballot(kp);
                if (lane == 0) mask[w] = m;
                all &= m == (nT - 64 * w >= 64 ? ~0ull : (1ull << (nT - 64 * w)) - 1ull);
            }
        } else if (!keep_all) {
            for (int t = tid; t < nT && all; t += 256) all = kept(t) ? 1 : 0;
            for (int t = tid; t < nT; t += 256) {
                const ColBlock b = blocks[t];
                if (__builtin_isnan(b.lse)) continue;
                double dmin2, dmax2;
                box_d2(rlo, rhi, b, D, dmin2, dmax2);
                ref_take(t, b, dmax2);
            }
        }
        all = __syncthreads_and(all);      // (also: the bit set and the reference list are written)
        if (tid == 0) home[k] = (keep_all || all) ? -1 : best;
        // the list in ascending block order, whatever order the atomics gave it; unused entries: -1
        if (tid < kPruneRefBlocks) {
            const int n = min(ref_n, kPruneRefBlocks);
            int rank = tid, v = -1;
            if (tid < n) {
                v = ref_l[tid];
                rank = 0;
                for (int j = 0; j < n; ++j) rank += ref_l[j] < v;
            }
            refs_out[(long)k * kPruneRefBlocks + rank] = v;
        }
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
// The sum reference (glhip_autosort.h): the budget is a share of e^ls(W), ls(W) = min_i max(seed_i, ls_i), where ls_i — thread = row
// again — is the log of the sum over the groups G of the slab's reference blocks (`refs`, staged in LDS with their lowered records) of
// e^(lse_dn(G) - dmaxpen(x_i, G)): a lower bound of the row's SUM where the seed is one term of it.
struct RefGroup {           // one group of a reference block: its box and lse_dn (-inf: no such group, or a special one)
    float lo[3], hi[3];
    double dn;
};
constexpr int kRefGroups = kPruneRefBlocks * (kPruneColBlock / 32);
static_assert(kPruneRuns + kPruneGrid <= 256 && kSortSlab == 256, "one thread per interval slot / per row");
template <typename T>
__global__ void __launch_bounds__(256) prune_tiles_kernel(const T* __restrict__ xs, const T* __restrict__ ys, const float* __restrict__ h,
                                                          const float* __restrict__ pot, float pot_scale, int N, int M, int D,
                                                          const GroupBox* __restrict__ groups, const int32_t* __restrict__ red, int S,
                                                          const int32_t* __restrict__ home, const int32_t* __restrict__ refs, double inv2eps,
                                                          double L, float* __restrict__ t2) {
    constexpr int kTiles = kSortSlab / 32;
    __shared__ RefGroup rg[kRefGroups];
    __shared__ double lsw[kTiles];
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
    // the groups of the reference blocks (the list is ascending, its unused entries at the end)
    const int n_ref = __syncthreads_count(tid < kPruneRefBlocks && refs[(long)k * kPruneRefBlocks + tid] >= 0);
    for (int q = tid; q < n_ref * (kPruneColBlock / 32); q += 256) {
        const int t = refs[(long)k * kPruneRefBlocks + q / (kPruneColBlock / 32)];
        const long g = (long)t * (kPruneColBlock / 32) + q % (kPruneColBlock / 32);
        RefGroup r;
        for (int d = 0; d < 3; ++d) r.lo[d] = r.hi[d] = 0.f;
        r.dn = -INFINITY;
        if (t >= 0 && t < (M + kPruneColBlock - 1) / kPruneColBlock && g < (M + 31) / 32) {
            const GroupBox b = groups[g];
            if (!b.special && !__builtin_isnan(b.lse)) {
                for (int d = 0; d < 3; ++d) {
                    r.lo[d] = b.lohi[d][0];
                    r.hi[d] = b.lohi[d][1];
                }
                r.dn = lse_dn(b.lse, 2.0);
            }
        }
        rg[q] = r;
    }
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
        // ls_i: float32 exponentials on arguments relative to the row's own seed, the result lowered by kPruneLsSlack.  A term more
        // than 60 nats above the reference (dual values hundreds of nats apart at a small eps: another block can hold far more than
        // the home block does) becomes the reference, so no exponential overflows; what was summed so far is scaled down with it.
        double ls = INFINITY;
        if (row && __builtin_isfinite(seed)) {
            double mref = seed;
            float acc = 0.f;
            for (int q = 0; q < n_ref * (kPruneColBlock / 32); ++q) {
                const RefGroup& r = rg[q];
                double d2 = 0.0;
                for (int d = 0; d < 3; ++d) {
                    const double far = fmax(fabs(xd[d] - (double)r.lo[d]), fabs((double)r.hi[d] - xd[d]));
                    d2 = fma(far, far, d2);
                }
                double arg = r.dn - d2 * inv2eps - mref;      // (dn = -inf: e^-inf = 0)
                if (arg > 60.0) {
                    acc *= __expf((float)-arg);
                    mref += arg;
                    arg = 0.0;
                }
                acc += __expf((float)arg);      // (the hardware exponential: its error is part of kPruneLsSlack)
            }
            // the seed is one term of the same sum: the better of the two bounds (acc = 0, every reference term under e^-87 of
            // the seed in float32: the seed)
            ls = fmax(seed, mref + (double)logf(acc) - kPruneLsSlack);
        }
        for (int off = 16; off > 0; off >>= 1) {
            v = fmin(v, __shfl_xor(v, off, 64));
            ls = fmin(ls, __shfl_xor(ls, off, 64));      // (a NaN — none should be — is dropped here or fails the test below)
            ok &= __shfl_xor(ok, off, 64);
        }
        if ((tid & 31) == 0) {
            ms[w] = (ok && r0 + 32 * w < r1) ? v : NAN;      // NaN: no rows, or no finite seed
            lsw[w] = (__builtin_isfinite(ls) && ls > v) ? ls : v;
        }
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
            // the masses stay relative to ms and the budget is multiplied by e^(ls - ms): the same comparison
            const int fk = prune_first_kept(hist[tid], hist[tid][kPruneBuckets], kPruneBudget2 * exp(lsw[tid] - m));
            const double v = (m - L + fk * kPruneBucketNats) * 1.4426950408889634;
            out = (float)v;
            if ((double)out > v) out = nextafterf(out, -INFINITY);
        }
        t2[(r0 >> 5) + tid] = out;
    }
}

template <typename T>
void prune_ranges_typed(const void* xs_, const void* ys_, const float* h, const float* pot, float pot_scale, int N, int M, int D, float eps,
                        int32_t* ranges_i, int32_t* slices_i, int32_t* red, void* blocks_, void* groups_, int32_t* home, float* t2,
                        double* mlb, double* t1, int32_t* refs, hipStream_t st) {
    const T *xs = static_cast<const T*>(xs_), *ys = static_cast<const T*>(ys_);
    const PrunePlan pp = prune_plan(M);
    const int C = (N + kSortSlab - 1) / kSortSlab;
    ColBlock* blocks = static_cast<ColBlock*>(blocks_);
    GroupBox* groups = static_cast<GroupBox*>(groups_);
    const double inv2eps = 0.5 / (double)eps;
    const double L = prune_L(M);
    hipLaunchKernelGGL(prune_blocks_kernel<T>, dim3((pp.nT + 3) / 4), dim3(256), 0, st, ys, h, pot, pot_scale, M, D, pp.nT, blocks, groups);
    hipLaunchKernelGGL(prune_slabs_kernel<T>, dim3(C), dim3(256), 0, st, xs, N, M, D, blocks, pp.nT, pp.PB, pp.S, inv2eps, L, ranges_i, slices_i,
                       red, home, mlb, t1, refs);
    hipLaunchKernelGGL(prune_tiles_kernel<T>, dim3(C), dim3(256), 0, st, xs, ys, h, pot, pot_scale, N, M, D, groups, red, pp.S, home, refs, inv2eps, L,
                       t2);
}

// Which sweep takes the sorted p = 2 launch on the f16 x 2 layout (glhip_list_cursor.h: list_takes_launch on kListRefSlabs reference
// slabs), once per launch: one wavefront, after prune_slabs_kernel has written the slots and home blocks the rule reads, writes the
// int that both sweeps read (Level2::list_takes) — the workgroups of the sweep that is not named return on one load, and no working
// wavefront scans slabs.
__global__ void __launch_bounds__(64) list_decide_kernel(const int32_t* __restrict__ slices_i, const int32_t* __restrict__ red,
                                                         const int32_t* __restrict__ home, int n_slabs, int M, int keep_pct,
                                                         int32_t* __restrict__ out) {
    const int lane = threadIdx.x;
    long long kept = 0;
    bool all_free = true;
    for (int k = 0; k < kListRefSlabs; ++k) {
        const int s = list_ref_slab(k, n_slabs);
        all_free = all_free && home[s] < 0;
        // the columns of all the intervals of the slab (disjoint intervals of one cloud: at most M, an int)
        int cols = 0;
        for (int q = (s == 0 ? 0 : slices_i[s - 1]) + lane; q < slices_i[s]; q += 64) cols += max(red[2 * q + 1] - red[2 * q], 0);
        for (int off = 32; off > 0; off >>= 1) cols += __shfl_xor(cols, off, 64);
        kept += cols;
    }
    if (lane == 0) *out = list_takes_launch(all_free, kept, (long long)kListRefSlabs * M, keep_pct) ? 1 : 0;
}

}  // namespace

namespace glhip {

void list_decide(const int32_t* slices_i, const int32_t* red, const int32_t* home, int n_slabs, int M, int keep_pct, int32_t* out,
                 hipStream_t st) {
    hipLaunchKernelGGL(list_decide_kernel, dim3(1), dim3(64), 0, st, slices_i, red, home, n_slabs, M, keep_pct, out);
}

size_t prune_blocks_bytes(int M) { return (size_t)prune_plan(M).nT * sizeof(ColBlock); }
size_t prune_groups_bytes(int M) { return (size_t)((M + 31) / 32) * sizeof(GroupBox); }

void prune_ranges(const void* xs, const void* ys, const float* h, const float* pot, float pot_scale, int N, int M, int D, int in_dtype,
                  float eps, int32_t* ranges_i, int32_t* slices_i, int32_t* red, void* blocks, void* groups, int32_t* home, float* t2,
                  double* mlb, double* t1, int32_t* refs, hipStream_t st) {
    if (in_dtype == GLHIP_F32) prune_ranges_typed<float>(xs, ys, h, pot, pot_scale, N, M, D, eps, ranges_i, slices_i, red, blocks, groups, home, t2, mlb, t1, refs, st);
    else prune_ranges_typed<bf16_t>(xs, ys, h, pot, pot_scale, N, M, D, eps, ranges_i, slices_i, red, blocks, groups, home, t2, mlb, t1, refs, st);
}

}  // namespace glhip
