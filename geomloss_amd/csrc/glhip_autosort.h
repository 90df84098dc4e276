// glhip_autosort.h — big dense DISTANCE reductions sort their clouds themselves (round 6; round-5 review, missing #4).
//
// The matrix-core distance kernel of glhip_dist_x32.h (p = 1 soft-min, laplacian / energy products, D <= 3) needs spatially compact
// row blocks.  Until round 5 only the Python side knew how to provide them (voxel sort + boustrophedon chaining, hip.py:_CompactRows),
// so a caller binding glhip_softmin_fwd(p = 1) through INTEGRATION.md's stub — the `lse_genred("Norm2(X-Y)")` call site,
// _legacy/sinkhorn_samples.py:316-334 — got the generic explicit-difference kernel: 346 ms instead of 191 at N = M = 1e6.
// Now the entry points do it behind the ABI, inside the caller's workspace and on the caller's stream, without a host round trip:
//   bounding box -> voxel edge (~256 rows per voxel; columns: 512; the pruned p = 2 call: 256 / 256 and a minor key, below) ->
//   boustrophedon path index of every point as the sort key ->
//   rocPRIM radix sort (-> the pruned p = 2 call: balanced cells inside blocks of 1024, below) -> gathered clouds and column / row vectors -> the block-sparse launch "every slab of 256 rows x all columns"
//   with GLHIP_FLAG_MFMA_DIST -> results scattered back to the caller's row order.
// Conditions: B = 1, dense, D <= 3, N >= 65536, N M >= 5e8 (p = 2: >= 1e11, prune_applies), neither GLHIP_FLAG_NO_MFMA / _DIRECT nor GLHIP_FLAG_NO_SORT, and a
// workspace of glhip_workspace_bytes(...) (smaller: the generic kernel, as before).  Two sorts of ~0.5 ms against ~200 ms.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "glhip_error.h"
#include "glhip_split_policy.h"      // align256

namespace glhip {

constexpr int kSortSlab = 256;        // rows per row block = the row tile of the distance kernel (8 wavefronts x 32 rows)
constexpr int kSortColChunks = 8;     // column intervals per slab: something for the column splits to split
constexpr int kSortRowsPerVoxel = 256;

// p = 2 soft-min / half-step (round 7): the sorted launch keeps only the column blocks that can matter in float32.
//   T: kPruneColBlock consecutive sorted columns; R: a slab of kSortSlab sorted rows; h_j the dual value of column j (logw + pot / eps
//   for the half-step).  With boxes of R and T and dmin / dmax their smallest / largest distance,
//     Mlb(R) = max_T [hmax(T) - dmax(R,T)^2 / (2 eps)]        <= max_j [h_j - |x_i - y_j|^2 / (2 eps)] for every row i of R,
//   and T is kept iff hmax(T) - dmin(R,T)^2 / (2 eps) >= Mlb(R) - L, L = ln M + 26 ln 2 + kPruneMarginNats.  Every term of a dropped
//   block is below e^(Mlb - L) <= 2^-26 e^-margin / M times the row's largest term, so all of them together are below 2^-26 of the row
//   sum: the output -eps log(sum) moves by less than eps 2^-26, under one float32 ulp of it.  The bound is evaluated in float64 from
//   the exact float32 box corners; the margin (1 nat) covers the exponent error of the f16 x 2 layout on the dropped terms and on the
//   row maximum (2^-21 of up to ~2.6e5 log2 units: 0.09 nat each) and the float32 rounding of logw + pot / eps.
//   Special values keep the dense launch's behaviour: a column block with a non-finite coordinate or a NaN dual value is kept by every
//   slab (and left out of Mlb); a slab with a non-finite coordinate or a non-finite Mlb (all h = -inf, h = +inf, ...) keeps everything;
//   a block whose dual values are all -inf may go.
//   Kept blocks become column intervals per slab: at most kPruneRuns runs (a slab with more closes its smallest gaps: more work,
//   never less), cut on a grid of pieces so that the column splits of the inner launch, which take a slab's intervals round robin,
//   get even shares even when nothing prunes.
//   Second level (round 9; the test and its exactness argument: glhip_softmin_x32.h, P2): inside the kept intervals every wavefront of
//   the reducing kernel skips the groups of 32 columns that cannot matter to its own 32 rows, against its rows' running maxima seeded
//   with their exact maxima over the slab's HOME BLOCK — the block that attains Mlb(R), always kept (its dmin <= its dmax).  For it
//   prune_blocks_kernel also writes one record per aligned group of 32 sorted columns (intervals start on multiples of kPruneColBlock,
//   so a tile's group g is a global group) and prune_slabs_kernel the home block of every slab (-1: a slab that keeps everything, for
//   lack of a finite bound or because every block passes it — no second level, no cost of it, for such a slab).
//   The sweep (library 137).  bf16 x 3: softmin_fwd_x32_p2_kernel, 8 wavefronts on one staged 512-column LDS tile, the test per tile
//   on its 16 groups.  f16 x 2: one of two kernels, chosen per launch on the device from the records of eight reference slabs
//   (glhip_list_cursor.h, list_takes_launch; library 140: once, by list_decide, which writes one int behind `refs` that both sweeps
//   read) — where the first level keeps at most 30 % of the columns, or no slab has a home block,
//   softmin_fwd_list_p2_kernel (glhip_softmin_list.h): one wavefront per tile of 32 rows, no LDS tile and no barrier, one test and
//   one ballot per batch of up to 64 groups of a piece, the kept groups read straight from the group-major packed columns through
//   a ring of four operands in registers, the lazy maximum with a batch = one ballot; otherwise the staged kernel on 4 wavefronts
//   (same test per tile of 16 groups).  Same seed, same test expression, same thresholds, same guarantee in both.
//   The sorted p = 2 call orders both clouds in voxels of kSortRowsPerVoxel
//   points with a minor key of sub-voxels of ~32 points (prune_sort_sub), so that 32 consecutive points are compact; the distance
//   launches (p = 1, laplacian, energy) keep the order they had.
//   Balanced cells (library 128).  Voxels and sub-voxels hold 256 and 32 points on average, with Poisson counts: an ALIGNED run of exactly
//   256 (32) sorted points — what both levels put a box around — usually straddles two of them, and its box is up to twice the size
//   it could be.  So after the radix sort the sorted p = 2 call splits every whole aligned block of kBalanceBlock = 1024 positions
//   of the path order like a k-d tree (balance_kernel, glhip_compact_sort.hip; the rules: glhip_balance.h): five levels with segments of
//   1024, 512, 256, 128 and 64 points, each segment sorted by (coordinate on the axis of its largest finite extent — ties: the lowest
//   axis — in an order where -inf < ... < +inf < NaN, position the point had in the block).  The result: cells of exactly 512, 256,
//   128, 64 and 32 points, every one the half of a median cut, which slabs, column blocks, row tiles and column groups are aligned to.
//   (The kernel sorts in full on the last level only.  The words carry the position a point had in the incoming block, so a level
//   above the last matters through the SET of each half alone, and the first step of a segment's last merge already separates the
//   halves: glhip_balance.h, balance_step_runs.  The order is the one five full sorts give, position for position.)
//   The order is a function of the input alone; the set of points of every block of 1024 is what the path order put there, so the
//   voxel path still decides which blocks are neighbours; the last n mod 1024 points keep the path order (the minor key orders them).
//   The pruning is exact for any order: the order only decides how much is kept.  Bench problem at 1e6, eps = 0.05^2 (tools/prune_model.py,
//   profiles/balanced_order_model.txt): kept by the first level 0.262 -> 0.227 of the blocks, evaluated after the second 0.155 -> 0.134 (device counter: 0.158 -> 0.140).
//   Mass rule (round 10).  Both tests above pay ln M of their L for the case that all M columns sit exactly at the threshold.  What the
//   guarantee needs is that the SUM of everything dropped stays under 2^-26 of the row sum, and that sum is bounded from the records:
//   with lse(S) = log sum_{j in S} e^(h_j) and pen(A, S) = dmin(A, S)^2 / (2 eps), the terms of a set S of columns sum to at most
//   e^(lse(S) - pen(A, S)) for every row in the box A.  The 2^-26 is split three ways, each piece with its own proof:
//     first level, kPruneBudget1 = 2^-26 (1 - 1 / e - 1 / 2) = 0.132 x 2^-26 of e^Mlb(R): a block T has the key k(T) = lse(T) - pen(R, T); prune_slabs_kernel finds the largest threshold
//       t1(R) such that the masses e^(k(T) - Mlb(R)) of the blocks with k(T) < t1 sum to at most the budget, and keeps T iff k(T) >= t1(R)
//       (or T is special, or the slab keeps everything).  Mlb and the home block are what they were: Mlb is a term the row really has.
//     second level, term rule, 2^-26 / e: the kernel's test against the rows' running maxima, unchanged (at most M terms, each under
//       e^-L of the row's largest).  The group records hold lse(G) in the place of hmax(G): lse >= hmax, the test stays valid.
//     second level, mass rule, kPruneBudget2 = 2^-26 / 2 of e^ms(W), ms(W) the smallest of the exact largest exponents of the tile's 32 rows
//       over the home block (each of them a term its row really has): prune_tiles_kernel finds, over the groups inside the slab's
//       emitted intervals, the largest t2(W) such that the masses e^(k(W, G) - ms(W)) of the groups with k(W, G) = lse(G) - pen(W, G)
//       < t2 sum to at most the budget; the kernel's threshold is max(term rule's, t2(W)).
//   Thresholds come from histograms, not sorts: kPruneBuckets buckets of kPruneBucketNats from the term rule's threshold (Mlb - L,
//   ms - L) up, each holding the actual mass of its keys; keys below the range share an underflow bucket that is always counted (and
//   can never exceed a budget by itself: glhip_prune.hip, prune_first_kept), keys above it are never dropped; the threshold is the
//   lower edge of the first bucket at which the running sum passes the budget.  Rounding: the first level and t2 are float64 from the
//   exact float32 corners; lse is a float32 rounded UP (kPruneLseSlack); t2 is stored in log2 units as a float32 rounded toward minus
//   infinity; the kernel's ub carries its slack on the keep side.  Special blocks and groups are never dropped and enter no sum; a
//   slab with home = -1 gets no threshold work; a tile without a finite seed gets t2 = -inf.  The thresholds live in the sort scratch.
//   Headline law at 1e6: tools/prune_model.py, profiles/r10_*.
//   Sum reference (library 136).  The two mass budgets above are stated relative to ONE term the row has (e^Mlb, e^ms); the guarantee
//   is relative to the row SUM S_i = sum_j e^(h_j - |x_i - y_j|^2 / (2 eps)), which exceeds its largest term by ln(S_i / max) nats
//   (bench law 1.35, a uniform dual vector 7.5 at the headline density).  Both budgets now refer to a lower bound of log S_i that the
//   records give; everything else — Mlb, the home block, the bucket grids anchored at Mlb - L and ms - L, t1 and t2 as stored, the
//   term rule, the three shares — is what it was.
//     Notation.  lse_dn(S): the record's rounded-up lse lowered again, in float64, by twice its own slack for a group and four times
//       for a block (a block's record is rounded up twice: it is formed from its groups' rounded-up values), lse_dn(v, n) =
//       v - n 2^-20 (|v| + 8).  The float32 value before rounding up is within 0.3 slacks of the true lse (glhip_prune.hip, lse_up),
//       so a group's record is at most 1.3 slacks and a block's at most 2.3 slacks + 2.7 x 2^-20 < 3 slacks above the truth (the
//       groups' slacks s (|g| + 8) enter a block with their weights e^(g - b): sum_g w_g |g| <= |b| + sum_g w_g ln(1 / w_g) <= |b| +
//       ln 8): lse_dn(S) <= log sum_{j in S} e^(h_j).  dmaxpen(A, S) = dmax(A, S)^2 / (2 eps), dmax the largest distance between the
//       box (or point) A and the box of S, float64 from the exact float32 corners.
//     First level.  Slb(R) = log sum_T e^(lse_dn(T) - dmaxpen(R, T)) over the non-special blocks T, lowered by kPruneSumSlack (float64
//       sums of at most 2^23 terms; terms below e^-40 of e^Mlb are left out, which only lowers it), and max(Slb, Mlb).  For every
//       row i of R and column j of T, |x_i - y_j| <= dmax(R, T), so S_i >= sum_T e^(-dmaxpen(R, T)) sum_{j in T} e^(h_j) >= e^Slb(R).
//       The masses of the first-level histogram are e^(k(T) - Slb(R)): the kernel keeps them relative to Mlb and multiplies the
//       budget by e^(Slb - Mlb) instead, which is the same comparison.  Dropped: at most kPruneBudget1 e^Slb <= kPruneBudget1 S_i.
//     Reference set.  Per slab a list of at most kPruneRefBlocks blocks with the largest scores s(T) = lse_dn(T) - dmaxpen(R, T),
//       ranked on a grid: cell(T) = floor((Mlb + kPruneRefTop - s(T)) kPruneRefCellsPerNat) (>= 0: lse(T) <= hmax(T) + ln 256 and
//       hmax(T) - dmaxpen(R, T) <= Mlb), whole cells taken from cell 0 up while at most kPruneRefBlocks - 1 blocks are in, then the
//       home block if it is not among them.  Blocks of one cell go in together or not at all, so no tie needs breaking and the list
//       is a function of the records alone; it is written in ascending block order, unused entries -1.  (A list that takes the
//       largest scores one by one would win 1.5 points more of the evaluated pairs on the bench law; it needs a sort per slab.)
//     Second level.  For every row, ls_i = log sum_G e^(lse_dn(G) - dmaxpen(x_i, G)) over the non-special groups G of the reference
//       blocks (point to box, float64), the exponentials in float32 on arguments relative to the row's seed — or to the last term
//       that lay more than 60 nats above the reference: it becomes the reference, and what was summed before it, now under
//       128 e^-60 of the sum, is scaled down with it — lowered by kPruneLsSlack = 1e-4: the float32 argument (at most 60 nats:
//       3.6e-6), the hardware exponential __expf (the argument times log2 e, 87 log2 units at most, rounds by 5.2e-6; v_exp_f32
//       itself 1 ulp), the sum of 128 terms (7.6e-6) and logf (2 ulp of at most 65: 1.6e-5) stay under 3.3e-5.
//       S_i >= e^ls_i as above, and S_i >= e^seed_i, the row's exact largest exponent over the home block (one term of the same sum; rows
//       of one tile can lie a hundred nats apart when the dual values do).  ls(W) = min_i max(seed_i, ls_i) >= ms(W); the masses of the
//       tile's histogram are e^(k(W, G) - ls(W)), again as a budget multiplied by e^(ls - ms).  Dropped: at most kPruneBudget2
//       e^ls(W) <= kPruneBudget2 S_i for every row of the tile.  With the term rule's 2^-26 / e of the largest term <= 2^-26 / e S_i
//       the three pieces stay under 2^-26 S_i.  The underflow argument of prune_first_kept holds: the budgets only grew.
//     Special values: special blocks and groups enter no sum and no list; a slab with a non-finite coordinate or Mlb keeps everything;
//       a tile without a finite seed gets t2 = -inf; a Slb or ls that is not finite, or below Mlb or ms, falls back to Mlb or ms.
//     Bench problem at 1e6 (tools/prune_model.py --balanced, profiles/sum_reference.txt): first level keeps 0.2378 -> 0.2287, 512-column
//     tiles 1 946 177 -> 1 873 861, evaluated 0.1333 -> 0.1232 (-7.6 %); a uniform dual vector: 0.1820 -> 0.1378 (-24 %).  With 32
//     reference blocks: 0.1220 and 0.1358 in the model; what prune_tiles_kernel then costs on the device: profiles/sum_reference.txt.
constexpr int kPruneColBlock = 256;   // columns per column block T (a multiple of 64)
constexpr int kPruneRuns = 160;       // runs of kept blocks per slab (the bench problem under the mass rule: mean 71, max 175 — 8 of 3907 slabs
                                      // close their one-block gaps, 0.01 % more kept pairs: profiles/r10_prune_model.txt; with balanced
                                      // cells: profiles/balanced_order_model.txt — 562 slabs, which take their gap lengths, g and
                                      // their pieces from the 64-bit words of the kept-block bit set: glhip_prune_words.h)
constexpr int kBalanceBlock = 1024;   // positions of the path order that are balanced together (a multiple of kSortSlab and kPruneColBlock)
constexpr int kBalanceLeaf = 32;      // points of the smallest cell: the row tile of a wavefront, the column group
constexpr int kPruneGrid = 64;        // pieces a whole row of column blocks is cut into, at most
constexpr double kPruneMarginNats = 1.0;
// The mass rule (round 10): thresholds are found on histograms of the keys, kPruneBuckets buckets of kPruneBucketNats starting at the
// classic threshold.  28 nats cover ln M + 4 for every M an int holds (ln 2^31 = 21.5).  The budgets: the row sum may lose 2^-26 in
// all — 2^-26 / e by the term rule of the second level (fixed: it is the kernel's L), half of the 2^-26 by the mass rule of the second
// level, the remaining 2^-26 (1 - 1 / e - 1 / 2) by the first.  Earlier builds gave the first level 1 / e and the mass rule 1 - 2 / e =
// 0.264; only the mass rule decides how many exponentials run, and the first level's threshold moves by ln(0.368 / 0.132) ~ one nat.
// Bench problem at 1e6 (tools/prune_model.py, profiles/chunk_skip.txt): first level keeps 0.2295 -> 0.2378 of the blocks, evaluated
// 0.1434 -> 0.1389; measured: transcendental instructions of the sweep -3.2 %, the call 15.96 -> 15.72 ms.
constexpr int kPruneBuckets = 112;
constexpr double kPruneBucketNats = 0.25;
constexpr double kPruneMassShare = 0.5;                                                                           // the mass rule's part of the 2^-26
constexpr double kPruneBudget1 = 1.4901161193847656e-08 * (1.0 - 1.0 / 2.718281828459045 - kPruneMassShare);      // 2^-26 (1 - 1 / e - 1 / 2)
constexpr double kPruneBudget2 = 1.4901161193847656e-08 * kPruneMassShare;                                        // 2^-26 / 2
// The sum reference (above): the reference list of a slab and the grid its scores are ranked on (32 nats below Mlb + kPruneRefTop,
// kPruneRefTop >= ln 256 + the records' slack), and what the two lower bounds of the row sum are lowered by.
constexpr int kPruneRefBlocks = 16;      // 8 and 32 modelled and 32 measured: profiles/sum_reference.txt
constexpr double kPruneRefTop = 5.625;
constexpr int kPruneRefCellsPerNat = 16;
constexpr int kPruneRefCells = 512;
constexpr double kPruneSumSlack = 1e-9;
constexpr double kPruneLsSlack = 1e-4;

struct PrunePlan {
    int nT;    // column blocks
    int PB;    // column blocks per grid piece
    int S;     // interval slots per slab
};
inline PrunePlan prune_plan(int M) {
    PrunePlan p;
    p.nT = (M + kPruneColBlock - 1) / kPruneColBlock;
    p.PB = (p.nT + kPruneGrid - 1) / kPruneGrid;
    p.PB = p.PB > 64 ? p.PB : 64;                  // pieces of at least 16384 columns
    p.S = kPruneRuns + (p.nT + p.PB - 1) / p.PB;   // runs + grid cuts inside them
    return p;
}
// From 1e11 pairs on: the two sorts, the bound and the scatter cost ~1 ms per call, and the online loss at N = M = 1e5 (1e10 pairs per
// half-step, ~0.8 ms each dense) went from 34.4 to 46.8 ms with every call pruned.  Interval slots address red[2 q] with an int.
constexpr double kPruneMinPairs = 1e11;
inline bool prune_applies(int N, int M) {
    const long C = (N + kSortSlab - 1) / kSortSlab;
    return (double)N * M >= kPruneMinPairs && C * (long)prune_plan(M).S * 2 < (1L << 31) - 1;
}

// implemented in glhip_compact_sort.hip (rocPRIM's radix sort lives there)
size_t compact_sort_scratch_bytes(int n);
// sub > 1: inside a voxel, points are ordered by sub-voxel of edge voxel / sub (the minor key of path_keys_kernel), then every whole
// block of kBalanceBlock positions is split into balanced cells (balance_kernel).  hinted: `perm` already holds the order, from an
// earlier call on the same cloud (glhip_sinkhorn_step_perm) — nothing but the gather runs, with every index clamped into [0, n)
// (glhip_perm_index.h); the same flag on gather_f32 / scatter_f32 clamps theirs.
int compact_sort(const void* z, int n, int D, int in_dtype, int rows_per_voxel, int32_t* perm, void* z_sorted, void* scratch,
                 size_t scratch_bytes, hipStream_t st, int sub = 1, bool hinted = false);
void gather_f32(const float* src, const int32_t* perm, float* dst, int n, hipStream_t st, bool hinted = false);       // dst[k] = src[perm[k]]
void scatter_f32(const float* src, const int32_t* perm, float* dst, int n, hipStream_t st, int width = 1, bool hinted = false);      // dst[perm[k], :] = src[k, :]
void slab_ranges(int N, int M, int32_t* ranges_i, int32_t* slices_i, int32_t* red, hipStream_t st);
// implemented in glhip_prune.hip
size_t prune_blocks_bytes(int M);
size_t prune_groups_bytes(int M);
// the kept column intervals of every slab of the sorted clouds xs (N, D), ys (M, D) for the column vector h (+ pot * pot_scale); for the
// second level: the records of the groups of 32 columns (`groups`, prune_groups_bytes), every slab's home block (`home`, C ints) and the
// mass-rule threshold of every tile of 32 rows (`t2`, ceil(N / 32) floats); for glhip_prune_inspect: every slab's Mlb and t1 (C doubles each);
// between the two kernels: every slab's reference blocks (`refs`, C x kPruneRefBlocks ints)
void prune_ranges(const void* xs, const void* ys, const float* h, const float* pot, float pot_scale, int N, int M, int D, int in_dtype,
                  float eps, int32_t* ranges_i, int32_t* slices_i, int32_t* red, void* blocks, void* groups, int32_t* home, float* t2,
                  double* mlb, double* t1, int32_t* refs, hipStream_t st);
// L of the bound in nats
inline double prune_L(int M) { return std::log((double)M) + 26.0 * 0.6931471805599453 + kPruneMarginNats; }
// sub-voxels per axis of the sorted p = 2 call: sub^D ~ 8 sub-voxels of ~32 points in a voxel of kSortRowsPerVoxel
inline int prune_sort_sub(int D) { return D >= 3 ? 2 : (D == 2 ? 3 : 8); }

inline bool autosort_applies(int B, int N, int M, int D, int n_ranges, int flags) {
    return B == 1 && n_ranges == 0 && D <= 3 && N >= 65536 && (double)N * M >= 5e8 &&
           !(flags & (2 /* NO_MFMA */ | 1 /* DIRECT */ | 512 /* NO_SORT */));
}

struct AutoSort {
    bool on = false;
    int C = 0;                              // slabs
    int32_t *perm_x = nullptr, *perm_y = nullptr, *ranges_i = nullptr, *slices_i = nullptr, *red = nullptr;
    bool hint_x = false, hint_y = false;    // perm_x / perm_y is the caller's hint: whatever indexes through it clamps (glhip_perm_index.h)
    void *xs = nullptr, *ys = nullptr;
    float *col0 = nullptr, *col1 = nullptr, *row0 = nullptr, *out = nullptr;      // gathered per-column / per-row vectors, sorted output
    float* out_rows = nullptr;              // (N, D) sorted output (row gradients)
    void* blocks = nullptr;                 // per-column-block boxes and dual maxima (pruned p = 2 launches)
    void* groups = nullptr;                 // the same per group of 32 columns, and every slab's home block: the second level
    int32_t* home = nullptr;
    float* t2 = nullptr;                    // per tile of 32 rows: the second level's mass-rule threshold; per slab: Mlb and the first
    double *mlb = nullptr, *t1 = nullptr;   // level's threshold.  All three live in the sort scratch, dead once both sorts have run,
    int32_t* refs = nullptr;                // and so do the reference blocks of every slab (the sum reference)
    int32_t* list_takes = nullptr;          // and the one int behind them: which sweep takes the f16 x 2 launch (Level2::list_takes)
    void* inner_ws = nullptr;
    size_t inner_bytes = 0;
};

// bytes the sorted call carves off the FRONT of the workspace (everything but the inner launch's own scratch)
inline size_t autosort_bytes(int N, int M, int D) {
    const int C = (N + kSortSlab - 1) / kSortSlab;
    const int L = N > M ? N : M;
    const size_t slots = (size_t)(kSortColChunks > prune_plan(M).S ? kSortColChunks : prune_plan(M).S);   // interval slots per slab
    return align256((size_t)N * 4) + align256((size_t)M * 4) + align256((size_t)N * D * 4) + align256((size_t)M * D * 4) +
           2 * align256((size_t)M * 4) + 2 * align256((size_t)N * 4) + align256((size_t)N * D * 4) + align256((size_t)C * 8) +
           align256((size_t)C * 4) +
           align256((size_t)C * slots * 8) + align256(prune_blocks_bytes(M)) + align256(prune_groups_bytes(M)) +
           align256((size_t)C * 4) + compact_sort_scratch_bytes(L);
}

// Sorts both clouds into the workspace; `a.on` stays false when the workspace is too small for the sorted call plus `inner_min`
// bytes of scratch for the launch itself (the caller then runs the generic kernel).  slabs = false: the caller fills the ranges
// itself (prune_ranges) once its column vector is gathered.
// Reused permutations (library 134; the pruned p = 2 call only, slabs = false).  Bounding box, voxel edge, path keys, the 64-bit sort
// and the balanced cells of a cloud depend on its coordinates alone, and a Sinkhorn loop calls a few hundred times on the same two
// clouds.  ext_x / ext_y: a caller's buffer of N / M ints that takes the place of the workspace's perm_x / perm_y, without a copy —
// with its bit of `perm_flags` (1: x, 2: y; GLHIP_PERM_HINT_*) it HOLDS the order and only the gather runs for that cloud, without it
// the sort and balance_kernel write the order straight into it.  A hint is safe because the pruning is exact for any order (above):
// every box of both levels is recomputed from the gathered coordinates on every call, so a stale hint costs kept pairs, never accuracy.
// Only permutations are reused for that reason, never sorted coordinates or box records.  The workspace layout stays what it was.
inline int autosort_prepare(AutoSort& a, const void* x, const void* y, int N, int M, int D, int in_dtype, void* workspace,
                            size_t workspace_bytes, size_t inner_min, hipStream_t st, bool slabs = true, int32_t* ext_x = nullptr,
                            int32_t* ext_y = nullptr, int perm_flags = 0) {
    const size_t need = autosort_bytes(N, M, D);
    if (!workspace || workspace_bytes < need + inner_min) return 0;
    char* w = static_cast<char*>(workspace);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = w + off; off += align256(bytes); return p; };
    a.C = (N + kSortSlab - 1) / kSortSlab;
    a.perm_x = reinterpret_cast<int32_t*>(take((size_t)N * 4));
    a.perm_y = reinterpret_cast<int32_t*>(take((size_t)M * 4));
    a.xs = take((size_t)N * D * 4);
    a.ys = take((size_t)M * D * 4);
    a.col0 = reinterpret_cast<float*>(take((size_t)M * 4));
    a.col1 = reinterpret_cast<float*>(take((size_t)M * 4));
    a.row0 = reinterpret_cast<float*>(take((size_t)N * 4));
    a.out = reinterpret_cast<float*>(take((size_t)N * 4));
    a.out_rows = reinterpret_cast<float*>(take((size_t)N * D * 4));
    a.ranges_i = reinterpret_cast<int32_t*>(take((size_t)a.C * 8));
    a.slices_i = reinterpret_cast<int32_t*>(take((size_t)a.C * 4));
    const size_t slots = (size_t)(kSortColChunks > prune_plan(M).S ? kSortColChunks : prune_plan(M).S);
    a.red = reinterpret_cast<int32_t*>(take((size_t)a.C * slots * 8));
    a.blocks = take(prune_blocks_bytes(M));
    a.groups = take(prune_groups_bytes(M));
    a.home = reinterpret_cast<int32_t*>(take((size_t)a.C * 4));
    const int L = N > M ? N : M;
    const size_t sb = compact_sort_scratch_bytes(L);
    void* scratch = take(sb);
    if (!slabs && ext_x) { a.perm_x = ext_x; a.hint_x = (perm_flags & 1) != 0; }
    if (!slabs && ext_y) { a.perm_y = ext_y; a.hint_y = (perm_flags & 2) != 0; }
    // (slabs = false is the pruned p = 2 call: both clouds in voxels of kSortRowsPerVoxel points, compact sub-voxels inside)
    int rc = compact_sort(x, N, D, in_dtype, kSortRowsPerVoxel, a.perm_x, a.xs, scratch, sb, st, slabs ? 1 : prune_sort_sub(D), a.hint_x);
    if (rc) return rc;
    rc = compact_sort(y, M, D, in_dtype, slabs ? 2 * kSortRowsPerVoxel : kSortRowsPerVoxel, a.perm_y, a.ys, scratch, sb, st,
                      slabs ? 1 : prune_sort_sub(D), a.hint_y);
    if (rc) return rc;
    if (slabs) slab_ranges(N, M, a.ranges_i, a.slices_i, a.red, st);
    // (the scratch holds 20 bytes per point of the larger cloud and more: N / 8 + (16 + 4 kPruneRefBlocks) C + 4 bytes, 0.7 bytes per
    // row, fit many times over)
    static_assert(kPruneRefBlocks <= 256, "the reference lists stay under 4 bytes per row");
    a.mlb = reinterpret_cast<double*>(scratch);
    a.t1 = a.mlb + a.C;
    a.t2 = reinterpret_cast<float*>(a.t1 + a.C);
    a.refs = reinterpret_cast<int32_t*>(a.t2 + (N + 31) / 32);
    a.list_takes = a.refs + (size_t)a.C * kPruneRefBlocks;
    a.inner_ws = w + off;
    a.inner_bytes = workspace_bytes - off;
    a.on = true;
    return 0;
}

// The sorted call of a laplacian / energy kernel product (glhip_kernel_conv_fwd, glhip_kernel_conv_fwd_grad) where autosort_applies: both
// clouds sorted into the workspace, v gathered, `inner(a, flags)` — the entry point itself on the sorted clouds, block-sparse over the
// slabs, writing a.out (and a.out_rows) — and the product (and the rows of `rows_out`, where given) scattered back to the caller's order.
// GLHIP_FLAG_GRAD_FAMILY travels with the inner flags: both entry points sort the same way, so the two still round alike.
// *ran stays false when the workspace is too small: the caller launches on the clouds as they are.
template <class Inner>
int autosort_conv(const char* fn, const void* x, const void* y, const float* v, float* out, float* rows_out, int N, int M, int D,
                  int in_dtype, void* workspace, size_t workspace_bytes, int flags, hipStream_t st, bool* ran, Inner inner) {
    AutoSort a;
    *ran = false;
    const int C = (N + kSortSlab - 1) / kSortSlab;
    int rc = autosort_prepare(a, x, y, N, M, D, in_dtype, workspace, workspace_bytes, glhip_workspace_bytes(1, N, M, D, C), st);
    if (rc || !a.on) return rc;
    *ran = true;
    gather_f32(v, a.perm_y, a.col0, M, st);
    rc = inner(a, flags | GLHIP_FLAG_MFMA_DIST | GLHIP_FLAG_NO_SORT);
    if (rc) return rc;
    scatter_f32(a.out, a.perm_x, out, N, st);
    if (rows_out) scatter_f32(a.out_rows, a.perm_x, rows_out, N, st, D);
    return check_launch(fn);
}

}  // namespace glhip
