// glhip_split_policy.h — THE column-split policy of every row-tiled reduction launch, and the workspace size that goes with it.  Plain
// C++ (no HIP header, no HIP type: a host compiler builds a stand-alone program around it, tests/test_split_policy_cpu.py), like
// glhip_prune_words.h and glhip_balance.h.
//
// A launch decides three things on the host: how many column splits it takes, whether it moves to the XCD-aware grid, and whether it
// places pre-packed column records behind the split partials, and where.  Here: the rules (choose_splits, xcd_splits, free_splits, ...),
// the arithmetic of a split workspace (SplitGeom), the decision as a value (SplitPlan), one plan function per distinct policy — pure
// functions of the shape, the workspace size and the Scratch booleans, which queue nothing — and forward_workspace_bytes, what
// glhip_workspace_bytes is assembled from.  The launchers of glhip_launch.h / glhip_mapreduce.h execute plans (SplitLaunch); the plan
// family (glhip_launch_plan.h) reads plan_splits and plan_pass_workspace_bytes.  A launcher caps its plan at what the workspace holds,
// so a sizing call that promises less than a launcher would take never faults: the launch runs with fewer splits or without pre-packed
// columns.  Where that happens today is listed in profiles/split_policy_caps.txt.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace glhip {

// resident 8-wave workgroups on the chip (256 CUs x workgroups per CU) of ...
constexpr long kFwdSlots = 256 * 3;   // ... the forward / gaussian x32 kernels (<= 84 VGPRs, 32 KiB LDS)
constexpr long kXdSlots = 256 * 2;    // ... the kernels of 4 <= D <= 16 (<= 48 KiB of LDS, <= 128 VGPRs)
constexpr long kXkSlots = 256 * 2;    // ... the kernels of 17 <= D <= 4095 (78.75 KiB of LDS, <= 128 VGPRs)
constexpr long kXkPlanSlots = 256;    // ... xk_plan_kernel: one per CU (glhip_plan_apply_xk.h)
constexpr long kXkTopkSlots = 256;    // ... argkmin_xk_kernel with lists of 8 / 16 candidates: one per CU (> 128 VGPRs; glhip_argkmin_xk.h)

constexpr int kXdMaxD = 16;           // 4 <= D <= 16: the xd kernels (glhip_softmin_xd.h); beyond, up to kSizedMaxD, the K-chunked ones
// Rows per workgroup of the kernel shapes the sizing rule counts with, and the last dimension it sizes; glhip_launch.h asserts each
// against the kernels' own constants.
constexpr int kRowsNW4 = 4 * 32, kRowsNW8 = 8 * 32, kRowsNW8x2 = 2 * 8 * 32;   // 4 / 8 wavefronts x 32 rows, 8 wavefronts x 2 row tiles
constexpr int kRowsValu2 = 2 * 256;   // the VALU skeleton with two rows per thread (glhip_mapreduce.h)
constexpr int kRowsXk = 256;          // glhip_softmin_xk.h
constexpr int kSizedMaxD = 4095;
constexpr int kChunkRowsMin = 64;     // the smallest row tile of a block-sparse launch (GLHIP_FLAG_SMALL_ROW_BLOCKS): what the chunk table is sized for
constexpr int kMaxPackedQ = 4;        // q components per column behind the packed records of the weighted-sum kernels (WsumShape::kNQ, D <= 3)
constexpr double kPrepackMinPairs = 5e8;   // pre-packed column records pay for their extra launch from ~5e8 pairs on

// ---- the rules -----------------------------------------------------------------------------------------

// Number of column splits: enough workgroups for >= ~16 rounds over the chip.
static inline int choose_splits(long row_blocks, int M, int n_ranges, long max_by_workspace) {
    // dense launches that already fill the chip four times over gain nothing from splits and pay one prologue / epilogue / merge share
    // per split: B = 256 x 4096 x 4096 (4096 row blocks, 3 splits by the rule below): 17.4 -> 15.9 ms per loss without (round 4)
    // (short column loops only: with long ones the last partial round of long-lived workgroups is what splits are for)
    if (n_ranges == 0 && row_blocks >= 4L * 768 && M <= 16384) return 1;
    const long target = 256L * 4 * 10;   // ~10 rounds of 4 workgroups per CU
    long ns = (target + row_blocks - 1) / row_blocks;
    const long by_cols = (n_ranges > 0) ? 8 : (long)M / 512;   // at least 512 columns per split
    ns = ns < by_cols ? ns : by_cols;
    ns = ns < 32 ? ns : 32;
    ns = ns < max_by_workspace ? ns : max_by_workspace;
    return ns < 1 ? 1 : (int)ns;
}

// THE rule line of every split launch: `fit` = column splits the workspace holds
static inline int rule_splits(long row_blocks, int M, int n_ranges, long fit, bool allow_split) {
    return (allow_split && fit >= 2) ? choose_splits(row_blocks, M, n_ranges, fit) : 1;
}

// XCD-aware dense launches use a multiple of 8 column splits (split s runs on XCD s % 8).  All workgroups take the
// same time, so the kernel lasts ceil(workgroups / resident slots) rounds: with 8 splits a 1e5-row problem is 4.07
// rounds of work spread over 5 (81 %).  Take the smallest multiple of 8 (up to 32) that fills its last round to
// >= 93 %, else the best one.  `slots` = workgroups resident on the chip (256 CUs x workgroups per CU).
static inline int xcd_splits(long row_blocks, int M, long slots, long max_by_workspace) {
    int best = 8;
    double best_eff = 0.0;
    for (int ns = 8; ns <= 32; ns += 8) {
        if (ns > max_by_workspace || (long)M / ns < 2048) break;
        const double w = (double)row_blocks * ns / (double)slots;
        const double rounds = (double)((row_blocks * ns + slots - 1) / slots);
        const double eff = w / rounds;
        if (eff >= 0.93) return ns;
        if (eff > best_eff + 0.02) { best_eff = eff; best = ns; }
    }
    return best;
}

// Mid-size dense launches whose packed columns fit the L2 of EVERY XCD at once (<= 3.5 MB: M = 1e5 at 32 bytes per column) need no
// XCD-aware placement, so the number of splits need not be a multiple of 8: the smallest ns in [4, 32] (>= 2048 columns per split)
// that fills its last round of resident workgroups to >= 97 %, else the best.  N = M = 1e5, 196 row blocks of 512 rows on 512
// slots: ns = 32 is 12.25 rounds spread over 13 (0.94) with 6 tiles per workgroup; ns = 13 is 4.98 rounds over 5 with 15 tiles.
static inline int free_splits(long row_blocks, int M, long slots, long max_by_workspace, double* eff_out) {
    int best = 0;
    double best_eff = 0.0;
    for (int ns = 4; ns <= 32; ++ns) {
        if (ns > max_by_workspace || (long)M / ns < 2048) break;
        const double w = (double)row_blocks * ns / (double)slots;
        const double eff = w / (double)((row_blocks * ns + slots - 1) / slots);
        if (eff >= 0.97) { best = ns; best_eff = eff; break; }
        if (eff > best_eff + 0.01) { best_eff = eff; best = ns; }
    }
    if (eff_out) *eff_out = best_eff;
    return best;
}

// ... and when the columns are pre-packed (64 bytes each), enough splits for one split's records to stay resident in the
// 4 MB L2 of the XCD that streams them (workgroup_coords runs one split per XCD at a time).
static inline int xcd_splits_prepacked(long row_blocks, int M, long slots, long max_by_workspace, double bytes_per_column = 64.0) {
    int ns = xcd_splits(row_blocks, M, slots, max_by_workspace);
    while (ns + 8 <= 32 && ns + 8 <= max_by_workspace && (double)M / ns * bytes_per_column > 2.5e6) ns += 8;
    return ns;
}

// Space reserved at the front of the caller's workspace for the row-chunk table of a block-sparse launch.
static inline size_t chunk_table_bytes(int n_ranges, int N, int rows) {
    return (((size_t)(1 + 3 * ((size_t)n_ranges + (size_t)N / rows + 1)) * sizeof(int32_t)) + 255) & ~(size_t)255;
}

// Block-sparse calls reserve the front of the workspace for that table, sized for the smallest row tile of the call: 128 rows, or 64 under
// GLHIP_FLAG_SMALL_ROW_BLOCKS (64-row workgroups cut a cluster into twice as many chunks; glhip_workspace_bytes reserves that much for
// every block-sparse call) and, with less workspace, 128 all the same.  Rows per chunk of the table that fits; 0: none does.
static inline int chunk_table_rows(size_t bytes, int n_ranges, int N, bool small_rows) {
    for (int rows = small_rows ? 64 : 128; rows <= 128; rows *= 2)
        if (bytes >= chunk_table_bytes(n_ranges, N, rows)) return rows;
    return 0;
}

// 256-row workgroups of the distance kernels (glhip_dist_xd.h) on a few thousand points are a handful (N = 1000: 4 per problem): launches
// with fewer than 512 workgroups split their columns down to 128 per split, up to 32 splits and what the workspace holds
// (online p = 1 losses at N = 1000 / 2000: 0.53 / 0.49 -> 0.35 / 0.38 ms)
static inline int dist_small_launch_splits(int n_splits, long row_blocks, int M, long fit, bool allow_split) {
    constexpr int min_cols = 128;
    if (!allow_split || row_blocks * n_splits >= 512) return n_splits;
    long want = (512 + row_blocks - 1) / row_blocks;
    const long by_cols = M / min_cols;
    want = want < by_cols ? want : by_cols;
    want = want < 32 ? want : 32;
    want = want < fit ? want : fit;
    return want > n_splits ? (int)want : n_splits;
}

// ---- the plan family (glhip_launch_plan.h) ---------------------------------------------------------------

constexpr size_t kPlanMaxWorkspace = (size_t)1 << 30;     // no *_workspace_bytes call of this family asks for more than 1 GiB (glhip.h)

// THE split policy of a pass, shared by the launcher and by the sizing calls: the rule of every split launch (choose_splits), or — dense
// launches with room for 8 splits over >= 65536 columns (SplitGeom::xcd_eligible) — the XCD-aware grid with xcd_splits.
// `fit`: splits the workspace holds; `slots`: resident workgroups of the kernel shape.
struct PlanSplits { int n; bool xcd; };
inline PlanSplits plan_splits(long row_blocks, int M, long fit, bool allow_split, long slots) {
    if (!allow_split || fit < 2) return PlanSplits{1, false};
    if (fit >= 8 && M >= 65536) return PlanSplits{xcd_splits(row_blocks, M, slots, fit), true};
    return PlanSplits{choose_splits(row_blocks, M, 0, fit), false};
}

// The workspace of the widest pass (nv sums) of a call: what launch_plan_pass would take with up to 1 GiB, for the largest of the
// resident-workgroup counts its kernel shapes have; 0 where the pass runs unsplit.
inline size_t plan_pass_workspace_bytes(int B, int N, int M, int rows, int nv, std::initializer_list<long> slots) {
    const size_t per_split = (size_t)B * N * (nv + 2) * sizeof(float);
    const long row_blocks = (long)B * ((N + rows - 1) / rows);
    long fit = (long)(kPlanMaxWorkspace / per_split);
    fit = fit < 32 ? fit : 32;
    int ns = 0;
    for (long s : slots) {
        const int n = plan_splits(row_blocks, M, fit, true, s).n;
        ns = n > ns ? n : ns;
    }
    return ns >= 2 ? (size_t)ns * per_split : 0;
}

// ---- the arithmetic of a split workspace ------------------------------------------------------------------

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// pre-packed column records (16 bytes each) live in whole groups of 32 columns: records per batch item, bytes per launch
static inline long packed_stride(int M, int recs_per_column) { return (long)((M + 31) / 32) * (32 * recs_per_column); }
static inline size_t packed_cols_bytes(int B, int M, int recs_per_column) { return (size_t)B * (size_t)packed_stride(M, recs_per_column) * 16; }

// the Scratch booleans a plan reads
struct SplitFlags {
    bool ws;            // the call came with a workspace
    bool allow_split;   // no GLHIP_FLAG_NO_SPLIT
    bool force_pre;     // GLHIP_FLAG_PREPACK
    double prepack_min = kPrepackMinPairs;
    // pre-packed columns live in the workspace, which GLHIP_FLAG_NO_SPLIT tells us to leave alone
    bool prepack(double pairs) const { return ws && (force_pre || (allow_split && pairs >= prepack_min)); }
};

// One launch on a workspace of `bytes`: `rows` per workgroup of the main kernel, `partial` floats per row and split
struct SplitGeom {
    int n_ranges, B, N, M;
    int gx;             // dense launches: row blocks per batch item
    long row_blocks;    // what the split rules count: row blocks (not chunks) of block-sparse launches
    long per_split;     // bytes of workspace per column split
    long fit;           // column splits the workspace holds
    size_t bytes;       // the workspace
    SplitGeom(int n_ranges_, int B_, int N_, int M_, int rows, int partial, bool ws, size_t bytes_)
        : n_ranges(n_ranges_), B(B_), N(N_), M(M_), gx((N_ + rows - 1) / rows), bytes(bytes_) {
        row_blocks = n_ranges > 0 ? (long)n_ranges : (long)B * gx;
        per_split = (long)B * N * partial * sizeof(float);
        fit = (ws && per_split > 0) ? (long)(bytes / per_split) : 0;
    }
    double pairs() const { return (double)B * N * M; }
    // dense launches with room for 8 splits and enough columns for them may run on the XCD-aware 1-D grid (workgroup_coords) ...
    bool xcd_eligible(bool allow_split) const { return n_ranges == 0 && allow_split && fit >= 8 && M >= 65536; }
    // small clusters come with short column intervals: the block-sparse forward kernels gather them into full tiles
    int gather() const { return (n_ranges > 0 && N / n_ranges < 128) ? 1 : 0; }
    // byte offset in the workspace of what a launch places behind the partials of its splits (pre-packed columns)
    size_t packed_offset(int n_splits) const { return align256((size_t)(n_splits > 1 ? n_splits : 0) * per_split); }
};

// What a launch does with its workspace
struct SplitPlan {
    int n_splits = 1;           // 1 = no split
    bool xcd = false;           // the XCD-aware 1-D grid was taken
    int gather = 0, share = 0;  // SplitInfo's bits of the block-sparse forward kernels
    bool pre = false;           // pre-packed columns, at ...
    size_t packed_offset = 0, packed_bytes = 0;
    size_t bytes = 0;           // bytes of workspace the plan touches
};

// moves a plan to the XCD-aware grid with nx splits; a grid beyond 2^31 workgroups keeps what it has
static inline bool take_xcd(SplitPlan& p, const SplitGeom& g, int nx) {
    if ((long)g.gx * g.B * nx < (1L << 31)) { p.n_splits = nx; p.xcd = true; }
    return p.xcd;
}

// THE pre-pack placement: `packed_bytes` behind the split partials, where the launch wants them and they fit
static inline void place_packed(SplitPlan& p, const SplitGeom& g, bool want, size_t packed_bytes) {
    const size_t off = g.packed_offset(p.n_splits);
    p.pre = want && g.bytes >= off + packed_bytes;
    if (p.pre) { p.packed_offset = off; p.packed_bytes = packed_bytes; }
}

static inline SplitPlan plan_done(SplitPlan p, long per_split) {
    p.bytes = p.n_splits > 1 ? (size_t)p.n_splits * per_split : 0;
    if (p.pre && p.packed_offset + p.packed_bytes > p.bytes) p.bytes = p.packed_offset + p.packed_bytes;
    return p;
}

// ---- one plan function per distinct policy ------------------------------------------------------------------

// Rule only (launch_mapreduce, launch_dist, launch_dist_grad, launch_xk_l, launch_xk_dist, launch_dist_xd, launch_dist_xd_grad,
// launch_wsum_t32_rt); optionally the XCD-aware grid for `xcd_slots` resident workgroups (0: never), the small-launch rule of the distance
// kernels, the gather bit.
static inline SplitPlan plan_rule(const SplitGeom& g, bool allow_split, long xcd_slots = 0, bool small_dist = false, bool gather = false) {
    SplitPlan p;
    p.n_splits = rule_splits(g.row_blocks, g.M, g.n_ranges, g.fit, allow_split);
    if (small_dist) p.n_splits = dist_small_launch_splits(p.n_splits, g.row_blocks, g.M, g.fit, allow_split);
    if (gather) p.gather = g.gather();
    if (xcd_slots > 0 && g.xcd_eligible(allow_split)) take_xcd(p, g, xcd_splits(g.row_blocks, g.M, xcd_slots, g.fit));   // one column split per XCD at a time
    return plan_done(p, g.per_split);
}

// The x32 forward (launch_softmin_mfma_nw): `nw` wavefronts per workgroup, `nr` records per column (X32Layout<L>::NR), `share`: the chunk
// table was built in share mode.
static inline SplitPlan plan_x32_fwd(const SplitGeom& g, const SplitFlags& f, int nw, int nr, bool share) {
    SplitPlan p;
    // the number of column splits is derived from the number of row BLOCKS: deriving it from the (larger) chunk count
    // gives fewer, longer-lived workgroups and measured 3 % slower on uniform clusters (multiscale at 1e6: 258 vs 250 ms)
    p.n_splits = rule_splits(g.row_blocks, g.M, g.n_ranges, g.fit, f.allow_split);
    // block-sparse: small row clusters come with short column intervals (the reference's cluster_scale rule makes ~2000 clusters
    // whatever N is) — gather them into full tiles; clusters of hundreds of points already fill theirs
    p.gather = g.gather();
    p.share = share ? 1 : 0;
    // 2-wavefront workgroups (small clusters): 12 of them are resident per CU, three times the 4-wavefront case choose_splits is
    // tuned for — at least 6 splits (two-scale loss at N = 3e4 / 5e4 / 1e5: 2.11 / 3.01 / 5.30 -> 2.08 / 2.96 / 5.21 ms, three runs each)
    if (nw == 2 && g.n_ranges > 0 && f.allow_split && g.fit >= 6 && p.n_splits > 1 && p.n_splits < 6) p.n_splits = 6;
    // large dense problem: one column split per XCD at a time (workgroup_coords)
    const bool want_pre = f.prepack(g.pairs());
    if (g.xcd_eligible(f.allow_split))
        take_xcd(p, g, want_pre ? xcd_splits_prepacked(g.row_blocks, g.M, kFwdSlots, g.fit, nr * 16.0) : xcd_splits(g.row_blocks, g.M, kFwdSlots, g.fit));
    // launches with enough work to pay for one more (tiny) launch split the columns into MFMA records ONCE, behind the split partials
    place_packed(p, g, want_pre, packed_cols_bytes(g.B, g.M, nr));   // either layout fits: ceil(M / 32) whole groups hold the M records-of-NR of [M][NR]
    return plan_done(p, g.per_split);
}

// The weighted sums of D <= 3 (launch_wsum): `x32`: the launch runs wsum_x32_kernel, which takes packed records (`nr` per column) and
// `nq` q components per column behind them; the 16x16x32 kernel takes 8 splits on the XCD-aware grid and packs nothing.
static inline SplitPlan plan_wsum(const SplitGeom& g, const SplitFlags& f, bool x32, int nr, int nq) {
    SplitPlan p;
    p.n_splits = rule_splits(g.row_blocks, g.M, g.n_ranges, g.fit, f.allow_split);
    const bool want_pre = x32 && f.prepack(g.pairs());
    if (g.xcd_eligible(f.allow_split))   // one column split per XCD (workgroup_coords)
        take_xcd(p, g, !x32 ? 8 : want_pre ? xcd_splits_prepacked(g.row_blocks, g.M, kFwdSlots, g.fit) : xcd_splits(g.row_blocks, g.M, kFwdSlots, g.fit));
    if (x32) place_packed(p, g, want_pre, packed_cols_bytes(g.B, g.M, nr) + (size_t)nq * g.B * g.M * sizeof(float));
    return plan_done(p, g.per_split);
}

// 4 <= D <= 16 forward (launch_xd_cfg): `nw` wavefronts per workgroup, `nbp` records per column (XdShape<D, L>::NBP)
static inline SplitPlan plan_xd(const SplitGeom& g, const SplitFlags& f, int nw, int nbp) {
    SplitPlan p;
    p.n_splits = rule_splits(g.row_blocks, g.M, g.n_ranges, g.fit, f.allow_split);
    p.gather = g.gather();   // small clusters: gathered tiles, as in the x32 forward
    // pre-packed columns (glhip_softmin_xd.h): the records of all columns once, behind the split partials of at least 8 splits
    const size_t packed_bytes = packed_cols_bytes(g.B, g.M, nbp);
    const long fit_pre = (f.ws && g.bytes > packed_bytes + 256) ? (long)((g.bytes - packed_bytes - 256) / g.per_split) : 0;
    const bool pre = nw == 8 && f.prepack(g.pairs()) && fit_pre >= 8;      // (A/B knob GLHIP_XD_PRE of rounds 4-5: pre-packed columns won)
    // Packed columns that fit every XCD's L2 (<= 3.5 MB: M = 1e5 at 32 bytes per column) need no XCD-aware placement: any number
    // of splits, on the plain 3-D grid, chosen to fill the chip's rounds of resident workgroups (free_splits).  BASELINE config 2,
    // online N = M = 1e5: 13 splits instead of 32: 0.937 -> 0.896 ms per soft-min, 35.3 -> 34.2 ms per loss; N = 7e4: 0.489 -> 0.439 ms.
    // From M = 8192 (below 65536 the launch used to pack its columns per workgroup, on up to 32 splits: raw soft-mins at N = M = 5e4,
    // D = 4 / 5 / 8: 0.318 / 0.402 / 0.396 -> 0.280 / 0.303 / 0.300 ms).
    if (g.n_ranges == 0 && f.allow_split && pre && g.M >= 8192 && (double)g.M * nbp * 16.0 <= 3.5e6) {
        const long gxB = g.row_blocks;
        double eff_free = 0.0;
        const int nf = free_splits(gxB, g.M, kXdSlots, fit_pre, &eff_free);
        double eff_x = 0.0;
        if (g.M >= 65536) {
            const int nx8 = xcd_splits_prepacked(gxB, g.M, kXdSlots, fit_pre, nbp * 16.0);
            eff_x = ((double)gxB * nx8 / (double)kXdSlots) / (double)((gxB * nx8 + kXdSlots - 1) / kXdSlots);
        }
        if (nf >= 1 && eff_free > eff_x + 0.02) {
            p.n_splits = nf;
            place_packed(p, g, true, packed_bytes);
            return plan_done(p, g.per_split);
        }
    }
    if (g.xcd_eligible(f.allow_split)) {   // one column split per XCD at a time (workgroup_coords)
        const int nx = pre ? xcd_splits_prepacked(g.row_blocks, g.M, kXdSlots, fit_pre, nbp * 16.0) : xcd_splits(g.row_blocks, g.M, kXdSlots, g.fit);
        if (take_xcd(p, g, nx) && pre) place_packed(p, g, true, packed_bytes);
    }
    return plan_done(p, g.per_split);
}

// glhip_sinkhorn_iter4 / _extrapolate4: `count` dense reductions in one launch of a multi kernel (MultiSplit and the three launch_iter4*).
// Their geometry is that of one launch of the widest N against the narrowest M whose partial holds the 2 floats of every problem; the
// rules count the row blocks of all problems.
static inline SplitGeom multi_geom(int count, const int* N, const int* M, int B, int rows, bool ws, size_t bytes) {
    int maxN = 0, minM = M[0];
    long row_blocks = 0;
    for (int k = 0; k < count; ++k) {
        maxN = N[k] > maxN ? N[k] : maxN;
        minM = M[k] < minM ? M[k] : minM;
        row_blocks += (long)B * ((N[k] + rows - 1) / rows);
    }
    SplitGeom g(0, B, maxN, minM, rows, 2 * count, ws, bytes);
    g.row_blocks = row_blocks;
    return g;
}
enum MultiKind { MULTI_X32 = 0, MULTI_XD = 1, MULTI_DIST = 2 };

// `nr`, `offs`: MULTI_X32 only — records per column, and where each problem's packed records go
static inline SplitPlan plan_multi(const SplitGeom& g, const SplitFlags& f, int kind, int count, const int* N, const int* M, int nr = 0,
                                   size_t* offs = nullptr) {
    SplitPlan p;
    p.n_splits = rule_splits(g.row_blocks, g.M, 0, g.fit, f.allow_split);
    // the distance kernels: (no tiny-launch rule: p = 1 at N = M = 2000 runs 0.54 ms per loss with 3 splits, 0.84 ms with one) — the other way round
    if (kind == MULTI_DIST) p.n_splits = dist_small_launch_splits(p.n_splits, g.row_blocks, g.M, g.fit, f.allow_split);
    // the xd kernel: (no tiny-launch rule: N = M = 2000, D = 4 / 16 run 0.35 / 0.42 ms per loss with 3 splits, 0.43 / 0.58 ms with one)
    // (and more splits than the rule's do not pay either: 7 splits of 256 columns at N = M = 2000 measure like 3 — these loops are host-bound)
    if (kind != MULTI_X32) return plan_done(p, g.per_split);
    int maxM = 0;
    double pairs = 0.0;
    for (int k = 0; k < count; ++k) {
        maxM = M[k] > maxM ? M[k] : maxM;
        pairs += (double)g.B * N[k] * M[k];
    }
    // ... with at least 3 column tiles per split: a 128-row workgroup that runs one tile of 512 columns is mostly prologue and
    // epilogue (N = M = 1e4, 19 splits by the rule: 64 us per iteration; 6: 57 us; 2e4: 173 -> 166 us; 5e3 and 3e4: unchanged)
    if (g.M >= 3072 && g.M / p.n_splits < 1536) p.n_splits = g.M / 1536;
    // ... and none on tiny unbatched problems (rows x columns of one problem up to 5e6, measured): the launch takes as long either
    // way (N = M = 2000: 17.8 us with 3 splits + merge, 18.1 us with one), and a loop of such launches is bound by the host's launch
    // rate — the merge kernel is one launch in three
    if (g.B == 1 && (double)g.N * maxM <= 5e6) p.n_splits = 1;
    // Pre-packed columns (as in the x32 forward), from 1e8 pairs on: with 128-row workgroups every column is split into its bf16 pieces
    // (maxN / 128) times per problem; one more small launch does it once.  Measured (round 3): B x 4096^2 bf16 with B = 128 / 64 / 32
    // (the 2- / 4- / 8-GPU shards of configs[3]): 8.65 -> 8.28, 4.54 -> 4.35, 2.43 -> 2.32 ms per loss; N = M = 3e4: 4.07 -> 3.84 ms;
    // N = M = 1e4 and below: no difference (0.9 ms).
    const size_t first = g.packed_offset(p.n_splits);
    size_t off = first, end = first;
    p.pre = f.ws && f.allow_split && pairs >= 1e8;
    for (int k = 0; k < count && p.pre; ++k) {
        end = off + packed_cols_bytes(g.B, M[k], nr);
        p.pre = end <= g.bytes;
        if (offs) offs[k] = off;
        off = align256(end);
    }
    if (p.pre) { p.packed_offset = first; p.packed_bytes = end - first; }
    return plan_done(p, g.per_split);
}

// ---- the workspace size (glhip_workspace_bytes) ----------------------------------------------------------------

// the most splits a rule asks of a launch with `rows`-row workgroups, whatever the workspace
static inline long sized_row_blocks(int B, int N, int n_ranges, int rows) { return n_ranges > 0 ? (long)n_ranges : (long)B * ((N + rows - 1) / rows); }
static inline int want_rule(int B, int N, int M, int n_ranges, int rows) { return choose_splits(sized_row_blocks(B, N, n_ranges, rows), M, n_ranges, 1L << 30); }
static inline int want_xcd(int B, int N, int M, int rows, long slots) { return xcd_splits(sized_row_blocks(B, N, 0, rows), M, slots, 32); }
static inline int want_xcd_prepacked(int B, int N, int M, int rows, long slots) { return xcd_splits_prepacked(sized_row_blocks(B, N, 0, rows), M, slots, 32); }
// `ns` splits of `floats` per row
static inline size_t partial_bytes(int ns, int B, int N, int floats) { return (size_t)(ns < 2 ? 0 : ns) * (size_t)B * (size_t)N * (size_t)floats * sizeof(float); }
template <class T> static inline T max_of(std::initializer_list<T> v) { T m = 0; for (T x : v) m = x > m ? x : m; return m; }

// What the forward, half-step, product and D <= 16 gradient launches of one call split into, the sorted calls' own buffers aside
// (glhip_autosort.h): per dimension range the largest of a short list of candidates, each a launcher shape under a rule above.
// `x32_nr` = X32Layout<XL_BF16X3>::NR, `xd_nbp` = XdShape<D>::NBP (4 <= D <= 16).  The value decides what every launch does and is
// pinned (tests/test_workspace_bytes_cpu.py): a candidate changes only with timings on an MI355X.  Launcher configurations the lists
// leave out run capped; they are listed in profiles/split_policy_caps.txt.
static inline size_t forward_workspace_bytes(int B, int N, int M, int D, int n_ranges, int x32_nr, int xd_nbp) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 1 || D > kSizedMaxD) return 0;   // the generic-D kernels do not split
    const bool dense = n_ranges == 0, xcd = dense && M >= 65536;
    // row-chunk table of block-sparse launches (64-row tiles: the smallest)
    const size_t table = dense ? 0 : chunk_table_bytes(n_ranges, N, kChunkRowsMin);
    if (D > kXdMaxD) {   // 17 <= D <= 4095: split partials of 2 floats per row — what launch_xk_l takes, nothing else
        const int nf = max_of({want_rule(B, N, M, n_ranges, kRowsXk), xcd ? want_xcd(B, N, M, kRowsXk, kXkSlots) : 0});
        return partial_bytes(nf, B, N, 2) + table;
    }
    if (D > 3) {   // 4 <= D <= 16
        // forward (launch_xd_cfg, launch_dist_xd), 2 floats per row: the rule at 128 rows, the XCD grid at 256 and 512
        // (missing: the rule at 256 and 512 rows — the 512-row shape of big launches; profiles/split_policy_caps.txt)
        int nf = max_of({want_rule(B, N, M, n_ranges, kRowsNW4), xcd ? want_xcd(B, N, M, kRowsNW8, kXdSlots) : 0,
                         xcd ? want_xcd(B, N, M, kRowsNW8x2, kXdSlots) : 0});
        // small dense launches of the distance kernels split further
        if (dense) nf = dist_small_launch_splits(nf, sized_row_blocks(B, N, 0, kRowsNW8), M, 32, true);
        const size_t fwd = partial_bytes(nf, B, N, 2);
        // gradient kernels (glhip_wsum_t32.h, launch_dist_xd_grad; 256-row blocks): up to D + 1 floats per row
        const size_t grad = partial_bytes(max_of({want_rule(B, N, M, n_ranges, kRowsNW8), xcd ? want_xcd(B, N, M, kRowsNW8, kXdSlots) : 0}), B, N, D + 1);
        // forward, big dense launches: up to 32 splits (one split's records per XCD L2) + the pre-packed column records
        // (missing: pre-packed launches of 8192 <= M < 65536 under the free-split rule; profiles/split_policy_caps.txt)
        const size_t pre = (xcd && (double)B * N * M >= kPrepackMinPairs) ? partial_bytes(32, B, N, 2) + 256 + packed_cols_bytes(B, M, xd_nbp) : 0;
        return max_of({fwd, grad, pre}) + table;
    }
    // D <= 3
    // the VALU skeleton (launch_mapreduce, two rows per thread) and the distance kernels: the widest partial is D + 1 floats;
    // the XCD-aware grids want 8 splits
    const int ns = want_rule(B, N, M, n_ranges, kRowsValu2);
    const size_t valu = max_of({partial_bytes(ns, B, N, D + 1), xcd ? partial_bytes(8, B, N, D + 1) : 0});
    // forward (launch_softmin_mfma_nw, 128- and 256-row workgroups): 2 floats per row + the packed column records
    const int nf = !dense ? ns
                          : max_of({want_rule(B, N, M, 0, kRowsNW4), want_rule(B, N, M, 0, kRowsNW8),
                                    xcd ? want_xcd_prepacked(B, N, M, kRowsNW4, kFwdSlots) : 0, xcd ? want_xcd_prepacked(B, N, M, kRowsNW8, kFwdSlots) : 0});
    const size_t fwd = partial_bytes(nf, B, N, 2) + 256 + packed_cols_bytes(B, M, x32_nr);
    // weighted-sum kernels (launch_wsum: soft-min gradient, gaussian product / gradient): up to D + 1 floats per row
    // + packed records + up to kMaxPackedQ q components per column
    const int nw = max_of({ns, xcd ? want_xcd_prepacked(B, N, M, kRowsNW8, kFwdSlots) : 0});
    const size_t wsum = partial_bytes(nw, B, N, D + 1) + 256 + packed_cols_bytes(B, M, x32_nr) + (size_t)kMaxPackedQ * B * M * sizeof(float);
    return max_of({valu, fwd, wsum}) + table;
}

}  // namespace glhip
