// split_policy_cases.cpp — a stand-alone host program around geomloss_amd/csrc/glhip_split_policy.h (no HIP, no device): every plan function
// over the grid of shapes of tests/golden/make_golden_workspace_bytes.py.
//
//   split_policy_cases check    (tests/test_split_policy_cpu.py) every plan under four workspaces per shape — the size the sizing rule
//       gives (forward_workspace_bytes, from the same header; 4 x for the multi launches, as their callers ask), half of it, 4096 bytes
//       and none — and under every combination of the Scratch booleans: the memory bounds of a split launch.  Prints one line per
//       violation, then "plans <count> violations <count>".
//   split_policy_cases report   (tools/split_policy_report.py) for the configuration a launcher takes at each shape under default flags:
//       the plan under the sized workspace next to the plan under an unlimited one, wherever they differ.
//
// Two things are restated here because their headers are not plain C++: the records per column of the K layouts (XdShape<D, L>::NBP,
// X32Layout<L>::NR; glhip_klayout.h, glhip_softmin_x32.h) and, for the report only, which workgroup shape a launcher picks (launch_softmin_mfma,
// launch_xd_l; glhip_launch.h).
#include <cstdio>
#include <cstring>
#include <string>

#include "glhip_split_policy.h"

using namespace glhip;

static int xd_nbp(int D, int f16) { return 2 * ((6 + (f16 ? 3 : 6) * D + 15) / 16); }   // XdShape<D, L>::NBP
static int x32_nr(int f16) { return f16 ? 2 : 4; }                                       // X32Layout<L>::NR

static const int kB[] = {1, 4, 64, 256};
static const int kNM[] = {1, 127, 128, 1000, 4096, 16384, 16385, 32768, 65535, 65536, 100000, 300000, 1000000};
static const int kD[] = {1, 2, 3, 4, 5, 8, 12, 16, 17, 64, 4095, 4096};
static const int kRanges[] = {0, 1, 7, 2000};

struct Shape { int B, N, M, D, n_ranges; };
struct Checked { SplitPlan p; long per_split; bool dense; int M; };

static bool g_report = false;
static long g_plans = 0, g_violations = 0;

static void violation(const char* what, const char* policy, const std::string& cfg, const Shape& s, size_t bytes, const SplitFlags& f, const Checked& c) {
    ++g_violations;
    std::printf("VIOLATION %s: %s %s B=%d N=%d M=%d D=%d ranges=%d bytes=%zu allow=%d force_pre=%d -> splits=%d xcd=%d pre=%d off=%zu packed=%zu per_split=%ld\n",
                what, policy, cfg.c_str(), s.B, s.N, s.M, s.D, s.n_ranges, bytes, (int)f.allow_split, (int)f.force_pre, c.p.n_splits, (int)c.p.xcd,
                (int)c.p.pre, c.p.packed_offset, c.p.packed_bytes, c.per_split);
}

static void check(const char* policy, const std::string& cfg, const Shape& s, size_t bytes, const SplitFlags& f, const Checked& c) {
    ++g_plans;
    const SplitPlan& p = c.p;
    // (a launch on one split writes no partial: its packed columns may start at the front of the workspace)
    const size_t partials = p.n_splits > 1 ? (size_t)p.n_splits * c.per_split : 0;
    if (p.n_splits < 1) violation("n_splits < 1", policy, cfg, s, bytes, f, c);
    if (partials > bytes) violation("partials beyond the workspace", policy, cfg, s, bytes, f, c);
    if (p.xcd && !(c.dense && c.M >= 65536 && p.n_splits % 8 == 0)) violation("XCD grid", policy, cfg, s, bytes, f, c);
    if (p.pre && !(p.packed_offset >= partials && p.packed_offset % 256 == 0 && p.packed_offset + p.packed_bytes <= bytes))
        violation("packed columns", policy, cfg, s, bytes, f, c);
    if (p.bytes > bytes) violation("touches more than the workspace", policy, cfg, s, bytes, f, c);
    if (bytes == 0 && (p.n_splits != 1 || p.pre)) violation("no workspace", policy, cfg, s, bytes, f, c);
    if (!f.allow_split && p.n_splits != 1) violation("GLHIP_FLAG_NO_SPLIT", policy, cfg, s, bytes, f, c);
}

// what make_scratch leaves of a block-sparse call's workspace behind the row-chunk table
static size_t behind_table(size_t bytes, const Shape& s, bool small_rows) {
    if (s.n_ranges == 0 || bytes == 0) return bytes;
    const int rows = chunk_table_rows(bytes, s.n_ranges, s.N, small_rows);
    return rows ? bytes - chunk_table_bytes(s.n_ranges, s.N, rows) : bytes;
}

// `make(bytes, flags)`: the plan of one launcher configuration on a workspace of `bytes`; `sized`: what the caller allocates;
// `taken`: the launcher picks this configuration at this shape under default flags (the report lists only those)
template <class F>
static void run(const char* policy, const std::string& cfg, const Shape& s, size_t sized, bool small_rows, bool taken, F&& make) {
    if (g_report) {
        if (!taken) return;
        const size_t w = behind_table(sized, s, small_rows);
        const Checked a = make(w, SplitFlags{w > 0, true, false}), b = make((size_t)1 << 42, SplitFlags{true, true, false});
        ++g_plans;
        if (a.p.n_splits == b.p.n_splits && a.p.xcd == b.p.xcd && a.p.pre == b.p.pre) return;
        ++g_violations;
        std::printf("%-12s %-22s B=%-3d N=%-7d M=%-7d D=%-4d ranges=%-4d bytes=%-11zu sized: splits=%-2d xcd=%d pre=%d | unlimited: splits=%-2d xcd=%d pre=%d\n",
                    policy, cfg.c_str(), s.B, s.N, s.M, s.D, s.n_ranges, sized, a.p.n_splits, (int)a.p.xcd, (int)a.p.pre, b.p.n_splits, (int)b.p.xcd, (int)b.p.pre);
        return;
    }
    const size_t sizes[4] = {sized, sized / 2, 4096, 0};
    for (size_t whole : sizes) {
        const size_t w = behind_table(whole, s, small_rows);
        for (int flags = 0; flags < 4; ++flags) {
            const SplitFlags f{w > 0, (flags & 1) == 0, (flags & 2) != 0};
            check(policy, cfg, s, w, f, make(w, f));
        }
    }
}

static std::string cfg(const char* fmt, int a = 0, int b = 0, int c = 0) {
    char buf[64];
    std::snprintf(buf, sizeof buf, fmt, a, b, c);
    return buf;
}

static void single_launches(const Shape& s) {
    const int B = s.B, N = s.N, M = s.M, D = s.D, nr = s.n_ranges;
    const bool dense = nr == 0;
    const size_t sized = forward_workspace_bytes(B, N, M, D, nr, x32_nr(0), D > 3 && D <= kXdMaxD ? xd_nbp(D, 0) : 0);
    const double pairs = (double)B * N * M;
    const bool big = pairs >= kPrepackMinPairs && (dense ? (long)B * N >= 32768 : N / nr >= 192);
    auto rule = [&](const char* name, int rows, int partial, long slots, bool small, bool gather, bool taken) {
        run("rule", cfg(name, rows, partial), s, sized, false, taken, [&](size_t w, const SplitFlags& f) {
            const SplitGeom g(nr, B, N, M, rows, partial, f.ws, w);
            return Checked{plan_rule(g, f.allow_split, slots, small, gather), g.per_split, dense, M};
        });
    };
    if (D <= 3) {
        // launch_mapreduce: one or two rows per thread (use_two_rows), partials of 2 (forward) and D + 1 floats
        const bool two = !dense || ((sized > 0) ? (long)B * N >= 4 * 256 : (long)B * ((N + 511) / 512) >= 1024);
        for (int rows = 256; rows <= 512; rows *= 2)
            for (int partial : {2, D + 1}) rule("valu rows=%d part=%d", rows, partial, 0, false, false, two == (rows == 512));
        if (!dense) {      // launch_dist, launch_dist_grad: block-sparse, B = 1
            rule("dist rows=%d part=%d", 256, 2, 0, false, false, true);
            rule("dist_grad rows=%d part=%d", 256, D + 1, 0, false, false, true);
        }
        // launch_softmin_mfma_nw: 2 (block-sparse only), 4 or 8 wavefronts, both layouts, share mode where it exists
        for (int l = 0; l < 2; ++l)
            for (int nw = dense ? 4 : 2; nw <= 8; nw *= 2)
                for (int share = 0; share <= (nw == 4 && l == 1 && !dense ? 1 : 0); ++share) {
                    const bool small_rows = nw == 2;
                    const bool taken = l == 0 && share == 0 && nw == (big ? 8 : 4);
                    run("x32_fwd", cfg("nw=%d f16=%d share=%d", nw, l, share), s, sized, small_rows, taken, [&](size_t w, const SplitFlags& f) {
                        const SplitGeom g(nr, B, N, M, nw * 32, 2, f.ws, w);
                        return Checked{plan_x32_fwd(g, f, nw, x32_nr(l), share != 0), g.per_split, dense, M};
                    });
                }
        // launch_wsum: the x32 gaussian product (1 float per row, 1 q component) and the 16x16x32 kernels (up to D + 1 of each)
        for (int x32 = 0; x32 < 2; ++x32)
            run("wsum", cfg("x32=%d", x32), s, sized, false, true, [&](size_t w, const SplitFlags& f) {
                const SplitGeom g(nr, B, N, M, kRowsNW8, x32 ? 1 : D + 1, f.ws, w);
                return Checked{plan_wsum(g, f, x32 != 0, x32_nr(0), x32 ? 1 : D + 1), g.per_split, dense, M};
            });
    }
    if (D <= kXdMaxD) {
        // launch_xd_cfg: 4 <= D <= 16 on either layout, D <= 3 on f16 x 2 (big dense launches); the three workgroup shapes
        for (int l = D <= 3 ? 1 : 0; l < 2; ++l) {
            const int nm = xd_nbp(D, l) / 2;
            const int rt_big = nm <= 4 || (nm == 5 && dense) ? 2 : 1;
            for (int shape = 0; shape < 3; ++shape) {
                const int rt = shape == 2 ? 2 : 1, nw = shape == 0 ? 4 : 8;
                const bool taken = D > 3 && l == 0 && (big ? nw == 8 && rt == rt_big : nw == 4);
                for (int partial = 1; partial <= 2; ++partial)
                    run("xd", cfg("rows=%d part=%d f16=%d", rt * nw * 32, partial, l), s, sized, false, taken, [&](size_t w, const SplitFlags& f) {
                        const SplitGeom g(nr, B, N, M, rt * nw * 32, partial, f.ws, w);
                        return Checked{plan_xd(g, f, nw, xd_nbp(D, l)), g.per_split, dense, M};
                    });
            }
        }
    }
    if (D > 3 && D <= kXdMaxD) {
        if (dense) {
            rule("dist_xd rows=%d part=%d", 256, 2, 0, true, false, true);            // launch_dist_xd
            rule("dist_xd_grad rows=%d part=%d", 256, D + 1, 0, false, false, true);  // launch_dist_xd_grad
        }
        rule("wsum_t32 rows=%d part=%d", kRowsNW8, D + 1, kXdSlots, false, false, true);   // launch_wsum_t32_rt
    }
    if (D > kXdMaxD && D <= kSizedMaxD) {
        rule("xk rows=%d part=%d", kRowsXk, 2, kXkSlots, false, true, true);               // launch_xk_l
        if (dense) rule("xk_dist rows=%d part=%d", kRowsXk, 2, kXkSlots, false, false, true);   // launch_xk_dist
    }
}

// glhip_sinkhorn_iter4 on (x, y): four problems (N x M, M x N, N x N, M x M) on 4 x the workspace of the larger cloud against itself
static void multi_launches(const Shape& s) {
    if (s.n_ranges > 0 || s.D > kXdMaxD) return;
    const int L = s.N > s.M ? s.N : s.M;
    const size_t sized = 4 * forward_workspace_bytes(s.B, L, L, s.D, 0, x32_nr(0), s.D > 3 ? xd_nbp(s.D, 0) : 0);
    const int Ns[4] = {s.N, s.M, s.N, s.M}, Ms[4] = {s.M, s.N, s.N, s.M};
    auto multi = [&](const char* name, int kind, int rows, int l, bool taken) {
        run("multi", cfg(name, rows, l), s, sized, false, taken, [&](size_t w, const SplitFlags& f) {
            const SplitGeom g = multi_geom(4, Ns, Ms, s.B, rows, f.ws, w);
            size_t offs[4];
            return Checked{plan_multi(g, f, kind, 4, Ns, Ms, x32_nr(l), offs), g.per_split, true, g.M};
        });
    };
    if (s.D <= 3)
        for (int l = 0; l < 2; ++l) multi("x32 rows=%d f16=%d", MULTI_X32, kRowsNW4, l, l == 0);
    else
        multi("xd rows=%d", MULTI_XD, kRowsNW4, 0, true);
    multi("dist rows=%d", MULTI_DIST, kRowsNW8, 0, true);
}

int main(int argc, char** argv) {
    if (argc != 2 || (std::strcmp(argv[1], "check") && std::strcmp(argv[1], "report"))) {
        std::fprintf(stderr, "usage: %s check|report\n", argv[0]);
        return 2;
    }
    g_report = !std::strcmp(argv[1], "report");
    long shapes = 0;
    for (int nr : kRanges)
        for (int B : kB) {
            if (nr > 0 && B != 1) continue;
            for (int N : kNM)
                for (int M : kNM)
                    for (int D : kD) {
                        const Shape s{B, N, M, D, nr};
                        single_launches(s);
                        multi_launches(s);
                        ++shapes;
                    }
        }
    if (g_report) std::printf("shapes %ld plans %ld capped %ld\n", shapes, g_plans, g_violations);
    else std::printf("shapes %ld plans %ld violations %ld\n", shapes, g_plans, g_violations);
    return 0;
}
