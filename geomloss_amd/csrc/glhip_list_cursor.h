// glhip_list_cursor.h — how the list-driven sweep (glhip_softmin_list.h) walks a slab's column intervals: interval slots q_begin +
// split, + n_splits, ... < q_end of Ranges::redranges_j (the column splits take a slab's intervals round robin), every interval a
// piece of whole blocks of 256 sorted columns [j0, je) (je a multiple of 32 or the cloud's end), cut into batches of up to 64
// consecutive groups of 32 columns; within a batch the kept groups are taken in ascending order from a 64-bit keep set.
// Plain C++, no HIP types: the host test compiles it alone and plays it against a serial walk.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GLHIP_LIST_HD __host__ __device__
#else
#define GLHIP_LIST_HD
#endif

namespace glhip {

constexpr int kListBatch = 64;      // groups per batch: one lane per group, one ballot

struct ListCursor {
    int q, j0, je;      // interval slot, next column, end of the interval; q >= q_end: no more batches
};

// skip empty intervals from slot c.q on
GLHIP_LIST_HD inline void list_open(const int32_t* redranges_j, int q_end, int ns, ListCursor& c) {
    while (c.q < q_end) {
        const int js = redranges_j[2 * c.q], je = redranges_j[2 * c.q + 1];
        if (js < je) {
            c.j0 = js;
            c.je = je;
            return;
        }
        c.q += ns;
    }
}

GLHIP_LIST_HD inline ListCursor list_begin(const int32_t* redranges_j, int q_begin, int q_end, int split, int ns) {
    ListCursor c{q_begin + split, 0, 0};
    list_open(redranges_j, q_end, ns, c);
    return c;
}

// the batch at c (c.q < q_end): its first group g0 and its number of groups ng in [1, 64]; returns the cursor behind it
GLHIP_LIST_HD inline ListCursor list_next(const int32_t* redranges_j, int q_end, int ns, const ListCursor& c, int& g0, int& ng) {
    g0 = c.j0 >> 5;
    const int left = (c.je - c.j0 + 31) >> 5;
    ng = left < kListBatch ? left : kListBatch;
    ListCursor n = c;
    n.j0 += kListBatch * 32;
    if (n.j0 >= n.je) {
        n.q += ns;
        list_open(redranges_j, q_end, ns, n);
    }
    return n;
}

// Which sweep takes a launch.  The sorted p = 2 launch on the f16 x 2 layout starts two kernels on one grid, the list-driven sweep
// (glhip_softmin_list.h) and the staged one (glhip_softmin_x32.h, P2); one wavefront evaluates this rule in front of them
// (list_decide, glhip_prune.hip), and all workgroups of the kernel it does not name return at once.  The list-driven sweep reads one
// operand per wavefront and group through L2, the staged one per workgroup: four times the L2 traffic (measured:
// profiles/list_sweep.txt).  That pays where
// the staged kernel's per-tile test and barriers buy little — the first level keeps a small share of the columns, and the second
// keeps half of a tile's groups — and loses where most groups of a tile are kept anyway.  A launch whose slabs have no home block runs
// no test in either kernel and all its workgroups sweep the columns in one order (L2 hits): the list-driven sweep wins again.
// The decision is for the whole launch, never per slab: two kernels that each sweep a part of the slabs run one after the other,
// each with its own tail, and lose to either kernel alone (measured).  The statistic: kListRefSlabs reference slabs spread evenly
// over the sorted rows — `kept`: the columns of all their intervals, `cols` = kListRefSlabs M, `all_free`: none of them has a home block.
constexpr int kListRefSlabs = 8;
constexpr int kListKeepPct = 30;      // bench law at 1e6: mean share 0.229 at eps = 0.05^2 (list-driven: -0.8 ms), 0.389 at 0.07^2 (+0.7 ms)
GLHIP_LIST_HD inline int list_ref_slab(int k, int n_slabs) {
    const long long s = ((long long)(2 * k + 1) * n_slabs) / (2 * kListRefSlabs);
    return s < n_slabs ? (int)s : n_slabs - 1;
}
GLHIP_LIST_HD inline bool list_takes_launch(bool all_free, long long kept, long long cols, int pct) {
    return all_free || kept * 100 <= cols * pct;
}

// lanes [0, ng) of a batch
GLHIP_LIST_HD inline unsigned long long list_lanes(int ng) { return ng >= 64 ? ~0ull : (1ull << ng) - 1ull; }

GLHIP_LIST_HD inline int list_clamp(int g, int glast) { return g < 0 ? 0 : (g > glast ? glast : g); }

// the next kept group of the batch, taken out of `todo`; past the last one: the batch's first group (loaded by the ring's prefetch,
// never consumed).  Always inside [0, glast].
GLHIP_LIST_HD inline int list_pop(unsigned long long& todo, int g0, int glast) {
    const int g = g0 + (todo ? __builtin_ctzll(todo) : 0);
    todo &= todo - 1ull;
    return list_clamp(g, glast);
}

}  // namespace glhip
