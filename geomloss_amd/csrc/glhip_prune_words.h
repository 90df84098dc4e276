// glhip_prune_words.h — the kept column blocks of a slab as a bit set, and its pieces for a gap length g, one 64-bit word at a time
// (prune_slabs_kernel, glhip_prune.hip; the rule itself: glhip_autosort.h).  Word w holds the blocks 64 w ... 64 w + 63, bit b set =
// block 64 w + b is kept; bits from nT on are 0.  A piece starts at a kept block that opens a run (the first kept block, or one with
// at least g blocks that are not kept in front of it: g = 1, its predecessor is not kept) or that is a multiple of PB (a cut on the
// piece grid, on the kept bits as they are, also inside a run that closed a gap); it ends where the next piece starts, or behind the
// last kept block before a run.  g itself is one more than the kPruneRuns-th longest gap (prune_gap_lengths, prune_gap_select).
// Plain C++, no HIP types: the host tests compile it alone and run it against the block-by-block walk.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GLHIP_HD __host__ __device__
#else
#define GLHIP_HD
#endif

namespace glhip {

GLHIP_HD inline int prune_popc(unsigned long long v) { return __builtin_popcountll(v); }

// one past the last kept block among the words [0, w] below bit b of word w (b = 64: all of word w); 0 if there is none
GLHIP_HD inline int prune_kept_end(const unsigned long long* mask, int w, int b) {
    unsigned long long below = b >= 64 ? mask[w] : mask[w] & ((1ull << b) - 1ull);
    while (!below) {
        if (w == 0) return 0;
        below = mask[--w];
    }
    return 64 * w + 64 - __builtin_clzll(below);
}

// run / start bits of word w for gap length g.  PB >= 64 (prune_plan): at most one multiple of PB per word.  g = 1: a kept block whose
// predecessor is not kept opens a run, from this word and the top bit of the one before alone; g > 1 drops those of them that have a
// kept block fewer than g blocks in front (the gap between the two is closed).
GLHIP_HD inline void prune_word_starts(const unsigned long long* mask, int w, int PB, int g, unsigned long long& run,
                                       unsigned long long& start) {
    const unsigned long long m = mask[w];
    run = m & ~((m << 1) | (w > 0 ? mask[w - 1] >> 63 : 0ull));
    if (g > 1) {
        for (unsigned long long r = run; r; r &= r - 1ull) {
            const int b = __builtin_ctzll(r), end = prune_kept_end(mask, w, b);
            if (end > 0 && 64 * w + b - end < g) run &= ~(1ull << b);
        }
    }
    const long long first = 64LL * w, t0 = ((first + PB - 1) / PB) * PB;
    const unsigned long long grid = t0 < first + 64 ? 1ull << (t0 - first) : 0ull;
    start = run | (m & grid);
}

// runs and pieces that start in the words [w0, w1)
GLHIP_HD inline void prune_count_words(const unsigned long long* mask, int w0, int w1, int PB, int& runs, int& pieces, int g = 1) {
    runs = 0;
    pieces = 0;
    for (int w = w0; w < w1; ++w) {
        unsigned long long run, start;
        prune_word_starts(mask, w, PB, g, run, start);
        runs += prune_popc(run);
        pieces += prune_popc(start);
    }
}

// The gaps in front of the runs (g = 1) that start in the words [w0, w1): the k-th run of the slab, k = idx0, idx0 + 1, ... (idx0: the
// runs that start before word w0), has the blocks that are not kept between it and the kept block before; their number goes to
// gaps[k - 1].  The slab's first run has no gap.  Lengths from index `cap` on are not written.
GLHIP_HD inline void prune_gap_lengths(const unsigned long long* mask, int w0, int w1, int idx0, int cap, int32_t* gaps) {
    int idx = idx0;
    for (int w = w0; w < w1; ++w) {
        const unsigned long long m = mask[w];
        for (unsigned long long r = m & ~((m << 1) | (w > 0 ? mask[w - 1] >> 63 : 0ull)); r; r &= r - 1ull, ++idx) {
            if (idx == 0 || idx - 1 >= cap) continue;
            const int b = __builtin_ctzll(r);
            gaps[idx - 1] = 64 * w + b - prune_kept_end(mask, w, b);
        }
    }
}

// The gap length for a limit of `runs` runs: the smallest g with 1 + #{gaps >= g} <= runs, that is one more than the runs-th longest
// gap (1 if there are fewer).  Serial: the rule; prune_slabs_kernel finds the same g with one count over the workgroup per step.
GLHIP_HD inline int prune_gap_select(const int32_t* gaps, int n, int runs, int nT) {
    int lo = 0, hi = nT;      // lo leaves too many runs (0: not a gap length), hi does not (no gap has nT blocks: one run)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        int c = 0;
        for (int q = 0; q < n; ++q) c += gaps[q] >= mid;
        if (1 + c > runs) lo = mid; else hi = mid;
    }
    return hi;
}

// The pieces that start in the words [w0, w1), numbered from idx0 (the pieces that start before word w0), into slots[2 idx] (first
// column) and slots[2 idx - 1] (end of the piece before; columns are blocks x C, ends clipped to M).  Pieces from S on are not written.
GLHIP_HD inline void prune_emit_words(const unsigned long long* mask, int w0, int w1, int idx0, int PB, int S, int C, int M, int32_t* slots,
                                      int g = 1) {
    int idx = idx0;
    for (int w = w0; w < w1; ++w) {
        unsigned long long run, start;
        prune_word_starts(mask, w, PB, g, run, start);
        for (; start; start &= start - 1ull, ++idx) {
            if (idx >= S) continue;
            const int b = __builtin_ctzll(start), t = 64 * w + b;
            slots[2 * idx] = t * C;
            if (idx == 0) continue;
            // a cut on the grid: the piece before ends where this one starts; a run: behind the last kept block before it
            const long long end = (long long)(((run >> b) & 1ull) ? prune_kept_end(mask, w, b) : t) * C;
            slots[2 * idx - 1] = (int32_t)(end < M ? end : M);
        }
    }
}

// end of the last piece written (n = min(pieces, S) > 0 of them): behind the last kept block of all nW words
GLHIP_HD inline void prune_emit_last(const unsigned long long* mask, int nW, int n, int C, int M, int32_t* slots) {
    const long long end = (long long)prune_kept_end(mask, nW - 1, 64) * C;
    slots[2 * n - 1] = (int32_t)(end < M ? end : M);
}

}  // namespace glhip
