// glhip_prune_words.h — the kept column blocks of a slab as a bit set, and its pieces for gap length g = 1, one 64-bit word at a time
// (prune_slabs_kernel, glhip_cluster.hip; the rule itself: glhip_autosort.h).  Word w holds the blocks 64 w ... 64 w + 63, bit b set =
// block 64 w + b is kept; bits from nT on are 0.  A piece starts at a kept block whose predecessor is not kept (a run) or that is a
// multiple of PB (a cut on the piece grid); it ends where the next piece starts, or behind the last kept block before a run.
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

// run / start bits of word w (prev63: bit 63 of word w - 1, 0 for w = 0).  PB >= 64 (prune_plan): at most one multiple of PB per word
GLHIP_HD inline void prune_word_starts(unsigned long long m, unsigned long long prev63, int w, int PB, unsigned long long& run,
                                       unsigned long long& start) {
    run = m & ~((m << 1) | (prev63 & 1ull));
    const long long first = 64LL * w, t0 = ((first + PB - 1) / PB) * PB;
    const unsigned long long grid = t0 < first + 64 ? 1ull << (t0 - first) : 0ull;
    start = run | (m & grid);
}

// runs and pieces that start in the words [w0, w1)
GLHIP_HD inline void prune_count_words(const unsigned long long* mask, int w0, int w1, int PB, int& runs, int& pieces) {
    runs = 0;
    pieces = 0;
    for (int w = w0; w < w1; ++w) {
        unsigned long long run, start;
        prune_word_starts(mask[w], w > 0 ? mask[w - 1] >> 63 : 0ull, w, PB, run, start);
        runs += prune_popc(run);
        pieces += prune_popc(start);
    }
}

// one past the last kept block among the words [0, w] below bit b of word w (b = 64: all of word w); 0 if there is none
GLHIP_HD inline int prune_kept_end(const unsigned long long* mask, int w, int b) {
    unsigned long long below = b >= 64 ? mask[w] : mask[w] & ((1ull << b) - 1ull);
    while (!below) {
        if (w == 0) return 0;
        below = mask[--w];
    }
    return 64 * w + 64 - __builtin_clzll(below);
}

// The pieces that start in the words [w0, w1), numbered from idx0 (the pieces that start before word w0), into slots[2 idx] (first
// column) and slots[2 idx - 1] (end of the piece before; columns are blocks x C, ends clipped to M).  Pieces from S on are not written.
GLHIP_HD inline void prune_emit_words(const unsigned long long* mask, int w0, int w1, int idx0, int PB, int S, int C, int M, int32_t* slots) {
    int idx = idx0;
    for (int w = w0; w < w1; ++w) {
        const unsigned long long m = mask[w];
        unsigned long long run, start;
        prune_word_starts(m, w > 0 ? mask[w - 1] >> 63 : 0ull, w, PB, run, start);
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
