// glhip_balance.h — the balancing pass of the sorted p = 2 call (balance_kernel, glhip_compact_sort.hip; why: glhip_autosort.h).  Every whole
// aligned block of kBalanceBlock positions of the path order is split like a k-d tree: five levels with segments of 1024, 512, 256,
// 128 and 64 points; a segment is sorted by (coordinate on its own longest axis, position the point had in the block), so its halves
// are the two sides of a median cut.  The pieces here are what the kernel and the CPU model (tools/prune_model.py: balanced_order)
// must agree on: the order of the coordinates, the axis rule, the sort word and the direction rule of the bitonic network.
// Plain C++, no HIP types: the host tests compile it alone and run it against a serial sort.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GLHIP_HD __host__ __device__
#else
#define GLHIP_HD
#endif

namespace glhip {

GLHIP_HD inline unsigned balance_bits(float f) {
    unsigned b;
    __builtin_memcpy(&b, &f, 4);
    return b;
}
GLHIP_HD inline bool balance_finite(float f) { return (balance_bits(f) & 0x7F800000u) != 0x7F800000u; }

// order-preserving image of a float: -inf < ... < -0 < +0 < ... < +inf < every NaN (either sign, any payload: one value)
GLHIP_HD inline unsigned balance_key(float f) {
    const unsigned b = balance_bits(f);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// what a segment is sorted by: the key, then the position the point had in the incoming block (< 2^32): no two words are equal
GLHIP_HD inline unsigned long long balance_word(unsigned key, unsigned pos) { return ((unsigned long long)key << 32) | pos; }

// one point of a segment into the running extent of one coordinate (start: lo = +inf, hi = -inf); non-finite values take no part
GLHIP_HD inline void balance_extent_add(float v, float& lo, float& hi) {
    if (!balance_finite(v)) return;
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
}

// the axis a segment is cut along: the largest extent hi - lo over the finite values (float32; a difference that overflows is +inf),
// ties to the lowest axis; an axis without a finite value loses to every other; none at all: axis 0
GLHIP_HD inline int balance_axis(const float* lo, const float* hi, int D) {
    int axis = 0;
    float best = -1.f;
    for (int d = 0; d < D; ++d) {
        const float e = lo[d] <= hi[d] ? hi[d] - lo[d] : -1.f;
        if (e > best) { best = e; axis = d; }
    }
    return axis;
}

// Bitonic network over aligned segments of `seg` elements (a power of two), element i of the block: in the step (k, j) — k = 2, 4, ...,
// seg, j = k / 2, ..., 1 — element i meets element i ^ j and keeps the smaller word iff this holds.  The direction comes from the
// index inside the segment, so that every segment ends ascending.
GLHIP_HD inline bool balance_keeps_min(int i, int j, int k, int seg) {
    const bool ascending = ((i & (seg - 1)) & k) == 0;
    return ((i & j) == 0) == ascending;
}

// Which steps of the network a level runs.  The next level sorts both halves of a segment again, by words that carry the position a
// point had in the incoming block, not the one it has now: of a level above the last only the SET of each half matters.  Before the
// last merge (k = seg) the two halves of a segment are sorted, the lower ascending and the upper descending, so the segment is
// bitonic, and the first step of that merge (j = seg / 2) already leaves the seg / 2 smallest words in the lower half and the others
// in the upper one; the steps j = seg / 4, ..., 1 would only order each half.  Those are left out (30 of the 185 steps of the five
// levels, 6 of the 20 that go through LDS); the last level (seg = last_seg) runs all of its steps, it decides the order.
GLHIP_HD inline bool balance_step_runs(int j, int k, int seg, int last_seg) { return seg == last_seg || k < seg || j == (k >> 1); }

}  // namespace glhip
