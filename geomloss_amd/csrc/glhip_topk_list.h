// glhip_topk_list.h — the sorted candidate lists of the top-k arg-reduction (glhip_argkmin_xk.h): CAP entries (u, index), best first,
// in two statically indexed arrays.  "Best" is the lexicographic rule of argmin_beats — larger exponent u, then smaller index — and an
// empty entry is (-inf, -1).  Every loop is fully unrolled and every subscript a compile-time constant, so that on the device the
// arrays stay in registers (a run-time subscript would send them to scratch).
// Plain C++, no HIP types: the host test (tests/test_topk_list_cpu.py) compiles it alone and plays it against std::stable_sort.
//
//   topk_clear        every entry empty
//   topk_push         a candidate from a stream whose indices ASCEND: strict `u > entry` — on a tie the earlier candidate stays
//                     ahead, u = -inf and u = NaN never enter.  One compare decides whether anything happens (u > last entry).
//   topk_insert_lex   a candidate in any index order: (u, index) lexicographic; an empty entry, u = -inf and NaN never enter.
//   topk_merge        topk_insert_lex of every entry of a second list: the best CAP of the union (the lists hold distinct indices).
#pragma once

#if defined(__HIPCC__)
#define GLHIP_TOPK_HD __host__ __device__ __forceinline__
#else
#define GLHIP_TOPK_HD inline
#endif

namespace glhip {

// (u, -index) lexicographic: does (u2, i2) beat (u1, i1)?  The rule of argmin_beats (glhip_argmin_xk.h).
GLHIP_TOPK_HD bool topk_beats(float u2, int i2, float u1, int i1) { return u2 > u1 || (u2 == u1 && i2 < i1); }

template <int CAP>
GLHIP_TOPK_HD void topk_clear(float (&lu)[CAP], int (&li)[CAP]) {
#pragma unroll
    for (int r = 0; r < CAP; ++r) {
        lu[r] = -__builtin_inff();
        li[r] = -1;
    }
}

// Entry r takes its upper neighbour where the candidate beats that one too, the candidate where it beats entry r only; from the last
// entry upwards, so that every right-hand side is still the old list.
template <int CAP>
GLHIP_TOPK_HD void topk_push(float (&lu)[CAP], int (&li)[CAP], float u, int i) {
#pragma unroll
    for (int r = CAP - 1; r > 0; --r) {
        const bool up = u > lu[r - 1], here = u > lu[r];
        li[r] = up ? li[r - 1] : (here ? i : li[r]);
        lu[r] = up ? lu[r - 1] : (here ? u : lu[r]);
    }
    const bool here = u > lu[0];
    li[0] = here ? i : li[0];
    lu[0] = here ? u : lu[0];
}

template <int CAP>
GLHIP_TOPK_HD void topk_insert_lex(float (&lu)[CAP], int (&li)[CAP], float u, int i) {
    // (no test for u = -inf: against an empty entry the exponents tie and no index is smaller than -1; NaN compares false throughout)
#pragma unroll
    for (int r = CAP - 1; r > 0; --r) {
        const bool up = topk_beats(u, i, lu[r - 1], li[r - 1]), here = topk_beats(u, i, lu[r], li[r]);
        const int ni = up ? li[r - 1] : (here ? i : li[r]);
        lu[r] = up ? lu[r - 1] : (here ? u : lu[r]);
        li[r] = ni;
    }
    const bool here = topk_beats(u, i, lu[0], li[0]);
    li[0] = here ? i : li[0];
    lu[0] = here ? u : lu[0];
}

template <int CAP>
GLHIP_TOPK_HD void topk_merge(float (&lu)[CAP], int (&li)[CAP], const float (&ou)[CAP], const int (&oi)[CAP]) {
#pragma unroll
    for (int r = 0; r < CAP; ++r) topk_insert_lex<CAP>(lu, li, ou[r], oi[r]);
}

}  // namespace glhip
