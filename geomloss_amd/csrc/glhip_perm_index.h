// glhip_perm_index.h — the index a kernel takes from a permutation that came from OUTSIDE the call (the hinted permutations of
// glhip_sinkhorn_step_perm, include/glhip.h; gather_points_kernel, gather_f32_kernel, scatter_f32_kernel of glhip_compact_sort.hip).  A hint
// is meant to be a permutation of 0 .. n-1 that this library wrote for a cloud of the same n; the library cannot check that, so every
// entry is clamped into [0, n): with anything else the outputs are unspecified, but every access stays in bounds.  n >= 1.
// Plain C++, no HIP types: the host tests compile it alone.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GLHIP_HD __host__ __device__
#else
#define GLHIP_HD
#endif

namespace glhip {

GLHIP_HD inline int32_t perm_index(int32_t j, int32_t n) { return j < 0 ? 0 : (j < n ? j : n - 1); }

}  // namespace glhip
