/*
 * glhip.h — C-ABI of libgeomloss_hip.so: the MI355X (gfx950) map-reduce kernels
 * behind geomloss's `SamplesLoss(backend="online"|"multiscale")`.
 *
 * The reference (jeanfeydy/geomloss 0.3.1) has no FFI of its own for this path:
 * it calls the third-party, un-vendored `pykeops` package, which JIT-compiles
 * one CUDA map-reduce per formula.  Each entry point below replaces one such
 * pykeops call site; the call site is cited next to it (paths relative to
 * /root/reference/src/geomloss/_legacy/).
 *
 * Conventions (all entry points)
 *   - plain C: raw device pointers, ints, floats; no C++ / torch types.
 *   - the caller owns every buffer; the library never allocates, frees or
 *     retains device memory.  All arrays are contiguous, row-major.
 *   - point clouds are (B, N, D) "array of structs", exactly as torch stores
 *     a contiguous (B,N,D) tensor; `in_dtype` selects their element type
 *     (GLHIP_F32 | GLHIP_BF16).  Dual vectors, weights, outputs and all
 *     accumulation are fp32.
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream) on the current device; nothing synchronises.
 *   - return value: 0 on success, a negative GLHIP_E* code otherwise; the
 *     message is available (thread-local) from glhip_last_error().
 *   - NaN/Inf propagate, they are not trapped (reference behaviour).
 *
 * Block-sparse reductions ("ranges", KeOps convention, int32 device arrays;
 * built at sinkhorn_samples.py:515 / kernel_samples.py:254-256 by
 * pykeops.torch.cluster.from_matrix):
 *   ranges_i    (n_ranges, 2)  row blocks [start, end) inside [0, N) — rows outside every
 *                              block are left untouched in the output.  Blocks are meant to be disjoint
 *                              (clusters of a sorted cloud); overlapping blocks are reduced correctly (a row
 *                              in two blocks is written by both) but one workgroup per block, without the
 *                              load-balancing row chunks
 *   slices_i    (n_ranges,)    CSR end offsets into redranges_j; block k owns
 *                              redranges_j[slices_i[k-1] : slices_i[k]] (slices_i[-1] = 0)
 *   redranges_j (nnz, 2)       column intervals [start, end) to reduce over
 *   n_ranges == 0 (pointers may be NULL) means a dense reduction over all j.
 *   Block-sparse mode requires B == 1 (as in the reference: samples_loss.py:249-257).
 *   A row block with no column interval reduces over the empty set.
 */
#ifndef GLHIP_H
#define GLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLHIP_VERSION 140 /* 0.1.40 */

/* element type of the point clouds x, y */
#define GLHIP_F32 0
#define GLHIP_BF16 1

/* kernel-convolution kinds (kernel_samples.py:62-82) */
#define GLHIP_GAUSSIAN 0  /* k = exp(-|x-y|^2 / (2 blur^2))  kernel_samples.py:62-68 */
#define GLHIP_LAPLACIAN 1 /* k = exp(-|x-y| / blur)          kernel_samples.py:71-77 */
#define GLHIP_ENERGY 2    /* k = -|x-y|  (blur ignored)      kernel_samples.py:80-82 */

/* flags (bitmask) */
#define GLHIP_FLAG_DIRECT 1   /* p=2 softmin: evaluate |x-y|^2 as sum (x_d-y_d)^2 (KeOps' SqDist)
                                 instead of the per-workgroup-centred expansion. Slower, tighter. */
#define GLHIP_FLAG_NO_MFMA 2  /* p=2 softmin / gaussian: form the exponents on the VALU instead of the matrix cores */
#define GLHIP_FLAG_NO_SPLIT 4 /* never split the columns of a row over several workgroups (ignore the workspace) */
#define GLHIP_FLAG_F32_MFMA 8 /* accepted for compatibility (the fp32-MFMA tiling of the p=2 softmin forward served A/B runs only and is
                                 gone): the forward runs its default kernel; big dense F16X2 forwards with D <= 3 stay on the bf16x3 kernel */
#define GLHIP_FLAG_XDL16 16   /* gaussian product: bf16x3 on 16x16x32 MFMAs (the previous tiling) instead of 32x32x16 — the tiling of the
                                 gradient kernels, see GLHIP_FLAG_GRAD_FAMILY.  p=2 softmin forward: as GLHIP_FLAG_F32_MFMA */
#define GLHIP_FLAG_GRAD_FAMILY GLHIP_FLAG_XDL16 /* kernel products: round like the product of glhip_kernel_conv_fwd_grad of the same
                                 kind — gaussian: the 16x16x32 tiling above; laplacian / energy: explicit differences with |.| = m rsq(m)
                                 (bit-identical to that product).  For the other two terms of a kernel norm whose gradient is on. */
#define GLHIP_FLAG_PREPACK 32 /* pre-pack the columns whatever the launch size (default: launches of >= 5e8 pairs); needs workspace */
#define GLHIP_FLAG_MFMA_DIST 64 /* p = 1 soft-min forward / laplacian / energy product, block-sparse launches, D <= 3: squared distances on
                                 the matrix cores, centred on each row block (glhip_dist_x32.h).  2-3x fewer VALU instructions; accurate
                                 (~2^-24 (rho + d)^2 / d on a potential, rho = row-block diameter) when row blocks are spatially compact:
                                 the caller's responsibility (voxel clusters of the multiscale backends, voxel-sorted dense clouds). */
#define GLHIP_FLAG_SMALL_ROW_BLOCKS 128 /* block-sparse soft-min forward / half-step, D <= 3: the pairs sit in row blocks of up to 64 points
                                  (sum of squared block sizes / N <= 64): launch 2-wavefront workgroups over 256-column tiles.  A hint: results
                                  do not depend on it.  The caller knows the block sizes (glhip_block_ranges_kept_pairs returns the sum). */

#define GLHIP_FLAG_F16X2 256 /* p = 2 soft-min (forward, half-step, gradient) and gaussian product / gradient, 4 <= D <= 16, the D <= 3
                                  soft-min forward, and (version 121) the soft-min forward / half-step / gaussian product of 17 <= D <= 4095: form the exponents from TWO f16 pieces per coordinate (3 products, v_mfma_f32_32x32x16_f16)
                                  instead of three bf16 pieces (6 products) — about half the matrix instructions and LDS bytes.  Cross terms
                                  good to ~2^-21 relative instead of 2^-24 (csrc/glhip_softmin_xd.h).  THE CALLER VOUCHES FOR THE RANGE: every
                                  exponent term (log2(e) h_j, |x - y|^2 / (2 eps ln 2)) must stay below ~2.6e5 in magnitude, i.e. roughly
                                  (cloud diameter)^2 / eps < 3e5; beyond that f16 overflows and the results are inf / nan.  The bound is on the
                                  exponents, so it is the same in every dimension (diameter^2 grows like D on a unit cube).  Ignored by kernels
                                  without that layout (p = 1, laplacian, energy — GLHIP_FLAG_XK_DIST included: bf16 x 3 only —, the gradients of D > 16 other than GLHIP_FLAG_XK_GRAD, D > 4095, float64). */

#define GLHIP_FLAG_XK_GRAD 1024 /* glhip_softmin_bwd_x (version 126) and, gaussian kind, glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad
                                  (version 130, below).  glhip_softmin_bwd_x: the gradient of p == 2, 17 <= D <= 4095, dense launches (n_ranges == 0),
                                  B <= 65535, without GLHIP_FLAG_NO_MFMA / _DIRECT runs xk_plan_kernel on XkGradParams (csrc/glhip_softmin_grad_xk.h): the K-chunked
                                  plan application of glhip_plan_apply_nd with the centred column cloud as its features, ceil(D / 64) passes.
                                  glhip_softmin_bwd_x_uses_plan is the predicate.  Ignored everywhere else — every other entry point, p = 1,
                                  D <= 16, D > 4095, block-sparse ranges, the float64 symbols: those launches are the ones version 125 makes,
                                  bit for bit.  Without the flag nothing changes: the one-thread-per-row kernel of glhip_generic.h.
                                  GLHIP_FLAG_F16X2 selects the exponent layout of the new kernel, under that flag's range contract.
                                  glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad: the gaussian gradient of 17 <= D <= 4095 under the same
                                  conditions runs xk_plan_kernel on XkGaussGradParams (csrc/glhip_gauss_grad_xk.h);
                                  glhip_kernel_conv_grad_uses_xk is the predicate.  Laplacian / energy, D <= 16, D > 4095, block-sparse ranges,
                                  GLHIP_FLAG_NO_MFMA / _DIRECT and glhip_kernel_conv_fwd ignore the flag, bit for bit. */

#define GLHIP_FLAG_XK_DIST 2048 /* version 131.  glhip_softmin_fwd / glhip_sinkhorn_step with p == 1 and glhip_kernel_conv_fwd of the laplacian /
                                  energy kinds: 17 <= D <= 4095, dense launches (n_ranges == 0), B <= 65535, without GLHIP_FLAG_NO_MFMA / _DIRECT
                                  run xk_dist_kernel (csrc/glhip_dist_xk.h): the squared distances from the K-chunked matrix-core chain of
                                  glhip_softmin_xk.h (bf16 x 3 pieces only; GLHIP_FLAG_F16X2 is ignored), centred on the first row of each block of 256
                                  rows, near pairs (d^2 < max(guard |xs_i|^2, 4 clamp^2), GLHIP_DIST_GUARD) re-evaluated on explicit differences.
                                  The family predicates report GLHIP_FAMILY_DIST there, and glhip_sinkhorn_step with p == 1 runs as ONE fused
                                  launch instead of returning GLHIP_EUNSUPPORTED.  Opt-in: without the flag every launch is the one version 130
                                  makes, bit for bit (the one-thread-per-row kernel of glhip_generic.h).  Ignored, bit for bit, by p == 2, the
                                  gaussian kind, D <= 16, D > 4095, block-sparse ranges, the gradients (glhip_kernel_conv_bwd_x /
                                  glhip_kernel_conv_fwd_grad / glhip_softmin_bwd_x), the float64 symbols and glhip_sinkhorn_iter4 / _anneal /
                                  _extrapolate4.  Workspace: glhip_workspace_bytes as it is (2 floats per row and split for D > 16 is what the
                                  soft-min takes; the products take 1). */

#define GLHIP_FLAG_XK_DIST_GRAD 4096 /* version 132.  The row gradients of the distance reductions: glhip_softmin_bwd_x with p == 1 and
                                  glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad of the laplacian / energy kinds, 17 <= D <= 4095, dense
                                  launches (n_ranges == 0), B <= 65535, without GLHIP_FLAG_NO_MFMA / _DIRECT run xk_dist_grad_kernel
                                  (csrc/glhip_dist_grad_xk.h): the exact squared distances of xk_dist_kernel (bf16 x 3 only, near pairs repaired
                                  and added on explicit differences) and the K-chunked product of xk_plan_kernel against the centred column
                                  cloud, in passes of glhip_dist_grad_pass_width() coordinates.  The p = 1 gradient normalises itself from the
                                  same launch (the saved forward value is not read).  glhip_kernel_conv_fwd_grad stops being GLHIP_EUNSUPPORTED
                                  for those kinds.  glhip_dist_grad_uses_xk is the predicate, glhip_dist_grad_workspace_bytes the sizing call.
                                  Opt-in: without the flag every launch of every entry point is the one version 131 makes, bit for bit.
                                  Ignored, bit for bit, by p == 2, the gaussian kind, D <= 16, D > 4095, block-sparse ranges, every forward and
                                  the float64 symbols.  GLHIP_FLAG_XK_GRAD is a different bit: its predicates stay 0 for these gradients. */

/* ops of glhip_dist_grad_uses_xk */
#define GLHIP_DIST_GRAD_SOFTMIN_P1 0 /* glhip_softmin_bwd_x, p == 1 */
#define GLHIP_DIST_GRAD_LAPLACIAN 1  /* glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad, GLHIP_LAPLACIAN */
#define GLHIP_DIST_GRAD_ENERGY 2     /* ... GLHIP_ENERGY */

#define GLHIP_FLAG_NO_SORT 512 /* p = 1 soft-min / half-step, laplacian and energy products: big dense launches (B = 1, D <= 3, N >= 65536,
                                  N M >= 5e8, a workspace of glhip_workspace_bytes) sort both clouds into the workspace themselves — voxel sort along a
                                  boustrophedon path, csrc/glhip_autosort.h — so that the squared distances can come from the matrix cores
                                  (GLHIP_FLAG_MFMA_DIST on slabs of 256 compact rows): 346 -> ~200 ms at N = M = 1e6.  Results come back in the
                                  caller's order; values differ from the unsorted launch by rounding only.  This flag keeps the clouds as they
                                  are (the generic explicit-difference kernel), e.g. for callers that hand in sorted clouds and their own ranges.
                                  p = 2 soft-min / half-step (version 120), same conditions and N M >= 1e11: the sorted launch reduces only the column blocks
                                  that can change a float32 result — exact block pruning, csrc/glhip_autosort.h.  Per slab R of 256 sorted rows
                                  and block T of 256 sorted columns, Mlb(R) = max_T [hmax(T) - dmax(R,T)^2 / (2 eps)] bounds every row's
                                  largest exponent from below; T is dropped when hmax(T) - dmin(R,T)^2 / (2 eps) < Mlb(R) - (ln M + 26 ln 2 + 1),
                                  so a row loses less than 2^-26 of its sum and its value moves by less than eps 2^-26 (float64 bound; the
                                  1-nat margin covers the f16 x 2 exponent error).  Non-finite inputs behave as in the dense launch (their
                                  blocks / slabs keep everything).  The kept blocks run on the block-sparse kernel (either exponent layout),
                                  results return in the caller's order, with no host synchronisation.  Headline law at 1e6 x 1e6
                                  (eps = 0.05^2): 36 % of the pairs kept, 81 -> 35 ms.  Version 122: a second level of the same bound inside
                                  the reducing kernel — every wavefront skips the groups of 32 columns that cannot matter to its own 32 rows,
                                  against their running maxima seeded with exact maxima over the slab's best block (csrc/glhip_softmin_x32.h,
                                  P2); both clouds are ordered in voxels of 256 points with compact sub-voxels inside.  Same guarantee (both
                                  levels together drop < 2^-26 of a row sum); headline law: 35 -> 24 ms (profiles/r09_*).
                                  Version 123: both levels drop by the SUM of what they drop instead of by single terms.  The terms of a
                                  set S of columns sum to at most e^(lse(S) - dmin(box, S)^2 / (2 eps)) for every row of the box; per slab
                                  (blocks of 256 columns) and per tile of 32 rows (groups of 32 columns) the largest threshold on that key
                                  is taken whose dropped masses stay within a budget — 0.132 x 2^-26, and 2^-26 / 2 beside the 2^-26 / e
                                  of the term rule — found on 0.25-nat histograms in float64 (csrc/glhip_autosort.h).  Same guarantee:
                                  a row loses < 2^-26 of its sum.  glhip_prune_inspect shows the thresholds (profiles/r10_*).
                                  Version 128: balanced cells.  After the radix sort, every whole aligned block of 1024 positions of both
                                  sorted clouds is split by median cuts along the longest axis into cells of exactly 512, 256, 128, 64 and
                                  32 points (csrc/glhip_balance.h), which the slabs, blocks, tiles and groups of both levels are aligned
                                  to: their boxes no longer straddle two voxels.  The guarantee does not depend on the order; perm_x / perm_y
                                  of glhip_prune_inspect show it.  The last N mod 1024 (M mod 1024) points keep the path order.
                                  Version 136: the two mass budgets are shares of a lower bound of the row SUM, not of one term of it.
                                  Per slab, Slb = log sum_T e^(lse_dn(T) - dmax(R, T)^2 / (2 eps)) over the column blocks (lse_dn: the
                                  rounded-up record lowered by twice its slack, four times for a block); per row of a tile the same sum
                                  over the groups of at most 16 reference blocks of its slab, point to box, or the row's exact largest
                                  exponent over the home block where that is more.  A smooth dual vector gains ~6 nats of threshold, the
                                  bench law 1-1.7; Mlb, home, the bucket grids and the stored t1 / t2 mean what they did, and
                                  glhip_prune_inspect shows them (csrc/glhip_autosort.h, "Sum reference"; profiles/sum_reference.txt).
                                  Version 137: on the f16 x 2 layout the sorted launch is swept by a list-driven kernel (one wavefront per
                                  tile of 32 rows, one keep test per 64 groups, operands straight from the packed columns: csrc/
                                  glhip_softmin_list.h).  Same test, same guarantee; the order of summation differs (profiles/list_sweep.txt).
                                  Version 140: which of the two sweeps takes a launch is decided once per launch, not by every wavefront
                                  of both.  Same bits as version 137 (profiles/list_pair.txt).
                                  Here this flag means the dense xd / x32 launch. */

/* Environment variables read ONCE per process by the library itself (test / tuning knobs; everything else is an argument):
 *   GLHIP_FWD_NW = 2 | 4 | 8  force the workgroup height (wavefronts) of the soft-min forward kernels instead of the size heuristic
 *   GLHIP_PREPACK_MIN = <p>   pairs per launch from which the columns are split into matrix-core records once per launch (default 5e8)
 *   GLHIP_DIST_GUARD = <x>    near-pair threshold of the matrix-core distance kernels: pairs with d^2 < x |xs_i|^2 are re-evaluated
 *                             on explicit differences (default 2^-8; 1e30 = every pair, used by the tests to check the register
 *                             <-> column map; 0 = none)
 * They are latched in function-local statics on first use: the library keeps no other global state (re-entrant apart from the
 * thread-local error string).  (Seven more A/B knobs of rounds 3-5 — GLHIP_ITER4_PRE_MIN, _ITER4_SPLITS, _TINY_MULTI_PAIRS,
 * _DIST_MULTI_MIN_COLS, _WQ_MIN_D, _XD_PRE, _H2_VIA_XD — were removed in round 6: their measured optimum is a constant now.) */

/* error codes */
#define GLHIP_OK 0
#define GLHIP_EINVAL (-1)       /* bad argument (NULL pointer, negative size, bad enum) */
#define GLHIP_EUNSUPPORTED (-2) /* valid request this build has no kernel for */
#define GLHIP_ELAUNCH (-3)      /* hipGetLastError() after the launch was not hipSuccess */

/* kernel families of the soft-min forward / fused half-step (glhip_softmin_fwd_family) and of the kernel products (glhip_kernel_conv_fwd_family).
 * The same codes name the gradient routes inside the library (csrc/glhip_family.h: there _X32 / _XD / _XK are the weighted-sum and plan kernels
 * of the same dimensions, _DIST the distance-gradient kernels); the gradient predicates below (glhip_softmin_bwd_x_uses_plan,
 * glhip_kernel_conv_grad_uses_xk, glhip_dist_grad_uses_xk) report the routes of 17 <= D <= 4095 as 1 / 0. */
#define GLHIP_FAMILY_VALU 0    /* D <= 3 on the VALU map-reduce skeleton (glhip_mapreduce.h): p = 1, GLHIP_FLAG_DIRECT / _NO_MFMA */
#define GLHIP_FAMILY_X32 1     /* p = 2, D <= 3: matrix cores, glhip_softmin_x32.h */
#define GLHIP_FAMILY_XD 2      /* p = 2, 4 <= D <= 16 (and big dense GLHIP_FLAG_F16X2 launches of D <= 3): matrix cores, glhip_softmin_xd.h */
#define GLHIP_FAMILY_XK 3      /* p = 2, 17 <= D <= 4095: matrix cores, K-chunked, D a run-time argument, glhip_softmin_xk.h */
#define GLHIP_FAMILY_DIST 4    /* p = 1 / laplacian / energy with the squared distances on the matrix cores: glhip_dist_x32.h (block-sparse, D <= 3,
                                  GLHIP_FLAG_MFMA_DIST) / glhip_dist_xd.h (dense, 4 <= D <= 16) / glhip_dist_xk.h (dense, 17 <= D <= 4095,
                                  GLHIP_FLAG_XK_DIST) */
#define GLHIP_FAMILY_GENERIC 5 /* D > 3 on the one-thread-per-row kernel of glhip_generic.h: p = 1 block-sparse, D > 16 without
                                  GLHIP_FLAG_XK_DIST or D > 4095; p = 2 with D > 4095 or under GLHIP_FLAG_NO_MFMA / _DIRECT */

int glhip_version(void);
const char* glhip_last_error(void);

/*
 * Scratch memory.  Every reduction below accepts an optional caller-owned device buffer
 * (`workspace`, `workspace_bytes`; NULL / 0 is always valid).  With it, the columns of a row may be
 * split over several workgroups (load balance on 256 CUs) and merged by a second small kernel on the
 * same stream, and launches of >= 5e8 pairs of the p = 2 soft-min forward / gaussian product write every
 * column once as 64 bytes of bf16x3 matrix-core operands (+ 4 bytes of weight) that all row blocks then
 * copy instead of recomputing.  glhip_workspace_bytes returns a size that lets every entry point use its
 * preferred plan for the given problem (208 MB at B = 1, N = M = 1e6, D = 3); smaller buffers are used as
 * far as they go.  The buffer must stay alive until the work queued on `stream` has run; its contents
 * are scratch.  17 <= D <= 4095 (version 121; 0 before): the column-split partials of the forward kernels (2 floats per row and
 * split, up to 32 splits) — those kernels stage their operands on the fly and keep nothing else there; the gradients of D > 16 and
 * every launch of D > 4095 use no workspace.
 */
size_t glhip_workspace_bytes(int B, int N, int M, int D, int n_ranges);

/*
 * Which kernel family (GLHIP_FAMILY_*) glhip_softmin_fwd / glhip_sinkhorn_step select for a launch of this shape: the predicate the
 * launch itself evaluates, exposed so that tests and callers can see the choice.  Host arithmetic only: no device, no stream, no
 * launch.  For the big dense D <= 3 launches that sort their clouds first (see GLHIP_FLAG_NO_SORT) it reports the family of the
 * inner block-sparse launch, which assumes a workspace of glhip_workspace_bytes.  Returns GLHIP_EINVAL for sizes, p or dtype the
 * entry points reject.
 */
int glhip_softmin_fwd_family(int B, long N, long M, int D, int p, int dtype, int flags, int n_ranges);
/* ... and the same for the products of glhip_kernel_conv_fwd.  Gaussian: _X32 (D <= 3; here the matrix-core product of glhip_wsum_x32.h /
 * glhip_wsum_mfma.h), _XD, _XK, or _VALU / _GENERIC under GLHIP_FLAG_NO_MFMA and beyond D = 4095; laplacian / energy: _DIST where the
 * squared distances come from the matrix cores, _VALU / _GENERIC elsewhere. */
int glhip_kernel_conv_fwd_family(int kind, int B, long N, long M, int D, int dtype, int flags, int n_ranges);

/*
 * What the exact pruning of a big dense p = 2 call decides (version 123): runs the sort and the bounds of glhip_softmin_fwd (pot = NULL,
 * logw = h) or glhip_sinkhorn_step (the column vector is fma(pot, 1 / eps, logw)) on `stream` and copies the records into the caller's
 * DEVICE buffers; it launches no reduction.  The mass dropped by the pruning is below one ulp of the output by design, so no output can
 * tell a correct budget from a generous one: the thresholds themselves are checkable here.  With C = ceil(N / 256) slabs of sorted rows
 * and S = glhip_prune_inspect_slots(M) interval slots per slab (any output may be NULL):
 *   perm_x (N), perm_y (M)   sorted position -> caller's index
 *   mlb, t1 (C doubles)      per slab: Mlb and the first level's key threshold, in nats (t1 = -inf: the slab keeps everything)
 *   home (C)                 per slab: the home column block, -1: no second level
 *   intervals (C S 2)        per slab: S (begin, end) pairs of sorted columns; unused slots are empty
 *   t2 (ceil(N / 32) floats) per tile of 32 sorted rows: the second level's mass threshold, in log2 units as the kernel compares it
 *                            (-inf: not written — home = -1 — or no finite seed)
 * GLHIP_EUNSUPPORTED for shapes the p = 2 call does not prune (see GLHIP_FLAG_NO_SORT); GLHIP_EINVAL for a workspace below
 * glhip_workspace_bytes(1, N, M, D, 0).
 */
int glhip_prune_inspect_slots(int M);
int glhip_prune_inspect(const void* x, const void* y, const float* logw, const float* pot, int N, int M, int D, float eps, int in_dtype,
                        int32_t* perm_x, int32_t* perm_y, double* mlb, double* t1, int32_t* home, int32_t* intervals, float* t2,
                        void* workspace, size_t workspace_bytes, void* stream);

/*
 * Soft-C-transform  out[b,i] = -eps * log sum_j exp( h[b,j] - C(x[b,i], y[b,j]) / eps ),
 * C = |x-y|^2 / 2 (p == 2) or |x-y| (p == 1).
 *
 * Replaces: pykeops generic_logsumexp("(B - (P * cost))", ...) built by
 *   lse_genred  sinkhorn_samples.py:322-334  and  keops_lse  :432-442,
 *   as called by softmin_online :337-346, softmin_online_lazytensor :229-290 (B > 1)
 *   and softmin_multiscale :445-450 (ranges != NULL).
 * Same function as softmin_tensorized :32-71 on C = cost_routines[p](x, y) :26-29.
 *
 *   x (B,N,D)  y (B,M,D)  h (B,M) fp32  out (B,N) fp32
 *
 * Kernels by (p, D): p = 2 on the matrix cores for D <= 4095 (glhip_softmin_x32.h / _xd.h up to D = 16, the K-chunked glhip_softmin_xk.h
 * from D = 17 on, version 121; GLHIP_FLAG_F16X2 selects the two-piece f16 layout); p = 1 on the matrix cores for block-sparse launches of D <= 3 with GLHIP_FLAG_MFMA_DIST (glhip_dist_x32.h) and, since
 * round 5, for every DENSE launch of 4 <= D <= 16 (glhip_dist_xd.h: squared distances from the MFMA chain, pairs closer than 1/16 of
 * their offset from the cloud's centre re-evaluated exactly); everything else (p = 1 in D > 16 without GLHIP_FLAG_XK_DIST, p = 2 in D > 4095, block-sparse p = 1 in D > 3, GLHIP_FLAG_NO_MFMA /
 * GLHIP_FLAG_DIRECT) on explicit differences.
 * Accuracy of the matrix-core distances (p = 1; laplacian / energy products): the squared distance of a pair carries ~2^-23 t^2 R^2
 * (t = log2(e) / eps, R = offset of the pair from the centre the launch subtracts), so the EXPONENT of a pair just above the near-pair
 * threshold d = R / 16 is off by ~2^-20 t R — it grows like diameter / eps — while out = -eps log(...) is off by
 * ~2^-20 log2(e) R <= 1.4e-6 diameter whatever eps is; a kernel VALUE of the products carries the relative error 2^-20 t R at the
 * threshold (random sign), 2^-24 t R for pairs at distance R.  Measured at eps / diameter = 0.005 and 0.002, D = 4, 5, 9
 * (tests/test_xd_kernels_gpu.py::test_distance_reductions_xd_small_blur).  GLHIP_DIST_GUARD raises the threshold.
 */
int glhip_softmin_fwd(const void* x, const void* y, const float* h, float* out,
                      int B, int N, int M, int D, float eps, int p, int in_dtype,
                      const int32_t* ranges_i, const int32_t* slices_i,
                      const int32_t* redranges_j, int n_ranges,
                      void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * One fused half-step of the symmetric Sinkhorn iteration (every kernel of D <= 3; p = 2 for D <= 4095 (D > 16: version 121); p = 1 on
 * dense launches for D <= 16 and, under GLHIP_FLAG_XK_DIST (version 131), for D <= 4095; GLHIP_EUNSUPPORTED elsewhere — compose glhip_softmin_fwd):
 *   t_i   = soft-min(eps, C(x,y), logw + pot / eps)_i          (pot == NULL: logw alone, the initialisation)
 *   out_i = damping * t_i                                       (prev == NULL)
 *   out_i = (prev_i + damping * t_i) / 2                        (prev != NULL; out must not alias prev)
 * Replaces, per soft-min call of the loop at sinkhorn_divergence.py:461-465 and :480-493, the elementwise
 * ops `log_w + pot/eps`, `damping * (...)` and `0.5 * (f + ft)` that the reference runs as separate torch kernels
 * (SURVEY §8f, N1).  Same kernels, splits and flags as glhip_softmin_fwd.
 *   logw (B,M), pot (B,M) or NULL, prev (B,N) or NULL, out (B,N): fp32.
 */
int glhip_sinkhorn_step(const void* x, const void* y, const float* logw, const float* pot, const float* prev,
                        float* out, int B, int N, int M, int D, float eps, float damping, int p, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i,
                        const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * glhip_sinkhorn_step with the permutations of the sorted p = 2 call handed in and out (version 134).  The big dense p = 2 call (see
 * GLHIP_FLAG_NO_SORT) orders both clouds before it prunes: bounding box, voxel edge, path keys, a 64-bit radix sort and the balanced
 * cells, all of them functions of a cloud's coordinates alone — 0.65 of 16.7 ms at N = M = 1e6, a fifth of the call at eps = 0.01^2 —
 * while a Sinkhorn loop calls a few hundred times on the same two clouds.  A cloud gets the same order as rows and as columns.
 *   perm_x (N ints), perm_y (M ints): DEVICE buffers, either may be NULL (no hint and no export for that cloud).
 *   perm_flags & GLHIP_PERM_HINT_X: perm_x HOLDS the order of x — box, keys, sort and balancing are not launched for x, the call
 *     reads the buffer and does not write it; GLHIP_PERM_HINT_Y: the same for perm_y and y.
 *   A non-NULL buffer without its bit RECEIVES the order the call computes (sorted position -> caller's index, what
 *     glhip_prune_inspect reports), written straight by the sort: no copy, no extra launch.
 *   The x side is prepared first: where x and y are one cloud, one buffer may be passed as perm_x (export) and as perm_y with
 *     GLHIP_PERM_HINT_Y, and the cloud is sorted once.
 * Contract of a hint: a permutation of 0 .. n-1 that this library wrote for a cloud of the same n points, alive and unchanged until
 * the work queued on `stream` has run, produced on `stream` or synchronised with it by the caller.  With anything else the outputs
 * are unspecified, but every access stays in bounds: each kernel that indexes through a hint clamps the index into [0, n).
 * A STALE hint — the right size, the order of other coordinates — changes no result beyond the pruned call's guarantee (a row loses
 * < 2^-26 of its sum): the pruning is exact for any order, every box it uses is recomputed from the gathered coordinates on every
 * call, and the order only decides how much is kept, that is, the time.  Only permutations are reused for this reason.
 * Where glhip_softmin_perm_applies says 0, or the workspace is below glhip_workspace_bytes, the three arguments are ignored: nothing
 * is read or written through them, and the call is glhip_sinkhorn_step.  glhip_softmin_fwd is this call with pot = prev = NULL,
 * damping = 1.  The workspace size and layout are those of glhip_sinkhorn_step.
 */
#define GLHIP_PERM_HINT_X 1
#define GLHIP_PERM_HINT_Y 2
int glhip_sinkhorn_step_perm(const void* x, const void* y, const float* logw, const float* pot, const float* prev,
                             float* out, int B, int N, int M, int D, float eps, float damping, int p, int in_dtype,
                             const int32_t* ranges_i, const int32_t* slices_i,
                             const int32_t* redranges_j, int n_ranges,
                             void* workspace, size_t workspace_bytes, int flags, void* stream,
                             int32_t* perm_x, int32_t* perm_y, int perm_flags);
/* Whether a call of this shape is the sorted p = 2 call, the one that takes and gives permutations: 1 / 0, host arithmetic only, like
 * glhip_softmin_fwd_family (1 exactly where that predicate routes a p = 2 call through the sort; 0 for p = 1, B > 1, ranges,
 * GLHIP_FLAG_NO_SORT and below 1e11 pairs).  The workspace condition is the caller's.  GLHIP_EINVAL for arguments the entry points reject. */
int glhip_softmin_perm_applies(int B, long N, long M, int D, int p, int dtype, int flags, int n_ranges);

/*
 * One whole iteration of the symmetric Sinkhorn loop in ONE launch (+ one merge launch): the four
 * simultaneous updates of sinkhorn_divergence.py:480-493 (or the four initialisations of :461-465 when
 * `first` != 0), each reading the OLD potentials:
 *   f_ba' = avg(C_xy, b_log, g_ab, f_ba)    g_ab' = avg(C_yx, a_log, f_ba, g_ab)
 *   f_aa' = avg(C_xx, a_log, f_aa, f_aa)    g_bb' = avg(C_yy, b_log, g_bb, g_bb)        (debias only)
 * with avg(C, logw, pot, prev) = (prev + damping * softmin(eps, C, logw + pot/eps)) / 2  (`first` = 0),
 * damping * softmin(eps, C, logw)  (`first` = 1: initial potentials, :461-465), or
 * damping * softmin(eps, C, logw + pot/eps)  (`first` = 2: the non-averaged last update, :612-623).  C_xy = C(x_i, y_j) etc. on the clouds x (B,N,D), y (B,M,D).
 *   f_aa / g_bb and their outputs may be NULL together (debias = False: two reductions).
 * Outputs must not alias inputs.  Dense, D <= 16; p = 2 (4 <= D <= 16 since round 5) or p = 1 (round 5: the dense distance kernel
 * of glhip_dist_xd.h) (GLHIP_EUNSUPPORTED otherwise: issue four
 * glhip_sinkhorn_step calls instead); meant for small and mid-size problems, where four separate launches
 * leave the chip under-filled.  Workspace: 4 * glhip_workspace_bytes(B, max(N,M), max(N,M), D, 0).
 */
int glhip_sinkhorn_iter4(const void* x, const void* y, const float* a_log, const float* b_log,
                         const float* f_ba, const float* g_ab, const float* f_aa, const float* g_bb,
                         float* f_ba_out, float* g_ab_out, float* f_aa_out, float* g_bb_out,
                         int B, int N, int M, int D, float eps, float damping, int p, int in_dtype, int first,
                         void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * A whole run of the symmetric eps-scaling loop, queued by ONE call: the initialisation at eps[0] (sinkhorn_divergence.py:461-465)
 * followed by one averaged iteration per temperature eps[0..n_eps-1] (:468-493), each a glhip_sinkhorn_iter4 launch (+ merge) with
 * its own temperature and damping[i] — what the Python loop queues with one host-side call per iteration, minus the interpreter
 * between the launches (loops on a few thousand points are bound by the host's launch rate: N = 2000, 10 temperatures: 0.46 -> 0.36 ms).
 * The temperatures are plain host arrays, computed after whatever the caller measured (a diameter), so nothing is baked in.
 *   set0, set1: two sets of output buffers {f_ba (B,N), g_ab (B,M), f_aa (B,N), g_bb (B,M)} (the last two NULL in both sets without
 *   debiasing).  The initial potentials go to set0, iteration i reads set[i % 2] and writes set[(i + 1) % 2]: on return (queued) the
 *   final potentials are in set[n_eps % 2] and the inputs of the last iteration in the other one.  No buffer may appear twice.
 *   flags: as glhip_sinkhorn_iter4, with GLHIP_FLAG_F16X2 applied to the iterations whose eps[i] >= f16x2_min_eps only (the caller's
 *   range vouching is per temperature; pass 0 to apply it everywhere, a huge value or no flag for never).
 * Dense, D <= 16, p = 1 or 2, n_eps >= 1; workspace as glhip_sinkhorn_iter4.  Used for single-scale losses and for the coarse level of
 * the two-scale ones (everything up to the jump).
 */
int glhip_sinkhorn_anneal(const void* x, const void* y, const float* a_log, const float* b_log, float* const* set0, float* const* set1,
                          int B, int N, int M, int D, const float* eps, const float* damping, int n_eps, int p, int in_dtype,
                          void* workspace, size_t workspace_bytes, int flags, float f16x2_min_eps, void* stream);

/*
 * The coarse-to-fine jump of the two-scale loop in ONE launch (+ one merge launch): the four extrapolations of
 * sinkhorn_divergence.py:590-599, each `extrapolate_samples` (sinkhorn_samples.py:533-544) — one soft-min of the FINE points against
 * a COARSE measure:
 *   f_ba'(x_i) = damping * softmin(eps, C(x_i, yc_j), b_log_c + g_ab / eps)    g_ab'(y_i) = damping * softmin(eps, C(y_i, xc_j), a_log_c + f_ba / eps)
 *   f_aa'(x_i) = damping * softmin(eps, C(x_i, xc_j), a_log_c + f_aa / eps)    g_bb'(y_i) = damping * softmin(eps, C(y_i, yc_j), b_log_c + g_bb / eps)
 * x (B,N,D), y (B,M,D): the fine clouds; xc (B,Nc,D), yc (B,Mc,D): the coarse ones (centroids), with their log-weights a_log_c (B,Nc),
 * b_log_c (B,Mc) and potentials f_ba, f_aa (B,Nc), g_ab, g_bb (B,Mc); outputs (B,N) / (B,M), all fp32.  f_aa / g_bb and their outputs
 * may be NULL together.  Same kernels, flags, limits (dense, D <= 16, p = 1 or 2) and error behaviour as glhip_sinkhorn_iter4, of which
 * this is the rows != columns form; replaces four glhip_softmin_fwd launches and their 12 elementwise torch kernels per jump.
 * Workspace: 4 * glhip_workspace_bytes(B, max(N, M), max(Nc, Mc), D, 0) (rows: the fine clouds, columns: the coarse ones); as with every
 * entry point a smaller (or NULL) workspace is accepted: fewer column splits, no pre-packed columns, same results up to rounding.
 */
int glhip_sinkhorn_extrapolate4(const void* x, const void* y, const void* xc, const void* yc, const float* a_log_c, const float* b_log_c,
                                const float* f_ba, const float* g_ab, const float* f_aa, const float* g_bb,
                                float* f_ba_out, float* g_ab_out, float* f_aa_out, float* g_bb_out,
                                int B, int N, int M, int Nc, int Mc, int D, float eps, float damping, int p, int in_dtype,
                                void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * The elementwise front and back end of a Sinkhorn loss, for problems of a few thousand points whose time is the host's launch rate
 * (round 6; a 2000-point loss is 26 launches of which the soft-mins are 9):
 *   glhip_log_weights: out_k[i] = log(w_k[i]) with log(0) -> -100000 for up to 4 vectors in ONE launch — `log_weights`
 *     (sinkhorn_divergence.py:61-65; NaN weights stay NaN).  w, out, n: HOST arrays of `count` device pointers / lengths.
 *   glhip_sinkhorn_cost: out[b] = <a_b, f_ba_b - f_aa_b> + <b_b, g_ab_b - g_bb_b> — `sinkhorn_cost`, balanced case
 *     (sinkhorn_divergence.py:171-199) — accumulated in float64 in a fixed order; f_aa = g_bb = NULL: without debiasing.
 *     f_*, (B,N) and g_*, (B,M) fp32; a (B,N) if a_batched else (N) shared by the batch, b likewise; out (B) fp32.  One workgroup per
 *     batch item: meant for N, M up to a few 1e4 (beyond, a tree of torch reductions is faster).
 *   glhip_bounding_box: lo_hi (2 D) fp32 out = the D minima then the D maxima of the coordinates of x (nx, D) and y (ny, D) together
 *     (either may be empty: +inf / -inf there) — the reductions of `max_diameter` (sinkhorn_divergence.py:96-112: cat, aminmax) in one
 *     launch of one workgroup; exact (minima and maxima); D <= 16; meant for clouds of up to ~1e4 points (one workgroup sweeps them).
 */
int glhip_bounding_box(const void* x, long nx, const void* y, long ny, int D, int in_dtype, float* lo_hi, void* stream);
int glhip_log_weights(const float* const* w, float* const* out, const long* n, int count, void* stream);
int glhip_sinkhorn_cost(const float* a, const float* f_ba, const float* f_aa, const float* b, const float* g_ab, const float* g_bb,
                        float* out, int B, int N, int M, int a_batched, int b_batched, void* stream);

/*
 * Log-sum-exp along the lines of a regular grid — the separable soft-min of the reference's image / volume path
 * (SURVEY §8f, N4):
 *   out[r, i] = log sum_j exp( h[r, j] - c(i, j) ),   c(i, j) = (x_i - x_j)^2 / (2 eps)  (p = 2)  or  |x_i - x_j| / eps  (p = 1),
 *   x_i = i / N, for R independent lines of N <= 4096 fp32 samples stored contiguously.
 * Replaces: the KeOps `LazyTensor.logsumexp(dim=2)` inside `softmin_grid` (_legacy/utils.py:254-270), which the
 * reference applies once per image axis (:272-283; the caller permutes the axis of interest to the last position).
 * glhip_lse_lines_bwd is its vector-Jacobian product:  grad_h[r, j] = sum_i grad_out[r, i] exp(h[r, j] - c(i, j) - lse[r, i]).
 */
int glhip_lse_lines_fwd(const float* h, float* out, long R, int N, float eps, int p, void* stream);
int glhip_lse_lines_bwd(const float* h, const float* lse, const float* grad_out, float* grad_h, long R, int N,
                        float eps, int p, void* stream);

/*
 * Gradient of glhip_softmin_fwd with respect to x (the only differentiable argument on the
 * reference's path: y and h are detached at sinkhorn_samples.py:392-393,628-651 and
 * sinkhorn_divergence.py:616-623):
 *   grad_x[b,i,:] = grad_out[b,i] * sum_j P_ij * dC/dx(x_i, y_j),
 *   P_ij = exp( h_j - C_ij/eps + out_i/eps )   (rows of P sum to 1; we renormalise by the
 *   recomputed row sum, as autograd's logsumexp backward does).
 * Replaces: the symbolic KeOps `Grad` of the generic_logsumexp above.
 * (p = 1, dense, 4 <= D <= 16: glhip_dist_xd.h since round 5 — distances from the MFMA chain, near pairs from the points themselves.)
 * D > 16: the one-thread-per-row kernel of glhip_generic.h, in ANY dimension (version 121; D <= 64 before): 64 output coordinates
 * per pass over the columns, ceil(D / 64) passes.  The same holds for glhip_kernel_conv_bwd_x.  The weighted sums sum_j w_ij q_j as
 * a second MFMA product over all 32 MFMA rows live in glhip_plan_apply below (glhip_plan_apply.h, version 124: any number of feature
 * columns, D <= 16) and, for 17 <= D <= 4095, in glhip_plan_apply_nd (glhip_plan_apply_xk.h, version 125).
 * GLHIP_FLAG_XK_GRAD (version 126) routes the p = 2 gradient of 17 <= D <= 4095 through that product: xk_plan_kernel on
 * XkGradParams (glhip_plan_apply_xk.h, glhip_softmin_grad_xk.h) takes the column cloud itself, centred on the first row of each 256-row block, as its features and writes
 * g_i ((x_i - centre) - sum_j P_ij (y_j - centre)) — 64 coordinates per pass, ceil(D / 64) passes, float32 and bfloat16 clouds, both
 * exponent layouts; a row without mass gets 0; a one-hot plan row gives g_i (x_i - y_j) with an exact difference.  The flag is opt-in
 * at this level: the default stays the one-thread-per-row kernel, whose explicit differences meet 5e-6 at eps = 0.3 where the
 * exponents of a long MFMA chain are bounded by 4 x the error of plain float32 arithmetic instead (DESIGN section 4 has the measured
 * figures of both routes).
 *   glhip_softmin_bwd_x_uses_plan: host arithmetic only, the very predicate the launch evaluates — 1: that kernel; 0: the launch
 *   of version 125; GLHIP_EINVAL: negative sizes, D < 1, a bad p or dtype.
 *   glhip_softmin_bwd_x_workspace_bytes: the split partials of the widest pass of the new route (sums of <= 64 centred coordinates,
 *   mass, row maximum per row and split), never more than 1 GiB, 0 where the predicate is 0 (those launches size their workspace
 *   with glhip_workspace_bytes, which does not change) or under GLHIP_FLAG_NO_SPLIT.  NULL or a short workspace: fewer or no splits,
 *   the same results up to summation order.  N == 0 or B == 0 launches nothing; M == 0 zeroes grad_x.
 *   out = the saved forward result (B,N);  grad_out (B,N) fp32;  grad_x (B,N,D) fp32.
 *   A row without mass — every h_j = -inf (or no column at all in its ranges), whose saved forward value is +inf or the huge
 *   finite value the forward kernels return where their neutral padding was all they saw — gets grad_x = 0, never NaN: in every
 *   dimension, on every route and in both exponent layouts; glhip_softmin_fwd_grad likewise (its value there: +inf or that huge value).
 *   glhip_softmin_bwd_x_f64 below does the same.  Columns with h_j = -inf weigh exactly 0 whatever finite coordinates they hold
 *   (under GLHIP_FLAG_F16X2: inside that flag's range contract).
 */
int glhip_softmin_bwd_x(const void* x, const void* y, const float* h,
                        const float* out, const float* grad_out, float* grad_x,
                        int B, int N, int M, int D, float eps, int p, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i,
                        const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream);
int glhip_softmin_bwd_x_uses_plan(int B, long N, long M, int D, int p, int dtype, int flags, int n_ranges);
size_t glhip_softmin_bwd_x_workspace_bytes(int B, int N, int M, int D, int flags);

/*
 * Application of the transport plan of a p = 2 soft-min to a feature matrix (version 124; glhip_plan_apply.h).  With
 * C_ij = |x_i - y_j|^2 / 2 and fwd (B,N) the saved result of glhip_softmin_fwd for the same x, y, h, eps:
 *   w_ij       = exp( h_j - C_ij/eps + fwd_i/eps )
 *   mass_i     = sum_j w_ij                                   (= 1 up to rounding)
 *   out[b,i,v] = sum_j w_ij feat[b,j,v] / mass_i              (0 where mass_i == 0: a row whose columns all carry h = -inf; either layout)
 * Dividing by the recomputed mass cancels the common-mode error of a row's exponents, as in glhip_softmin_bwd_x; a caller that wants
 * the unnormalised product multiplies by exp(-fwd_i / eps), which the forward gives exactly.
 * Replaces: `P @ S` on the reference's symbolic plans (ot/_implementations/sample.py lazy_plan / plan_operator / density_operator).
 *   feat (B,M,V) row-major fp32, V >= 1 any size;  out (B,N,V) fp32;  mass (B,N) fp32 or NULL;  x, y fp32 or bf16.
 *   One pass over the columns per 128 features for D <= 4, per 64 for 5 <= D <= 11, per 32 beyond (a remainder is a pass of its own): the exponent block and the two f16 pieces of its 16
 *   weights per lane are shared by up to four chunks of 32 features, each a second MFMA product (three piece products = six MFMAs per
 *   chunk, fresh accumulator per 32 columns); features are split into two f16 pieces under a power-of-two scale per column and tile,
 *   found on the device.  Inside the kernel the weights are taken relative to the running maximum of their row (fwd centres the
 *   exponents and scales `mass`; an inaccurate fwd costs no accuracy in `out`), so the largest weight of a row is exact and a one-hot
 *   plan row returns its features as the two f16 pieces carry them: bit for bit where they hold them (22 significant bits below the
 *   power of two above the column's largest |f| within the tile: integers, fixed-point grids), within 1.5 x 2^-23 of that largest
 *   |f| for arbitrary float32 features.  A column with h_j = -inf (exactly; not a large negative stand-in for log 0) has its
 *   features staged as 0, whatever finite value they hold: they do not enter the scale of their tile.
 *   Rounding of the product: <= 2e-7 of sum_j w_ij |feat_jv| (tools/plan_apply_model.py), next to the ~1e-6 the
 *   exponents leave.
 *   Supported: p == 2, 1 <= D <= 16 (this contract stays: D >= 17 goes through glhip_plan_apply_nd below), dense launches
 *   (n_ranges == 0), any B; anything else returns GLHIP_EUNSUPPORTED (the range
 *   arguments are there so that block-sparse plans can follow without an ABI change).  N == 0, M == 0, V == 0: nothing is launched
 *   (M == 0 with N > 0: out and mass are zeroed; V == 0: out is empty and mass is left as it is — glhip_plan_apply_nd zeroes it).
 *   flags: GLHIP_FLAG_F16X2 (exponents from f16 x 2 pieces, under that flag's range contract), GLHIP_FLAG_NO_SPLIT; others are ignored.
 *   Workspace: glhip_plan_apply_workspace_bytes holds the (sums, mass, row maximum) partials of the column splits the launch would like,
 *   and never asks for more than 1 GiB (big launches have row blocks enough and split little); NULL or short means fewer or
 *   no splits — the same results up to summation order.
 */
size_t glhip_plan_apply_workspace_bytes(int B, int N, int M, int D, int V);

int glhip_plan_apply(const void* x, const void* y, const float* h, const float* fwd, const float* feat,
                     float* out, float* mass,
                     int B, int N, int M, int D, int V, float eps, int p, int in_dtype,
                     const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                     void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * The same application in any dimension up to 4095 (version 125).  glhip_plan_apply and glhip_plan_apply_workspace_bytes keep their
 * D <= 16 contract (D = 17 returns GLHIP_EUNSUPPORTED there); these symbols take the same argument lists with the same meaning:
 *   1 <= D <= 16:     forwards to glhip_plan_apply — the very same launch, bit-identical results.
 *   17 <= D <= 4095:  xk_plan_kernel (glhip_plan_apply_xk.h): the K-chunked exponent blocks of the forward kernel of these dimensions
 *                     (glhip_softmin_xk.h: 256 x 128 blocks, stages of 6 MFMAs, operands split on the fly, both layouts, float32 and
 *                     bfloat16 clouds), handed after the last stage of a column tile to the second MFMA product of glhip_plan_apply.h.
 *                     One pass over the columns per 64 features (a remainder is a pass of its own).  Same semantics: out = 0 and
 *                     mass = 0 for a row whose columns all carry h = -inf, in either layout; a one-hot plan row returns its features
 *                     bit for bit; M == 0 or V == 0 with N > 0 zeroes out and mass; N == 0 launches nothing.
 *   p != 2, block-sparse ranges (n_ranges > 0) and D > 4095 return GLHIP_EUNSUPPORTED.
 * glhip_plan_apply_nd_workspace_bytes holds the split partials only and never asks for more than 1 GiB; NULL or a short buffer means
 * fewer or no splits, with the same results up to summation order.
 * glhip_plan_apply_nd_family: host arithmetic only, the predicate the launch itself evaluates — GLHIP_FAMILY_XD for D <= 16,
 * GLHIP_FAMILY_XK for 17 <= D <= 4095, GLHIP_EUNSUPPORTED for valid requests without a kernel (p = 1, ranges, D > 4095),
 * GLHIP_EINVAL for what the entry point rejects (negative sizes, D < 1, bad p or dtype).  `flags` does not change the family.
 * glhip_plan_apply_nd_pass_width: feature columns one pass over the columns carries — 128 / 64 / 32 for D <= 4 / <= 11 / <= 16,
 * 64 for 17 <= D <= 4095, 0 for a dimension without a kernel.
 * glhip_softmin_bwd_x of 17 <= D <= 4095 runs a gradient mode of this product under GLHIP_FLAG_XK_GRAD (version 126), see above.
 */
size_t glhip_plan_apply_nd_workspace_bytes(int B, int N, int M, int D, int V);
int glhip_plan_apply_nd_family(int B, long N, long M, int D, int V, int p, int dtype, int flags, int n_ranges);
int glhip_plan_apply_nd_pass_width(int D);
int glhip_plan_apply_nd(const void* x, const void* y, const float* h, const float* fwd, const float* feat,
                        float* out, float* mass,
                        int B, int N, int M, int D, int V, float eps, int p, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * The plan of a p = 1 soft-min applied to features (version 135), 1 <= D <= 4095, float32 / bfloat16 clouds, dense and batched launches:
 *     w_ij = exp(h_j - c_ij / eps),  c_ij = sqrt(max(|x_i - y_j|^2, 1e-8))      (the clamp of utils.py:56-61)
 *     out[b,i,v] = sum_j w_ij feat[b,j,v] / sum_j w_ij          softmin[b,i] = -eps log sum_j w_ij      (softmin may be NULL)
 * xk_dist_plan_kernel (glhip_dist_plan_xk.h): the exact squared distances of the p = 1 forward kernel of 17 <= D <= 4095 (near pairs
 * re-evaluated on explicit differences), handed to the second MFMA product of glhip_plan_apply.h.  ONE kernel for the whole range of D.  It
 * normalises itself — no saved forward value comes in — and returns the soft-min it has computed on the side.  One pass over the columns
 * per glhip_plan_apply_p1_pass_width() features (a remainder is a pass of its own).  Results are bit-identical run to run; a one-hot plan row
 * returns its features bit for bit; a row whose columns all carry h = -inf gets out = 0 and softmin = +inf, never NaN.
 *   M == 0 with N > 0 zeroes out (softmin: +inf); V == 0 writes nothing to out (softmin, where wanted, is still computed); N == 0 or
 *   B == 0 writes nothing at all.  Validation in the order of glhip_plan_apply_nd.
 *   Block-sparse ranges (n_ranges > 0: the arguments are in the ABI for later), D > 4095 and B > 65535 return GLHIP_EUNSUPPORTED.
 *   GLHIP_FLAG_NO_SPLIT is honoured; GLHIP_FLAG_F16X2 is ignored (a squared distance needs all 24 bits); no other flag changes the result.
 * glhip_plan_apply_p1_workspace_bytes holds the split partials only and never asks for more than 1 GiB; NULL or a short buffer means
 * fewer or no splits, with the same results up to summation order.
 * glhip_plan_apply_p1_supported: host arithmetic only, the predicate the launch itself evaluates — 1, 0 for valid requests without a
 * kernel, GLHIP_EINVAL for what the entry point rejects (negative sizes, D < 1, bad dtype).
 * glhip_plan_apply and glhip_plan_apply_nd keep refusing p = 1.
 */
int glhip_plan_apply_p1_supported(int B, long N, long M, int D, int V, int dtype, int n_ranges);
int glhip_plan_apply_p1_pass_width(void);
size_t glhip_plan_apply_p1_workspace_bytes(int B, int N, int M, int D, int V);
int glhip_plan_apply_p1(const void* x, const void* y, const float* h, const float* feat, float* out, float* softmin,
                        int B, int N, int M, int D, int V, float eps, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * Kernel-matrix × vector product  out[b,i] = sum_j k(x[b,i], y[b,j]) * v[b,j].
 *
 * Replaces: `K @ v` on a KeOps LazyTensor K (kernel_samples.py:128,130,132,136-137)
 *   with K from gaussian_kernel / laplacian_kernel / energy_kernel (:62-82),
 *   optionally block-sparse (K.ranges = ranges, :66-67,75-76).
 *   The transposed product K^T @ a (:135-137) is the same call with x and y swapped.
 *
 *   v (B,M) fp32, out (B,N) fp32.
 *   gaussian: matrix cores for D <= 4095 (glhip_softmin_xk.h from D = 17 on, version 121); laplacian / energy: matrix-core distances for block-sparse D <= 3 launches with
 *   GLHIP_FLAG_MFMA_DIST and for dense launches of 4 <= D <= 16 (glhip_dist_xd.h, round 5); explicit differences elsewhere.
 */
int glhip_kernel_conv_fwd(int kind, const void* x, const void* y, const float* v, float* out,
                          int B, int N, int M, int D, float blur, int in_dtype,
                          const int32_t* ranges_i, const int32_t* slices_i,
                          const int32_t* redranges_j, int n_ranges,
                          void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * Gradient of sum_i g_i * out_i (out from glhip_kernel_conv_fwd) with respect to x:
 *   grad_x[b,i,:] = g[b,i] * sum_j v[b,j] * dk/dx(x_i, y_j),
 *   with the convention d|z|/dz = 0 at z = 0 (what KeOps' Norm2 gradient returns and what the
 *   clamp at utils.py:61 yields in the dense code).
 * The gradient with respect to y is the same call with (x,g) and (y,v) swapped; the gradient
 * with respect to v is glhip_kernel_conv_fwd with x and y swapped and v := g.
 * Replaces: KeOps autograd of the reductions at kernel_samples.py:128-137.
 * D > 16 runs the one-thread-per-row kernel of glhip_generic.h.  GLHIP_FLAG_XK_GRAD (version 130) routes the GAUSSIAN gradient of
 * 17 <= D <= 4095, dense launches, B <= 65535, without GLHIP_FLAG_NO_MFMA / _DIRECT, to the matrix cores instead: xk_plan_kernel on
 * XkGaussGradParams (glhip_gauss_grad_xk.h) — the exponents of the gaussian product, features v_j (y_j - centre), the signed sum
 * sum_j k_ij v_j, and g_i / blur^2 [ S_i - (x_i - centre) U_i ] at the end; 64 coordinates per pass, float32 and bfloat16 clouds, both
 * exponent layouts (GLHIP_FLAG_F16X2 under its range contract).  A row that no column reaches writes 0.  The same flag makes
 * glhip_kernel_conv_fwd_grad below accept those launches.  Opt-in at this level, as for glhip_softmin_bwd_x: the exponents of a long
 * MFMA chain are bounded by max(5e-6, 4 x the error of plain float32 arithmetic), not by a flat 5e-6.
 *   glhip_kernel_conv_grad_uses_xk: host arithmetic only, the very predicate both entry points evaluate — 1: that kernel; 0: the launch
 *   of version 129; GLHIP_EINVAL: a bad kind or dtype, negative sizes, D < 1.
 *   glhip_kernel_conv_grad_workspace_bytes: the split partials of the widest pass of that route (sums of <= 64 coordinates, signed
 *   mass, row maximum per row and split), never more than 1 GiB, 0 where the predicate is 0 or under GLHIP_FLAG_NO_SPLIT.  NULL or a
 *   short workspace: fewer or no splits, the same results up to summation order.  M == 0 zeroes grad_x (and out).
 */
/* GLHIP_FLAG_XK_DIST_GRAD (version 132): the predicate, the workspace and the pass width of xk_dist_grad_kernel (glhip_dist_grad_xk.h).
 *   glhip_dist_grad_uses_xk: host arithmetic only, the very predicate glhip_softmin_bwd_x (op GLHIP_DIST_GRAD_SOFTMIN_P1, asked for p == 1) and
 *   glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad (laplacian, energy) evaluate — 1: that kernel (dense, 17 <= D <= 4095, B <= 65535, the
 *   flag set, neither GLHIP_FLAG_NO_MFMA nor _DIRECT); 0: the launch of version 131; GLHIP_EINVAL: a bad op or dtype, negative sizes, D < 1.
 *   glhip_dist_grad_workspace_bytes: the split partials of the widest pass (the direction sums of <= glhip_dist_grad_pass_width()
 *   coordinates, one scalar — the normaliser Z, or the product — and the row maximum per row and split), never more than 1 GiB, 0 where the
 *   predicate is 0 or under GLHIP_FLAG_NO_SPLIT.  NULL or a short workspace: fewer or no splits.  M == 0 zeroes grad_x (and out).
 *   Results are bit-identical run to run.  Pairs inside the clamp (|x - y|^2 <= 1e-8 in the kernel's units) get no direction. */
int glhip_dist_grad_uses_xk(int op, int B, long N, long M, int D, int dtype, int flags, int n_ranges);
size_t glhip_dist_grad_workspace_bytes(int B, int N, int M, int D, int flags);
int glhip_dist_grad_pass_width(void);
int glhip_kernel_conv_grad_uses_xk(int kind, int B, long N, long M, int D, int dtype, int flags, int n_ranges);
size_t glhip_kernel_conv_grad_workspace_bytes(int B, int N, int M, int D, int flags);
int glhip_kernel_conv_bwd_x(int kind, const void* x, const void* y, const float* v,
                            const float* g, float* grad_x,
                            int B, int N, int M, int D, float blur, int in_dtype,
                            const int32_t* ranges_i, const int32_t* slices_i,
                            const int32_t* redranges_j, int n_ranges,
                            void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * Row-wise soft-min of an explicit (B,N,M) fp32 cost matrix:
 *   out[b,i] = -eps * log sum_j exp( h[b,j] - C[b,i,j] / eps ).
 * Replaces: softmin_tensorized sinkhorn_samples.py:32-71 for CUDA tensors
 *   (the `backend="tensorized"` path, including user-supplied `cost` callables).
 */
int glhip_softmin_dense_fwd(const float* C, const float* h, float* out,
                            int B, int N, int M, float eps, void* stream);

/*
 * Soft-min AND its gradient with respect to the row points in ONE pass (p = 2, D <= 16), for callers that know the answer
 * approximately — the last, differentiable update of the Sinkhorn loop (sinkhorn_divergence.py:612-623), whose previous iterate
 * bounds it: the soft-min is 1-Lipschitz in its dual vector, so |out - guess| <= margin := sup_j |h_j - h_j(previous)| * eps.
 *   guess (B,N): soft-min values for the previous dual vector;  margin >= 0 (natural units, like out).
 *   out[b,i]          = -eps log sum_j exp(h_j - C_ij / eps)                      (exact, whatever the guess)
 *   grad_unit[b,i,:]  = d out[b,i] / d x[b,i,:] = sum_j P_ij (x_i - y_j)
 * The weights are formed relative to guess + margin (an upper bound of out), so none exceeds 1 and their sum is >= exp(-2 margin/eps):
 * keep margin / eps below ~25 (the caller checks; beyond that run glhip_softmin_fwd + glhip_softmin_bwd_x).  Rounding: out is
 * guess plus a correction of up to 2 margins, so it carries a few ulps of the margin (<= 4e-7 margin, measured by
 * tools/fuzz_kernels.py) on top of the error of glhip_softmin_fwd.  One reduction of the cost of glhip_softmin_bwd_x instead of a
 * forward plus a backward reduction.
 */
int glhip_softmin_fwd_grad(const void* x, const void* y, const float* h, const float* guess, float margin, float* out,
                           float* grad_unit, int B, int N, int M, int D, float eps, int p, int in_dtype,
                           const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                           void* workspace, size_t workspace_bytes, int flags, void* stream);
/*
 * Kernel product AND its gradient with respect to the row points in ONE pass (gaussian kernel, D <= 3):
 *   out[b,i]         = sum_j k(x_i, y_j) v_j                      (what glhip_kernel_conv_fwd returns)
 *   grad_unit[b,i,:] = d out[b,i] / d x[b,i,:] = -(1/blur^2) sum_j v_j k(x_i, y_j) (x_i - y_j)
 * i.e. glhip_kernel_conv_bwd_x for grad_out = 1 — the mass accumulator of that reduction IS the product.  The autograd
 * forward of the kernel norms calls this when x requires gradients; the backward pass is then grad_out[b,i] * grad_unit[b,i,:],
 * an elementwise product (kernel_samples.py:92-146 with gradients: 3 + 2 reductions become 3).
 * gaussian: matrix-core kernel (GLHIP_FLAG_NO_MFMA: explicit differences).  laplacian / energy: explicit differences with
 * |.| = m rsq(m); the product is then bit-identical to glhip_kernel_conv_fwd under GLHIP_FLAG_GRAD_FAMILY, which is what the
 * three terms of one kernel norm are sent to when gradients are on (their rounding must be common to cancel).  Coincident points (inside the 1e-4
 * clamp of utils.py:61) add k(0) v_j to the product and nothing to the gradient.  D > 3 (gaussian on the matrix cores: D > 16):
 * GLHIP_EUNSUPPORTED (call the two entry points above) — except, version 130, the gaussian kernel of 17 <= D <= 4095 under
 * GLHIP_FLAG_XK_GRAD where glhip_kernel_conv_grad_uses_xk is 1: out and grad_unit from the passes of glhip_gauss_grad_xk.h.
 */
int glhip_kernel_conv_fwd_grad(int kind, const void* x, const void* y, const float* v, float* out, float* grad_unit,
                               int B, int N, int M, int D, float blur, int in_dtype,
                               const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                               void* workspace, size_t workspace_bytes, int flags, void* stream);
/*
 * Hard C-transforms — the eps -> 0 limits of the two soft-mins above (min / max reductions, no exponential).
 *   glhip_cmin_fwd:       out[b,i] = min_j [ C(x[b,i], y[b,j]) - g[b,j] ],  C = |x-y|^2/2 (p = 2) or |x-y| (p = 1), D <= 3;
 *                         +inf over an empty column set.  Replaces the `eps == 0` branch of softmin_sample
 *                         (ot/_implementations/sample.py:156-166: `(C_xy - g_y_j).min(axis=1)` on a LazyTensor).
 *   glhip_max_lines_fwd:  out[r,i] = max_j [ g[r,j] - c(i,j) ],  c = (step (i-j))^2 (p = 2) or step |i-j| (p = 1), for R lines
 *                         of N <= 4096 samples.  Replaces the LazyTensor `.max(dim=2)` of `C_transform`
 *                         (_legacy/utils.py:116-182), applied once per image axis.
 */
int glhip_cmin_fwd(const void* x, const void* y, const float* g, float* out, int B, int N, int M, int D, int p, int in_dtype,
                   const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                   void* workspace, size_t workspace_bytes, int flags, void* stream);
int glhip_max_lines_fwd(const float* g, float* out, long R, int N, float step, int p, void* stream);
/*
 * Arg-reduction (version 129; glhip_argmin_xk.h): for every row the column of the smallest dual-shifted cost,
 *   index[b,i] = argmin_j [ |x[b,i] - y[b,j]|^2 / 2 - g[b,j] ],   value[b,i] = that minimum.
 * Replaces: KeOps' generic_argmin("SqDist(x,y)", ...) of the reference's K-means recipe
 * (examples/sinkhorn_multiscale/plot_optimal_transport_cluster.py:151-191) with g = NULL, and gives the hard correspondences of a
 * transport plan with g = dual potential + eps log weight.
 *   x (B,N,D), y (B,M,D) fp32 | bf16;  g (B,M) fp32 or NULL (= 0: nearest neighbour);  index (B,N) int32;  value (B,N) fp32 or NULL.
 *   Supported: p == 2, 1 <= D <= 4095, dense launches (n_ranges == 0), any B <= 65535; p = 1, D > 4095 and block-sparse ranges return
 *   GLHIP_EUNSUPPORTED (the range arguments are there so that block-sparse launches can follow without an ABI change).
 *   The kernel is the staging and MFMA chain of the forward reduction of 17 <= D <= 4095 (glhip_softmin_xk.h: 256 x 128 blocks, bf16 x 3
 *   pieces split on the fly, points centred per row block) for every D from 1, with a compare-and-select epilogue.
 *   Ties go to the smallest column index, whatever the number of column splits: exact duplicates among the columns return the first
 *   copy.  g[b,j] = -inf marks a column that cannot be chosen; a row without an admissible column (M == 0, every g = -inf) gets
 *   index -1 and value +inf.  N == 0 or B == 0 launches nothing.
 *   Accuracy: the exponents of glhip_softmin_xk.h with s = 1 — the cost of the returned column exceeds the true minimum by at most
 *   2 (NM + 5) 2^-24 (diam^2 + max |g|), NM = ceil((6 + 6 D) / 16), and value is within that of the minimum.
 *   flags: GLHIP_FLAG_NO_SPLIT; GLHIP_FLAG_F16X2 is accepted and ignored (bf16 x 3 only: no range precondition); others are ignored.
 *   Workspace: glhip_argmin_workspace_bytes holds the (exponent, index) partials of the column splits the launch would like; NULL or
 *   short means fewer or no splits, with the same results index for index.
 * glhip_argmin_supported: host arithmetic only, the predicate the launch itself evaluates — 1 / 0, GLHIP_EINVAL for what the entry
 * point rejects (negative sizes, D < 1, a bad p or dtype).
 */
int glhip_argmin_supported(int B, long N, long M, int D, int p, int dtype, int n_ranges);
size_t glhip_argmin_workspace_bytes(int B, int N, int M, int D);
int glhip_argmin(const void* x, const void* y, const float* g, int32_t* index, float* value,
                 int B, int N, int M, int D, int p, int in_dtype,
                 const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                 void* workspace, size_t workspace_bytes, int flags, void* stream);
/*
 * Top-k arg-reduction (version 138; glhip_argkmin_xk.h): for every row the k columns of the smallest dual-shifted cost, best first,
 *   index[b,i,r] = column of the (r+1)-th smallest c_ij = |x[b,i] - y[b,j]|^2 / 2 - g[b,j],   value[b,i,r] = that cost.
 * Replaces: KeOps' `.argKmin(k, dim=1)` / `.Kmin_argKmin` on a LazyTensor — k nearest neighbours with g = NULL (SqDist: the squared
 * distance is 2 value), and the k heaviest entries of every row of a transport plan with g = dual potential + eps log weight, what a
 * user of the reference extracts from `ot.solve_sample(...).lazy_plan` (ot/_implementations/sample.py:562-617).
 *   x (B,N,D), y (B,M,D) fp32 | bf16;  g (B,M) fp32 or NULL (= 0);  index (B,N,k) int32;  value (B,N,k) fp32 or NULL.
 *   Supported: p == 2, 1 <= D <= 4095, dense launches (n_ranges == 0), any B <= 65535, 1 <= k <= glhip_argkmin_max_k() (16); p = 1,
 *   D > 4095, a larger k and block-sparse ranges return GLHIP_EUNSUPPORTED (the range arguments are there so that block-sparse launches
 *   can follow without an ABI change); k < 1 is GLHIP_EINVAL.
 *   The kernel is argmin's — staging, MFMA chain and exponents u_ij of glhip_softmin_xk.h, bit for bit — with another epilogue: every
 *   lane keeps a sorted list of 4 / 8 / 16 candidates per row in registers (the smallest capacity that holds k), filtered by one
 *   compare against the list's last entry; lane halves, the workgroup's column halves and the column splits merge k-lists.
 *   Order: entries are sorted by (u descending, index ascending), u the float32 exponent of the kernel — the rule of glhip_argmin.
 *   So the result of a call with k is the first k entries of a call with any larger k, k = 1 is glhip_argmin (index and value), bit for
 *   bit both, and exact duplicates among the columns come in ascending index order.  u_ij does not depend on the tile or split a column
 *   falls into: the result is the same with any number of column splits, under GLHIP_FLAG_NO_SPLIT, with a short or NULL workspace.
 *   g[b,j] = -inf marks a column that is never returned; NaN exponents never enter a list; a row with fewer than k admissible columns
 *   (M < k, masks, M == 0) fills its last ranks with index -1 and value +inf.  N == 0 or B == 0 launches nothing.
 *   Accuracy: per entry that of glhip_argmin — the cost of the column at rank r is within 2 (NM + 5) 2^-24 (diam^2 + max |g|) of the
 *   row's (r+1)-th smallest cost, NM = ceil((6 + 6 D) / 16), and value is within that of the same number.
 *   flags: GLHIP_FLAG_NO_SPLIT; GLHIP_FLAG_F16X2 is accepted and ignored (bf16 x 3 only: no range precondition); others are ignored.
 *   Workspace: glhip_argkmin_workspace_bytes (<= 1 GiB) holds the k (exponent, index) partials per row of the column splits the launch
 *   would like; NULL or short means fewer or no splits, with the same results.
 * glhip_argkmin_supported: host arithmetic only, the predicate the launch itself evaluates — 1 / 0, GLHIP_EINVAL for what the entry
 * point rejects (negative sizes, D < 1, k < 1, a bad p or dtype).
 */
int glhip_argkmin_max_k(void);
int glhip_argkmin_supported(int B, long N, long M, int D, int k, int p, int dtype, int n_ranges);
size_t glhip_argkmin_workspace_bytes(int B, int N, int M, int D, int k);
int glhip_argkmin(const void* x, const void* y, const float* g, int32_t* index, float* value,
                  int B, int N, int M, int D, int k, int p, int in_dtype,
                  const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                  void* workspace, size_t workspace_bytes, int flags, void* stream);
/*
 * The plan of a p = 2 soft-min contracted with a bilinear per-pair weight (version 139; glhip_plan_bilinear_xk.h) — the one reduction
 * behind the gradients of `P @ S` and of the barycentric map with respect to the points and the potentials (geomloss_amd/transport.py):
 *     w_ij   = exp(h_j - |x_i - y_j|^2 / (2 eps) + fwd_i / eps)
 *     pi_ij  = w_ij / sum_j w_ij                    (normalised by the recomputed mass, as every plan kernel: fwd only centres the weights)
 *     tau_ij = <rowfeat[b,i,:], colfeat[b,j,:]>
 *     out[b,i,:] = sum_j pi_ij tau_ij (y_j - x_i)           wsum[b,i] = sum_j pi_ij tau_ij          (wsum may be NULL)
 *   x (B,N,D), y (B,M,D) fp32 | bf16;  h (B,M), fwd (B,N) fp32;  rowfeat (B,N,K), colfeat (B,M,K) fp32 always;  out (B,N,D), wsum (B,N) fp32.
 *   Supported: p == 2, dense launches, any B <= 65535, 1 <= D <= 4095, 0 <= K <= 4095.  ONE kernel for the whole range of D.  p = 1,
 *   block-sparse ranges (the arguments are in the ABI for later), D or K > 4095 and B > 65535 return GLHIP_EUNSUPPORTED.
 *   The exponents come from the K-chunked matrix-core chain of glhip_softmin_xk.h (GLHIP_FLAG_F16X2 applies to them alone), tau from a second
 *   run of that chain over the features (uncentred, always bf16 x 3: float32 accuracy, no range contract), and the product w tau — split
 *   into two f16 pieces relative to a running per-row maximum of its magnitude, so that features of any finite magnitude neither overflow
 *   nor flush — meets the centred coordinates in the second MFMA product of glhip_plan_apply.h.  One pass over the columns per
 *   glhip_plan_bilinear_pass_width() coordinates (32; a remainder is a pass of its own); every pass recomputes both chains.
 *   Accuracy: within 4 x the error of plain float32 arithmetic on the same expression, relative to the unsigned sums
 *   max_{i,d} sum_j pi_ij |tau_ij| |y_j[d] - x_i[d]| (out) and max_i sum_j pi_ij |tau_ij| (wsum).
 *   A row without mass (every h_j = -inf; its fwd is +inf) gets 0 in both outputs, never NaN; a column with h_j = -inf weighs exactly 0
 *   whatever finite colfeat_j it holds.  No float atomics: results are bit-identical run to run.
 *   N == 0 or B == 0 launches nothing; M == 0 or K == 0 with N > 0 zeroes out and wsum.
 *   flags: GLHIP_FLAG_NO_SPLIT, GLHIP_FLAG_F16X2 (the caller vouches for the range of the clouds, as everywhere); others are ignored.
 * glhip_plan_bilinear_workspace_bytes holds the split partials (T[nv], W, mass, m) only and never asks for more than 1 GiB; 0 for
 * unsupported or empty shapes; NULL or a short buffer means fewer or no splits, with the same results up to summation order.
 * glhip_plan_bilinear_supported: host arithmetic only, the predicate the launch itself evaluates — 1, 0 for valid requests without a
 * kernel, GLHIP_EINVAL for what the entry point rejects (negative sizes, D < 1, K < 0, a bad p or dtype).
 * Not here: gradients with respect to the weights, second derivatives, float64, a resident-operand variant for D <= 16.
 */
int glhip_plan_bilinear_supported(int B, long N, long M, int D, int K, int p, int dtype, int n_ranges);
int glhip_plan_bilinear_pass_width(void);
size_t glhip_plan_bilinear_workspace_bytes(int B, int N, int M, int D, int K);
int glhip_plan_bilinear(const void* x, const void* y, const float* h, const float* fwd, const float* rowfeat, const float* colfeat,
                        float* out, float* wsum, int B, int N, int M, int D, int K, float eps, int p, int in_dtype,
                        const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                        void* workspace, size_t workspace_bytes, int flags, void* stream);
/*
 * The cluster pyramid of the two-scale ("multiscale") backends, on the device.
 *
 * glhip_grid_cluster — voxel clustering of a weighted cloud.  Replaces the chain
 *   pykeops.torch.cluster.grid_cluster -> cluster_ranges_centroids -> sort_clusters
 * of `clusterize`, sinkhorn_samples.py:453-490, and kernel_samples.py:214-236: points are binned in cubic voxels of edge
 * `voxel` (bin of a coordinate c: floor((c / pre_div) / voxel); kernel_multiscale clusters x / blur, sinkhorn passes 1),
 * clusters are numbered in lexicographic voxel order (first axis most significant), and the cloud is sorted by cluster with
 * a STABLE sort, so that cluster k is the contiguous row range [ranges[2k], ranges[2k+1]) of the sorted cloud.
 *   x (N,D) fp32|bf16, D <= 3;  weights (N) fp32 or NULL (all ones)
 *   perm (N) int32 out: sorted row p is input row perm[p];   x_sorted (N,D) / w_sorted (N) out, may be NULL
 *   ranges (N,2) int32, centroids (N,D) fp32 (weighted means of x / pre_div), weights_c (N) fp32: the first C rows are
 *   written, C <= N = the number of non-empty voxels;  n_clusters (8) int32 out: {C, overflow, qmin[3], qmax[3]} — overflow != 0
 *   means a voxel coordinate exceeded 2^21 bins along an axis (result invalid; use a larger voxel); qmin / qmax are the smallest
 *   and largest voxel index of the cloud along each axis (0 beyond D; since version 114): the cloud lies in the box
 *   [qmin voxel pre_div, (qmax + 1) voxel pre_div) — its bounding box to one voxel, which is how a caller that was GIVEN a
 *   diameter (it only parametrises the schedule, _legacy/sinkhorn_divergence.py:154-163) learns the true extent of the data
 *   before vouching for GLHIP_FLAG_F16X2, in the round trip that reads C anyway.
 * Sums are accumulated in float64 in a fixed order: the same inputs give the same centroids bit for bit.  Nothing comes
 * back to the host: read n_clusters when the sizes are needed.  workspace: glhip_cluster_workspace_bytes(N, D).
 *
 * glhip_block_ranges — a keep rule on pairs of clusters -> block-sparse reduction ranges for both orientations.
 * Replaces `keep = ...` + pykeops.torch.cluster.from_matrix at sinkhorn_samples.py:512-530 (GLHIP_KEEP_DUAL_SLACK:
 * keep (i,j) iff f_i + g_j > C(rows_i, cols_j) - thr, C the cost of exponent p on the centroids, thr = truncate * eps) and
 * kernel_samples.py:244-256 (GLHIP_KEEP_WITHIN: keep iff |rows_i - cols_j|^2 <= thr, thr = (truncate + cell diameter)^2).
 *   rows (Cr,D), cols (Cc,D) fp32 centroids;  f (Cr), g (Cc) dual values (dual slack only);
 *   ranges_rows (Cr,2), ranges_cols (Cc,2): row ranges of the clusters in their sorted clouds;
 *   out: slices_rows (Cr) + red_cols (capacity,2) = the (slices_i, redranges_j) of a reduction over the columns of every
 *        row cluster, slices_cols (Cc) + red_rows (capacity,2) = the same for the transposed reduction.  Kept column
 *        clusters that are adjacent in memory are merged into one interval (same pair set, fewer and longer tiles).
 *   capacity: intervals each `red_*` array can hold (64-bit); Cr * ((Cc + 1) / 2) (resp. Cc * ((Cr + 1) / 2)) always suffices,
 *             glhip_block_ranges_count gives the exact number.
 *   status (1) int32 out: != 0 if capacity was exceeded (intervals beyond it are dropped, never written out of bounds).
 *   slices_cols == red_rows == NULL (since version 117): the row-major pattern only — for symmetric patterns (rows = cols, f = g: the
 *   debiasing terms C_xx, C_yy of sinkhorn_divergence.py:284-289), whose transposed pattern is the same arrays.
 */
#define GLHIP_KEEP_DUAL_SLACK 0
#define GLHIP_KEEP_WITHIN 1
size_t glhip_cluster_workspace_bytes(int N, int D);
int glhip_grid_cluster(const void* x, const float* weights, int N, int D, int in_dtype, float pre_div, float voxel,
                       int32_t* perm, void* x_sorted, float* w_sorted, int32_t* ranges, float* centroids,
                       float* weights_c, int32_t* n_clusters, void* workspace, size_t workspace_bytes, void* stream);
int glhip_block_ranges(int kind, const float* rows, const float* cols, const float* f, const float* g, int Cr, int Cc,
                       int D, int p, float thr, const int32_t* ranges_rows, const int32_t* ranges_cols,
                       int32_t* slices_rows, int32_t* red_cols, int32_t* slices_cols, int32_t* red_rows, long long capacity,
                       int32_t* status, void* stream);
/* The counting half of glhip_block_ranges alone: writes the CSR offsets slices_rows (Cr) / slices_cols (Cc) and
 * totals (2) = { number of intervals of the row-major pattern, of the column-major pattern } (= the last offsets).  A caller that
 * reads `totals` back can size red_cols / red_rows exactly instead of for the worst case (which is quadratic in the number of
 * clusters: 3.2 GB at 2e4 clusters a side) and then call glhip_block_ranges with capacity = max(totals). */
int glhip_block_ranges_count(int kind, const float* rows, const float* cols, const float* f, const float* g, int Cr, int Cc,
                             int D, int p, float thr, const int32_t* ranges_rows, const int32_t* ranges_cols,
                             int32_t* slices_rows, int32_t* slices_cols, int32_t* totals, void* stream);

/* Pairs of POINTS the keep rule of glhip_block_ranges retains (same arguments), without building the intervals:
 * kept (3) int64 out = { sum over the kept cluster pairs (i, j) of |rows_i| x |cols_j|,  sum_i |rows_i|^2,  sum_j |cols_j|^2 }.
 * The reference prints the first figure at the level of clusters when verbose (sinkhorn_samples.py:516-522); the host side costs a
 * block-sparse fine level against a dense one with it BEFORE building the pattern (geomloss_amd/sinkhorn_samples.py:
 * kernel_truncation; `truncate=None` at :504-505 is the dense one).  The other two give the size of the block a typical PAIR lives in
 * (sum of squares / number of points), which is what GLHIP_FLAG_SMALL_ROW_BLOCKS is set from. */
int glhip_block_ranges_kept_pairs(int kind, const float* rows, const float* cols, const float* f, const float* g, int Cr, int Cc,
                                  int D, int p, float thr, const int32_t* ranges_rows, const int32_t* ranges_cols, long long* kept,
                                  void* stream);

/* ---- the four reductions in DOUBLE precision (round 4) ---------------------------------------------------------------------
 * The reference's matrix-free backends keep the dtype of their inputs: float64 clouds are reduced in float64 by KeOps
 * (softmin_online_lazytensor, sinkhorn_samples.py:229-290, `.logsumexp` on LazyTensors of the input dtype; lse_genred :322-334
 * with dtype = float64; kernel_online, kernel_samples.py:128-137).  These entry points are that path: every array — clouds, dual
 * vector / weights, gradients, outputs — is `double`; same argument meaning, ranges convention and semantics (clamp of
 * utils.py:61, zero direction at clamped pairs) as glhip_softmin_fwd / glhip_softmin_bwd_x / glhip_kernel_conv_fwd /
 * glhip_kernel_conv_bwd_x above; any D up to 4095 (D > 16 since round 5: run-time coordinate loops, slower); no workspace, no flags.
 * 1 to 64 threads per row, explicit differences, no matrix cores: ~5e11 pairs/s, for callers who need the digits.  Of the fused entry points
 * only the half-step has a float64 form (below); iteration and value + gradient: compose these. */
int glhip_softmin_fwd_f64(const double* x, const double* y, const double* h, double* out, int B, int N, int M, int D, double eps, int p,
                          const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges, void* stream);
/* glhip_sinkhorn_step in double precision (round 6): out_i = damping * t_i (prev == NULL) or (prev_i + damping * t_i) / 2, with
 * t = soft-min(eps, C(x,y), logw + pot / eps) (pot == NULL: logw alone); out must not alias prev.  One launch instead of the soft-min
 * and five elementwise float64 torch kernels per half-step of sinkhorn_divergence.py:461-465,480-493. */
int glhip_sinkhorn_step_f64(const double* x, const double* y, const double* logw, const double* pot, const double* prev, double* out,
                            int B, int N, int M, int D, double eps, double damping, int p, const int32_t* ranges_i,
                            const int32_t* slices_i, const int32_t* redranges_j, int n_ranges, void* stream);
/* (a row without mass — every h_j = -inf, saved forward value +inf — gets grad_x = 0, never NaN) */
int glhip_softmin_bwd_x_f64(const double* x, const double* y, const double* h, const double* out, const double* grad_out, double* grad_x,
                            int B, int N, int M, int D, double eps, int p, const int32_t* ranges_i, const int32_t* slices_i,
                            const int32_t* redranges_j, int n_ranges, void* stream);
int glhip_kernel_conv_fwd_f64(int kind, const double* x, const double* y, const double* v, double* out, int B, int N, int M, int D,
                              double blur, const int32_t* ranges_i, const int32_t* slices_i, const int32_t* redranges_j, int n_ranges,
                              void* stream);
int glhip_kernel_conv_bwd_x_f64(int kind, const double* x, const double* y, const double* v, const double* grad_out, double* grad_x, int B,
                                int N, int M, int D, double blur, const int32_t* ranges_i, const int32_t* slices_i,
                                const int32_t* redranges_j, int n_ranges, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GLHIP_H */
