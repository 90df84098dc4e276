"""The Python mirror of ``include/glhip.h``: its constants, the ctypes signature of every symbol it declares, and the loader of
``libgeomloss_hip.so``.  Private: the rest of the package, the tests and the tools reach all of it as ``geomloss_amd.hip.NAME``
(``hip.py`` re-exports every name, ``SIGNATURES`` as this very dict).  Nothing here needs torch or a GPU.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgeomloss_hip.so")

GAUSSIAN, LAPLACIAN, ENERGY = 0, 1, 2
KERNEL_KINDS = {"gaussian": GAUSSIAN, "laplacian": LAPLACIAN, "energy": ENERGY}
F32, BF16 = 0, 1
FLAG_DIRECT, FLAG_NO_MFMA, FLAG_NO_SPLIT, FLAG_F32_MFMA, FLAG_XDL16, FLAG_PREPACK, FLAG_MFMA_DIST, FLAG_SMALL_ROW_BLOCKS = 1, 2, 4, 8, 16, 32, 64, 128
FLAG_F16X2 = 256                # exponents from two f16 pieces per coordinate; the caller vouches for the range (glhip.h)
FLAG_NO_SORT = 512              # big dense distance reductions: do not voxel-sort the clouds inside the library (glhip.h)
FLAG_XK_GRAD = 1024             # glhip_softmin_bwd_x: the p = 2 gradient of 17 <= D <= 4095 on the matrix cores (glhip_softmin_grad_xk.h);
                                # glhip_kernel_conv_bwd_x / _fwd_grad: the gaussian gradient of those dimensions (glhip_gauss_grad_xk.h)
FLAG_XK_DIST = 2048             # p = 1 soft-min / half-step, laplacian and energy products of 17 <= D <= 4095, dense launches: squared distances
                                # from the K-chunked matrix-core chain (glhip_dist_xk.h); opt-in, the gradients stay on the generic kernel
FLAG_XK_DIST_GRAD = 4096        # the p = 1 soft-min, laplacian and energy row gradients of 17 <= D <= 4095, dense launches, on the matrix cores
                                # (glhip_dist_grad_xk.h); glhip_kernel_conv_fwd_grad takes those kinds under it
DIST_GRAD_OPS = {"softmin_p1": 0, "laplacian": 1, "energy": 2}      # ops of glhip_dist_grad_uses_xk (GLHIP_DIST_GRAD_*)
FLAG_GRAD_FAMILY = FLAG_XDL16   # kernel products rounded like the product-and-gradient kernel of the same kind (glhip.h)
XD_MAX_DIM = 16                 # the fused four-softmin iteration / annealing / extrapolation, the one-pass value + gradient and the matrix-core
                                # gradients stop at this dimension (glhip_softmin_xd.h, glhip_wsum_t32.h)
MFMA_FWD_MAX_DIM = 4095         # p = 2 soft-min forward / half-step and gaussian product run on the matrix cores up to this dimension
                                # (17 ... 4095: the K-chunked kernel of glhip_softmin_xk.h; kept in step with the library by tests/test_anyd_kernels_gpu.py)
DIST_XK_MAX_DIM = 4095          # ... and under FLAG_XK_DIST the p = 1 soft-min / half-step and the laplacian / energy products too (glhip_dist_xk.h)
ARGMIN_MAX_DIM = 4095           # argmin takes p = 2 clouds of every dimension up to this one (glhip_argmin_xk.h)
PLAN_MAX_DIM = 4095             # plan_apply_nd applies p = 2 transport plans to features up to this dimension (17 ... 4095: glhip_plan_apply_xk.h)
PLAN_P1_MAX_DIM = 4095          # plan_apply_p1 applies p = 1 transport plans to features in every dimension up to this one (glhip_dist_plan_xk.h)
PLAN_BILINEAR_MAX_DIM = 4095    # plan_bilinear contracts p = 2 plans with <rowfeat_i, colfeat_j> (y_j - x_i) up to this dimension and feature count
                                # (glhip_plan_bilinear_xk.h)
# kernel families reported by softmin_fwd_family (GLHIP_FAMILY_* of glhip.h)
FAMILY_VALU, FAMILY_X32, FAMILY_XD, FAMILY_XK, FAMILY_DIST, FAMILY_GENERIC = 0, 1, 2, 3, 4, 5

# every symbol include/glhip.h declares, with its ctypes signature
_c_int, _c_float, _vp, _c_size = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
_c_long = ctypes.c_long
_RANGES = [_vp, _vp, _vp, _c_int]
_TAIL = [_vp, _c_size, _c_int, _vp]  # workspace, workspace_bytes, flags, stream
SIGNATURES = {
    "glhip_version": (_c_int, []),
    "glhip_last_error": (ctypes.c_char_p, []),
    "glhip_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_softmin_fwd_family": (_c_int, [_c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_kernel_conv_fwd_family": (_c_int, [_c_int, _c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int]),
    "glhip_prune_inspect_slots": (_c_int, [_c_int]),
    "glhip_prune_inspect": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_float, _c_int] + [_vp] * 7 + [_vp, _c_size, _vp]),
    "glhip_softmin_fwd": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int]
                          + _RANGES + _TAIL),
    "glhip_sinkhorn_step": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_float,
                                     _c_int, _c_int] + _RANGES + _TAIL),
    "glhip_sinkhorn_step_perm": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_float,
                                          _c_int, _c_int] + _RANGES + _TAIL + [_vp, _vp, _c_int]),
    "glhip_softmin_perm_applies": (_c_int, [_c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_sinkhorn_iter4": (_c_int, [_vp] * 12 + [_c_int, _c_int, _c_int, _c_int, _c_float, _c_float, _c_int, _c_int, _c_int]
                             + _TAIL),
    "glhip_sinkhorn_anneal": (_c_int, [_vp] * 6 + [_c_int] * 4 + [_vp, _vp, _c_int, _c_int, _c_int, _vp, _c_size, _c_int, _c_float, _vp]),
    "glhip_sinkhorn_extrapolate4": (_c_int, [_vp] * 14 + [_c_int] * 6 + [_c_float, _c_float, _c_int, _c_int] + _TAIL),
    "glhip_softmin_bwd_x": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int,
                                     _c_int] + _RANGES + _TAIL),
    "glhip_softmin_bwd_x_uses_plan": (_c_int, [_c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_softmin_bwd_x_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_kernel_conv_grad_uses_xk": (_c_int, [_c_int, _c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int]),
    "glhip_kernel_conv_grad_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_dist_grad_uses_xk": (_c_int, [_c_int, _c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int]),
    "glhip_dist_grad_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_dist_grad_pass_width": (_c_int, []),
    "glhip_plan_apply_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_plan_apply": (_c_int, [_vp] * 7 + [_c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int] + _RANGES + _TAIL),
    "glhip_plan_apply_nd_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_plan_apply_nd_family": (_c_int, [_c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_plan_apply_nd_pass_width": (_c_int, [_c_int]),
    "glhip_plan_apply_nd": (_c_int, [_vp] * 7 + [_c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int] + _RANGES + _TAIL),
    "glhip_plan_apply_p1_supported": (_c_int, [_c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int]),
    "glhip_plan_apply_p1_pass_width": (_c_int, []),
    "glhip_plan_apply_p1_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_plan_apply_p1": (_c_int, [_vp] * 6 + [_c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int] + _RANGES + _TAIL),
    "glhip_plan_bilinear_supported": (_c_int, [_c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_plan_bilinear_pass_width": (_c_int, []),
    "glhip_plan_bilinear_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_plan_bilinear": (_c_int, [_vp] * 8 + [_c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int] + _RANGES + _TAIL),
    "glhip_kernel_conv_fwd": (_c_int, [_c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int]
                              + _RANGES + _TAIL),
    "glhip_kernel_conv_bwd_x": (_c_int, [_c_int, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float,
                                         _c_int] + _RANGES + _TAIL),
    "glhip_softmin_fwd_grad": (_c_int, [_vp, _vp, _vp, _vp, _c_float, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int,
                                        _c_int] + _RANGES + _TAIL),
    "glhip_kernel_conv_fwd_grad": (_c_int, [_c_int, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float,
                                            _c_int] + _RANGES + _TAIL),
    "glhip_softmin_dense_fwd": (_c_int, [_vp, _vp, _vp, _c_int, _c_int, _c_int, _c_float, _vp]),
    "glhip_bounding_box": (_c_int, [_vp, _c_long, _vp, _c_long, _c_int, _c_int, _vp, _vp]),
    "glhip_log_weights": (_c_int, [_vp, _vp, _vp, _c_int, _vp]),
    "glhip_sinkhorn_cost": (_c_int, [_vp] * 7 + [_c_int] * 5 + [_vp]),
    "glhip_lse_lines_fwd": (_c_int, [_vp, _vp, ctypes.c_long, _c_int, _c_float, _c_int, _vp]),
    "glhip_lse_lines_bwd": (_c_int, [_vp, _vp, _vp, _vp, ctypes.c_long, _c_int, _c_float, _c_int, _vp]),
    "glhip_cmin_fwd": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int] + _RANGES + _TAIL),
    "glhip_max_lines_fwd": (_c_int, [_vp, _vp, ctypes.c_long, _c_int, _c_float, _c_int, _vp]),
    "glhip_argmin_supported": (_c_int, [_c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int]),
    "glhip_argmin_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int]),
    "glhip_argmin": (_c_int, [_vp] * 5 + [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int] + _RANGES + _TAIL),
    "glhip_argkmin_max_k": (_c_int, []),
    "glhip_argkmin_supported": (_c_int, [_c_int, _c_long, _c_long, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_argkmin_workspace_bytes": (_c_size, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "glhip_argkmin": (_c_int, [_vp] * 5 + [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int] + _RANGES + _TAIL),
    "glhip_cluster_workspace_bytes": (_c_size, [_c_int, _c_int]),
    "glhip_grid_cluster": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_float, _c_float] + [_vp] * 7 + [_vp, _c_size, _vp]),
    "glhip_block_ranges": (_c_int, [_c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float] + [_vp] * 6
                           + [ctypes.c_longlong, _vp, _vp]),
    "glhip_block_ranges_count": (_c_int, [_c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float] + [_vp] * 5 + [_vp]),
    "glhip_block_ranges_kept_pairs": (_c_int, [_c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float] + [_vp] * 4),
}
_c_double = ctypes.c_double
SIGNATURES.update({
    # float64 reductions (glhip_api_f64.hip): every array is double; no workspace, no flags
    "glhip_softmin_fwd_f64": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_double, _c_int] + _RANGES + [_vp]),
    "glhip_sinkhorn_step_f64": (_c_int, [_vp] * 6 + [_c_int, _c_int, _c_int, _c_int, _c_double, _c_double, _c_int] + _RANGES + [_vp]),
    "glhip_softmin_bwd_x_f64": (_c_int, [_vp] * 6 + [_c_int, _c_int, _c_int, _c_int, _c_double, _c_int] + _RANGES + [_vp]),
    "glhip_kernel_conv_fwd_f64": (_c_int, [_c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_double] + _RANGES + [_vp]),
    "glhip_kernel_conv_bwd_x_f64": (_c_int, [_c_int] + [_vp] * 5 + [_c_int, _c_int, _c_int, _c_int, _c_double] + _RANGES + [_vp]),
})
KEEP_DUAL_SLACK, KEEP_WITHIN = 0, 1
PERM_HINT_X, PERM_HINT_Y = 1, 2     # perm_flags of glhip_sinkhorn_step_perm (GLHIP_PERM_HINT_*)
# symbols younger than the oldest C-ABI that GEOMLOSS_HIP_LIB may name for an A/B run: an older build is bound without them, and the
# calls that would use them take the entry points that build has (no permutation is reused with it)
_SINCE = {"glhip_sinkhorn_step_perm": 134, "glhip_softmin_perm_applies": 134,
          "glhip_plan_apply_p1_supported": 135, "glhip_plan_apply_p1_pass_width": 135, "glhip_plan_apply_p1_workspace_bytes": 135,
          "glhip_plan_apply_p1": 135,
          "glhip_argkmin_max_k": 138, "glhip_argkmin_supported": 138, "glhip_argkmin_workspace_bytes": 138, "glhip_argkmin": 138,
          "glhip_plan_bilinear_supported": 139, "glhip_plan_bilinear_pass_width": 139, "glhip_plan_bilinear_workspace_bytes": 139,
          "glhip_plan_bilinear": 139}

_lib = None


def bind(lib, names=None):
    """Gives the functions ``names`` (default: every entry of ``SIGNATURES``) of the ``ctypes.CDLL`` ``lib`` their declared result and
    argument types; returns ``lib``.  ``AttributeError`` if the library does not export a declared symbol."""
    for name in SIGNATURES if names is None else names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return lib


def load_library(path=None):
    """Loads (once) and returns the shared library; raises ``RuntimeError`` if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("GEOMLOSS_HIP_LIB") or LIB_PATH      # GEOMLOSS_HIP_LIB: another build of the same C-ABI (A/B runs)
    if not os.path.exists(path):
        raise RuntimeError(
            f"geomloss_amd: the HIP extension {path} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C geomloss_amd/csrc`). "
            "The 'online' and 'multiscale' backends have no CPU or PyTorch fallback."
        )
    lib = ctypes.CDLL(path)
    version = int(bind(lib, ["glhip_version"]).glhip_version())
    _lib = bind(lib, [name for name in SIGNATURES if version >= _SINCE.get(name, 0) or path == LIB_PATH])
    return _lib


def library_available():
    return os.path.exists(LIB_PATH)


def _check(rc, lib):
    if rc != 0:
        msg = lib.glhip_last_error().decode()
        if rc == -1:
            raise ValueError(msg)
        if rc == -2:
            raise NotImplementedError(msg)
        raise RuntimeError(msg)
