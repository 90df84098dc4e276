"""``geomloss_amd.hip`` is the one name under which the package, the tests, the tools and bench.py reach the binding; its leaves live in
private modules (``_glhip``, ``_perm_cache``, ``_graphs``) and are re-exported.  The list below is every name the module had before
that split — ``sorted(n for n in vars(hip) if not n.startswith("__"))`` — and each must stay an attribute.  No GPU, no built library."""

from geomloss_amd import _glhip, hip

NAMES = """
    ARGMIN_MAX_DIM BF16 BlockRanges DIST_GRAD_OPS DIST_XK_MAX_DIM ENERGY ENV_FLAGS F32 FAMILY_DIST FAMILY_GENERIC FAMILY_VALU
    FAMILY_X32 FAMILY_XD FAMILY_XK FLAG_DIRECT FLAG_F16X2 FLAG_F32_MFMA FLAG_GRAD_FAMILY FLAG_MFMA_DIST FLAG_NO_MFMA FLAG_NO_SORT
    FLAG_NO_SPLIT FLAG_PREPACK FLAG_SMALL_ROW_BLOCKS FLAG_XDL16 FLAG_XK_DIST FLAG_XK_DIST_GRAD FLAG_XK_GRAD GAUSSIAN GraphCache
    Iter4Plan KEEP_DUAL_SLACK KEEP_WITHIN KERNEL_KINDS LAPLACIAN LIB_PATH MFMA_FWD_MAX_DIM PERM_CACHE_ENTRIES PERM_HINT_X
    PERM_HINT_Y PLAN_MAX_DIM SIGNATURES XD_MAX_DIM _BBOX_MAX_POINTS _DIST_COL_CHUNKS _DIST_MIN_PAIRS _DIST_MIN_ROWS
    _DIST_ROWS_PER_VOXEL _DIST_SLAB _GAUSS_SORT_MIN_PAIRS _HERE _KernelConv _Last4 _LseLines _NO_RANGES _PermCache _RANGES
    _RANGES_WORST_CASE_MAX _SINCE _SMALL_ENDS_MAX _SinkhornCost _Softmin _SoftminBwdX _SoftminDense _SoftminValueGrad _TAIL
    _VALUE_GRAD_MAX_MARGIN _VALUE_GRAD_MIN_PAIRS _acc_dtype _as_batched _bwd_x _c_double _c_float _c_int _c_long _c_size _check
    _conv_grad_routes _cost_raw _dist_on_mfma _dtype_code _f32 _fuse_kernel_grad _gauss_compact_rows _grad_workspace _lib
    _perm_cache _perm_plan _plan_apply _plan_apply_call _plan_moments _points _range_args _range_flags _route_predicate _serpentine
    _stream _unsort_rows _vec _voxel_for _vp _workspace _worst_case_intervals argmin argmin_supported autosort_applies
    block_ranges_raw bounding_box bounding_box_applies cmin compact_order ctypes dist_grad_uses_xk forget_permutations
    fused_step_applies grid_cluster_raw half_step_applies is_f64 kept_pairs_raw kernel_conv kernel_conv_bwd_x_raw
    kernel_conv_fwd_family kernel_conv_fwd_grad_raw kernel_conv_fwd_raw kernel_conv_grad_uses_xk kernel_conv_row_gradient
    kernel_conv_with_unit kernel_grad_fusion library_available load_library log_weights_raw lse_lines max_lines once_differentiable
    os perm_cache_enabled perm_cache_key perm_cache_stats plan_apply plan_apply_applies plan_apply_nd plan_apply_nd_applies
    plan_apply_nd_family plan_apply_nd_raw plan_apply_raw read_back set_distance_on_mfma set_kernel_grad_fusion settle_host
    sinkhorn_cost_fused sinkhorn_extrapolate4 sinkhorn_extrapolate4_raw sinkhorn_iter4 sinkhorn_iter4_raw sinkhorn_last4
    sinkhorn_step sinkhorn_step_raw small_ends_apply softmin softmin_bwd_x_raw softmin_bwd_x_uses_plan softmin_dense
    softmin_dense_fwd_raw softmin_fwd_family softmin_fwd_grad_raw softmin_fwd_raw softmin_perm_applies softmin_value_and_grad
    stable_clouds torch voxel_extent warnings
""".split()


def test_every_name_of_the_binding_is_still_reachable():
    assert len(NAMES) == len(set(NAMES)) == 172
    missing = [n for n in NAMES if not hasattr(hip, n)]
    assert not missing, missing


def test_the_moved_names_are_the_same_objects():
    # tools delete keys from hip.SIGNATURES before hip.load_library(): one dict, not a copy
    assert hip.SIGNATURES is _glhip.SIGNATURES and hip._SINCE is _glhip._SINCE
    assert hip.load_library is _glhip.load_library and hip.bind is _glhip.bind and hip._check is _glhip._check
    assert hip._lib is _glhip._lib      # the loaded library (None before the first load), read through
