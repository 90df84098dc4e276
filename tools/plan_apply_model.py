"""NumPy model of the split arithmetic of the plan-application kernel (geomloss_amd/csrc/glhip_plan_apply.h): what the second MFMA
product makes of fp32 weights and fp32 features.

    pieces     every value = TWO f16 pieces, hi = f16(v) and lo = f16(v - hi), both rounded to nearest even, subnormal pieces kept
    products   three: lo hi, hi lo, hi hi (an f16 x f16 product is exact in fp32); lo lo is dropped
    scaling    weights are relative to the largest weight of their row and carry 2^13 (kWqShift); features carry a power of two per feature column and LDS tile of `tile` columns that puts
               the largest |f| of the tile's column into [2^14, 2^15) (plan_scale_exponent: biased exponent clamped to [1, 240]);
               both are undone on the block result, exactly

The accumulation is modelled exactly (float64): the model isolates what the SPLIT loses — the dropped product and the bits beyond the
two pieces — from the fp32 accumulation of the MFMA and of the per-block v_fma_f32, which the GPU tests bound together with the
exponents.

    python tools/plan_apply_model.py        # worst column error of the test inputs, relative to max_i sum_j w_ij |f_jv|
"""
import numpy as np

WQ_SHIFT = 13


def split2(v):
    """fp32 array -> (hi, lo) as float64 arrays holding f16 values: hi = f16(v), lo = f16(v - hi), round to nearest even."""
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)      # the difference is exact in fp32
    return hi.astype(np.float64), lo.astype(np.float64)


def scale_exponent(max_abs):
    """Biased exponent of the power-of-two scale for a tile column whose largest |f| is max_abs (fp32 array)."""
    e = (np.asarray(max_abs, dtype=np.float32).view(np.uint32) >> 23).astype(np.int64)
    return np.clip(127 + 14 - (e - 127), 1, 254 - WQ_SHIFT - 1)


def product(w, feat, tile=128):
    """The kernel's w @ feat for fp32 weights w (N, M) and fp32 features feat (M, V), tile by tile of `tile` columns (128; 64 when a pass
    carries four chunks): the kept piece products, summed in float64."""
    w = np.asarray(w, dtype=np.float32)
    feat = np.asarray(feat, dtype=np.float32)
    top = w.max(1, keepdims=True)                      # the kernel's running maximum, at the end of the row
    top = np.where(top > 0, top, np.float32(1.0))
    whi, wlo = split2((w / top) * np.float32(2.0 ** WQ_SHIFT))
    out = np.zeros((w.shape[0], feat.shape[1]))
    for j0 in range(0, feat.shape[0], tile):
        f = feat[j0:j0 + tile]
        se = scale_exponent(np.abs(f).max(0))
        sc = np.ldexp(1.0, se - 127).astype(np.float32)
        fhi, flo = split2(f * sc[None, :])
        a, b = whi[:, j0:j0 + tile], wlo[:, j0:j0 + tile]
        out += (a @ flo + b @ fhi + a @ fhi) * np.ldexp(1.0, 127 - WQ_SHIFT - se)[None, :]
    return out * top.astype(np.float64)


def weights(x, y, h, eps):
    """Exact float64 plan rows W = exp(E - lse(E)), E_ij = h_j - |x_i - y_j|^2 / (2 eps), rounded to fp32 as the kernel holds them."""
    x, y, h = (np.asarray(t, dtype=np.float64) for t in (x, y, h))
    E = h[None, :] - ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1) / (2.0 * eps)
    E -= E.max(1, keepdims=True)
    W = np.exp(E)
    return (W / W.sum(1, keepdims=True)).astype(np.float32)


def matrix_part_error(w, feat, tile=128):
    """Per feature column: max_i |model - exact| / max_i sum_j w_ij |f_jv| for the fp32 weights w (exact = float64 product of the
    same fp32 numbers)."""
    w64, f64 = w.astype(np.float64), np.asarray(feat, dtype=np.float32).astype(np.float64)
    exact = w64 @ f64
    scale = (w64 @ np.abs(f64)).max(0)
    err = np.abs(product(w, feat, tile) - exact).max(0)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err)


def _clouds(seed, N, M, D):      # tests/test_hip_kernels.py::_clouds
    rng = np.random.default_rng(seed)
    x = rng.random((N, D)).astype(np.float32)
    y = (rng.random((M, D)) * 0.8 + 0.1).astype(np.float32)
    h = rng.standard_normal(M).astype(np.float32)
    return x, y, h


if __name__ == "__main__":
    worst = 0.0
    for eps in (0.01, 0.0025):
        x, y, h = _clouds(0, 300, 257, 3)
        f = np.random.default_rng(1).standard_normal((257, 6)).astype(np.float32)
        f[:, 0] *= 1e12
        f[:, 1] *= 1e-12
        for tile in (128, 64):
            e = matrix_part_error(weights(x, y, h, eps), f, tile)
            print(f"eps = {eps}, tiles of {tile}: worst column error {e.max():.2e}")
            worst = max(worst, e.max())
    print(f"worst matrix-part error {worst:.2e}")
