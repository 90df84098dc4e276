"""Host arithmetic of ``glhip_argkmin`` beyond k = 16 (version 141; geomloss_amd/csrc/glhip_api_argkmin.hip) through the library.  No device."""
import pytest

from geomloss_amd import hip


def test_passes_limit_and_support():
    lib = hip.load_library()
    assert [lib.glhip_argkmin_passes(k) for k in (1, 16, 17, 32, 33, 128)] == [1, 1, 2, 2, 3, 8]
    assert lib.glhip_argkmin_passes(0) == -1 == lib.glhip_argkmin_passes(129)      # GLHIP_EINVAL
    assert lib.glhip_argkmin_max_k() == 128 == hip.ARGKMIN_MAX_K
    assert hip._SINCE["glhip_argkmin_passes"] == 141 <= lib.glhip_version() and hip.argkmin_passes(40) == 3
    with pytest.raises(ValueError):
        hip.argkmin_passes(129)
    assert all(lib.glhip_argkmin_supported(1, 1000, 2000, D, k, 2, 0, 0) == 1 for D in (1, 17, 4095) for k in (17, 128))


def split_bytes(N, M, k):
    """One pass of k <= 16 ranks, B = 1, by glhip_split_policy.h: choose_splits; from 65536 columns on also xcd_splits and 8; <= 32, <= 1 GiB."""
    blocks, per_split, slots = (N + 255) // 256, N * 2 * k * 4, 512 if k <= 4 else 256
    fit = min(2**30 // per_split, 32)
    ns = 1 if blocks >= 4 * 768 and M <= 16384 else max(min(-(-256 * 4 * 10 // blocks), M // 512, 32, fit), 1)
    if M >= 65536 and fit >= 8:
        best, best_eff = 8, 0.0
        for nx in range(8, min(fit, M // 2048, 32) + 1, 8):
            eff = (blocks * nx / slots) / -(-blocks * nx // slots)
            if eff >= 0.93 or eff > best_eff + 0.02:
                best, best_eff = nx, eff
            if eff >= 0.93:
                break
        ns = max(ns, best, 8)
    return ns * per_split if ns >= 2 else 0


def test_workspace_bytes():
    ws = hip.load_library().glhip_argkmin_workspace_bytes
    for N, M in ((40, 5000), (3000, 20000), (200000, 200000), (10**6, 10**6), (300, 129)):      # k <= 16: what version 138 sized
        for k in (1, 4, 5, 8, 16):
            assert ws(1, N, M, 24, k) == split_bytes(N, M, k), (N, M, k)
    assert ws(1, 300, 129, 3, 17) >= 300 * 8      # k > 16: the floors of every row, split or not
    for N, M in ((40, 5000), (3000, 20000), (200000, 200000)):
        sizes = [ws(1, N, M, 24, k) for k in range(1, 129)]
        assert sizes == sorted(sizes), (N, M)
    for N in (40, 3000, 200000):      # the M ladder of tests/test_argkmin_cpu.py
        for k in (17, 20, 64, 128):
            sizes = [ws(1, N, M, 24, k) for M in (1, 100, 511, 1024, 5000, 20000, 65535, 65536, 200000, 10**6)]
            assert sizes == sorted(sizes), (N, k, sizes)
    assert ws(1, 10**6, 10**6, 64, 128) - 10**6 * 8 <= 2**30      # (8e6 is a multiple of 256)
