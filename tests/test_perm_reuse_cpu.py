"""Host side of the reused permutations of the sorted p = 2 call (library 134: glhip_sinkhorn_step_perm, glhip_softmin_perm_applies;
geomloss_amd/_perm_cache.py: _PermCache; geomloss_amd/hip.py: _perm_plan).

* The clamp every kernel applies to an index it takes from a hinted permutation (csrc/glhip_perm_index.h) against a plain loop, with
  indices below 0, at n and at INT_MAX, as a stand-alone host program under the address and undefined-behaviour sanitizers (built the
  way tests/test_prep_kernels_cpu.py builds its programs).
* The cache key and the cache on CPU tensors: a view and a ``.detach()`` of the same storage hit, ``add_`` misses, a freed and
  re-allocated tensor misses, another stream id misses, more than 8 clouds evict the oldest, ``forget_permutations`` empties the cache,
  the environment switch disables it.
* ``glhip_softmin_perm_applies`` against the rule of csrc/glhip_api.hip (softmin_sorts with p == 2) restated here, on a grid of shapes
  and flags: 1 exactly for one dense problem of D <= 3, N >= 65536, N M >= 1e11 without NO_MFMA / DIRECT / NO_SORT; 0 for p = 1,
  B > 1, ranges, NO_SORT and below 1e11.
"""

import ctypes
import gc
import os
import shutil
import subprocess

import pytest
import torch

from geomloss_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "geomloss_amd", "csrc")


def _build(tmp_path_factory, name, program):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp(name)
    src = d / f"{name}.cpp"
    src.write_text(program)
    exe = d / name
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", HEADER_DIR, str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:      # a compiler without the sanitizer runtimes: the comparison is the same
        subprocess.run(base, check=True)
    return str(exe)


# ---- the clamp ---------------------------------------------------------------------------------------------------------------------------

CLAMP_PROGRAM = r"""
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "glhip_perm_index.h"
// For every n of a list: gathers and scatters through a "permutation" full of out-of-range entries, into buffers of exactly n elements
// (the sanitizer sees any access outside them), and compares every clamped index with a plain loop's.
static int32_t plain(int32_t j, int32_t n) {
    int32_t k = 0;
    if (j < 0) return 0;
    while (k < n - 1 && k < j) ++k;      // min(j, n - 1), one step at a time
    return k;
}
int main() {
    const int32_t sizes[] = {1, 2, 3, 31, 32, 1000};
    long checked = 0;
    for (int32_t n : sizes) {
        std::vector<int32_t> perm;
        for (int32_t j = -3; j <= n + 3; ++j) perm.push_back(j);
        const int32_t extra[] = {INT_MIN, INT_MIN + 1, -n, -1, 0, n - 1, n, n + 1, 2 * n, INT_MAX - 1, INT_MAX};
        for (int32_t j : extra) perm.push_back(j);
        std::vector<float> src(n), dst(n, 0.f);
        for (int32_t i = 0; i < n; ++i) src[i] = (float)i;
        for (size_t k = 0; k < perm.size(); ++k) {
            const int32_t j = glhip::perm_index(perm[k], n);
            if (j < 0 || j >= n) return 2;
            if (perm[k] >= 0 && perm[k] < n && j != perm[k]) return 3;      // a true permutation entry is untouched
            if (perm[k] > -100000 && perm[k] < 100000 && j != plain(perm[k], n)) return 4;
            if (perm[k] <= -100000 && j != 0) return 5;
            if (perm[k] >= 100000 && j != n - 1) return 6;
            const float v = src[j];      // gather
            dst[j] = v;                  // scatter
            ++checked;
        }
    }
    std::printf("%ld\n", checked);
    return 0;
}
"""


def test_clamp_keeps_every_index_in_bounds(tmp_path_factory):
    exe = _build(tmp_path_factory, "perm_clamp", CLAMP_PROGRAM)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert int(out.stdout) >= 6 * 18


# ---- the cache key and the cache -----------------------------------------------------------------------------------------------------------

@pytest.fixture
def cache(monkeypatch):
    monkeypatch.delenv("GEOMLOSS_HIP_PERM_CACHE", raising=False)
    hip.forget_permutations()
    yield hip._perm_cache
    hip.forget_permutations()


def _put(cache, t, stream=0):
    key = hip.perm_cache_key(t, stream)
    perm = torch.arange(t.shape[-2], dtype=torch.int32)
    cache.store(key, t, perm)
    return perm


def _get(cache, t, stream=0):
    return cache.lookup(hip.perm_cache_key(t, stream))


def test_views_and_detach_share_an_entry(cache):
    x = torch.rand(100, 3, requires_grad=True)
    perm = _put(cache, x[None])
    h0, m0, _ = hip.perm_cache_stats()
    for t in (x, x.detach(), x[None], x.detach()[None], x.detach().unsqueeze(0), x.view(100, 3)):
        assert _get(cache, t) is perm
    assert hip.perm_cache_stats()[:2] == (h0 + 6, m0)
    # other parts of the key: a slice (shape), a transposed view (strides), another dtype's tensor (storage), another stream
    y = torch.rand(3, 100)
    _put(cache, y)
    assert _get(cache, x[:50]) is None and _get(cache, y.t()) is None and _get(cache, x.detach().double()) is None
    assert _get(cache, x, stream=0x7F00) is None and _get(cache, x, stream=0) is perm
    assert hip.perm_cache_stats()[:2] == (h0 + 7, m0 + 4)


def test_in_place_write_misses(cache):
    x = torch.rand(64, 3)
    perm = _put(cache, x)
    assert _get(cache, x) is perm
    x.add_(1.0)
    assert _get(cache, x) is None and _get(cache, x.detach()) is None
    x2 = torch.rand(64, 3)
    _put(cache, x2)
    x2[None].mul_(1.0)                      # through a view: the counter is shared
    assert _get(cache, x2) is None


def test_freed_storage_misses_and_is_dropped(cache):
    x = torch.rand(4096, 3)
    _put(cache, x)
    ptr = x.data_ptr()
    assert hip.perm_cache_stats()[2] == 1
    del x
    gc.collect()
    again = [torch.rand(4096, 3) for _ in range(4)]      # the allocator usually hands the freed block out again
    print("address reused:", any(t.data_ptr() == ptr for t in again))
    for t in again:
        assert _get(cache, t) is None
    assert hip.perm_cache_stats()[2] == 0                 # the dead storage's entry went at the first lookup


def test_least_recently_used_goes_first(cache):
    assert hip.PERM_CACHE_ENTRIES == 8
    clouds = [torch.rand(16, 3) for _ in range(10)]
    perms = [_put(cache, t) for t in clouds[:8]]
    assert _get(cache, clouds[0]) is perms[0]            # 0 is now the most recently used, 1 the oldest
    _put(cache, clouds[8])
    assert hip.perm_cache_stats()[2] == 8
    assert _get(cache, clouds[1]) is None and _get(cache, clouds[0]) is perms[0] and _get(cache, clouds[2]) is perms[2]
    _put(cache, clouds[9])
    assert _get(cache, clouds[3]) is None and hip.perm_cache_stats()[2] == 8


def test_forget_and_the_environment_switch(cache, monkeypatch):
    x = torch.rand(16, 3)
    _put(cache, x)
    hip.forget_permutations()
    assert hip.perm_cache_stats()[2] == 0 and _get(cache, x) is None
    assert hip.perm_cache_enabled()
    monkeypatch.setenv("GEOMLOSS_HIP_PERM_CACHE", "0")
    assert not hip.perm_cache_enabled()
    before = hip.perm_cache_stats()
    assert hip._perm_plan(None, x[None], x[None], 2, None, 0) is None      # off: no library call, no lookup, no entry
    assert hip.perm_cache_stats() == before
    monkeypatch.setenv("GEOMLOSS_HIP_PERM_CACHE", "1")
    assert hip.perm_cache_enabled()


# ---- the predicate -------------------------------------------------------------------------------------------------------------------------

def _sorts_p2(B, N, M, D, p, flags, n_ranges):
    """csrc/glhip_api.hip: softmin_sorts with p == 2 (prune_applies and autosort_applies of csrc/glhip_autosort.h)"""
    nT = (M + 255) // 256
    PB = max((nT + 63) // 64, 64)
    S = 160 + (nT + PB - 1) // PB
    C = (N + 255) // 256
    prunes = float(N) * M >= 1e11 and C * S * 2 < 2**31 - 1
    auto = (B == 1 and n_ranges == 0 and D <= 3 and N >= 65536 and float(N) * M >= 5e8
            and not (flags & (hip.FLAG_NO_MFMA | hip.FLAG_DIRECT | hip.FLAG_NO_SORT)))
    return int(p == 2 and prunes and auto)


def test_predicate_is_the_sorted_p2_call():
    assert hip.library_available(), "libgeomloss_hip.so is not built"
    lib = ctypes.CDLL(hip.LIB_PATH)
    fn = lib.glhip_softmin_perm_applies
    fn.restype, fn.argtypes = hip.SIGNATURES["glhip_softmin_perm_applies"]
    fam = lib.glhip_softmin_fwd_family
    fam.restype, fam.argtypes = hip.SIGNATURES["glhip_softmin_fwd_family"]
    shapes = [(65536, 1525900), (65536, 1525878), (65535, 1600000), (1525900, 65536), (317000, 320037), (316227, 316227), (316228, 316228),
              (1000000, 1000000), (100000, 100000), (70000, 70000), (4096, 4096), (65536, 2**31 - 1), (2**31 - 1, 2**31 - 1), (20000000, 20000000)]
    flag_sets = [0, hip.FLAG_F16X2, hip.FLAG_NO_SORT, hip.FLAG_NO_MFMA, hip.FLAG_DIRECT, hip.FLAG_F16X2 | hip.FLAG_NO_SORT, hip.FLAG_PREPACK]
    n = ones = 0
    for N, M in shapes:
        for D in (1, 2, 3, 4, 16):
            for p in (1, 2):
                for B in (1, 2):
                    for n_ranges in (0, 5):
                        for flags in flag_sets:
                            for dtype in (hip.F32, hip.BF16):
                                got = fn(B, N, M, D, p, dtype, flags, n_ranges)
                                assert got == _sorts_p2(B, N, M, D, p, flags, n_ranges), (B, N, M, D, p, dtype, flags, n_ranges)
                                assert fam(B, N, M, D, p, dtype, flags, n_ranges) >= 0      # a launch the entry points accept
                                n += 1
                                ones += got
    print(f"{n} launches, {ones} of them the sorted p = 2 call")
    assert ones > 50
    # one case of each kind by name
    assert fn(1, 65536, 1525900, 3, 2, hip.F32, 0, 0) == 1 and fn(1, 317000, 320037, 2, 2, hip.BF16, hip.FLAG_F16X2, 0) == 1
    assert fn(1, 65536, 1525900, 3, 1, hip.F32, 0, 0) == 0            # p = 1
    assert fn(2, 65536, 1525900, 3, 2, hip.F32, 0, 0) == 0            # B > 1
    assert fn(1, 65536, 1525900, 3, 2, hip.F32, 0, 7) == 0            # ranges
    assert fn(1, 65536, 1525900, 3, 2, hip.F32, hip.FLAG_NO_SORT, 0) == 0
    assert fn(1, 65536, 1525878, 3, 2, hip.F32, 0, 0) == 0            # 65536 x 1525878 = 99 999 940 608 < 1e11
    # arguments the entry points reject
    for bad in ((-1, 10, 10, 3, 2, 0, 0, 0), (1, -1, 10, 3, 2, 0, 0, 0), (1, 10, 2**31, 3, 2, 0, 0, 0), (1, 10, 10, 0, 2, 0, 0, 0),
                (1, 10, 10, 3, 3, 0, 0, 0), (1, 10, 10, 3, 2, 2, 0, 0), (1, 10, 10, 3, 2, 0, 0, -1)):
        assert fn(*bad) == -1, bad
