"""The balanced cells of the sorted p = 2 call (csrc/glhip_autosort.h: balanced cells; csrc/glhip_balance.h; balance_kernel in
csrc/glhip_compact_sort.hip), on the host.

Two things are checked here.  The CPU model tools/prune_model.py: balanced_order — every whole aligned block of 1024 positions of the
path order split into cells of 512, ..., 32 points by median cuts along the longest axis — keeps every block's set of points, leaves
the partial tail alone, has the split property at every level, is deterministic on NaN, infinities, duplicates and all-equal blocks,
and buys what it is for on the law of tests/test_prune_mass_gpu.py.  And the header's own functions: a small program around them plays
the kernel's 1024 threads (extents, axis, sort words, the bitonic network step by step) and prints the order of a block, which must
equal the model's; the key map is compared value by value.
"""

import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "geomloss_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import prune_model as pm  # noqa: E402

BLOCK, LEAF = 1024, 32


def _cloud(n, D, seed):
    return np.random.default_rng(seed).random((n, D), dtype=np.float32)


def _check_split(z, order, block=BLOCK, leaf=LEAF):
    """at every level and segment of every whole block: along the axis the rule picks from the segment's points, no key of the lower
    half exceeds a key of the upper half; returns the number of segments checked"""
    nb = order.shape[0] // block
    pts = z[order[:nb * block]]
    seg, checked = block, 0
    while seg >= 2 * leaf:
        p = pts.reshape(-1, seg, z.shape[1])
        axis = pm.balance_axes(p)
        key = pm.order_key(np.take_along_axis(p, axis[:, None, None], 2)[:, :, 0])
        assert (key[:, :seg // 2].max(1) <= key[:, seg // 2:].min(1)).all(), seg
        checked += p.shape[0]
        seg //= 2
    return checked


def _check_blocks(perm, order, block=BLOCK):
    n = perm.shape[0]
    nb = n // block
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(np.sort(order[:nb * block].reshape(nb, block), 1), np.sort(perm[:nb * block].reshape(nb, block), 1))
    assert np.array_equal(order[nb * block:], perm[nb * block:])


@pytest.mark.parametrize("D,n", [(1, 5 * 1024 + 37), (2, 7 * 1024 + 1000), (3, 9 * 1024 + 5), (3, 1000), (3, 4096)])
def test_model_keeps_blocks_and_splits_them(D, n):
    z = _cloud(n, D, 100 + D)
    perm = pm.compact_order2(z, 256, pm.sort_sub(D))
    order = pm.balanced_order(z, perm)
    _check_blocks(perm, order)
    assert _check_split(z, order) == (n // BLOCK) * 31
    assert np.array_equal(order, pm.balanced_order(z, perm))
    if n >= BLOCK:
        assert not np.array_equal(order, perm)


def _special_cloud():
    """3 whole blocks and a tail: NaN of both signs, infinities, signed zeros, duplicated points, and a block of identical points"""
    g = np.random.default_rng(5)
    n = 3 * BLOCK + 77
    z = g.random((n, 3), dtype=np.float32)
    z[g.integers(0, BLOCK, 40), g.integers(0, 3, 40)] = np.nan
    z[7, 0] = -np.float32(np.nan)
    z[g.integers(0, BLOCK, 10), g.integers(0, 3, 10)] = np.inf
    z[g.integers(0, BLOCK, 10), g.integers(0, 3, 10)] = -np.inf
    z[100:110, 1] = 0.0
    z[110:120, 1] = -0.0
    z[200:600] = z[200]                       # duplicated points inside a block
    z[BLOCK:2 * BLOCK] = np.float32(0.25)     # an all-equal block
    z[2 * BLOCK:2 * BLOCK + 64] = np.nan      # a cell's worth of points without one finite coordinate
    return z


def test_model_on_special_values():
    z = _special_cloud()
    n = z.shape[0]
    perm = np.random.default_rng(6).permutation(n)
    order = pm.balanced_order(z, perm)
    _check_blocks(perm, order)
    _check_split(z, order)
    assert np.array_equal(order, pm.balanced_order(z.copy(), perm.copy()))
    # a block of identical points comes out in its incoming order
    same = perm[(perm >= BLOCK) & (perm < 2 * BLOCK)]      # the all-equal points, shuffled, as the first block of an order
    p2 = np.concatenate([same, perm[(perm < BLOCK) | (perm >= 2 * BLOCK)]])
    assert np.array_equal(pm.balanced_order(z, p2)[:BLOCK], same)
    # the key map: one value for every NaN, above +inf; -0 below +0; monotone on the rest
    v = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan, -np.nan], np.float32)
    k = pm.order_key(v)
    assert (np.diff(k[:9].astype(np.int64)) > 0).all() and k[8] == k[9] == 0xFFFFFFFF


def test_first_level_on_the_mass_law():
    """the law of tests/test_prune_mass_gpu.py (n = 320000, seed 21, eps = 0.05^2): the balanced order keeps at most 0.9 of the blocks
    the path order keeps (modelled 0.3183 against 0.3802), and no slab has more than RUNS runs"""
    import torch

    n, eps = 320000, 0.05**2
    g = torch.Generator().manual_seed(21)
    x = torch.rand(1, n, 3, generator=g)[0].numpy()
    y = torch.rand(1, n, 3, generator=g)[0].numpy()
    h = (torch.full((1, n), -math.log(n)) + 0.01 * torch.randn(1, n, generator=g) / (0.05**2))[0].numpy()
    px, py = pm.compact_order2(x, 256, 2), pm.compact_order2(y, 256, 2)
    keep0 = pm.plan_mass(x[px], y[py], h[py], eps)[0]
    bx, by = pm.balanced_order(x, px), pm.balanced_order(y, py)
    keep1 = pm.plan_mass(x[bx], y[by], h[by], eps)[0]
    r = pm.runs_per_slab(keep1)
    print(f"first level keeps {keep1.mean():.4f} (path order {keep0.mean():.4f}); runs per slab mean {r.mean():.1f} max {r.max()}")
    assert keep1.mean() <= 0.9 * keep0.mean()
    assert (r <= pm.RUNS).all()


def test_closed_gaps():
    k = np.zeros(40, bool)
    k[[0, 2, 3, 7, 8, 20, 22]] = True      # gaps of 1, 3, 11, 1 blocks: 5 runs
    assert np.array_equal(pm.closed_gaps(k, 5), k)
    c = pm.closed_gaps(k, 3)               # the two gaps of one block close
    assert pm.runs_per_slab(c[None])[0] == 3 and c.sum() == k.sum() + 2 and c[1] and c[21]
    c = pm.closed_gaps(k, 4)               # gaps close by length: both of them, not one
    assert pm.runs_per_slab(c[None])[0] == 3
    assert pm.runs_per_slab(pm.closed_gaps(k, 1)[None])[0] == 1


# ---- the header's functions, played by a host program -------------------------------------------------------------------------------

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "glhip_balance.h"
// stdin: mode.  mode 0: count, then float bit patterns in hex -> balance_key of each.
// mode 1: D, then 1024 x D bit patterns of a block's points in their incoming order -> the incoming position of the point at every place
// after the five levels, with the kernel's structure: one word per "thread", extents per segment, the bitonic network step by step.
using namespace glhip;
static float from_bits(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
int main() {
    int mode;
    if (std::scanf("%d", &mode) != 1) return 1;
    if (mode == 0) {
        int n;
        if (std::scanf("%d", &n) != 1) return 1;
        for (int i = 0; i < n; ++i) {
            unsigned b;
            if (std::scanf("%x", &b) != 1) return 1;
            std::printf("%u\n", balance_key(from_bits(b)));
        }
        return 0;
    }
    const int B = 1024;
    int D;
    if (std::scanf("%d", &D) != 1 || D < 1 || D > 3) return 1;
    std::vector<float> pts(3 * B, 0.f);
    for (int i = 0; i < B; ++i)
        for (int d = 0; d < D; ++d) {
            unsigned b;
            if (std::scanf("%x", &b) != 1) return 1;
            pts[d * B + i] = from_bits(b);
        }
    std::vector<int> p(B);
    for (int i = 0; i < B; ++i) p[i] = i;
    std::vector<unsigned long long> v(B), o(B);
    for (int seg = B; seg >= 64; seg >>= 1) {
        for (int s0 = 0; s0 < B; s0 += seg) {
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int i = s0; i < s0 + seg; ++i)
                for (int d = 0; d < D; ++d) balance_extent_add(pts[d * B + p[i]], lo[d], hi[d]);
            const int axis = balance_axis(lo, hi, 3);
            if (axis != balance_axis(lo, hi, D)) return 2;      // (the axes beyond D lose to every other)
            for (int i = s0; i < s0 + seg; ++i) v[i] = balance_word(balance_key(pts[axis * B + p[i]]), (unsigned)p[i]);
        }
        for (int k = 2; k <= seg; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = 0; i < B; ++i) o[i] = v[i ^ j];
                for (int i = 0; i < B; ++i) v[i] = (balance_keeps_min(i, j, k, seg) == (o[i] < v[i])) ? o[i] : v[i];
            }
        for (int i = 0; i < B; ++i) p[i] = (int)(unsigned)v[i];
    }
    for (int i = 0; i < B; ++i) std::printf("%d\n", p[i]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def balance_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("balance")
    src = d / "balance.cpp"
    src.write_text(PROGRAM)
    exe = d / "balance"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _hex(a):
    return "\n".join(f"{int(b):x}" for b in np.ascontiguousarray(a, np.float32).view(np.uint32).ravel())


def test_header_key_map(balance_exe):
    g = np.random.default_rng(8)
    bits = np.concatenate([g.integers(0, 2**32, 4000, dtype=np.uint64).astype(np.uint32),
                           np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 1, 0x80000001], np.uint32)])
    v = bits.view(np.float32)
    out = subprocess.run([balance_exe], input=f"0\n{len(v)}\n{_hex(v)}\n", capture_output=True, text=True, check=True).stdout.split()
    assert np.array_equal(np.array(out, np.uint64).astype(np.uint32), pm.order_key(v))


def _header_order(exe, block_pts):
    D = block_pts.shape[1]
    out = subprocess.run([exe], input=f"1\n{D}\n{_hex(block_pts)}\n", capture_output=True, text=True, check=True).stdout.split()
    return np.array(out, np.int64)


def test_header_network_matches_the_model(balance_exe):
    """the header's rules, played thread by thread, give the order of the model's serial sorts: random blocks for D = 1, 2, 3, a bf16-like
    block with many ties, and the blocks of the special cloud"""
    blocks = [_cloud(BLOCK, D, 40 + D) for D in (1, 2, 3)]
    blocks.append((np.round(_cloud(BLOCK, 3, 50) * 8) / 8).astype(np.float32))      # many ties on every axis
    blocks.append((np.round(_cloud(BLOCK, 2, 51) * 4) / 4).astype(np.float32))
    z = _special_cloud()
    blocks += [z[:BLOCK], z[BLOCK:2 * BLOCK], z[2 * BLOCK:3 * BLOCK]]
    for pts in blocks:
        want = pm.balanced_order(pts, np.arange(BLOCK))
        got = _header_order(balance_exe, pts)
        assert np.array_equal(np.sort(got), np.arange(BLOCK))
        assert np.array_equal(got, want)
    assert np.array_equal(_header_order(balance_exe, z[BLOCK:2 * BLOCK]), np.arange(BLOCK))      # identical points: incoming order
