"""Reused permutations of the sorted p = 2 call (library 134: glhip_sinkhorn_step_perm; geomloss_amd/_perm_cache.py: _PermCache; geomloss_amd/hip.py: _perm_plan) at the smallest
shapes the pruned call accepts, those of tests/test_prep_kernels_gpu.py: 65536 x 1525900 (N at its minimum, N M just over 1e11) and
317000 x 320037 (a partial last block of 1024 in both clouds: the tail keeps the path order).  Unit-cube clouds, eps = 0.05^2, the
dual vector of bench.make_problem, the headline's f16 x 2 layout.

* export: the permutations the entry point writes are those glhip_prune_inspect reports (D = 3, D = 2, bf16);
* reuse: a call without permutation arguments, the exporting call and the calls that reuse both, only x's or only y's permutation
  return identical outputs, for glhip_softmin_fwd and for glhip_sinkhorn_step with pot and prev, and the glhip_prune_inspect records
  taken before and after them are identical;
* a stale hint — the identity, and the order of ANOTHER cloud of the same size — stays within the bound that
  prune_support.close applies to pruned against dense (4e-7 diam^2 + 2e-6 of the output's magnitude);
* hip.softmin_fwd_raw: two hits on the second call, a miss after ``x.mul_(1.0)`` with the output of a cache-disabled call, hits for both
  clouds on (y, x) after (x, y).
No test hands an out-of-range hint to the GPU: the clamp is tested on the host (tests/test_perm_reuse_cpu.py).
"""

import ctypes
import math

import numpy as np
import pytest
import torch

from geomloss_amd import hip

import prune_support as ps
from prune_support import RECORDS

pytestmark = pytest.mark.gpu

DEV = ps.DEV
EPS = 0.05**2
FLAGS = hip.FLAG_F16X2
SHAPES = {"wide": (65536, 1525900), "uneven": (317000, 320037)}


def _problem(shape, D=3, dtype=torch.float32, seed=0):
    """x (1,n,D), y (1,m,D), h (1,m) on the device: bench.make_problem's law"""
    n, m = SHAPES[shape]
    g = torch.Generator(device="cpu").manual_seed(900 + seed + 10 * D + (n % 7))
    x = torch.rand(n, D, generator=g).to(DEV, dtype)
    y = torch.rand(m, D, generator=g).to(DEV, dtype)
    h = (torch.full((m,), -math.log(m)) + 0.01 * torch.randn(m, generator=g) / EPS).to(DEV)
    return x[None].contiguous(), y[None].contiguous(), h[None].contiguous()


def _same_records(a, b):
    for k in RECORDS:
        assert np.array_equal(a[k], b[k], equal_nan=k in ("mlb", "t1", "t2")), k


def _step(x, y, logw, pot=None, prev=None, damping=1.0, perm_x=None, perm_y=None, bits=0, flags=FLAGS, entry="perm"):
    """one launch -> out (1,n).  entry: "perm" (glhip_sinkhorn_step_perm), "step" (glhip_sinkhorn_step), "fwd" (glhip_softmin_fwd)"""
    lib = hip.load_library()
    _, n, D = x.shape
    m = y.shape[1]
    ws, nbytes = ps.workspace(lib, n, m, D)
    out = torch.empty((1, n), dtype=torch.float32, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    tail = [None, None, None, 0, ctypes.c_void_p(ws.data_ptr()), nbytes, int(flags), hip._stream(x)]
    if entry == "fwd":
        assert pot is None and prev is None and damping == 1.0
        rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), logw.data_ptr(), out.data_ptr(), 1, n, m, D, float(EPS), 2, hip._dtype_code(x), *tail)
    else:
        head = [x.data_ptr(), y.data_ptr(), logw.data_ptr(), ptr(pot), ptr(prev), out.data_ptr(), 1, n, m, D, float(EPS), float(damping), 2,
                hip._dtype_code(x)]
        if entry == "step":
            rc = lib.glhip_sinkhorn_step(*head, *tail)
        else:
            rc = lib.glhip_sinkhorn_step_perm(*head, *tail, ptr(perm_x), ptr(perm_y), int(bits))
    assert rc == 0, lib.glhip_last_error()
    return out


def _buffers(x, y):
    return (torch.full((x.shape[1],), -1, dtype=torch.int32, device=DEV), torch.full((y.shape[1],), -1, dtype=torch.int32, device=DEV))


_PROBLEMS = {}


def _shared(shape):
    """the D = 3 float32 problem of a shape, its inspect records and its exported permutations: made once, left unchanged"""
    if shape not in _PROBLEMS:
        x, y, h = _problem(shape)
        rec = ps.inspect(x, y, h, EPS)
        px, py = _buffers(x, y)
        out = _step(x, y, h, perm_x=px, perm_y=py)
        _PROBLEMS[shape] = (x, y, h, rec, px, py, out)
    return _PROBLEMS[shape]


# ---- 1. export ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,dtype", [(3, torch.float32), (2, torch.float32), (3, torch.bfloat16)], ids=["d3", "d2", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exported_permutations_are_the_inspected_ones(shape, D, dtype):
    if D == 3 and dtype == torch.float32:
        x, y, h, rec, px, py, _ = _shared(shape)
    else:
        x, y, h = _problem(shape, D, dtype)
        rec = ps.inspect(x, y, h, EPS)
        px, py = _buffers(x, y)
        _step(x, y, h, perm_x=px, perm_y=py)
    n, m = x.shape[1], y.shape[1]
    gx, gy = px.cpu().numpy(), py.cpu().numpy()
    assert np.array_equal(np.sort(gx), np.arange(n)) and np.array_equal(np.sort(gy), np.arange(m))
    assert np.array_equal(gx, rec["perm_x"]) and np.array_equal(gy, rec["perm_y"])
    # one buffer alone, the other NULL: the same order, and nothing else is written
    qx, qy = _buffers(x, y)
    _step(x, y, h, perm_x=qx)
    _step(x, y, h, perm_y=qy)
    assert torch.equal(qx, px) and torch.equal(qy, py)


def test_calls_that_do_not_sort_leave_the_buffers_alone():
    """where glhip_softmin_perm_applies says 0 (here: GLHIP_FLAG_NO_SORT is too dear at these sizes, so a shape below 1e11 pairs) the
    three arguments are ignored: nothing is written, and a "hint" is not read"""
    g = torch.Generator(device="cpu").manual_seed(5)
    x, y = torch.rand(1, 70000, 3, generator=g).to(DEV), torch.rand(1, 70001, 3, generator=g).to(DEV)
    h = torch.randn(1, 70001, generator=g).to(DEV)
    assert hip.softmin_perm_applies(1, 70000, 70001, 3, 2, hip.F32, FLAGS, 0) == 0
    px, py = _buffers(x, y)
    ref = _step(x, y, h, entry="fwd")
    assert torch.equal(_step(x, y, h, perm_x=px, perm_y=py), ref)
    assert bool((px == -1).all()) and bool((py == -1).all())
    assert torch.equal(_step(x, y, h, perm_x=px, perm_y=py, bits=3), ref)


# ---- 2. reuse is bit-identical -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_reuse_is_bit_identical(shape):
    x, y, h, rec, px, py, exported = _shared(shape)
    keep_x, keep_y = px.clone(), py.clone()
    plain = _step(x, y, h, entry="fwd")
    assert torch.equal(exported, plain)
    both = _step(x, y, h, perm_x=px, perm_y=py, bits=hip.PERM_HINT_X | hip.PERM_HINT_Y)
    only_x = _step(x, y, h, perm_x=px, bits=hip.PERM_HINT_X)
    only_y = _step(x, y, h, perm_y=py, bits=hip.PERM_HINT_Y)
    qy = torch.full_like(py, -1)
    x_and_export_y = _step(x, y, h, perm_x=px, perm_y=qy, bits=hip.PERM_HINT_X)
    for out in (both, only_x, only_y, x_and_export_y):
        assert torch.equal(out, plain)
    assert torch.equal(qy, py)
    assert torch.equal(px, keep_x) and torch.equal(py, keep_y)      # a hint is read, never written
    _same_records(ps.inspect(x, y, h, EPS), rec)
    assert bool(torch.isfinite(plain).all())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_reuse_is_bit_identical_for_the_half_step(shape):
    x, y, h, rec, px, py, _ = _shared(shape)
    n, m = x.shape[1], y.shape[1]
    g = torch.Generator(device="cpu").manual_seed(17)
    logw = torch.full((1, m), -math.log(m), device=DEV)
    pot = (0.01 * torch.randn(1, m, generator=g)).to(DEV)
    prev = (0.01 * torch.randn(1, n, generator=g)).to(DEV)
    before = ps.inspect(x, y, logw, EPS, pot)
    plain = _step(x, y, logw, pot, prev, 0.9, entry="step")
    qx, qy = _buffers(x, y)
    export = _step(x, y, logw, pot, prev, 0.9, perm_x=qx, perm_y=qy)
    assert torch.equal(qx, px) and torch.equal(qy, py)
    both = _step(x, y, logw, pot, prev, 0.9, perm_x=px, perm_y=py, bits=3)
    only_x = _step(x, y, logw, pot, prev, 0.9, perm_x=px, bits=hip.PERM_HINT_X)
    only_y = _step(x, y, logw, pot, prev, 0.9, perm_y=py, bits=hip.PERM_HINT_Y)
    for out in (export, both, only_x, only_y):
        assert torch.equal(out, plain)
    _same_records(ps.inspect(x, y, logw, EPS, pot), before)
    assert np.array_equal(before["perm_x"], rec["perm_x"]) and np.array_equal(before["perm_y"], rec["perm_y"])
    assert bool(torch.isfinite(plain).all())


def test_one_cloud_on_both_sides_sorts_once():
    """x against itself through one buffer: exported for the rows, read as the hint of the columns (the x side is prepared first)"""
    g = torch.Generator(device="cpu").manual_seed(23)
    n = 316500                                   # n^2 just over 1e11; a partial last block
    x = torch.rand(1, n, 3, generator=g).to(DEV)
    h = (torch.full((1, n), -math.log(n)) + 0.01 * torch.randn(1, n, generator=g) / EPS).to(DEV)
    assert hip.softmin_perm_applies(1, n, n, 3, 2, hip.F32, FLAGS, 0) == 1
    plain = _step(x, x, h, entry="fwd")
    buf = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    assert torch.equal(_step(x, x, h, perm_x=buf, perm_y=buf, bits=hip.PERM_HINT_Y), plain)
    assert np.array_equal(buf.cpu().numpy(), ps.inspect(x, x, h, EPS)["perm_x"])


# ---- 3. a stale hint is exact ------------------------------------------------------------------------------------------------------------

def test_a_stale_hint_is_exact():
    x, y, h, rec, px, py, pruned = _shared("wide")
    n, m = x.shape[1], y.shape[1]
    dense = _step(x, y, h, flags=FLAGS | hip.FLAG_NO_SORT, entry="fwd")
    diam2 = ps.diam2(x, y)
    ps.close(pruned, dense, diam2, require_finite=True)
    ident_x, ident_y = torch.arange(n, dtype=torch.int32, device=DEV), torch.arange(m, dtype=torch.int32, device=DEV)
    ps.close(_step(x, y, h, perm_x=ident_x, perm_y=ident_y, bits=3), dense, diam2, require_finite=True)
    # the order of ANOTHER cloud of the same size
    x2, y2, h2 = _problem("wide", seed=1)
    ox, oy = _buffers(x2, y2)
    _step(x2, y2, h2, perm_x=ox, perm_y=oy)
    assert not torch.equal(ox, px) and not torch.equal(oy, py)
    ps.close(_step(x, y, h, perm_x=ox, perm_y=oy, bits=3), dense, diam2, require_finite=True)
    ps.close(_step(x, y, h, perm_x=ox, perm_y=py, bits=3), dense, diam2, require_finite=True)      # one stale, one right


# ---- 4. through hip.softmin_fwd_raw -------------------------------------------------------------------------------------------------------

def test_the_cache_behind_softmin_fwd_raw(monkeypatch):
    monkeypatch.delenv("GEOMLOSS_HIP_PERM_CACHE", raising=False)
    x0, y0, h, rec, px, py, want = _shared("uneven")
    x, y = x0.clone(), y0.clone()                # (the shared problem stays unchanged: x is written in place below)
    n, m = x.shape[1], y.shape[1]
    hip.forget_permutations()
    stats = lambda: hip.perm_cache_stats()[:2]  # noqa: E731
    h0, m0 = stats()
    first = hip.softmin_fwd_raw(x, y, h, EPS, 2, flags=FLAGS)
    assert stats() == (h0, m0 + 2) and hip.perm_cache_stats()[2] == 2
    second = hip.softmin_fwd_raw(x, y, h, EPS, 2, flags=FLAGS)
    assert stats() == (h0 + 2, m0 + 2)
    assert torch.equal(first, want) and torch.equal(second, want)
    cached = [p for _, p in hip._perm_cache.entries.values()]
    assert any(torch.equal(p, px) for p in cached) and any(torch.equal(p, py) for p in cached)
    # views and detached aliases, as the drivers pass them, hit
    hip.softmin_fwd_raw(x[0].detach()[None], y.detach(), h, EPS, 2, flags=FLAGS)
    assert stats() == (h0 + 4, m0 + 2)
    # an in-place write: x misses (and is sorted again), y hits
    x.mul_(1.0)
    after = hip.softmin_fwd_raw(x, y, h, EPS, 2, flags=FLAGS)
    assert stats() == (h0 + 5, m0 + 3)
    monkeypatch.setenv("GEOMLOSS_HIP_PERM_CACHE", "0")
    off = hip.softmin_fwd_raw(x, y, h, EPS, 2, flags=FLAGS)
    assert stats() == (h0 + 5, m0 + 3)
    monkeypatch.delenv("GEOMLOSS_HIP_PERM_CACHE")
    assert torch.equal(after, off) and torch.equal(after, want)
    # (y, x) after (x, y): both clouds hit, and the half-step shares the entries
    hx = (torch.full((1, n), -math.log(n), device=DEV))
    swapped = hip.softmin_fwd_raw(y, x, hx, EPS, 2, flags=FLAGS)
    assert stats() == (h0 + 7, m0 + 3)
    assert torch.equal(swapped, _step(y, x, hx, entry="fwd"))
    stepped = hip.sinkhorn_step_raw(x, y, h, None, None, EPS, 1.0, 2, flags=FLAGS)
    assert stats() == (h0 + 9, m0 + 3) and torch.equal(stepped, want)
    # another stream misses
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        other = hip.softmin_fwd_raw(x, y, h, EPS, 2, flags=FLAGS)
    s.synchronize()
    assert stats() == (h0 + 9, m0 + 5) and torch.equal(other, want)
    hip.forget_permutations()
    assert hip.perm_cache_stats()[2] == 0


def test_an_online_loss_sorts_each_cloud_once(monkeypatch):
    """SamplesLoss("sinkhorn", p=2) at N M >= 1e11: every half-step of the loop is the sorted call, on views of the same two storages —
    two misses per loss, whatever the layout the caller's clouds have (non-contiguous ones are copied once, not per call)."""
    from geomloss_amd import SamplesLoss

    monkeypatch.delenv("GEOMLOSS_HIP_PERM_CACHE", raising=False)
    g = torch.Generator(device="cpu").manual_seed(31)
    n, m = SHAPES["uneven"]
    wide_x, wide_y = torch.rand(n, 4, generator=g).to(DEV), torch.rand(m, 4, generator=g).to(DEV)
    loss = SamplesLoss("sinkhorn", p=2, blur=0.05, scaling=0.5, backend="online")
    counts, values = [], []
    for x, y in ((wide_x[:, :3].contiguous(), wide_y[:, :3].contiguous()), (wide_x[:, :3], wide_y[:, :3])):
        hip.forget_permutations()
        h0, m0, _ = hip.perm_cache_stats()
        with torch.no_grad():
            values.append(loss(x, y))
        h1, m1, _ = hip.perm_cache_stats()
        counts.append((h1 - h0, m1 - m0))
    print("hits, misses per loss:", counts)
    assert counts[0][1] == 2 and counts[1][1] == 2 and counts[0] == counts[1] and counts[0][0] >= 30
    assert torch.equal(values[0], values[1]) and bool(torch.isfinite(values[0]))
    hip.forget_permutations()
