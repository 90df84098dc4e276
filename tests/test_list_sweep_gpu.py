"""The list-driven sweep of the sorted p = 2 launch on the f16 x 2 layout (csrc/glhip_softmin_list.h): one wavefront per row tile, one
ballot over the records of up to 64 groups of a piece, the kept groups read straight from the group-major packed columns through a
ring of registers, the lazy maximum with a batch = one ballot.

Every shape is at or just above the 1e11 pairs from which the call prunes (smaller ones never reach the kernel).  Every case runs the
same call under GLHIP_FLAG_NO_SORT (the dense launch) next to it and is held to prune_support.close: |pruned - dense| <= 4e-7 diam^2 +
2e-6 max|out| with the same NaN / infinity pattern; ``compare`` adds 256 rows against float64 (prune_support.check_rows: at most 1.5 x
the dense launch's error + 2 ulp).  What the shapes are for:

* 320 000^2, D = 3, both clouds in the row role: the plain path (pieces of ~100 groups: full and partial ballots);
* 320 037 x 313 000: M mod 32 = 8 (a padded last group), M mod 256 = 168 (a last piece of 6 groups), N mod 128 = 37 (a last chunk of two
  row tiles, the second with 5 rows: two idle wavefronts);
* 65 536 x 1 525 900: 5961 column blocks against 256 slabs: 40 000 pieces, many far shorter than a ballot, next to pieces of several;
* rare columns 150 nats up: batches whose speculative sums overflow are redone with exact maxima and raise thr mid-sweep;
* eps = 1: no slab has a home block — no seed, no test, the first group taken exactly;
* special values, D < 3, bf16 clouds, the half-step, equal bits on a repeated call.

The launch picks the list-driven or the staged sweep on the device (csrc/glhip_list_cursor.h: list_takes_launch); at these sizes the
first level keeps more than at the headline size, so every case here sets GLHIP_LIST_KEEP=100 (the rule's threshold, read per launch:
always list-driven) for the pruned call.  The rule itself is checked at the end: the default and both forced choices agree within
the bound on a launch on either side of the threshold.
"""

import math

import numpy as np
import pytest
import torch

from geomloss_amd import hip

import prune_support as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def list_driven(monkeypatch):
    monkeypatch.setenv("GLHIP_LIST_KEEP", "100")

DEV, F16X2, NO_SORT = ps.DEV, ps.F16X2, ps.NO_SORT
N = 320000
EPS = 0.05**2
RN, RM = 320037, 313000
assert RM % 32 == 8 and RM % 256 == 168 and RN % 128 == 37 and RN * RM >= 1e11


@pytest.mark.parametrize("swap", [False, True], ids=["x_rows", "y_rows"])
def test_headline_law_both_clouds(swap):
    x, y, h = ps.law(N, N, 91)
    if swap:
        x, y = y, x
    ps.compare(x, y, h, EPS, F16X2)


def test_ragged_ends():
    x, y, h = ps.law(RN, RM, 92)
    rec = ps.inspect(x, y, h, EPS, records=("home",))
    assert (rec["home"] >= 0).any()
    ps.compare(x, y, h, EPS, F16X2)


def test_pieces_shorter_than_a_ballot():
    n, m = 65536, 1525900
    x, y, h = ps.law(n, m, 93)
    rec = ps.inspect(x, y, h, EPS, records=("home", "intervals"))
    iv = rec["intervals"].reshape(-1, 2)
    length = (iv[:, 1] - iv[:, 0])[iv[:, 1] > iv[:, 0]]
    print(f"pieces: median {np.median(length) / 32:.0f} groups, {float((length < 2048).mean()):.2f} of them under a ballot")
    assert (rec["home"] >= 0).any() and (length <= 1024).any() and (length > 2048).any()      # single ballots of half a batch, and pieces of several
    ps.compare(x, y, h, EPS, F16X2)


@pytest.mark.parametrize("D", [1, 2])
def test_lower_dimensions(D):
    x, y, h = ps.law(N, N, 93 + D, D=D, noise=0.001)
    ps.compare(x, y, h, 0.03**2, F16X2)


def test_bf16_clouds():
    x, y, h = ps.law(N, N, 96, dtype=torch.bfloat16)
    ps.compare(x, y, h, EPS, F16X2)


def test_half_step():
    eps, damping = 0.03**2, 0.9
    x, y, logw = ps.law(N, N, 97, noise=0.001)
    g = torch.Generator().manual_seed(6)
    pot = (0.002 * torch.randn(1, N, generator=g)).to(DEV)
    hcol = (pot.double() * float(np.float32(1.0) / np.float32(eps)) + logw.double()).float()      # fma(pot, 1 / eps, logw): one rounding
    p = hip.sinkhorn_step_raw(x, y, logw, pot, None, eps, damping, 2, None, F16X2)
    d = hip.sinkhorn_step_raw(x, y, logw, pot, None, eps, damping, 2, None, F16X2 | NO_SORT)
    ps.close(p, d, ps.diam2(x, y))
    rows = torch.linspace(0, N - 1, 256, device=DEV).long()
    ps.check_rows(p, d, damping * ps.oracle_rows(x, y, hcol, eps, rows), rows)


def test_redo_raises_the_threshold_mid_sweep():
    """the rare-column law of profiles/prep_kernels.txt: 0.3 % of the dual values 150 nats up — a row's seed is far above most of
    what it meets, or far below a rare column of a later batch, whose speculative sum then overflows"""
    g = torch.Generator().manual_seed(64)
    x = torch.rand(1, N, 3, generator=g)
    y = torch.rand(1, N, 3, generator=g)
    h = torch.full((1, N), -math.log(N)) + 0.01 * torch.randn(1, N, generator=g) / 0.05**2
    h[torch.rand(1, N, generator=g) < 0.003] += 150.0
    ps.compare(x.to(DEV), y.to(DEV), h.to(DEV), EPS, F16X2)


def test_no_slab_has_a_home_block():
    x, y, h = ps.law(N, N, 98)
    rec = ps.inspect(x, y, h, 1.0, records=("home",))
    assert (rec["home"] < 0).all()
    ps.compare(x, y, h, 1.0, F16X2)


@pytest.mark.parametrize("what", ["y_nan", "x_nan", "group_pinf", "all_minf"])
def test_special_values(what):
    x, y, h = ps.law(N, N, 99)
    x, y, h = x.clone(), y.clone(), h.clone()
    if what == "y_nan":
        y[0, 777::5003, 1] = math.nan
    elif what == "x_nan":
        x[0, 555::7001, 2] = math.nan
    elif what == "group_pinf":      # one whole aligned group of 32 sorted columns
        rec = ps.inspect(x, y, h, EPS, records=("perm_y",))
        grp = torch.from_numpy(rec["perm_y"][32 * 4321:32 * 4322].astype(np.int64)).to(DEV)
        h[0, grp] = math.inf
    else:
        h[:] = -math.inf
    a = ps.fwd(x, y, h, EPS, F16X2)
    b = ps.fwd(x, y, h, EPS, F16X2 | NO_SORT)
    ps.close(a, b, ps.diam2(x, y))
    if what == "all_minf":
        assert bool(torch.isinf(a).all())


@pytest.mark.parametrize("eps", [0.03**2, 0.1**2], ids=["keeps_little", "keeps_much"])
def test_dispatch_rule(monkeypatch, eps):
    """the default threshold and both forced choices: three launches of one call, each held to the dense launch"""
    x, y, h = ps.law(N, N, 101)
    rec = ps.inspect(x, y, h, eps, records=("intervals",))
    share = float(np.maximum(rec["intervals"][:, :, 1] - rec["intervals"][:, :, 0], 0).sum(1).mean()) / N
    print(f"the first level keeps {share:.3f} of the columns")
    assert (share < 0.25) == (eps < 0.05**2)      # well on either side of the rule's 30 %
    d = ps.fwd(x, y, h, eps, F16X2 | NO_SORT)
    out = {}
    for knob in (None, "100", "0"):
        if knob is None:
            monkeypatch.delenv("GLHIP_LIST_KEEP")
        else:
            monkeypatch.setenv("GLHIP_LIST_KEEP", knob)
        out[knob] = ps.fwd(x, y, h, eps, F16X2)
        ps.close(out[knob], d, ps.diam2(x, y))
    assert torch.equal(out[None], out["100" if eps < 0.05**2 else "0"])      # which sweep the default took


def test_equal_bits_on_a_repeated_call():
    x, y, h = ps.law(RN, RM, 100)
    a = ps.fwd(x, y, h, EPS, F16X2)
    b = ps.fwd(x, y, h, EPS, F16X2)
    assert torch.equal(a, b)
