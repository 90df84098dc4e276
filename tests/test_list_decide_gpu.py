"""Which sweep takes the sorted p = 2 launch on the f16 x 2 layout is decided once per launch: one wavefront (csrc/glhip_prune.hip,
list_decide) evaluates list_takes_launch (csrc/glhip_list_cursor.h) on eight reference slabs and writes one int into the sort scratch;
the list-driven sweep (csrc/glhip_softmin_list.h) and the staged one (csrc/glhip_softmin_x32.h) both read it, and the one it does not
name returns before anything else.

Shapes are at or just above the 1e11 pairs from which the call prunes (smaller ones never reach the kernels).  Every pruned call is held
to the dense launch of the same call (prune_support.close).  What is checked:

* the default threshold, GLHIP_LIST_KEEP=100 (always list-driven) and =0 (list-driven only without home blocks) at eps = 0.03^2 and
  0.1^2, and at eps = 1, where no slab has a home block and the list-driven sweep takes the launch whatever the threshold is;
* the default is equal, bit for bit, to the forced choice the rule names; which side an eps lies on is computed here from the kept
  share of the rule's own eight reference slabs (prune_support.inspect), not assumed;
* equal bits on a repeated call at 320 070 x 313 000 (N mod 128 = 70, M mod 32 = 8), with the knob moved in between: the int is
  written anew by every launch and nothing of an earlier launch is read.
"""

import numpy as np
import pytest
import torch

import prune_support as ps

pytestmark = pytest.mark.gpu

DEV, F16X2, NO_SORT = ps.DEV, ps.F16X2, ps.NO_SORT
N = 320000
AN, RM = 320070, 313000
assert AN % 128 == 70 and RM % 32 == 8 and AN * RM >= 1e11


def _rule(x, y, h, eps, pct=30):
    """list_takes_launch on the eight reference slabs, from the records of glhip_prune_inspect -> (takes, share, all_free)"""
    rec = ps.inspect(x, y, h, eps, records=("intervals", "home"))
    kept = np.maximum(rec["intervals"][:, :, 1] - rec["intervals"][:, :, 0], 0).sum(1)
    C, M = kept.shape[0], y.shape[1]
    refs = [min((2 * k + 1) * C // 16, C - 1) for k in range(8)]
    all_free = bool((rec["home"][refs] < 0).all())
    share = float(kept[refs].sum()) / (8 * M)
    return all_free or int(kept[refs].sum()) * 100 <= 8 * M * pct, share, all_free


@pytest.mark.parametrize("eps", [0.03**2, 0.1**2, 1.0], ids=["eps_0.03", "eps_0.1", "eps_1"])
def test_default_equals_the_choice_the_rule_names(monkeypatch, eps):
    x, y, h = ps.law(N, N, 121)
    takes, share, all_free = _rule(x, y, h, eps)
    print(f"reference slabs keep {share:.3f} of the columns, all without a home block: {all_free} -> "
          f"the {'list-driven' if takes else 'staged'} sweep")
    assert all_free or abs(share - 0.30) > 0.03      # not a launch on the rule's edge
    d = ps.fwd(x, y, h, eps, F16X2 | NO_SORT)
    out = {}
    for knob in (None, "100", "0"):
        if knob is None:
            monkeypatch.delenv("GLHIP_LIST_KEEP", raising=False)
        else:
            monkeypatch.setenv("GLHIP_LIST_KEEP", knob)
        out[knob] = ps.fwd(x, y, h, eps, F16X2)
        ps.close(out[knob], d, ps.diam2(x, y))
    # GLHIP_LIST_KEEP=100 names the list-driven sweep; =0 names it only where no reference slab has a home block
    assert torch.equal(out[None], out["100"] if takes else out["0"])
    if all_free:
        assert torch.equal(out["0"], out["100"])


def test_equal_bits_on_a_repeated_call(monkeypatch):
    x, y, h = ps.law(AN, RM, 120)
    monkeypatch.delenv("GLHIP_LIST_KEEP", raising=False)
    a = ps.fwd(x, y, h, 0.05**2, F16X2)
    monkeypatch.setenv("GLHIP_LIST_KEEP", "0" if _rule(x, y, h, 0.05**2)[0] else "100")      # the other sweep, in between
    c = ps.fwd(x, y, h, 0.05**2, F16X2)
    monkeypatch.delenv("GLHIP_LIST_KEEP")
    b = ps.fwd(x, y, h, 0.05**2, F16X2)
    assert torch.equal(a, b)
    ps.close(c, a, ps.diam2(x, y), what="the other sweep")
