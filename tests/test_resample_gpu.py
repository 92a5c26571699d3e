"""The three bootstrap kernels draw through one function (``csrc/resample.h``): for one seed
``ops.bootstrap_metrics``, ``ops.bootstrap_calibration`` and ``ops.bootstrap_compare`` must return the
same class totals ``pn [B, 2]`` on the device, plain and stratified, with the count arrays in LDS and in
the global workspace.  Where no score equals 0.5 the treat rules ``p ≥ 0.5`` (decision curve) and
``p > 0.5`` (confusion counts) select the same rows, so the decision-curve TP and FP at t = 0.5 must
equal the confusion counts' too.  Everything compared is an integer: equality is exact."""
import pytest
import torch

from hfens import ops
from hfens.ops import api
from test_calibration import make_scores

pytestmark = pytest.mark.gpu

B = 8
T = 99          # thresholds g/(T + 1), g = 1..T: index 49 is t = 50/100 = 0.5 exactly
G_HALF = 49


@pytest.mark.parametrize("force_global", [False, True])
@pytest.mark.parametrize("strat", [False, True])
@pytest.mark.parametrize("n", [65, 1025])
def test_three_ops_draw_the_same_rows(dev, monkeypatch, n, strat, force_global):
    for flag in ("_BOOTSTRAP_FORCE_GLOBAL", "_CALIBRATION_FORCE_GLOBAL", "_COMPARE_FORCE_GLOBAL"):
        monkeypatch.setattr(api, flag, force_global)
    y, p = make_scores(n, "continuous")
    assert (p != 0.5).all() and (G_HALF + 1) / (T + 1) == 0.5
    y, p = torch.as_tensor(y).to(dev), torch.as_tensor(p).to(dev)
    kw = dict(seed=11, stratified=strat)
    _, _, _, pn, conf, _ = ops.bootstrap_metrics(y, p, B, threshold=0.5, **kw)
    cal = ops.bootstrap_calibration(y, p, B, thresholds=T, **kw)
    cmp_ = ops.bootstrap_compare(y, torch.stack([p, 1.0 - p]), B, threshold=0.5, **kw)
    assert pn.shape == (B, 2) and int(pn.sum()) == B * n
    assert torch.equal(cal.pn, pn) and torch.equal(cmp_.pn, pn)
    assert torch.equal(cmp_.conf[:, 0], conf)
    if n == 1025:
        assert torch.equal(cal.dc[:, G_HALF], conf[:, :2])
