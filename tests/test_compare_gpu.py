"""The fused comparison kernel (``csrc/compare.hip``) against the host mirror and, column by column,
against ``ops.bootstrap_metrics`` on the same device; independence of the launch geometry, of the
storage path and of the replicate range; the LDS limit; degenerate replicates; ``compare_ci`` on
the device against the host.

Bounds, device against mirror (both evaluate one formula on equal integers): the integers and
``auroc`` bit-equal (one division of the same integers); ``|ap| ≤ 4·n·2^-53`` as in
``test_bootstrap_gpu.py`` (the two AP sums differ by summation order only); ``sums`` within
``test_compare.sums_budget`` (the mirror folds in the kernel's order, so the difference is
expected to be zero; the budget is what the fold itself allows)."""
import functools

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.ops import api
from hfens.ops import reference as ref
from hfens.utils import metrics
from test_compare import U, make_scores, sums_budget

pytestmark = pytest.mark.gpu

L = api.COMPARE_LDS_ROWS
NS = (2, 63, 64, 65, 1023, 1024, 1025, 2049)     # chunk 1 → 2 → 3, ragged last chunks
B = 8


@functools.lru_cache(maxsize=None)
def inputs(n, M, kind="decimal"):
    """``decimal``: one-decimal scores; ``heavy``: 4 distinct scores and (M ≥ 2) one constant column."""
    y, S = make_scores(n, M, ties=kind == "decimal")
    if kind == "heavy":
        S = np.floor(S * 4).clip(0, 3) / 4 + 0.125
        if M >= 2:
            S[-1] = 0.625
    return torch.as_tensor(y), torch.as_tensor(S)


@functools.lru_cache(maxsize=None)
def mirror(n, M, strat, kind="decimal", nb=B):
    y, S = inputs(n, M, kind)
    return ops.bootstrap_compare(y, S, nb, seed=3, stratified=strat)


def device(dev, n, M, strat, kind="decimal", nb=B, **kw):
    y, S = inputs(n, M, kind)
    return ops.bootstrap_compare(y.to(dev), S.to(dev), nb, seed=3, stratified=strat, **kw)


def assert_matches_mirror(got, want, n, ints_only=False):
    got = ref.CompareBootstrap(*(t.cpu() for t in got))
    for k in ("a2", "pn", "conf", "reclass"):
        assert getattr(got, k).dtype == torch.int64 and torch.equal(getattr(got, k), getattr(want, k)), k
    if ints_only:
        return
    nan = torch.isnan(want.auroc)
    assert torch.equal(torch.isnan(got.auroc), nan) and torch.equal(torch.isnan(got.ap), nan)
    ok = ~nan
    assert torch.equal(got.auroc[ok], want.auroc[ok])
    if bool(ok.any()):
        dap = float((got.ap[ok] - want.ap[ok]).abs().max())
        print(f"max|dap| {dap / U:.3g} u")
        assert dap <= 4 * n * U
    ds = (got.sums - want.sums).abs().numpy()
    print(f"max|dsums| {ds.max() / U:.3g} u")
    assert (ds <= sums_budget(n, want.sums.numpy())).all()


def equal_bits(a, b):
    return all(x.shape == y.shape and torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


@pytest.mark.parametrize("strat", [False, True])
@pytest.mark.parametrize("M", [1, 2, 8])
@pytest.mark.parametrize("n", NS)
def test_device_matches_mirror(dev, n, M, strat):
    assert_matches_mirror(device(dev, n, M, strat), mirror(n, M, strat), n)


@pytest.mark.parametrize("strat", [False, True])
@pytest.mark.parametrize("n", [65, 1025, 2049])
def test_heavy_ties_and_constant_column(dev, n, strat):
    got = device(dev, n, 3, strat, "heavy")
    assert_matches_mirror(got, mirror(n, 3, strat, "heavy"), n)
    P, N = got.pn[:, 0], got.pn[:, 1]
    assert torch.equal(got.a2[:, 2], P * N)               # a constant column: every pair is a tie


@pytest.mark.parametrize("n,M,strat", [(65, 3, True), (1025, 3, False), (2049, 8, True)])
def test_columns_match_bootstrap_metrics_on_device(dev, n, M, strat):
    y, S = (t.to(dev) for t in inputs(n, M))
    got = device(dev, n, M, strat)
    for m in range(M):
        auroc, ap, a2, pn, conf, _ = ops.bootstrap_metrics(y, S[m], B, seed=3, stratified=strat)
        assert torch.equal(a2, got.a2[:, m]) and torch.equal(pn, got.pn) and torch.equal(conf, got.conf[:, m])
        assert torch.equal(ap.view(torch.int64), got.ap[:, m].view(torch.int64))
        assert torch.equal(auroc.view(torch.int64), got.auroc[:, m].view(torch.int64))


@pytest.mark.parametrize("n,M,strat", [(1025, 3, False), (2049, 2, True)])
def test_grid_storage_and_range_invariance(dev, monkeypatch, n, M, strat):
    a = device(dev, n, M, strat)
    assert equal_bits(a, device(dev, n, M, strat))
    for grid in (1, 3):                                   # grid 3: three replicates per workgroup, re-zeroed between
        assert equal_bits(a, device(dev, n, M, strat, grid=grid))
    parts = [device(dev, n, M, strat, b0=lo, b1=hi) for lo, hi in ((0, 1), (1, 5), (5, 5), (5, B))]
    assert equal_bits([torch.cat([p[k] for p in parts]) for k in range(7)], a)
    monkeypatch.setattr(api, "_COMPARE_FORCE_GLOBAL", True)
    assert equal_bits(a, device(dev, n, M, strat))
    assert equal_bits(a, device(dev, n, M, strat, grid=3))
    monkeypatch.setattr(api, "BOOTSTRAP_WS_BYTES", 1)     # one slice: one workgroup runs every replicate
    assert equal_bits(a, device(dev, n, M, strat))


def test_lds_rows_limit(dev):
    out = torch.zeros(1, dtype=torch.int64)
    ops.ext().compare_lds_rows(out.data_ptr())
    assert int(out[0]) == L
    for n in (L, L + 1):
        assert_matches_mirror(device(dev, n, 2, False, nb=2), mirror(n, 2, False, nb=2), n, ints_only=True)


def test_f32_scores_and_external_stream(dev):
    y, S = inputs(1025, 3)
    S32 = S.float()
    want = ops.bootstrap_compare(y, S32, B, seed=3)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = ops.bootstrap_compare(y.to(dev), S32.to(dev), B, seed=3, stream=side.cuda_stream)
    side.synchronize()
    assert_matches_mirror(got, want, 1025)


def test_degenerate_replicates(dev):
    y = np.array([1, 0, 0], dtype=np.int64)
    S = np.array([[0.8, 0.4, 0.6], [0.3, 0.7, 0.6]])
    want = ref.compare_oracle(y, S, 64, seed=0)
    assert 0 < want["n_degenerate"] < 64
    got = ops.bootstrap_compare(torch.as_tensor(y).to(dev), torch.as_tensor(S).to(dev), 64, seed=0)
    g = {k: v.cpu().numpy() for k, v in zip(ref.CompareBootstrap._fields, got)}
    for k in ("a2", "pn", "conf", "reclass"):
        assert np.array_equal(g[k], want[k]), k
    deg = (want["pn"][:, 0] == 0) | (want["pn"][:, 1] == 0)
    assert int(deg.sum()) == want["n_degenerate"]
    for k in ("auroc", "ap"):
        assert np.array_equal(np.isnan(g[k]), np.repeat(deg[:, None], 2, 1))
    assert np.array_equal(g["auroc"][~deg], want["auroc"][~deg].astype(np.float64))
    ci = metrics.compare_ci(y, {"a": S[0], "b": S[1]}, "a", n_boot=64, seed=0, device=dev)
    assert ci["n_degenerate"] == want["n_degenerate"]
    assert not np.isnan(ci["comparisons"]["b"]["delta_auroc"]["se"])


def test_compare_ci_device_equals_host(dev):
    rng = np.random.default_rng(0)
    n = 2000
    y = (rng.random(n) < 0.25).astype(np.int64)
    shared = rng.standard_normal(n)
    cols = {name: 1 / (1 + np.exp(-(w * y + shared + s * rng.standard_normal(n) - 0.5)))
            for name, w, s in (("stack", 1.3, 0.3), ("svc", 1.1, 0.4), ("gbc", 1.0, 0.5), ("lg", 0.9, 0.6))}
    want = metrics.compare_ci(y, cols, "stack", n_boot=500, device="cpu")
    got = metrics.compare_ci(y, cols, "stack", n_boot=500, device=dev)
    assert got["n_degenerate"] == want["n_degenerate"] == 0 and got["auroc"] == want["auroc"]
    exact = ("delta_auroc", "delta_sensitivity", "delta_specificity", "delta_net_benefit", "nri", "nri_event",
             "nri_nonevent")
    for name in ("svc", "gbc", "lg"):
        g, w = got["comparisons"][name], want["comparisons"][name]
        for k in exact:
            assert g[k] == w[k], (name, k)                # ratios of equal integers
        assert g["delong"] == w["delong"]
        for k, bound in (("delta_ap", 2 * 4 * n * U), ("idi", 8 * 25 * U), ("delta_brier", 2 * 25 * U)):
            # a difference of two APs; four class means / two Brier scores, each ≤ 1 with relative
            # error ≤ (ceil(n/1024) + 22 + 1)·2^-53 = 25·2^-53 (the fold and the division)
            assert g[k]["point"] == w[k]["point"] and g[k]["p"] == w[k]["p"]
            for f in ("lo", "hi", "se"):
                d = abs(g[k][f] - w[k][f])
                print(f"{name} {k} {f}: |d| {d / U:.3g} u")
                assert d <= bound
