"""The fused bootstrap kernel (``csrc/bootstrap.hip``) against the host mirror and, at small n,
directly against the independent oracle; determinism and independence of the launch geometry and
of the storage path; the CI-level case and the training CLI on the device.

Bounds as in ``test_bootstrap.py``: the integers and ``auroc`` bit-equal, ``|ap| ≤ 4·n·2^-53``,
``|tpr| ≤ 16·2^-53`` (each side is within half of these of the exact value only through the
oracle; the same figures hold device against mirror because both evaluate one formula on equal
integers: their AP sums differ by summation order only, their TPR by nothing but the division
and product roundings)."""
import functools
import json

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.ops import api
from hfens.utils import metrics
from test_bootstrap import (U, assert_matches_oracle, edge_cases, make_case, oracle_of, run_op, sk_case)

pytestmark = pytest.mark.gpu

L = api.BOOTSTRAP_LDS_ROWS
THREADS = 1024                      # workgroup size of the kernel: thread t owns a contiguous chunk of rows
# (n, kind, stratified, B): chunk and wave edges, the LDS limit (L + 1 takes the global path), a few times L
SIZE_CASES = [(n, kind, strat, 8) for n in (THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1)
              for kind, strat in (("decimal", False), ("noties", True))]
SIZE_CASES += [(n, "decimal", strat, 8) for n in (L - 1, L, L + 1) for strat in (False, True)]
SIZE_CASES += [(3 * L + 7, "decimal", False, 4), (3 * L + 7, "noties", True, 4)]


def assert_matches_mirror(got, want, n):
    got = [t.cpu() for t in got]
    for k in (2, 3, 4):
        assert got[k].dtype == torch.int64 and torch.equal(got[k], want[k])
    nan = torch.isnan(want[0])
    assert torch.equal(torch.isnan(got[0]), nan) and torch.equal(torch.isnan(got[1]), nan)
    assert torch.equal(torch.isnan(got[5]), torch.isnan(want[5]))
    ok = ~nan
    assert torch.equal(got[0][ok], want[0][ok])
    if bool(ok.any()):
        dap = float((got[1][ok] - want[1][ok]).abs().max())
        dtpr = float((got[5][ok] - want[5][ok]).abs().max())
        print(f"max|dap| {dap / U:.3g} u  max|dtpr| {dtpr / U:.3g} u")
        assert dap <= 4 * n * U
        assert dtpr <= 16 * U


def equal_bits(a, b):
    return all(x.shape == y.shape and torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def size_inputs(n, kind):
    y, s = make_case(n, kind)
    return torch.as_tensor(y), torch.as_tensor(s)


@functools.lru_cache(maxsize=None)
def size_mirror(n, kind, strat, B):
    y, s = size_inputs(n, kind)
    return ops.bootstrap_metrics(y, s, B, seed=3, stratified=strat)


def size_device(dev, n, kind, strat, B, **kw):
    y, s = size_inputs(n, kind)
    return ops.bootstrap_metrics(y.to(dev), s.to(dev), B, seed=3, stratified=strat, **kw)


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_device_matches_mirror_and_oracle_small(dev, case):
    got = run_op(case, dev)
    assert_matches_mirror(got, run_op(case), case[0])
    assert_matches_oracle(got, oracle_of(case), case[0])


@pytest.mark.parametrize("n,kind,strat,B", SIZE_CASES)
def test_device_matches_mirror_sizes(dev, n, kind, strat, B):
    assert_matches_mirror(size_device(dev, n, kind, strat, B), size_mirror(n, kind, strat, B), n)


@pytest.mark.parametrize("n,kind,strat,B", [SIZE_CASES[0], (L + 1, "decimal", False, 8)])
def test_deterministic_and_grid_independent(dev, n, kind, strat, B):
    a = size_device(dev, n, kind, strat, B)
    assert equal_bits(a, size_device(dev, n, kind, strat, B))
    for grid in (1, 3):
        assert equal_bits(a, size_device(dev, n, kind, strat, B, grid=grid))


def test_one_workspace_slice(dev, monkeypatch):
    n, kind, strat, B = L + 1, "decimal", False, 8
    a = size_device(dev, n, kind, strat, B)
    monkeypatch.setattr(api, "BOOTSTRAP_WS_BYTES", 1)             # one slice: one workgroup runs every replicate
    assert equal_bits(a, size_device(dev, n, kind, strat, B))


@pytest.mark.parametrize("n,kind,strat,B", [SIZE_CASES[2], (L, "decimal", True, 8), (65, "decimal", False, 8)])
def test_lds_and_global_paths_agree(dev, monkeypatch, n, kind, strat, B):
    a = size_device(dev, n, kind, strat, B)
    monkeypatch.setattr(api, "_BOOTSTRAP_FORCE_GLOBAL", True)
    assert equal_bits(a, size_device(dev, n, kind, strat, B))
    assert equal_bits(a, size_device(dev, n, kind, strat, B, grid=3))


def test_f32_scores(dev):
    y, s = size_inputs(THREADS + 1, "decimal")
    s32 = s.float()
    want = ops.bootstrap_metrics(y, s32, 8, seed=3)
    assert_matches_mirror(ops.bootstrap_metrics(y.to(dev), s32.to(dev), 8, seed=3), want, THREADS + 1)
    assert equal_bits(want, ops.bootstrap_metrics(y, s32.double(), 8, seed=3))


def test_external_stream(dev):
    case = SIZE_CASES[1]
    want = size_device(dev, *case)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = size_device(dev, *case, stream=side.cuda_stream)
    side.synchronize()
    assert equal_bits(got, want)


@pytest.mark.parametrize("n", [THREADS + 1, L + 1])
def test_replicate_ranges(dev, n):
    y, s = (t.to(dev) for t in size_inputs(n, "decimal"))
    whole = ops.bootstrap_metrics(y, s, 12, seed=3)
    parts = [ops.bootstrap_metrics(y, s, 12, seed=3, b0=a, b1=b) for a, b in ((0, 1), (1, 7), (7, 7), (7, 12))]
    assert equal_bits([torch.cat([p[k] for p in parts]) for k in range(6)], whole)
    assert equal_bits(whole, size_device(dev, n, "decimal", False, 12)) is True
    assert not torch.equal(ops.bootstrap_metrics(y, s, 12, seed=4)[2], whole[2])


def test_ci_level_10k_by_2000(dev):
    rng = np.random.default_rng(0)
    n = 10_000
    y = (rng.random(n) < 0.2).astype(np.int64)
    s = np.clip(0.25 + 0.3 * y + 0.2 * rng.standard_normal(n), 0.0, 1.0)
    assert n <= L
    want = metrics.bootstrap_ci(y, s, n_boot=2000, device="cpu")
    got = metrics.bootstrap_ci(y, s, n_boot=2000, device=dev)
    assert got["n_degenerate"] == want["n_degenerate"] == 0
    assert got["auroc"] == want["auroc"]
    for k in ("precision", "recall", "specificity", "accuracy"):
        assert got[k] == want[k]                                  # ratios of equal integers
    for f in ("lo", "hi", "se"):
        d = abs(got["average_precision"][f] - want["average_precision"][f])
        print(f"ap {f}: |d| {d / U:.3g} u")
        assert d <= 4 * n * U
    assert got["average_precision"]["point"] == want["average_precision"]["point"]
    for k in ("tpr_lo", "tpr_median", "tpr_hi"):
        d = float(np.abs(np.asarray(got[k]) - np.asarray(want[k])).max())
        print(f"{k}: max|d| {d / U:.3g} u")
        assert d <= 16 * U
    assert want["auroc"]["lo"] < want["auroc"]["point"] < want["auroc"]["hi"]


def test_cli_bootstrap_cuda(tmp_path, monkeypatch, capsys):
    """``--device cuda --bootstrap 64`` prints what ``bootstrap_ci`` gives on the host for the same
    held-out probabilities, to the printed digits."""
    from hfens.cli.train_ensemble_public import main
    monkeypatch.chdir(tmp_path)
    seen = []
    real_ci = metrics.bootstrap_ci

    def spy(y, p, **kw):
        seen.append((y, p, kw, real_ci(y, p, **kw)))
        return seen[-1][3]
    monkeypatch.setattr(metrics, "bootstrap_ci", spy)
    assert main(["--device", "cuda", "--rows", "100", "--features", "12", "--data-dir", str(tmp_path),
                 "--json", "r.json", "--bootstrap", "64"]) == 0
    out = capsys.readouterr().out
    y, p, kw, on_dev = seen[0]
    assert p.is_cuda
    host = real_ci(y.cpu(), p.cpu(), **kw)
    cell = lambda ci, key: f"{ci[key]['point']:.4f} (95% CI {ci[key]['lo']:.4f}–{ci[key]['hi']:.4f})"  # noqa: E731
    for ci in (host, on_dev):
        assert f"AUROC = {cell(ci, 'auroc')}   AP = {cell(ci, 'average_precision')}" in out.splitlines()
        assert "   ".join(f"{m} = {cell(ci, m)}" for m in ("precision", "recall", "specificity", "accuracy")) \
            in out.splitlines()
    assert host["auroc"] == on_dev["auroc"] and host["n_degenerate"] == on_dev["n_degenerate"]
    assert json.loads(open("r.json").read().splitlines()[-1])["bootstrap"]["auroc"] == on_dev["auroc"]
    assert any((tmp_path / f"hf_roc.{e}").exists() for e in ("png", "svg"))
