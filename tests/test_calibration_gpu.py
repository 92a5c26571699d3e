"""The fused calibration kernel (``csrc/calibration.hip``) against the host mirror and, at small n,
directly against the independent oracle; determinism and independence of the launch geometry and
of the storage path; the CI-level case and the training CLI on the device.

Bounds as in ``test_calibration.py``: the integers bit-equal, ``|brier|``, ``|sum_p|/n`` and
``|bin_sum_p|/n`` ≤ ``4·n·2^-53`` (device and mirror evaluate one formula on equal integers and differ
by summation order only) and ``|coef| ≤ 1e-10·max(1, |a|, |b|)``: both sides stop on an undamped
Newton step of 1e-10, so each is within the square of that of the optimum."""
import functools
import json

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.ops import api
from hfens.ops import reference as ref
from hfens.utils import metrics
from test_calibration import FIELDS, INTS, U, assert_matches_oracle, edge_cases, make_scores, oracle_of, run_op

pytestmark = pytest.mark.gpu

L = api.CALIBRATION_LDS_ROWS
THREADS = 1024                      # workgroup size of the kernel: thread t owns a contiguous chunk of rows
# (n, kind, stratified, B): chunk and wave edges, the LDS limit (L + 1 takes the global path), a few times L
SIZE_CASES = [(n, kind, strat, 8) for n in (THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1)
              for kind, strat in (("decimal", False), ("continuous", True))]
SIZE_CASES += [(n, "decimal", strat, 8) for n in (L - 1, L, L + 1) for strat in (False, True)]
SIZE_CASES += [(3 * L + 7, "decimal", False, 4), (3 * L + 7, "continuous", True, 4)]


def assert_matches_mirror(got, want, n, all_fitted=False):
    got = ref.CalibrationBootstrap(*(t.cpu() for t in got))
    for k in INTS:
        assert getattr(got, k).dtype == torch.int64 and torch.equal(getattr(got, k), getattr(want, k)), k
    if all_fitted:
        assert bool((want.status == 0).all())
    db = float((got.brier - want.brier).abs().max())
    dsp = float((got.sum_p - want.sum_p).abs().max()) / n
    dbs = float((got.bin_sum_p - want.bin_sum_p).abs().max()) / n
    print(f"max|dbrier| {db / U:.3g} u  max|dsum_p|/n {dsp / U:.3g} u  max|dbin_sum_p|/n {dbs / U:.3g} u")
    assert db <= 4 * n * U and dsp <= 4 * n * U and dbs <= 4 * n * U
    ok = want.status == 0
    assert bool(torch.isnan(got.coef[~ok]).all()) and bool((got.iters[~ok] == 0).all())
    if bool(ok.any()):
        c, w = got.coef[ok], want.coef[ok]
        worst = float(((c - w).abs().max(1).values / w.abs().max(1).values.clamp(min=1.0)).max())
        print(f"max coef error / max(1, |a|, |b|) = {worst:.3g}  iters {int(got.iters.max())} / {int(want.iters.max())}")
        assert not bool(torch.isnan(c).any()) and worst <= 1e-10


def equal_bits(a, b):
    return all(x.shape == y.shape and torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def size_inputs(n, kind):
    y, p = make_scores(n, kind)
    return torch.as_tensor(y), torch.as_tensor(p)


@functools.lru_cache(maxsize=None)
def size_mirror(n, kind, strat, B):
    y, p = size_inputs(n, kind)
    return ops.bootstrap_calibration(y, p, B, seed=3, stratified=strat)


def size_device(dev, n, kind, strat, B, **kw):
    y, p = size_inputs(n, kind)
    return ops.bootstrap_calibration(y.to(dev), p.to(dev), B, seed=3, stratified=strat, **kw)


def test_lds_rows_mirror_the_kernel():
    out = torch.zeros(1, dtype=torch.int64)
    ops.ext().calibration_lds_rows(out.data_ptr())
    assert int(out) == L


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_device_matches_mirror_and_oracle_small(dev, case):
    got = run_op(case, dev)
    assert_matches_mirror(got, run_op(case), case[0])
    assert_matches_oracle(got, oracle_of(case), case[0])


@pytest.mark.parametrize("n,kind,strat,B", SIZE_CASES)
def test_device_matches_mirror_sizes(dev, n, kind, strat, B):
    assert_matches_mirror(size_device(dev, n, kind, strat, B), size_mirror(n, kind, strat, B), n, all_fitted=True)


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
    monkeypatch.setattr(api, "_CALIBRATION_FORCE_GLOBAL", True)
    assert equal_bits(a, size_device(dev, n, kind, strat, B))
    assert equal_bits(a, size_device(dev, n, kind, strat, B, grid=3))


def test_f32_scores(dev):
    y, p = size_inputs(THREADS + 1, "decimal")
    p32 = p.float()
    want = ops.bootstrap_calibration(y, p32, 8, seed=3)
    assert_matches_mirror(ops.bootstrap_calibration(y.to(dev), p32.to(dev), 8, seed=3), want, THREADS + 1)
    assert equal_bits(want, ops.bootstrap_calibration(y, p32.double(), 8, seed=3))


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
    y, p = (t.to(dev) for t in size_inputs(n, "decimal"))
    whole = ops.bootstrap_calibration(y, p, 12, seed=3)
    parts = [ops.bootstrap_calibration(y, p, 12, seed=3, b0=a, b1=b) for a, b in ((0, 1), (1, 7), (7, 7), (7, 12))]
    assert equal_bits([torch.cat([q[k] for q in parts]) for k in range(len(FIELDS))], whole)
    assert equal_bits(whole, size_device(dev, n, "decimal", False, 12)) is True
    assert not torch.equal(ops.bootstrap_calibration(y, p, 12, seed=4).bin_n, whole.bin_n)
    assert torch.equal(whole.pn, ops.bootstrap_metrics(y, p, 12, seed=3)[3])


def test_ci_level_10k_by_2000(dev):
    rng = np.random.default_rng(0)
    n = 10_000
    y = (rng.random(n) < 0.2).astype(np.int64)
    s = np.clip(0.25 + 0.3 * y + 0.2 * rng.standard_normal(n), 0.0, 1.0)
    assert n <= L
    want = metrics.calibration_ci(y, s, n_boot=2000, device="cpu")
    got = metrics.calibration_ci(y, s, n_boot=2000, device=dev)
    for k in ("n_degenerate", "n_separable", "n_unconverged"):
        assert got[k] == want[k] == 0
    assert got["reliability"] == want["reliability"]              # ratios of equal integers, host point estimates
    assert got["decision_curve"] == want["decision_curve"]
    for k in ("brier", "oe_ratio", "ece", "intercept", "slope"):
        assert got[k]["point"] == want[k]["point"]
    # a quantile or a standard deviation moves by no more than its replicates do.  ECE = Σ_k |bin_pos_k −
    # bin_sum_p_k|/n moves by at most the 10 bins' bounds; O:E = P/Σp by O:E·(n/Σp)·|dΣp|/n, and the mean
    # score of every resample is above 1/4 here (the scores centre on 0.25 + 0.3·y, its se is 0.002).
    for f in ("lo", "hi", "se"):
        for k, bound in (("brier", 4 * n * U), ("ece", 10 * 4 * n * U),
                         ("oe_ratio", 4 * n * U * 4 * want["oe_ratio"]["hi"])):
            d = abs(got[k][f] - want[k][f])
            print(f"{k} {f}: |d| {d / U:.3g} u")
            assert d <= bound
        for k in ("intercept", "slope"):
            d = abs(got[k][f] - want[k][f])
            print(f"{k} {f}: |d| {d:.3g}")
            assert d <= 1e-10 * max(1.0, abs(want["intercept"][f]), abs(want["slope"][f]))
    assert want["brier"]["lo"] < want["brier"]["point"] < want["brier"]["hi"]


def test_cli_calibration_cuda(tmp_path, monkeypatch, capsys):
    """``--device cuda --calibration --bootstrap 64`` prints what ``calibration_ci`` gives on the host
    for the same held-out probabilities, to the printed digits."""
    from hfens.cli.train_ensemble_public import main
    monkeypatch.chdir(tmp_path)
    seen = []
    real_ci = metrics.calibration_ci

    def spy(y, p, **kw):
        seen.append((y, p, kw, real_ci(y, p, **kw)))
        return seen[-1][3]
    monkeypatch.setattr(metrics, "calibration_ci", spy)
    assert main(["--device", "cuda", "--rows", "100", "--features", "12", "--data-dir", str(tmp_path),
                 "--json", "r.json", "--calibration", "--bootstrap", "64"]) == 0
    out = capsys.readouterr().out
    y, p, kw, on_dev = seen[0]
    assert p.is_cuda and kw["n_boot"] == 64
    host = real_ci(y.cpu(), p.cpu(), **kw)
    cell = lambda v: f"{v['point']:.4f} (95% CI {v['lo']:.4f}–{v['hi']:.4f})"  # noqa: E731
    for ci in (host, on_dev):
        assert "   ".join(f"{name} = {cell(ci[k])}" for name, k in (
            ("Brier", "brier"), ("O:E", "oe_ratio"), ("intercept", "intercept"), ("slope", "slope"),
            ("ECE", "ece"))) in out.splitlines()
    same = lambda a, b: json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)  # noqa: E731  (NaN for empty bins)
    assert same(host["decision_curve"], on_dev["decision_curve"]) and same(host["reliability"], on_dev["reliability"])
    j = json.loads(open("r.json").read().splitlines()[-1])
    assert same(j["calibration"]["decision_curve"], on_dev["decision_curve"]) and "bootstrap" in j
    assert any((tmp_path / f"hf_calibration.{e}").exists() for e in ("png", "svg"))
    assert any((tmp_path / f"hf_decision.{e}").exists() for e in ("png", "svg"))
