"""Permutation importance on the GPU: ``stack_permute`` against the host mirror, ``rank_rows`` against
the torch mirror fed the same f32 scores, the bit-identities (grid, LDS against presorted path, range,
workspace chunking), the exact zero of a constant column, the law across devices, and StackExplainer
and the CLI on ``cuda``.

Tolerances: 5e-6 per score is ``test_partial_gpu.py``'s bound for the same tile body; 4·n·2⁻⁵³ is the
project's bound for a fold of n f64 terms in [0, 1] (``ap``, ``brier``); ``a2`` and ``auroc`` are exact."""
import functools
import json

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.explain import StackExplainer
from hfens.io.checkpoint import load_checkpoint
from hfens.io.synth import MODEL_FEATURES, make_hf_cohort
from hfens.ops import api
from hfens.ops import reference as ref
from hfens.ops.packing import PackedStack, pack_forest, pack_svs, stump_table

pytestmark = pytest.mark.gpu


def _random_pstack(F, m, T, depth, device, seed=0, stumps=True):
    g = torch.Generator().manual_seed(seed)
    sv = torch.randn(m, F, generator=g, dtype=torch.float64)
    coef = torch.randn(m, generator=g, dtype=torch.float64) / m ** 0.5
    rng = np.random.default_rng(seed)
    K = 2 ** (depth + 1) - 1
    feat = np.full((T, K), -2)
    thr = np.full((T, K), -2.0)
    left = np.full((T, K), -1)
    right = np.full((T, K), -1)
    val = rng.normal(size=(T, K))
    for t in range(T):
        for i in range(2 ** depth - 1):
            feat[t, i] = rng.integers(0, F)
            thr[t, i] = rng.normal()
            left[t, i], right[t, i] = 2 * i + 1, 2 * i + 2
    tabs = [torch.as_tensor(a) for a in (feat, thr, left, right, val)]
    f = pack_forest(*tabs, device)
    return PackedStack(
        F=F, sv=pack_svs(sv, coef, device),
        mean=(0.1 * torch.randn(F, generator=g)).to(device), inv_scale=(0.5 + torch.rand(F, generator=g)).to(device),
        gamma=0.5 / F, svc_b=0.2, probA=-1.7, probB=0.1, forest=f,
        stumps=stump_table(*tabs, -0.4, 0.1, F, device) if stumps else None, gb_init=-0.4, gb_lr=0.1,
        lr_w=(0.3 * torch.randn(F, generator=g)).to(device), lr_b=-0.2,
        meta_w=(1.9, 0.5, 2.7), meta_b=-2.0)


# (F, m, T, depth, stumps, n): one F per stack_ks bucket, n around the 64-row tile, several tiles per
# workgroup, and SVs beyond LDS (restaging barriers inside the tile loop)
SHAPES = [
    (3, 64, 10, 2, False, 1),
    (17, 250, 30, 1, True, 63),
    (20, 64, 10, 1, True, 64),
    (30, 64, 8, 1, True, 65),
    (40, 64, 8, 1, True, 1000),
    (8, 6000, 20, 1, True, 65),
]
R_SHAPES = 3


def _inputs(shape):
    F, m, T, depth, stumps, n = shape
    g = torch.Generator().manual_seed(100 * F + n)
    x = torch.randn(n, F, generator=g, dtype=torch.float64)
    src = ops.permutation_sources(n, 0, R_SHAPES, seed=F)
    return x, src, [-1, 0, F // 2, F - 1]


@functools.lru_cache(maxsize=None)
def _mirror(shape):
    F, m, T, depth, stumps, n = shape
    x, src, feats = _inputs(shape)
    return ops.stack_permute_scores(x, _random_pstack(F, m, T, depth, "cpu", seed=F, stumps=stumps), src, feats)


@pytest.mark.parametrize("shape", SHAPES)
def test_scores_match_mirror_for_every_grid(dev, shape):
    F, m, T, depth, stumps, n = shape
    x, src, feats = _inputs(shape)
    pk = _random_pstack(F, m, T, depth, dev, seed=F, stumps=stumps)
    S = ops.stack_permute_scores(x.to(dev), pk, src.to(dev), feats)
    want = _mirror(shape)
    assert S.dtype == torch.float32 and S.shape == (4, R_SHAPES, n) and want.dtype == torch.float64
    d = float((S.cpu().double() - want).abs().max())
    print(f"max|dS| {d:.3g}")
    assert d <= 5e-6
    assert torch.equal(S[0, 0], S[0, 1])                    # −1: no substitution in any repeat
    if n > 2:
        assert not torch.equal(S[1], S[0])
    for grid in (1, 7):
        assert torch.equal(ops.stack_permute_scores(x.to(dev), pk, src.to(dev), feats, grid=grid), S)
    assert torch.equal(ops.stack_permute_scores(x.to(dev, torch.float32), pk, src.to(dev).long(),
                                                torch.tensor(feats, device=dev)), S)


@functools.lru_cache(maxsize=None)
def _ckpt(ckpt_path, device):
    return load_checkpoint(ckpt_path)._packed_stack(torch.device(device))


def _cohort(n, seed=5, binary=False):
    X, y, _ = make_hf_cohort(max(n, 8), 17, seed=seed, nan_frac=0.0)
    X, y = torch.as_tensor(X)[:n].clone(), torch.as_tensor(y)[:n].clone()
    if binary:
        X = (X > X.median(0).values[None, :]).to(torch.float64)
    y[0], y[-1] = 0.0, 1.0
    return X, y


def _check_rank(dev, ckpt_path, n, binary=False):
    X, y = _cohort(n, binary=binary)
    pk = _ckpt(ckpt_path, "cuda:0")
    S = ops.stack_permute_scores(X.to(dev), pk, ops.permutation_sources(n, 0, 2, seed=1, device=dev), [-1, 0, 11])
    S = S.reshape(-1, n)
    got = ops.rank_metrics(y.to(dev), S)
    want = ref.rank_metrics(y, S.cpu())
    assert got.a2.dtype == torch.int64 and all(t.shape == (6,) for t in got)
    assert torch.equal(got.a2.cpu(), want.a2)
    assert torch.equal(got.auroc.cpu(), want.auroc)
    dap = float((got.ap.cpu() - want.ap).abs().max())
    dbr = float((got.brier.cpu() - want.brier).abs().max())
    ties = n - int(torch.unique(S[2]).numel())
    print(f"n {n}  tied rows {ties}  |dap| {dap:.3g}  |dbrier| {dbr:.3g}  bound {4 * n * 2.0 ** -53:.3g}")
    assert dap <= 4 * n * 2.0 ** -53 and dbr <= 4 * n * 2.0 ** -53
    return got, ties


@pytest.mark.parametrize("n", [2, 1023, 1024, 1025, api.PERMUTE_LDS_ROWS, api.PERMUTE_LDS_ROWS + 1])
def test_rank_metrics_match_mirror(dev, ckpt_path, n, monkeypatch):
    got, _ = _check_rank(dev, ckpt_path, n)
    if n <= api.PERMUTE_LDS_ROWS:       # the presorted path on the same rows: every output, bit for bit
        monkeypatch.setattr(api, "_PERMUTE_FORCE_GLOBAL", True)
        again, _ = _check_rank(dev, ckpt_path, n)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert torch.equal(got.a2[0], got.a2[1])                # the two baseline rows


def test_rank_metrics_heavy_ties(dev, ckpt_path, monkeypatch):
    got, ties = _check_rank(dev, ckpt_path, 1025, binary=True)
    assert ties > 0
    monkeypatch.setattr(api, "_PERMUTE_FORCE_GLOBAL", True)
    again, _ = _check_rank(dev, ckpt_path, 1025, binary=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # −0 ties +0, and scores that are no probabilities
    y = torch.tensor([0.0, 1.0, 0.0, 1.0], device=dev)
    s = torch.tensor([[0.0, -0.0, -1.5, 2.0], [3.0, 3.0, 3.0, 3.0]], device=dev)
    out = ops.rank_metrics(y, s)
    assert out.a2.tolist() == [7, 4] and out.auroc.tolist() == [7 / 8, 0.5]


def test_lds_rows_mirror_the_kernel():
    out = torch.zeros(1, dtype=torch.int64)
    ops.ext().rank_lds_rows(out.data_ptr())
    assert int(out[0]) == api.PERMUTE_LDS_ROWS
    assert 13 * api.PERMUTE_LDS_ROWS + 544 <= 160 * 1024       # 13 B/row beside the kernel's static scratch


def test_rank_metrics_needs_both_classes(dev):
    with pytest.raises(ValueError, match="both classes must be present in y"):
        ops.rank_metrics(torch.ones(1, device=dev), torch.rand(3, 1, device=dev))


N_ID, R_ID = 300, 6


def _importance(dev, ckpt_path, **kw):
    X, y = _cohort(N_ID)
    X[:, 3] = 1.0                                             # a constant column
    return ops.permutation_importance(X.to(dev), y.to(dev), _ckpt(ckpt_path, "cuda:0"), R_ID, seed=2020, **kw)


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(a[1][m], b[1][m]) for m in a[1])


def test_bit_identity_and_exact_zero(dev, ckpt_path, monkeypatch):
    whole = _importance(dev, ckpt_path)
    assert all(v.shape == (17, R_ID) and v.dtype == torch.float64 and v.is_cuda for v in whole[1].values())
    for m in whole[1]:
        assert bool((whole[1][m][3] == 0.0).all())            # exactly zero, in all three metrics
    assert float(whole[1]["auroc"].abs().max()) > 0.0
    for grid in (1, 7):
        assert _same(_importance(dev, ckpt_path, grid=grid), whole)
    parts = [_importance(dev, ckpt_path, r0=0, r1=4), _importance(dev, ckpt_path, r0=4, r1=R_ID)]
    assert parts[0][0] == whole[0]
    assert all(torch.equal(torch.cat([parts[0][1][m], parts[1][1][m]], 1), whole[1][m]) for m in whole[1])
    monkeypatch.setattr(api, "PERMUTE_WS_BYTES", 4 * N_ID * 4)                # four score rows per chunk
    assert _same(_importance(dev, ckpt_path), whole)
    monkeypatch.setattr(api, "PERMUTE_WS_BYTES", 4 * N_ID * (2 * R_ID + 1))   # two columns per chunk
    assert _same(_importance(dev, ckpt_path), whole)
    monkeypatch.setattr(api, "PERMUTE_WS_BYTES", 256 << 20)
    monkeypatch.setattr(api, "_PERMUTE_FORCE_GLOBAL", True)
    assert _same(_importance(dev, ckpt_path), whole)


@pytest.mark.parametrize("n", [1, 65, 1000, 70000])
def test_sources_agree_across_devices(dev, n):
    assert torch.equal(ops.permutation_sources(n, 2, 6, seed=9, device=dev).cpu(), ops.permutation_sources(n, 2, 6, seed=9))


def _host_ranked(X, y, pk_cuda, R, seed, dev):
    """Importances from the f32 scores ``stack_permute`` makes on ``cuda``, ranked and differenced on the
    host by the torch mirror: ``(baseline, importances)`` as ``ops.permutation_importance`` returns them."""
    n, F = X.shape
    S = ops.stack_permute_scores(X.to(dev), pk_cuda, ops.permutation_sources(n, 0, R, seed=seed, device=dev),
                                 [-1] + list(range(F))).cpu()
    m = ref.rank_metrics(y.cpu(), S.reshape(-1, n))
    t = {k: getattr(m, k).reshape(F + 1, R) for k in ("auroc", "ap", "brier")}
    base = {k: float(v[0, 0]) for k, v in t.items()}
    return base, {"auroc": t["auroc"][0, 0] - t["auroc"][1:], "ap": t["ap"][0, 0] - t["ap"][1:],
                  "brier": t["brier"][1:] - t["brier"][0, 0]}


def _pair_bounds(X, y, pk_cpu, R, seed):
    """Per score row of the host mirror, the share of (positive, negative) pairs whose scores are within
    1e-5 of each other: ``[1 + F, R]``, row 0 the baseline."""
    n, F = X.shape
    S = ops.stack_permute_scores(X, pk_cpu, ops.permutation_sources(n, 0, R, seed=seed), [-1] + list(range(F)))
    pos, neg = S[:, :, y == 1], S[:, :, y == 0]
    return ((pos[..., :, None] - neg[..., None, :]).abs() <= 1e-5).sum((-1, -2)).double() / (pos.shape[-1] * neg.shape[-1])


def _check_against_host(got_base, got_imp, X, y, pk_cuda, pk_cpu, R, seed, dev):
    """``got``: baseline and importances computed on ``cuda``.  Two references on the host:

    * the torch mirror fed the same f32 scores (made on ``cuda``): AUROC is exact there, so baseline
      and importances are bit-equal; AP and Brier are folds of n f64 terms in [0, 1], each within the
      project's 4·n·2⁻⁵³ of the mirror, so a baseline is within that and an importance (a difference of
      two of them) within twice that;
    * the f64 mirror end to end.  Its scores differ by at most 5e-6 (the tile body's bound), so a
      (positive, negative) pair can change its share of a2 only if its host scores are within 1e-5 of each
      other: |Δauroc| of a score row is at most the share of such pairs (an importance: the row's share
      plus the baseline's).  |Δ(s − y)²| ≤ 2·5e-6 per row: 1e-5 for a Brier baseline, 2e-5 for an importance.
    Returns the host f64 result and the AUROC importance bounds [F, R]."""
    n = X.shape[0]
    fold = 4 * n * 2.0 ** -53
    hb, hi = _host_ranked(X, y, pk_cuda, R, seed, dev)
    assert got_base["auroc"] == hb["auroc"]
    assert torch.equal(got_imp["auroc"].cpu(), hi["auroc"])
    for k in ("ap", "brier"):
        d = float((got_imp[k].cpu() - hi[k]).abs().max())
        print(f"same f32 scores: max|d {k} importance| {d:.3g}  bound {2 * fold:.3g}")
        assert abs(got_base[k] - hb[k]) <= fold and d <= 2 * fold
    cb, ci = ops.permutation_importance(X.cpu(), y.cpu(), pk_cpu, R, seed=seed)
    close = _pair_bounds(X.cpu(), y.cpu(), pk_cpu, R, seed)
    bound = close[1:] + close[0, 0]
    d = (got_imp["auroc"].cpu() - ci["auroc"]).abs()
    print(f"f64 mirror: max|d auroc importance| {float(d.max()):.3g}  largest bound {float(bound.max()):.3g}")
    assert bool((d <= bound + 1e-15).all())
    assert abs(got_base["auroc"] - cb["auroc"]) <= float(close[0, 0]) + 1e-15
    dbr = float((got_imp["brier"].cpu() - ci["brier"]).abs().max())
    print(f"f64 mirror: max|d brier importance| {dbr:.3g}")
    assert dbr <= 2e-5 and abs(got_base["brier"] - cb["brier"]) <= 1e-5
    return (cb, ci), bound


def test_explainer_on_cuda_agrees_with_cpu(dev, ckpt_path):
    n, R = 200, 3
    X, y = _cohort(n)
    bg = X[:16]
    gpu = StackExplainer(load_checkpoint(ckpt_path), bg, device="cuda", feature_names=list(MODEL_FEATURES))
    cpu = StackExplainer(load_checkpoint(ckpt_path), bg, device="cpu", feature_names=list(MODEL_FEATURES))
    a, b = gpu.permutation_importance(X, y, R, seed=7), cpu.permutation_importance(X, y, R, seed=7)
    assert a.names == b.names and a.importances["auroc"].is_cuda
    (cb, ci), _ = _check_against_host(a.baseline, a.importances, X, y, _ckpt(ckpt_path, "cuda:0"),
                                      _ckpt(ckpt_path, "cpu"), R, 7, dev)
    assert b.baseline == cb and all(torch.equal(b.importances[k], ci[k]) for k in ci)


def test_cli_importance_cuda(dev, tmp_path, monkeypatch, capsys):
    from hfens import pipeline
    from hfens.cli.train_ensemble_public import main
    from hfens.io.synth import make_dev_select
    monkeypatch.chdir(tmp_path)
    real_develop, fits = pipeline.develop, {}

    def develop_spy(*a, **kw):
        fits["res"] = real_develop(*a, **kw)
        return fits["res"]
    monkeypatch.setattr(pipeline, "develop", develop_spy)
    R = 3
    assert main(["--device", "cuda", "--rows", "100", "--features", "12", "--data-dir", str(tmp_path),
                 "--json", "hf.json", "--no-plots", "--importance", str(R)]) == 0
    out = capsys.readouterr().out
    res = fits["res"]
    F = len(res.selected_names)
    mine = [ln for ln in out.splitlines() if "ΔAUROC " in ln]
    rec = json.loads(open("hf.json").read().splitlines()[-1])["importance"]
    assert len(mine) == F == len(rec["variables"]) and rec["n_repeats"] == R and rec["seed"] == 2020
    assert res.X_sel.is_cuda and res.X_sel.shape == (100, F)
    # the record against the op on the same tensors: the same bits
    y = torch.as_tensor(make_dev_select(100, 12, seed=2020)[3])
    pk = res.model._packed_stack(res.X_sel.device)
    base, imp = ops.permutation_importance(res.X_sel, y.to(dev), pk, R, seed=2020)
    assert rec["baseline"] == base
    means = {k: v.mean(1).tolist() for k, v in imp.items()}
    order = sorted(range(F), key=lambda k: (-means["auroc"][k], k))
    assert [v["name"] for v in rec["variables"]] == [res.selected_names[k] for k in order]
    for k in ("ap", "brier"):
        assert [v[k] for v in rec["variables"]] == [means[k][j] for j in order]
    assert [v["auroc"]["mean"] for v in rec["variables"]] == [means["auroc"][j] for j in order]
    # the record against the host: the held-out columns and labels on the host, the model packed there
    X = res.X_sel.cpu()
    pk_cpu = res.model._packed_stack(torch.device("cpu"))
    (cb, ci), bound = _check_against_host(rec["baseline"], imp, X, y, pk, pk_cpu, R, 2020, dev)
    by_name = {v["name"]: v for v in rec["variables"]}
    cmean = ci["auroc"].mean(1)
    mbound = bound.mean(1) + 4 * 2.0 ** -53        # a mean of R values, each within its bound, rounded
    for k, name in enumerate(res.selected_names):
        assert abs(by_name[name]["auroc"]["mean"] - float(cmean[k])) <= float(mbound[k])
        assert abs(by_name[name]["brier"] - float(ci["brier"].mean(1)[k])) <= 2e-5 + 4 * 2.0 ** -53
    # the order is the host's, unless the two means could change places within their bounds
    horder = sorted(range(F), key=lambda k: (-float(cmean[k]), k))
    for a_, b_ in zip(order, horder):
        assert a_ == b_ or abs(float(cmean[a_] - cmean[b_])) <= float(mbound[a_] + mbound[b_])
    # what was permuted is what the stack saw: the baseline AUROC is the held-out AUROC the run printed
    # (stack_infer's scores: same tile body, within 5e-6 of the mirror as well)
    assert abs(rec["baseline"]["auroc"] - res.scores["auroc"]) <= 2 * float(_pair_bounds(X, y, pk_cpu, 1, 2020)[0, 0]) + 1e-15
