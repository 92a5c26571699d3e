"""Bootstrap of the held-out metrics on the host: the torch mirror (``ops.bootstrap_metrics`` on
host tensors) against the independent oracle ``reference.bootstrap_oracle`` and against sklearn on
the materialised resample, the degenerate replicates, replicate ranges, ``metrics.bootstrap_ci``
and the training CLI's ``--bootstrap``.

Bounds against the oracle (longdouble, so its own error is negligible):
* the integers ``a2``, ``pn``, ``conf`` are equal and ``auroc`` is bit-equal to
  ``float(longdouble(A2) / (2·P·N))``;
* ``|ap − oracle| ≤ 4·n·2^-53``: the terms are non-negative and sum to at most 1, so any summation
  order is within ``(n−1)·2^-53`` plus the per-term roundings;
* ``|tpr − oracle| ≤ 16·2^-53``: at most 6 roundings on values ≤ 1 from an exact integer numerator.
"""
import functools
import json

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.ops import api
from hfens.ops import reference as ref
from hfens.utils import metrics

U = 2.0 ** -53
NS = (1, 2, 3, 63, 64, 65)
KINDS = ("noties", "equal", "decimal")
# (labels, threshold, stratified)
VARIANTS = (("mixed", 0.5, False), ("mixed", 0.5, True), ("allpos", 0.5, False),
            ("mixed", 2.0, False), ("mixed", -1.0, False))
B_EDGE = 16


def make_case(n, kind, labels="mixed", seed=0):
    """Labels (int64) and scores in (0, 1) (f64): about 30 % positives, both classes when n ≥ 2."""
    rng = np.random.default_rng(1000 * n + 10 * KINDS.index(kind) + seed)
    if labels == "allpos":
        y = np.ones(n, dtype=np.int64)
    else:
        y = (rng.random(n) < 0.3).astype(np.int64)
        if n >= 2:
            y[0], y[-1] = 1, 0
    s = {"noties": rng.permutation(n) / (n + 1.0) + 0.01, "equal": np.full(n, 0.625),
         "decimal": np.round(rng.random(n), 1)}[kind]
    return y, np.asarray(s, dtype=np.float64)


def edge_cases():
    out = []
    for n in NS:
        for kind in KINDS:
            for labels, thr, strat in VARIANTS:
                if strat and n < 2:
                    continue
                out.append((n, kind, labels, thr, strat))
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(case, B=B_EDGE, seed=7):
    n, kind, labels, thr, strat = case
    y, s = make_case(n, kind, labels)
    return ref.bootstrap_oracle(y, s, B, seed=seed, stratified=strat, threshold=thr)


def run_op(case, device="cpu", B=B_EDGE, seed=7, dtype=torch.float64, **kw):
    n, kind, labels, thr, strat = case
    y, s = make_case(n, kind, labels)
    return ops.bootstrap_metrics(torch.as_tensor(y).to(device), torch.as_tensor(s).to(device, dtype), B, seed=seed,
                                 stratified=strat, threshold=thr, **kw)


def assert_matches_oracle(got, want, n):
    auroc, ap, a2, pn, conf, tpr = (t.cpu().numpy() for t in got)
    assert auroc.dtype == ap.dtype == tpr.dtype == np.float64
    assert a2.dtype == pn.dtype == conf.dtype == np.int64
    assert np.array_equal(a2, want["a2"]) and np.array_equal(pn, want["pn"]) and np.array_equal(conf, want["conf"])
    nan = np.isnan(want["auroc"])
    assert np.array_equal(np.isnan(auroc), nan) and np.array_equal(np.isnan(ap), nan)
    assert np.array_equal(np.isnan(tpr), np.repeat(nan[:, None], tpr.shape[1], 1))
    ok = ~nan
    assert np.array_equal(auroc[ok], want["auroc"][ok].astype(np.float64))
    if ok.any():
        dap = float(np.abs(ap[ok] - want["ap"][ok]).max())
        dtpr = float(np.abs(tpr[ok] - want["tpr"][ok]).max())
        print(f"max|dap| {dap / U:.3g} u  max|dtpr| {dtpr / U:.3g} u")
        assert dap <= 4 * n * U
        assert dtpr <= 16 * U


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_mirror_matches_oracle(case):
    assert_matches_oracle(run_op(case), oracle_of(case), case[0])


# n, kind, replicates: the first 64 (n = 65) and the first 256 (n = 200) replicates are not degenerate
SK_CASES = ((50, "decimal", 64), (200, "noties", 256), (65, "noties", 64))


def sk_case(n, kind):
    rng = np.random.default_rng(0)
    y = (rng.random(n) < 0.2).astype(np.int64)
    s = rng.random(n)
    return y, (np.round(s, 1) if kind == "decimal" else s)


@pytest.mark.parametrize("n,kind,B", SK_CASES)
def test_mirror_matches_sklearn_on_resample(n, kind, B):
    from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve
    y, s = sk_case(n, kind)
    auroc, ap, _, pn, _, tpr = (t.numpy() for t in ops.bootstrap_metrics(torch.as_tensor(y), torch.as_tensor(s), B, seed=0))
    q = np.arange(101) / 100.0
    checked = 0
    for b in range(B):
        idx = ref.bootstrap_resample(y, b, 0)
        yy, ss = y[idx], s[idx]
        assert (int(yy.sum()), int(len(yy) - yy.sum())) == tuple(pn[b])
        if n == 50 and (yy.sum() == 0 or yy.sum() == n):
            assert np.isnan(auroc[b])
            continue
        checked += 1
        assert abs(roc_auc_score(yy, ss) - auroc[b]) <= 1e-12
        assert abs(average_precision_score(yy, ss) - ap[b]) <= 1e-12
        fpr, tp, _ = roc_curve(yy, ss, drop_intermediate=False)
        assert np.abs(np.interp(q, fpr, tp) - tpr[b]).max() <= 1e-12
    if n != 50:
        assert checked == B


def degenerate_case():
    y = np.array([1, 0, 0, 0, 0, 0, 0, 0], dtype=np.int64)     # the positive is row 0
    s = np.array([0.8, 0.4, 0.35, 0.1, 0.7, 0.2, 0.55, 0.6])
    return y, s


def test_degenerate_replicates():
    y, s = degenerate_case()
    want = ref.bootstrap_oracle(y, s, 64, seed=0)
    assert want["n_degenerate"] == 30
    got = ops.bootstrap_metrics(torch.as_tensor(y), torch.as_tensor(s), 64, seed=0)
    assert_matches_oracle(got, want, 8)
    assert int(torch.isnan(got[0]).sum()) == 30
    ci = metrics.bootstrap_ci(y, s, n_boot=64, seed=0)
    assert ci["n_degenerate"] == 30
    keep = got[0][~torch.isnan(got[0])].numpy()
    lo, hi = np.quantile(keep, [0.025, 0.975])
    assert ci["auroc"]["lo"] == float(lo) and ci["auroc"]["hi"] == float(hi)
    acc = ((got[4][:, 0] + got[4][:, 3]).double() / 8)[~torch.isnan(got[0])].numpy()
    assert ci["accuracy"]["lo"] == float(np.quantile(acc, 0.025))
    assert not any(np.isnan(ci[k][f]) for k in ("auroc", "average_precision", "specificity", "accuracy")
                   for f in ("lo", "hi", "se"))
    assert not np.isnan(ci["tpr_lo"]).any() and len(ci["tpr_hi"]) == len(ci["fpr_grid"]) == 101


def test_replicate_ranges_seed_and_strata():
    y, s = sk_case(200, "noties")
    yt, st = torch.as_tensor(y), torch.as_tensor(s)
    whole = ops.bootstrap_metrics(yt, st, 40, seed=5)
    parts = [ops.bootstrap_metrics(yt, st, 40, seed=5, b0=a, b1=b) for a, b in ((0, 1), (1, 17), (17, 17), (17, 40))]
    for k, w in enumerate(whole):
        cat = torch.cat([p[k] for p in parts])
        assert cat.shape == w.shape and torch.equal(cat.view(torch.int64), w.view(torch.int64))
    other = ops.bootstrap_metrics(yt, st, 40, seed=6)
    assert not torch.equal(other[2], whole[2])
    strat = ops.bootstrap_metrics(yt, st, 40, seed=5, stratified=True)
    P = int(y.sum())
    assert torch.equal(strat[3], torch.tensor([[P, 200 - P]]).expand(40, 2))
    assert not torch.equal(whole[3], strat[3])


def test_bootstrap_ci_brackets_point_and_is_deterministic():
    y, s = sk_case(200, "noties")
    a = metrics.bootstrap_ci(y, s, n_boot=64)
    b = metrics.bootstrap_ci(torch.as_tensor(y), torch.as_tensor(s), n_boot=64)
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    assert a["auroc"]["lo"] <= a["auroc"]["point"] <= a["auroc"]["hi"]
    assert a["auroc"]["point"] == metrics.roc_auc(y, s) and a["average_precision"]["point"] == metrics.average_precision(y, s)
    assert a["n_degenerate"] == 0 and a["n_boot"] == 64 and a["auroc"]["se"] > 0
    for k in ("auroc", "average_precision", "precision", "recall", "specificity", "accuracy"):
        assert a[k]["lo"] <= a[k]["hi"]
    assert all(l <= m <= h for l, m, h in zip(a["tpr_lo"], a["tpr_median"], a["tpr_hi"]))
    c = metrics.bootstrap_ci(y, s, n_boot=64, stratified=True)
    assert c["auroc"] != a["auroc"] and c["auroc"]["lo"] <= c["auroc"]["point"] <= c["auroc"]["hi"]


def test_validation_errors(monkeypatch):
    y = torch.tensor([0, 1, 1, 0])
    s = torch.tensor([0.1, 0.9, 0.4, 0.3], dtype=torch.float64)

    def rejects(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            ops.bootstrap_metrics(*a, **kw)
    rejects("y .* and score", y[:3], s, 8)
    rejects("score", y, torch.tensor([0.1, float("nan"), 0.4, 0.3]), 8)
    rejects("score", y, torch.tensor([0.1, float("inf"), 0.4, 0.3]), 8)
    rejects("y must hold labels", torch.tensor([0, 2, 1, 0]), s, 8)
    rejects("n = 0", y[:0], s[:0], 8)
    rejects("n_boot", y, s, 0)
    rejects("n_boot", y, s, (1 << 24) + 1)
    rejects("b0:b1", y, s, 8, b0=5, b1=4)
    rejects("b0:b1", y, s, 8, b1=9)
    rejects("grid_points", y, s, 8, grid_points=1)
    rejects("threshold", y, s, 8, threshold=float("nan"))
    rejects("stratified", torch.ones(4, dtype=torch.int64), s, 8, stratified=True)
    rejects("stratified", torch.zeros(4, dtype=torch.int64), s, 8, stratified=True)
    assert api.BOOTSTRAP_MAX_N == 1 << 25 and api.BOOTSTRAP_MAX_B == 1 << 24
    monkeypatch.setattr(api, "BOOTSTRAP_MAX_N", 3)
    rejects("n <= 3", y, s, 8)


def test_save_plots_band(tmp_path):
    y, s = sk_case(200, "noties")
    ci = metrics.bootstrap_ci(y, s, n_boot=16)
    roc, pr = metrics.save_plots(y, s, str(tmp_path / "b"), band=(ci["fpr_grid"], ci["tpr_lo"], ci["tpr_hi"]))
    roc0, pr0 = metrics.save_plots(y, s, str(tmp_path / "w"))
    read = lambda p: open(p, "rb").read()  # noqa: E731
    assert read(roc) != read(roc0) and read(pr) == read(pr0)


def test_cli_bootstrap_cpu(tmp_path, monkeypatch, capsys):
    from hfens import pipeline
    from hfens.cli.train_ensemble_public import main
    monkeypatch.chdir(tmp_path)
    real_develop, fits = pipeline.develop, {}

    def develop_once(*a, **kw):       # the three runs fit the same model: fit it once
        if "res" not in fits:
            fits["res"] = real_develop(*a, **kw)
        return fits["res"]
    monkeypatch.setattr(pipeline, "develop", develop_once)
    seen = []
    real_ci = metrics.bootstrap_ci

    def spy(*a, **kw):
        seen.append(real_ci(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(metrics, "bootstrap_ci", spy)
    base = ["--device", "cpu", "--rows", "100", "--features", "12", "--data-dir", str(tmp_path)]

    def run(tag, *extra):
        assert main(base + ["--json", f"{tag}.json", "--plots", tag] + list(extra)) == 0
        return capsys.readouterr().out, json.loads(open(f"{tag}.json").read().splitlines()[-1])
    plain, j_plain = run("hf")
    (tmp_path / "hf_roc.png").unlink(missing_ok=True)
    (tmp_path / "hf_roc.svg").unlink(missing_ok=True)
    zero, j_zero = run("hf", "--bootstrap", "0")
    assert plain == zero and not seen
    assert set(j_plain) == set(j_zero) and "bootstrap" not in j_plain
    out, j = run("hf", "--bootstrap", "64", "--bootstrap-seed", "11")
    assert len(seen) == 1 and j["bootstrap"]["n_boot"] == 64 and j["bootstrap"]["seed"] == 11
    assert set(j) == set(j_plain) | {"bootstrap"}
    ci = seen[0]
    lines = out.splitlines()
    k = lines.index(next(ln for ln in lines if ln.startswith("AUROC = ") and "CI" not in ln))
    assert [ln for i, ln in enumerate(lines) if i not in (k + 1, k + 2)] == plain.splitlines()
    cell = lambda key: f"{ci[key]['point']:.4f} (95% CI {ci[key]['lo']:.4f}–{ci[key]['hi']:.4f})"  # noqa: E731
    assert lines[k + 1] == f"AUROC = {cell('auroc')}   AP = {cell('average_precision')}"
    assert lines[k + 2] == "   ".join(f"{m} = {cell(m)}" for m in ("precision", "recall", "specificity", "accuracy"))
    assert any((tmp_path / f"hf_roc.{e}").exists() for e in ("png", "svg"))
    # --bootstrap alone (no figures) still gathers the held-out rows
    only, _ = run("nf", "--no-plots", "--bootstrap", "64", "--bootstrap-seed", "11")
    assert lines[k + 1] in only and "plots:" not in only
