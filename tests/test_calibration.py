"""Bootstrap of the calibration and decision-curve statistics on the host: the torch mirror
(``ops.bootstrap_calibration`` on host tensors) against the independent per-replicate oracle
``reference.calibration_oracle`` and against sklearn on a materialised resample, the replicates
without a fit, the joint resamples with ``ops.bootstrap_metrics``, replicate ranges,
``metrics.calibration_ci``, the figures and the training CLI's ``--calibration``.

Bounds against the oracle (longdouble sums and a longdouble Newton run to a step of 1e-16, so its
own error is negligible):
* the integers ``pn``, ``bin_n``, ``bin_pos``, ``dc`` and ``status`` are equal;
* ``|brier|``, ``|sum_p|/n`` and ``|bin_sum_p|/n`` ≤ ``4·n·2^-53``: non-negative terms that sum to at
  most 1 after the division, the bound the project uses for AP;
* ``|coef − oracle| ≤ 1e-10·max(1, |a|, |b|)`` wherever the oracle fitted: the tolerance the solve
  promises (it stops on an undamped Newton step of 1e-10; the step after it is quadratically smaller).
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
from test_bootstrap import degenerate_case, make_case

U = 2.0 ** -53
NS = (1, 2, 3, 63, 64, 65)
KINDS = ("continuous", "decimal", "uniform")
B_EDGE = 16
FIELDS = ref.CalibrationBootstrap._fields
INTS = ("pn", "bin_n", "bin_pos", "dc", "status")


def make_scores(n, kind, seed=0):
    """Labels (int64, about 35 % positives, both classes when n ≥ 2) and risks in [0, 1] (f64):
    ``continuous`` follows the label and is clipped to [0, 1]; ``decimal`` is the same rounded to one
    decimal (ties, scores on bin and threshold edges, exact 0 and 1); ``uniform`` ignores the label."""
    rng = np.random.default_rng(77 * n + seed)
    y = (rng.random(n) < 0.35).astype(np.int64)
    if n >= 2:
        y[0], y[-1] = 1, 0
    if kind == "uniform":
        return y, rng.random(n)
    p = np.clip(0.3 + 0.25 * y + 0.25 * rng.standard_normal(n), 0.0, 1.0)
    return y, (np.round(p, 1) if kind == "decimal" else p)


def case_inputs(case):
    n, kind, strat = case
    if kind.startswith("bootstrap-"):
        return make_case(n, kind.split("-", 1)[1])
    return make_scores(n, kind)


def edge_cases():
    """(n, kind, stratified): this file's three kinds and ``test_bootstrap.make_case``'s distinct and
    one-decimal scores.  Its constant scores never admit a fit and have a test of their own."""
    return [(n, kind, strat) for n in NS for kind in KINDS + ("bootstrap-noties", "bootstrap-decimal")
            for strat in (False, True) if not (strat and n < 2)]


@functools.lru_cache(maxsize=None)
def oracle_of(case, B=B_EDGE, seed=7):
    y, p = case_inputs(case)
    return ref.calibration_oracle(y, p, B, seed=seed, stratified=case[2])


def run_op(case, device="cpu", B=B_EDGE, seed=7, dtype=torch.float64, **kw):
    y, p = case_inputs(case)
    return ops.bootstrap_calibration(torch.as_tensor(y).to(device), torch.as_tensor(p).to(device, dtype), B, seed=seed,
                                     stratified=case[2], **kw)


def assert_matches_oracle(got, want, n):
    """Returns the worst coefficient error relative to its tolerance's scale ``max(1, |a|, |b|)``."""
    got = {k: v.cpu().numpy() for k, v in zip(FIELDS, got)}
    for k in INTS + ("iters",):
        assert got[k].dtype == np.int64
    for k in INTS:
        assert np.array_equal(got[k], want[k]), k
    for k in ("brier", "sum_p", "bin_sum_p", "coef"):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape
    db = float(np.abs(got["brier"] - want["brier"]).max())
    dsp = float(np.abs(got["sum_p"] - want["sum_p"]).max()) / n
    dbs = float(np.abs(got["bin_sum_p"] - want["bin_sum_p"]).max()) / n
    print(f"max|dbrier| {db / U:.3g} u  max|dsum_p|/n {dsp / U:.3g} u  max|dbin_sum_p|/n {dbs / U:.3g} u")
    assert db <= 4 * n * U and dsp <= 4 * n * U and dbs <= 4 * n * U
    ok = want["status"] == 0
    assert np.isnan(got["coef"][~ok]).all() and (got["iters"][~ok] == 0).all()
    worst = 0.0
    if ok.any():
        c, w = got["coef"][ok], want["coef"][ok]
        assert not np.isnan(c).any() and (got["iters"][ok] >= 1).all()
        worst = float((np.abs(c - w).max(1) / np.maximum(1.0, np.abs(w).max(1))).max())
        print(f"max coef error / max(1, |a|, |b|) = {worst:.3g}  max iters {int(got['iters'].max())}")
        assert worst <= 1e-10
    return worst


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_mirror_matches_oracle(case):
    assert_matches_oracle(run_op(case), oracle_of(case), case[0])


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_status_cap(case):
    """Against the oracle alone: the iteration cap is never hit, and from n = 63 on at least half of
    the replicates are fitted, so the coefficient bound above is not vacuous."""
    st = oracle_of(case)["status"]
    assert not (st == 3).any()
    if case[0] >= 63:
        assert 2 * int((st == 0).sum()) >= st.size


@pytest.mark.parametrize("n,strat", [(n, s) for n in NS for s in (False, True) if not (s and n < 2)])
def test_constant_scores_never_fit(n, strat):
    """One score for every row: the classes touch at a tie only, so no replicate has an MLE."""
    y, p = make_case(n, "equal")
    want = ref.calibration_oracle(y, p, B_EDGE, seed=7, stratified=strat)
    assert np.isin(want["status"], (1, 2)).all()
    assert_matches_oracle(ops.bootstrap_calibration(torch.as_tensor(y), torch.as_tensor(p), B_EDGE, seed=7,
                                                    stratified=strat), want, n)


def test_separable_and_degenerate_replicates():
    y, p = degenerate_case()                    # one positive, the top score: separable whenever it is drawn
    want = ref.calibration_oracle(y, p, 64, seed=0)
    assert (int((want["status"] == 1).sum()), int((want["status"] == 2).sum())) == (30, 34)
    got = ops.bootstrap_calibration(torch.as_tensor(y), torch.as_tensor(p), 64, seed=0)
    assert_matches_oracle(got, want, 8)
    # the same rows with the positive in the middle of the scores: some replicates overlap and are fitted
    y2 = np.roll(y, 4)
    want2 = ref.calibration_oracle(y2, p, 64, seed=0)
    counts = [int((want2["status"] == k).sum()) for k in range(4)]
    assert counts == [27, 15, 22, 0]
    got2 = ops.bootstrap_calibration(torch.as_tensor(y2), torch.as_tensor(p), 64, seed=0)
    assert_matches_oracle(got2, want2, 8)
    ci = metrics.calibration_ci(y2, p, n_boot=64, seed=0)
    assert (ci["n_degenerate"], ci["n_separable"], ci["n_unconverged"]) == (15, 22, 0)
    slope = got2.coef[:, 1].numpy()
    keep = slope[~np.isnan(slope)]
    assert keep.size == 27 and ci["slope"]["lo"] == float(np.quantile(keep, 0.025))
    assert not np.isnan(ci["brier"]["lo"])


def test_quasi_separation_is_status_2():
    """Positives and negatives meet at one tied score and nowhere else: the likelihood has no maximiser."""
    y = np.array([1, 1, 1, 0, 0, 0], dtype=np.int64)
    p = np.array([0.9, 0.8, 0.5, 0.5, 0.2, 0.1])
    for strat in (False, True):
        want = ref.calibration_oracle(y, p, 32, seed=1, stratified=strat)
        got = ops.bootstrap_calibration(torch.as_tensor(y), torch.as_tensor(p), 32, seed=1, stratified=strat)
        assert_matches_oracle(got, want, 6)
        assert np.isin(want["status"], (1, 2)).all() and (want["status"] == 2).any()
    assert (ops.bootstrap_calibration(torch.as_tensor(y), torch.as_tensor(p), 8, stratified=True).status == 2).all()
    pt = ref.calibration_point(y, p)
    assert pt["status"] == 2 and all(np.isnan(pt["coef"]))
    # one negative above the tie: the classes overlap and the fit exists
    assert ref.calibration_point(np.array([1, 0, 1, 1, 0, 0]), p)["status"] == 0


def sk_case(n=200):
    rng = np.random.default_rng(0)
    y = (rng.random(n) < 0.3).astype(np.int64)
    p = np.clip(0.3 * y + 0.7 * rng.random(n), 0.0, 1.0)
    return y, p


@pytest.mark.parametrize("strat", [False, True])
def test_joint_resamples_with_bootstrap_metrics(strat):
    y, p = sk_case()
    yt, pt = torch.as_tensor(y), torch.as_tensor(p)
    assert torch.equal(ops.bootstrap_calibration(yt, pt, 40, seed=5, stratified=strat).pn,
                       ops.bootstrap_metrics(yt, pt, 40, seed=5, stratified=strat)[3])


def test_replicate_ranges_and_seed():
    y, p = sk_case()
    yt, pt = torch.as_tensor(y), torch.as_tensor(p)
    whole = ops.bootstrap_calibration(yt, pt, 40, seed=5)
    parts = [ops.bootstrap_calibration(yt, pt, 40, seed=5, b0=a, b1=b) for a, b in ((0, 1), (1, 17), (17, 17), (17, 40))]
    for k, w in enumerate(whole):
        cat = torch.cat([q[k] for q in parts])
        assert cat.shape == w.shape and torch.equal(cat.view(torch.int64), w.view(torch.int64)), FIELDS[k]
    assert whole.bin_n is whole[3] and whole.coef.shape == (40, 2) and whole.dc.shape == (40, 99, 2)
    assert not torch.equal(ops.bootstrap_calibration(yt, pt, 40, seed=6).bin_n, whole.bin_n)


def test_sklearn_on_one_resample():
    sk = pytest.importorskip("sklearn")
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import brier_score_loss
    del sk
    y, p = sk_case()
    got = ops.bootstrap_calibration(torch.as_tensor(y), torch.as_tensor(p), 4, seed=0)
    b = 3
    idx = ref.bootstrap_resample(y, b, 0)
    yy, pp = y[idx], p[idx]
    assert int(got.status[b]) == 0
    assert abs(brier_score_loss(yy, pp) - float(got.brier[b])) <= 1e-12
    pc = np.clip(pp, 1e-12, 1 - 1e-12)
    lr = LogisticRegression(penalty=None, tol=1e-10, max_iter=1000).fit((np.log(pc) - np.log1p(-pc))[:, None], yy)
    d = max(abs(float(lr.intercept_[0]) - float(got.coef[b, 0])), abs(float(lr.coef_[0, 0]) - float(got.coef[b, 1])))
    print(f"sklearn lbfgs against the op: {d:.3g}")
    assert d <= 1e-5


def test_calibration_ci():
    y, p = sk_case()
    a = metrics.calibration_ci(y, p, n_boot=64)
    b = metrics.calibration_ci(torch.as_tensor(y), torch.as_tensor(p), n_boot=64)
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    assert a["brier"]["lo"] <= a["brier"]["point"] <= a["brier"]["hi"] and a["brier"]["se"] > 0
    assert a["brier"]["point"] == pytest.approx(float(np.mean((p - y) ** 2)), abs=1e-15)
    assert a["oe_ratio"]["point"] == pytest.approx(y.sum() / p.sum(), rel=1e-14)
    assert (a["n_degenerate"], a["n_separable"], a["n_unconverged"], a["n_boot"]) == (0, 0, 0, 64)
    rel, dcv = a["reliability"], a["decision_curve"]
    assert sum(rel["count"]) == 200 and len(rel["obs"]) == 10
    assert all(l <= h for l, h, c in zip(rel["obs_lo"], rel["obs_hi"], rel["count"]) if c)
    assert len(dcv["thresholds"]) == 99 and dcv["thresholds"][9] == 10 / 100
    assert all(l <= h for l, h in zip(dcv["net_benefit_lo"], dcv["net_benefit_hi"]))
    g = 19                                      # t = 0.2, treat p ≥ t
    tp, fp = int(((p >= 0.2) & (y == 1)).sum()), int(((p >= 0.2) & (y == 0)).sum())
    assert dcv["net_benefit"][g] == pytest.approx(tp / 200 - fp / 200 * 0.25, abs=1e-15)
    assert dcv["net_benefit_all"][g] == pytest.approx(y.mean() - (1 - y.mean()) * 0.25, abs=1e-15)
    c = metrics.calibration_ci(y, p, n_boot=64, stratified=True)
    assert c["brier"]["point"] == a["brier"]["point"] and c["brier"]["lo"] != a["brier"]["lo"]
    zero = metrics.calibration_ci(y, p, n_boot=0)
    for k in ("brier", "oe_ratio", "intercept", "slope", "ece"):
        assert zero[k]["point"] == a[k]["point"] and all(np.isnan(zero[k][f]) for f in ("lo", "hi", "se"))
    assert zero["reliability"]["obs"] == rel["obs"] and np.isnan(zero["decision_curve"]["net_benefit_lo"]).all()


def test_calibration_ci_sees_miscalibration():
    """The true risk is p⁴ (prevalence 0.2).  Reported as p⁴ the slope interval holds 1; reported as
    p², which understates how far the risks spread, the slope is above 1; reported as p⁸ it is below 1.
    (Squaring a calibrated risk r always gives a slope below 1, since d logit(r²)/d logit(r) =
    2/(1 + r) > 1: p² has a slope above 1 only against a truth that is more extreme than itself.)"""
    rng = np.random.default_rng(3)
    n = 2000
    p = rng.random(n)
    y = (rng.random(n) < p ** 4).astype(np.int64)
    good = metrics.calibration_ci(y, p ** 4, n_boot=64)
    assert good["slope"]["lo"] <= 1.0 <= good["slope"]["hi"]
    assert good["intercept"]["lo"] <= 0.0 <= good["intercept"]["hi"]
    bad = metrics.calibration_ci(y, p ** 2, n_boot=64)
    assert bad["slope"]["point"] > 1.0 and bad["slope"]["lo"] > 1.0
    assert bad["ece"]["point"] > good["ece"]["point"] and bad["brier"]["point"] > good["brier"]["point"]
    assert bad["oe_ratio"]["hi"] < 1.0          # mean p² = 1/3 against a prevalence of 0.2
    over = metrics.calibration_ci(y, p ** 8, n_boot=64)
    assert over["slope"]["hi"] < 1.0


def test_validation_errors():
    y = torch.tensor([0, 1, 1, 0])
    p = torch.tensor([0.1, 0.9, 0.4, 0.3], dtype=torch.float64)

    def rejects(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            ops.bootstrap_calibration(*a, **kw)
    rejects(r"\[0, 1\]", y, torch.tensor([0.1, 1.5, 0.4, 0.3]), 8)
    rejects(r"\[0, 1\]", y, torch.tensor([0.1, -0.01, 0.4, 0.3]), 8)
    rejects("finite", y, torch.tensor([0.1, float("nan"), 0.4, 0.3]), 8)
    rejects("bins", y, p, 8, bins=0)
    rejects("bins", y, p, 8, bins=65)
    rejects("thresholds", y, p, 8, thresholds=0)
    rejects("thresholds", y, p, 8, thresholds=4097)
    rejects("y .* and score", y[:3], p, 8)
    rejects("n_boot", y, p, 0)
    rejects("b0:b1", y, p, 8, b1=9)
    rejects("stratified", torch.ones(4, dtype=torch.int64), p, 8, stratified=True)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        metrics.calibration_ci(y, p * 2, n_boot=0)
    assert ops.bootstrap_calibration(y, p, 8, bins=64, thresholds=4096).dc.shape == (8, 4096, 2)
    assert api.CALIBRATION_LDS_ROWS >= 10_000 and "bootstrap_calibration" in api.__all__


def test_bin_and_threshold_edges():
    """0.3 is in [0.3, 0.4) and is treated at t = 0.3; 1.0 is in the last bin, 0.0 in the first."""
    y = np.array([1, 0, 1, 0], dtype=np.int64)
    p = np.array([0.3, 0.0, 1.0, 0.7])
    pt = ref.calibration_point(y, p, 10, 9)
    assert pt["bin_n"] == [1, 0, 0, 1, 0, 0, 0, 1, 0, 1]
    assert pt["bin_pos"] == [0, 0, 0, 1, 0, 0, 0, 0, 0, 1]
    assert pt["dc"][2] == [2, 1] and pt["dc"][3] == [1, 1] and pt["dc"][6] == [1, 1] and pt["dc"][7] == [1, 0]


def test_save_calibration_plots(tmp_path):
    y, p = sk_case()
    for tag, nb in (("b", 16), ("z", 0)):
        res = metrics.calibration_ci(y, p, n_boot=nb)
        cal, dec = metrics.save_calibration_plots(res, str(tmp_path / tag))
        assert cal.startswith(str(tmp_path / f"{tag}_calibration.")) and dec.startswith(str(tmp_path / f"{tag}_decision."))
        assert all(len(open(f, "rb").read()) > 500 for f in (cal, dec))
    svg = metrics._svg_plot(str(tmp_path / "s.svg"), [([0.0, 1.0], [0.0, float("nan")], "black", "", "c")],
                            ([0.0, 1.0], [0.0, 0.1], [0.2, 0.3]), ([0.5], [0.5]), "x", "y", (-0.1, 1.0))
    text = open(svg).read()
    assert "<polygon" in text and "<circle" in text and "nan" not in text


def test_cli_calibration_cpu(tmp_path, monkeypatch, capsys):
    from hfens import pipeline
    from hfens.cli.train_ensemble_public import main
    monkeypatch.chdir(tmp_path)
    real_develop, fits = pipeline.develop, {}

    def develop_once(*a, **kw):       # the runs fit the same model: fit it once
        if "res" not in fits:
            fits["res"] = real_develop(*a, **kw)
        return fits["res"]
    monkeypatch.setattr(pipeline, "develop", develop_once)
    seen = []
    real_ci = metrics.calibration_ci

    def spy(*a, **kw):
        seen.append((kw, real_ci(*a, **kw)))
        return seen[-1][1]
    monkeypatch.setattr(metrics, "calibration_ci", spy)
    base = ["--device", "cpu", "--rows", "100", "--features", "12", "--data-dir", str(tmp_path)]

    def run(tag, *extra):
        assert main(base + ["--json", f"{tag}.json", "--plots", tag] + list(extra)) == 0
        return capsys.readouterr().out, json.loads(open(f"{tag}.json").read().splitlines()[-1])
    plain, j_plain = run("hf")
    assert not seen and "calibration" not in j_plain
    assert not any((tmp_path / f"hf_calibration.{e}").exists() for e in ("png", "svg"))
    boot, j_boot = run("hf", "--bootstrap", "16")
    assert not seen and "calibration" not in j_boot
    out, j = run("hf", "--calibration", "--bootstrap", "16", "--bootstrap-seed", "11", "--stratified")
    assert len(seen) == 1 and set(j) == set(j_boot) | {"calibration"}
    kw, cal = seen[0]
    assert (kw["n_boot"], kw["seed"], kw["stratified"], kw["bins"], kw["thresholds"]) == (16, 11, True, 10, 99)
    assert j["calibration"]["n_boot"] == 16 and j["calibration"]["seed"] == j["bootstrap"]["seed"] == 11
    cell = lambda v: f"{v['point']:.4f} (95% CI {v['lo']:.4f}–{v['hi']:.4f})"  # noqa: E731
    line = "   ".join(f"{name} = {cell(cal[k])}" for name, k in (
        ("Brier", "brier"), ("O:E", "oe_ratio"), ("intercept", "intercept"), ("slope", "slope"), ("ECE", "ece")))
    lines = out.splitlines()
    assert line in lines
    nb = lines[lines.index(line) + 1]
    assert nb.startswith("net benefit   t = 0.10: ") and "t = 0.20: " in nb and "t = 0.50: " in nb
    assert nb.count("vs treat-all") == 3 and nb.count("95% CI") == 3
    assert any((tmp_path / f"hf_calibration.{e}").exists() for e in ("png", "svg"))
    assert any((tmp_path / f"hf_decision.{e}").exists() for e in ("png", "svg"))
    # without --bootstrap: points only; other bins and thresholds reach the op
    only, j_only = run("nf", "--no-plots", "--calibration", "--calibration-bins", "5", "--calibration-thresholds", "9")
    assert seen[1][0]["n_boot"] == 0 and "CI" not in only and "Brier = " in only and "calibration plots:" not in only
    assert len(j_only["calibration"]["reliability"]["obs"]) == 5
    assert j_only["calibration"]["decision_curve"]["thresholds"] == [g / 10 for g in range(1, 10)]
