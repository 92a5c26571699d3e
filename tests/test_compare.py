"""Paired bootstrap comparison on the host: the torch mirror (``ops.bootstrap_compare`` on host
tensors) against the independent oracle ``reference.compare_oracle`` and, column by column, against
``reference.bootstrap_metrics``; the algebra of paired columns; that the draws really are paired
(bootstrap se of ΔAUROC against DeLong's); ``metrics.delong_test`` against ``reference.delong_oracle``;
five wrong variants of the mirror that the oracle must reject; validation, ``metrics.compare_ci`` and
the training CLI's ``--compare``.

Bounds against the oracle (longdouble, so its own error is negligible):
* the integers ``a2``, ``pn``, ``conf``, ``reclass`` are equal and ``auroc`` is bit-equal to
  ``float(longdouble(A2) / (2·P·N))``;
* ``|ap − oracle| ≤ 4·n·2^-53``, the bound of ``test_bootstrap.py`` (same formula, same terms);
* ``|sums − oracle| ≤ (ceil(n/1024) + 22)·2^-53·Σc·|term|``: see :func:`sums_budget`.
"""
import functools
import json
import math

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.ops import api
from hfens.ops import reference as ref
from hfens.utils import metrics

U = 2.0 ** -53
B_SMALL = 6
SMALL = [(n, strat) for n in (2, 7, 40) for strat in (False, True)]


def sums_budget(n, sums):
    """The fold of ``sums`` adds a thread's ``chunk = ceil(n/1024)`` terms in sequence, then 6 levels of
    the wave's xor tree, then the 16 wave partials in order: chunk + 22 additions at most on the path
    of any term, each with relative error ≤ 2^-53 of a partial sum that is at most Σc·|term|.  The
    first addition of the chunk and of the wave sequence is to zero and exact, which leaves two of the
    22 for the roundings of the term itself: one for c·p; for c·(p − y)² the subtraction is exact
    whenever y = 0 or p ≥ ½ (Sterbenz), which leaves the square and the product by c, the worst case
    (an event with p < ½) being two more.  To first order the error is therefore at most
    (chunk + 22)·2^-53·Σc·|term|, a bound that is reached only if every rounding errs the same way.
    The scores of these tests are non-negative, so Σc·|term| is the sum itself, taken here from the
    reference side."""
    chunk = -(-n // 1024)
    return (chunk + 22) * U * np.abs(np.asarray(sums, dtype=np.float64))


def make_scores(n, M, seed=0, ties=True):
    """Labels with both classes (n ≥ 2) and M score columns in [0, 1]; ``ties``: rounded to one decimal
    (so rows sit exactly at the 0.5 threshold and in tie groups)."""
    rng = np.random.default_rng(100 * n + M + seed)
    y = (rng.random(n) < 0.4).astype(np.int64)
    y[0], y[-1] = 1, 0
    S = np.clip(0.3 * y[None, :] + 0.7 * rng.random((M, n)), 0.0, 1.0)
    return y, (np.round(S, 1) if ties else S)


@functools.lru_cache(maxsize=None)
def small_case(n, strat):
    y, S = make_scores(n, 3)
    return y, S, ref.compare_oracle(y, S, B_SMALL, seed=7, stratified=strat)


def run_mirror(y, S, B, **kw):
    return ops.bootstrap_compare(torch.as_tensor(y), torch.as_tensor(S), B, **kw)


def assert_matches_oracle(got, want, n):
    g = {k: v.cpu().numpy() for k, v in zip(ref.CompareBootstrap._fields, got)}
    for k in ("a2", "pn", "conf", "reclass"):
        assert g[k].dtype == np.int64 and np.array_equal(g[k], want[k]), k
    assert g["auroc"].dtype == g["ap"].dtype == g["sums"].dtype == np.float64
    nan = np.isnan(want["auroc"])
    assert np.array_equal(np.isnan(g["auroc"]), nan) and np.array_equal(np.isnan(g["ap"]), nan)
    ok = ~nan
    assert np.array_equal(g["auroc"][ok], want["auroc"][ok].astype(np.float64))
    if ok.any():
        dap = float(np.abs(g["ap"][ok] - want["ap"][ok]).max())
        print(f"max|dap| {dap / U:.3g} u")
        assert dap <= 4 * n * U
    ds = np.abs(g["sums"] - want["sums"]).astype(np.float64)
    bud = sums_budget(n, want["sums"])
    print(f"max|dsums| {ds.max() / U:.3g} u, largest share of the budget {np.max(ds / np.maximum(bud, 1e-300)):.3g}")
    assert (ds <= bud).all()


@pytest.mark.parametrize("n,strat", SMALL)
def test_mirror_matches_oracle(n, strat):
    y, S, want = small_case(n, strat)
    assert_matches_oracle(run_mirror(y, S, B_SMALL, seed=7, stratified=strat), want, n)


@pytest.mark.parametrize("n,strat", SMALL + [(1500, False)])
def test_columns_match_bootstrap_metrics(n, strat):
    y, S = make_scores(n, 3)
    got = run_mirror(y, S, B_SMALL, seed=7, stratified=strat)
    for m in range(3):
        auroc, ap, a2, pn, conf, _ = ref.bootstrap_metrics(torch.as_tensor(y), torch.as_tensor(S[m]), B_SMALL, seed=7,
                                                           stratified=strat)
        assert torch.equal(a2, got.a2[:, m]) and torch.equal(pn, got.pn) and torch.equal(conf, got.conf[:, m])
        assert torch.equal(ap.view(torch.int64), got.ap[:, m].view(torch.int64))
        assert torch.equal(auroc.view(torch.int64), got.auroc[:, m].view(torch.int64))
    assert int(got.reclass[:, 0].abs().sum()) == 0


def test_identical_and_negated_columns():
    y, S = make_scores(40, 2)
    got = run_mirror(y, np.stack([S[0], S[0], -S[0]]), 16, seed=1, threshold=0.5)
    assert torch.equal(got.a2[:, 0], got.a2[:, 1]) and int(got.reclass[:, 1].abs().sum()) == 0
    assert torch.equal(got.ap[:, 0].view(torch.int64), got.ap[:, 1].view(torch.int64))
    assert torch.equal(got.sums[:, 0].view(torch.int64), got.sums[:, 1].view(torch.int64))
    assert torch.equal(got.conf[:, 0], got.conf[:, 1])
    P, N = got.pn[:, 0], got.pn[:, 1]
    assert torch.equal(got.a2[:, 2], 2 * P * N - got.a2[:, 0])
    ci = metrics.compare_ci(y, {"a": S[0], "b": S[0].copy()}, "a", n_boot=16)
    for k in metrics.COMPARE_STATS:
        v = ci["comparisons"]["b"][k]
        assert v["point"] == 0.0 and v["lo"] == 0.0 and v["hi"] == 0.0 and v["se"] == 0.0 and v["p"] == 1.0


def test_single_column_and_replicate_ranges():
    y, S = make_scores(65, 3, ties=False)
    one = run_mirror(y, S[:1], 8, seed=5)
    whole = run_mirror(y, S, 8, seed=5)
    assert one.auroc.shape == (8, 1) and one.reclass.shape == (8, 1, 4) and one.sums.shape == (8, 1, 3)
    for k in ("auroc", "ap", "a2", "conf", "sums"):
        assert torch.equal(getattr(one, k)[:, 0], getattr(whole, k)[:, 0])
    parts = [run_mirror(y, S, 8, seed=5, b0=a, b1=b) for a, b in ((0, 1), (1, 5), (5, 5), (5, 8))]
    for k, w in enumerate(whole):
        cat = torch.cat([p[k] for p in parts])
        assert cat.shape == w.shape and torch.equal(cat.view(torch.int64), w.view(torch.int64))
    assert not torch.equal(run_mirror(y, S, 8, seed=6).a2, whole.a2)


def paired_fixture():
    rng = np.random.default_rng(0)
    n = 400
    y = (rng.random(n) < 0.3).astype(np.int64)
    shared = rng.standard_normal(n)
    a = 1.2 * y + shared + 0.3 * rng.standard_normal(n)
    b = 1.0 * y + shared + 0.3 * rng.standard_normal(n)
    return y, 1 / (1 + np.exp(-(a - 0.6))), 1 / (1 + np.exp(-(b - 0.5)))


def test_draws_are_paired():
    """Two models that share most of their noise: the se of their AUROC difference is far below what
    independent resamples would give, and DeLong's analytic se says how far.  Measured on this fixture
    (n = 400, B = 2000, seed 2020): bootstrap se of ΔAUROC 0.011978, DeLong se 0.012041 (ratio 0.995),
    unpaired sqrt(se_a² + se_b²) = 3.10 × the DeLong se."""
    y, pa, pb = paired_fixture()
    assert np.corrcoef(pa, pb)[0, 1] >= 0.8
    ci = metrics.compare_ci(y, {"a": pa, "b": pb}, "a", n_boot=2000, seed=2020)
    assert all(0.7 <= v <= 0.85 for v in ci["auroc"].values())
    c = ci["comparisons"]["b"]
    se_boot, se_delong = c["delta_auroc"]["se"], c["delong"]["se"]
    unpaired = math.hypot(metrics.bootstrap_ci(y, pa, n_boot=2000)["auroc"]["se"],
                          metrics.bootstrap_ci(y, pb, n_boot=2000)["auroc"]["se"])
    print(f"bootstrap se {se_boot:.6f}  DeLong se {se_delong:.6f}  unpaired {unpaired:.6f}")
    assert unpaired >= 1.5 * se_delong
    assert abs(se_boot - se_delong) <= 0.15 * se_delong


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", [30, 1000])
def test_delong_matches_oracle(n, ties):
    y, S = make_scores(n, 2, seed=3, ties=ties)
    got, want = metrics.delong_test(y, S[0], S[1]), ref.delong_oracle(y, S[0], S[1])
    for k in ("auc_a", "auc_b", "delta", "se"):
        assert abs(got[k] - float(want[k])) <= 1e-12, k
    assert got["auc_a"] == pytest.approx(metrics.roc_auc(y, S[0]), abs=1e-12)
    assert got["z"] == got["delta"] / got["se"]
    assert got["p"] == pytest.approx(math.erfc(abs(got["z"]) / math.sqrt(2)))
    assert set(got) == {"auc_a", "auc_b", "delta", "se", "z", "p"} and all(type(v) is float for v in got.values())


def test_delong_equal_columns():
    import warnings
    y, S = make_scores(50, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = metrics.delong_test(y, S[0], S[0].copy())
    assert got["se"] == 0.0 and got["p"] == 1.0 and got["delta"] == 0.0 and got["z"] == 0.0


# ---- wrong variants of the mirror: each must fail the comparison the true mirror passes -----------

def _fields(**kw):
    return ref.CompareBootstrap(*(kw[k] for k in ref.CompareBootstrap._fields))


def variant_unpaired(y, S, B, **kw):
    """Column m drawn with its own seed."""
    seed = kw.pop("seed")
    per = [run_mirror(y, np.stack([S[0], S[m]]), B, seed=seed + m, **kw) for m in range(S.shape[0])]
    d = {k: torch.stack([getattr(p, k)[:, 1] for p in per], 1) for k in ("auroc", "ap", "a2", "conf", "reclass", "sums")}
    return _fields(pn=per[0].pn, **d)


def variant_nri_swapped(y, S, B, **kw):
    r = run_mirror(y, S, B, **kw)
    return _fields(**dict(zip(ref.CompareBootstrap._fields, r), reclass=r.reclass[:, :, [1, 0, 3, 2]]))


def variant_ge_threshold(y, S, B, **kw):
    """score ≥ threshold: s > the next double below the threshold."""
    return run_mirror(y, S, B, threshold=float(np.nextafter(0.5, -np.inf)), **kw)


def variant_ties_broken(y, S, B, **kw):
    """Tied rows ordered by row instead of grouped (no score crosses the threshold: they only fall)."""
    return run_mirror(y, S - 1e-9 * np.arange(S.shape[1])[None, :], B, **kw)


def variant_original_totals(y, S, B, **kw):
    r = run_mirror(y, S, B, **kw)
    P = int(y.sum())
    auroc = r.a2.to(torch.float64) / float(2 * P * (len(y) - P))
    return _fields(**dict(zip(ref.CompareBootstrap._fields, r), auroc=torch.where(torch.isnan(r.auroc), r.auroc, auroc)))


VARIANTS = {"unpaired": variant_unpaired, "nri_swapped": variant_nri_swapped, "ge_threshold": variant_ge_threshold,
            "ties_broken": variant_ties_broken, "original_totals": variant_original_totals}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_oracle_rejects_wrong_variant(name):
    n, strat = 40, False
    y, S, want = small_case(n, strat)
    assert (S == 0.5).any() and len(np.unique(S[0])) < n       # rows at the threshold, and tie groups
    assert_matches_oracle(run_mirror(y, S, B_SMALL, seed=7, stratified=strat), want, n)
    with pytest.raises(AssertionError):
        assert_matches_oracle(VARIANTS[name](y, S, B_SMALL, seed=7, stratified=strat), want, n)


def test_validation_errors(monkeypatch):
    y = torch.tensor([0, 1, 1, 0])
    S = torch.tensor([[0.1, 0.9, 0.4, 0.3], [0.2, 0.8, 0.5, 0.1]], dtype=torch.float64)

    def rejects(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            ops.bootstrap_compare(*a, **kw)
    rejects(r"y .* must be \[n\]", y[:3], S, 8)
    rejects(r"y .* must be \[n\]", y, S[0], 8)
    rejects("M = 9", y, S[:1].expand(9, 4), 8)
    rejects("M = 0", y, S[:0], 8)
    rejects("n = 0", y[:0], S[:, :0], 8)
    rejects("finite", y, torch.tensor([[0.1, float("nan"), 0.4, 0.3]]), 8)
    rejects("finite", y, torch.tensor([[0.1, float("inf"), 0.4, 0.3]]), 8)
    rejects("finite", y, torch.tensor([[1, 0, 1, 0]]), 8)
    rejects("y must hold labels", torch.tensor([0, 2, 1, 0]), S, 8)
    rejects("n_boot", y, S, 0)
    rejects("n_boot", y, S, (1 << 24) + 1)
    rejects("b0:b1", y, S, 8, b0=5, b1=4)
    rejects("b0:b1", y, S, 8, b1=9)
    rejects("threshold", y, S, 8, threshold=float("nan"))
    rejects("stratified", torch.ones(4, dtype=torch.int64), S, 8, stratified=True)
    rejects("stratified", torch.zeros(4, dtype=torch.int64), S, 8, stratified=True)
    rejects("same device", y.to("meta"), S, 8)
    assert api.COMPARE_MAX_MODELS == 8 and api.COMPARE_LDS_ROWS * 12 + 1664 <= 160 * 1024
    monkeypatch.setattr(api, "BOOTSTRAP_MAX_N", 3)
    rejects("n <= 3", y, S, 8)


def test_compare_ci_contents():
    y, pa, pb = paired_fixture()
    pc = np.clip(pb + 0.2 * np.random.default_rng(1).standard_normal(len(y)), -0.2, 1.2)   # leaves [0, 1]
    ci = metrics.compare_ci(y, {"lg": pb, "stack": pa, "raw": pc}, "stack", n_boot=64, seed=3, threshold=0.4)
    assert json.loads(json.dumps(ci)) == ci
    assert ci["models"] == ["stack", "lg", "raw"] and ci["reference"] == "stack" and ci["n_boot"] == 64
    assert ci["n_degenerate"] == 0 and ci["threshold"] == 0.4 and set(ci["comparisons"]) == {"lg", "raw"}
    assert ci["auroc"]["stack"] == metrics.roc_auc(y, pa)
    c = ci["comparisons"]["lg"]
    assert set(c) == set(metrics.COMPARE_STATS) | {"delong"}
    for k in metrics.COMPARE_STATS:
        assert set(c[k]) == {"point", "lo", "hi", "se", "p"} and all(type(v) is float for v in c[k].values())
        assert c[k]["lo"] <= c[k]["hi"] and 0.0 < c[k]["p"] <= 1.0
    assert c["delta_auroc"]["point"] == metrics.roc_auc(y, pa) - metrics.roc_auc(y, pb)
    assert c["delta_ap"]["point"] == metrics.average_precision(y, pa) - metrics.average_precision(y, pb)
    assert c["nri"]["point"] == pytest.approx(c["nri_event"]["point"] + c["nri_nonevent"]["point"])
    # the definitions, on the original sample
    ev, ha, hb = y == 1, pa > 0.4, pb > 0.4
    nri = ((ha & ~hb & ev).sum() - (~ha & hb & ev).sum()) / ev.sum() \
        + ((~ha & hb & ~ev).sum() - (ha & ~hb & ~ev).sum()) / (~ev).sum()
    assert c["nri"]["point"] == pytest.approx(nri, abs=1e-15)
    idi = (pa[ev].mean() - pa[~ev].mean()) - (pb[ev].mean() - pb[~ev].mean())
    assert c["idi"]["point"] == pytest.approx(idi, abs=1e-14)
    assert c["delta_brier"]["point"] == pytest.approx(((pa - y) ** 2).mean() - ((pb - y) ** 2).mean(), abs=1e-14)
    assert c["delta_sensitivity"]["point"] == pytest.approx((ha & ev).sum() / ev.sum() - (hb & ev).sum() / ev.sum())
    assert c["delong"] == metrics.delong_test(y, pa, pb)
    # the p-value rule on the replicates themselves
    r = ops.bootstrap_compare(torch.as_tensor(y), torch.as_tensor(np.stack([pa, pb])), 64, seed=3, threshold=0.4)
    d = ((r.a2[:, 0] - r.a2[:, 1]).double() / (2 * r.pn[:, 0] * r.pn[:, 1]).double()).numpy()
    assert c["delta_auroc"]["p"] == min(1.0, 2 * min((d <= 0).sum() + 1, (d >= 0).sum() + 1) / 65)
    assert c["delta_auroc"]["se"] == float(np.std(d, ddof=1))
    raw = ci["comparisons"]["raw"]
    assert raw["idi"] is None and raw["delta_brier"] is None and raw["nri"] is not None
    zero = metrics.compare_ci(y, {"stack": pa, "lg": pb}, "stack", n_boot=0, threshold=0.4)
    z = zero["comparisons"]["lg"]
    assert z["delta_auroc"]["point"] == c["delta_auroc"]["point"] and z["delong"] == c["delong"]
    assert all(math.isnan(z["nri"][f]) for f in ("lo", "hi", "se", "p")) and zero["n_boot"] == 0
    with pytest.raises(ValueError, match="reference"):
        metrics.compare_ci(y, {"a": pa}, "stack")


def test_save_compare_plot(tmp_path):
    y, pa, pb = paired_fixture()
    path = metrics.save_compare_plot(y, {"stack": pa, "lg": pb}, str(tmp_path / "c"))
    assert path.startswith(str(tmp_path / "c_compare.")) and len(open(path, "rb").read()) > 200


def test_cli_compare_cpu(tmp_path, monkeypatch, capsys):
    from hfens import pipeline
    from hfens.cli.train_ensemble_public import main
    monkeypatch.chdir(tmp_path)
    real_develop, fits, kwargs = pipeline.develop, {}, []

    def develop_once(*a, **kw):       # the runs fit the same model: fit it once, with the base columns
        kwargs.append(kw.get("keep_bases", False))
        if "res" not in fits:
            fits["res"] = real_develop(*a, **dict(kw, keep_bases=True))
        return fits["res"]
    monkeypatch.setattr(pipeline, "develop", develop_once)
    seen = []
    real_ci = metrics.compare_ci

    def spy(*a, **kw):
        seen.append(real_ci(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(metrics, "compare_ci", spy)
    base = ["--device", "cpu", "--rows", "100", "--features", "12", "--data-dir", str(tmp_path)]

    def run(tag, *extra):
        assert main(base + ["--json", f"{tag}.json", "--plots", tag] + list(extra)) == 0
        return capsys.readouterr().out, json.loads(open(f"{tag}.json").read().splitlines()[-1])
    plain, j_plain = run("hf")
    assert not seen and kwargs == [False] and "compare" not in j_plain
    assert not any((tmp_path / f"hf_compare.{e}").exists() for e in ("png", "svg"))
    res = fits["res"]
    assert res.bases_sel.shape == (100, 3) and res.bases_sel.dtype == torch.float64
    assert res.base_names == [name for name, _ in res.model.estimators] and len(res.base_names) == 3
    out, j = run("hf", "--compare", "--bootstrap", "64", "--bootstrap-seed", "11")
    assert kwargs[-1] is True and len(seen) == 1
    assert set(j) == set(j_plain) | {"bootstrap", "compare"}
    assert j["compare"]["n_boot"] == 64 and j["compare"]["seed"] == 11 and j["compare"] == json.loads(json.dumps(seen[0]))
    lines = out.splitlines()
    mine = [ln for ln in lines if ln.startswith("stack vs ")]
    assert [ln.split(":")[0] for ln in mine] == [f"stack vs {name}" for name in res.base_names]
    for ln, name in zip(mine, res.base_names):
        c = seen[0]["comparisons"][name]
        d = c["delta_auroc"]
        assert (f"ΔAUROC {d['point']:+.4f} (95% CI {d['lo']:+.4f}–{d['hi']:+.4f}, p = {d['p']:.4f}, "
                f"DeLong p = {c['delong']['p']:.4f})") in ln
        assert all(s in ln for s in ("ΔAP ", "NRI ", "IDI "))
    assert any((tmp_path / f"hf_compare.{e}").exists() for e in ("png", "svg"))
    boot, j_boot = run("hb", "--bootstrap", "64", "--bootstrap-seed", "11")
    rest = [ln for ln in lines if not ln.startswith(("stack vs ", "comparison plot:"))]
    assert [ln.replace("'hf_", "'hb_") for ln in rest] == boot.splitlines() and set(j_boot) == set(j) - {"compare"}
    # --bootstrap 0: points and DeLong only; no figure with --no-plots
    only, j0 = run("nf", "--no-plots", "--compare")
    assert "DeLong p = " in only and "CI" not in only and "comparison plot:" not in only
    assert j0["compare"]["n_boot"] == 0 and set(j0) == set(j_plain) | {"compare"}
    assert [ln for ln in only.splitlines() if not ln.startswith("stack vs ")] == \
        [ln for ln in plain.splitlines() if not ln.startswith("plots:")]
