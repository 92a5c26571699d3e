"""Permutation importance on the host: the permutation law, the rank mirror against brute force and
scikit-learn, the whole op on the shipped checkpoint against explicit numpy loops, the validation
errors and the CLI."""
import functools
import json
import math

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score, brier_score_loss, roc_auc_score

from hfens import ops
from hfens.explain import PermutationImportance, StackExplainer
from hfens.io.checkpoint import load_checkpoint
from hfens.io.synth import MODEL_FEATURES, make_hf_cohort
from hfens.ops import api
from hfens.ops import reference as ref


# ---- the law ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000])
def test_sources_are_permutations(n):
    src = ops.permutation_sources(n, 0, 5, seed=7)
    assert src.shape == (5, n) and src.dtype == torch.int32
    assert torch.equal(torch.sort(src.long(), 1).values, torch.arange(n).expand(5, n))


def test_sources_follow_the_written_law():
    """Python integers, key by key; ties cannot be told from a stable sort of (key, i) pairs."""
    n, seed = 37, 99
    src = ops.permutation_sources(n, 3, 5, seed=seed)
    for row, r in zip(src.tolist(), (3, 4)):
        keys = [ref._splitmix64_py(seed ^ ref._splitmix64_py((r << 25) ^ i)) >> 1 for i in range(n)]
        assert row == sorted(range(n), key=lambda i: (keys[i], i))


def test_sources_do_not_depend_on_the_range_or_chunk():
    whole = ops.permutation_sources(65, 0, 9, seed=3)
    assert torch.equal(torch.cat([ops.permutation_sources(65, 0, 4, seed=3),
                                  ops.permutation_sources(65, 4, 9, seed=3)]), whole)
    assert torch.equal(ref.permutation_sources(65, 0, 9, 3, chunk_elems=130), whole)
    assert not torch.equal(ops.permutation_sources(65, 0, 9, seed=4), whole)


def test_sources_are_uniform_at_n4():
    """All 24 permutations of 4 rows over 24,000 repeats, each count inside a 5σ binomial band."""
    R = 24000
    src = ops.permutation_sources(4, 0, R, seed=2020).long()
    code = src[:, 0] * 64 + src[:, 1] * 16 + src[:, 2] * 4 + src[:, 3]
    counts = torch.unique(code, return_counts=True)[1]
    sigma = math.sqrt(R * (1 / 24) * (23 / 24))
    assert counts.numel() == 24
    assert float((counts.double() - R / 24).abs().max()) <= 5 * sigma


# ---- the rank mirror -------------------------------------------------------------------------------
def _tied_scores(M=5, n=300, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(n, generator=g) < 0.3).to(torch.float64)
    s = torch.round(torch.rand(M, n, generator=g, dtype=torch.float64) * 0.6 + 0.3 * y[None, :], decimals=2)
    return y, s


def test_rank_mirror_against_brute_force_and_sklearn():
    y, s = _tied_scores()
    out = ops.rank_metrics(y, s)
    assert out.a2.dtype == torch.int64 and out._fields == ("a2", "auroc", "ap", "brier")
    yn = y.numpy()
    P, N = int(yn.sum()), int((1 - yn).sum())
    for m in range(s.shape[0]):
        sm = s[m].numpy()
        pos, neg = sm[yn == 1], sm[yn == 0]
        a2 = int((2 * (pos[:, None] > neg[None, :]) + (pos[:, None] == neg[None, :])).sum())
        assert int(out.a2[m]) == a2
        assert float(out.auroc[m]) == a2 / (2 * P * N)
        assert abs(float(out.ap[m]) - average_precision_score(yn, sm)) <= 1e-12
        assert abs(float(out.brier[m]) - brier_score_loss(yn, sm)) <= 1e-12
    f32 = ops.rank_metrics(y, s.to(torch.float32))          # ties are those of the scores' own dtype
    assert torch.equal(f32.a2, out.a2) and torch.equal(f32.auroc, out.auroc)


# ---- end to end on the shipped checkpoint ------------------------------------------------------------
N_ROWS, R_SMALL, R_LARGE = 400, 8, 200


@functools.lru_cache(maxsize=None)
def _cohort(ckpt_path):
    X, y, _ = make_hf_cohort(N_ROWS, 17, seed=5, nan_frac=0.0)
    pk = load_checkpoint(ckpt_path)._packed_stack(torch.device("cpu"))
    return torch.as_tensor(X), torch.as_tensor(y), pk


@functools.lru_cache(maxsize=None)
def _importance(ckpt_path, R):
    X, y, pk = _cohort(ckpt_path)
    return ops.permutation_importance(X, y, pk, R, seed=2020)


def _loop(X, y, pk, perms):
    """AUROC importances [F, R] by an explicit loop: every hybrid matrix materialised in numpy, scored by
    ref.stack_infer, ranked by scikit-learn."""
    Xn = X.to(torch.float32).double().numpy()
    yn = y.numpy()
    base = roc_auc_score(yn, ref.stack_infer(torch.as_tensor(Xn), pk).numpy())
    out = np.empty((Xn.shape[1], len(perms)))
    for r, p in enumerate(perms):
        hs = []
        for k in range(Xn.shape[1]):
            h = Xn.copy()
            h[:, k] = Xn[p, k]
            hs.append(h)
        s = ref.stack_infer(torch.as_tensor(np.concatenate(hs)), pk).numpy().reshape(Xn.shape[1], -1)
        out[:, r] = [base - roc_auc_score(yn, s[k]) for k in range(Xn.shape[1])]
    return out


def test_mirror_equals_the_explicit_loop(ckpt_path):
    X, y, pk = _cohort(ckpt_path)
    base, imp = _importance(ckpt_path, R_SMALL)
    assert set(base) == set(imp) == {"auroc", "ap", "brier"}
    assert all(v.shape == (17, R_SMALL) and v.dtype == torch.float64 for v in imp.values())
    src = ops.permutation_sources(N_ROWS, 0, R_SMALL, seed=2020).numpy()
    want = _loop(X, y, pk, list(src))
    d = float(np.abs(imp["auroc"].numpy() - want).max())
    print(f"max|d importance| {d:.3g}")
    assert d <= 1e-12
    p = ref.stack_infer(X.to(torch.float32).double(), pk).numpy()
    assert abs(base["auroc"] - roc_auc_score(y.numpy(), p)) <= 1e-12
    assert abs(base["ap"] - average_precision_score(y.numpy(), p)) <= 1e-12
    assert abs(base["brier"] - brier_score_loss(y.numpy(), p)) <= 1e-12
    # repeats do not depend on the range, the columns asked for, or the workspace chunking
    part = ops.permutation_importance(X, y, pk, R_SMALL, seed=2020, features=[16, 2], r0=3, r1=6)[1]
    for m in imp:
        assert torch.equal(part[m], imp[m][[16, 2], 3:6])


def test_mean_importance_agrees_with_numpy_shuffles(ckpt_path):
    X, y, pk = _cohort(ckpt_path)
    mine = _importance(ckpt_path, R_LARGE)[1]["auroc"].numpy()
    rng = np.random.default_rng(12345)
    theirs = _loop(X, y, pk, [rng.permutation(N_ROWS) for _ in range(R_LARGE)])
    se = np.sqrt(mine.var(1, ddof=1) / R_LARGE + theirs.var(1, ddof=1) / R_LARGE)
    z = np.abs(mine.mean(1) - theirs.mean(1))
    print("|dmean| / se:", np.round(z / np.maximum(se, 1e-300), 2))
    assert np.all(z <= 4 * se)
    assert mine.mean(1).max() > 0.0


def test_explainer_result(ckpt_path):
    X, y, pk = _cohort(ckpt_path)
    ex = StackExplainer(load_checkpoint(ckpt_path), X[:16], device="cpu", feature_names=list(MODEL_FEATURES))
    pi = ex.permutation_importance(X, y, n_repeats=R_SMALL, seed=2020)
    base, imp = _importance(ckpt_path, R_SMALL)
    assert isinstance(pi, PermutationImportance) and pi.names == list(MODEL_FEATURES) and pi.baseline == base
    assert all(torch.equal(pi.importances[m], imp[m]) for m in imp)
    v = imp["auroc"].numpy()
    assert np.allclose(pi.mean("auroc").numpy(), v.mean(1), rtol=0, atol=1e-15)
    assert np.allclose(pi.std("ap").numpy(), imp["ap"].numpy().std(1, ddof=1), rtol=0, atol=1e-15)
    lo, hi = pi.interval("auroc", 0.95)
    assert np.allclose(lo.numpy(), np.percentile(v, 2.5, axis=1), rtol=0, atol=1e-15)
    assert np.allclose(hi.numpy(), np.percentile(v, 97.5, axis=1), rtol=0, atol=1e-15)
    top = pi.top(3)
    assert [k for k, _, _ in top] == sorted(range(17), key=lambda k: (-v.mean(1)[k], k))[:3]
    assert top[0][1] == MODEL_FEATURES[top[0][0]]
    one = PermutationImportance(pi.names, base, {m: t[:, :1] for m, t in imp.items()})
    assert bool(torch.isnan(one.std("auroc")).all())


# ---- validation ----------------------------------------------------------------------------------------
def _small(ckpt_path):
    X, y, pk = _cohort(ckpt_path)
    return X[:20].clone(), y[:20].clone(), pk


def test_rejects_bad_shapes(ckpt_path):
    X, y, pk = _small(ckpt_path)
    with pytest.raises(ValueError, match=r"permutation_importance: x .* must be \[n, F\]"):
        ops.permutation_importance(X[0], y, pk, 4)
    with pytest.raises(ValueError, match=r"permutation_importance: y .* must be \[n\]"):
        ops.permutation_importance(X, y[:-1], pk, 4)
    with pytest.raises(ValueError, match="x is empty"):
        ops.permutation_importance(X[:0], y[:0], pk, 4)
    with pytest.raises(ValueError, match=r"rank_metrics: y .* must be \[n\] and scores"):
        ops.rank_metrics(y, X[:, 0])
    with pytest.raises(ValueError, match=r"stack_permute_scores: src .* must be \[R, 20\]"):
        ops.stack_permute_scores(X, pk, torch.zeros(2, 19, dtype=torch.int32), [0])
    with pytest.raises(ValueError, match=r"src must hold row indices in \[0, 20\)"):
        ops.stack_permute_scores(X, pk, torch.full((1, 20), 20, dtype=torch.int32), [0])
    with pytest.raises(ValueError, match=r"features must be a non-empty list of columns in \[-1, 17\)"):
        ops.stack_permute_scores(X, pk, torch.zeros(1, 20, dtype=torch.int32), [17])
    with pytest.raises(ValueError, match=r"features must be a non-empty list of columns in \[0, 17\)"):
        ops.permutation_importance(X, y, pk, 4, features=[-1])


def test_rejects_devices_that_disagree(ckpt_path):
    X, y, pk = _small(ckpt_path)
    with pytest.raises(ValueError, match="x and the packed model must be on the same device"):
        ops.permutation_importance(X.to("meta"), y, pk, 4)
    with pytest.raises(ValueError, match="x and src must be on the same device"):
        ops.stack_permute_scores(X, pk, torch.zeros(1, 20, dtype=torch.int32, device="meta"), [0])


def test_rejects_a_feature_count_that_is_not_the_models(ckpt_path):
    X, y, pk = _small(ckpt_path)
    with pytest.raises(ValueError, match="x has 16 features, model has 17"):
        ops.permutation_importance(X[:, :16], y, pk, 4)


def test_rejects_rows_that_are_not_finite(ckpt_path):
    X, y, pk = _small(ckpt_path)
    X[3, 4] = float("nan")
    with pytest.raises(ValueError, match="x must be finite floating point"):
        ops.permutation_importance(X, y, pk, 4)
    with pytest.raises(ValueError, match="scores must be finite floating point"):
        ops.rank_metrics(y, X[:, :1].t().contiguous().expand(1, 20) * float("inf"))


def test_rejects_labels_outside_0_1(ckpt_path):
    X, y, pk = _small(ckpt_path)
    y[0] = 2.0
    with pytest.raises(ValueError, match="y must hold labels 0 and 1 only"):
        ops.permutation_importance(X, y, pk, 4)


def test_rejects_a_single_class(ckpt_path):
    X, y, pk = _small(ckpt_path)
    with pytest.raises(ValueError, match="both classes must be present in y"):
        ops.permutation_importance(X, torch.zeros_like(y), pk, 4)
    with pytest.raises(ValueError, match="both classes must be present in y"):
        ops.rank_metrics(torch.ones(1), torch.rand(3, 1))


def test_rejects_what_exceeds_the_limits(ckpt_path, monkeypatch):
    X, y, pk = _small(ckpt_path)
    with pytest.raises(ValueError, match=rf"n_repeats = {(1 << 24) + 1} outside 1\.\.{1 << 24}"):
        ops.permutation_importance(X, y, pk, (1 << 24) + 1)
    with pytest.raises(ValueError, match="n_repeats = 0 outside"):
        ops.permutation_importance(X, y, pk, 0)
    with pytest.raises(ValueError, match=r"r0:r1 = 3:2 is not a range within 0\.\.n_repeats = 4"):
        ops.permutation_importance(X, y, pk, 4, r0=3, r1=2)
    with pytest.raises(ValueError, match=rf"n = {(1 << 25) + 1} outside 1\.\.{1 << 25}"):
        ops.permutation_sources((1 << 25) + 1, 0, 1)
    with pytest.raises(ValueError, match="r0:r1 = 0:16777217 is not a range"):
        ops.permutation_sources(4, 0, (1 << 24) + 1)
    monkeypatch.setattr(api, "PERMUTE_MAX_N", 19)
    with pytest.raises(ValueError, match="x has 20 rows, the limit is n <= 19"):
        ops.permutation_importance(X, y, pk, 4)
    with pytest.raises(ValueError, match="y has 20 rows, the limit is n <= 19"):
        ops.rank_metrics(y, torch.rand(2, 20))


# ---- the CLI ---------------------------------------------------------------------------------------------
def test_cli_importance_cpu(tmp_path, monkeypatch, capsys):
    from hfens import pipeline
    from hfens.cli.train_ensemble_public import main
    monkeypatch.chdir(tmp_path)
    real_develop, fits, kwargs = pipeline.develop, {}, []

    def develop_once(*a, **kw):       # the runs fit the same model: fit it once, with the held-out columns
        kwargs.append(dict(kw))
        if "res" not in fits:
            fits["res"] = real_develop(*a, **dict(kw, keep_heldout=True))
        return fits["res"]
    monkeypatch.setattr(pipeline, "develop", develop_once)
    base = ["--device", "cpu", "--rows", "100", "--features", "12", "--data-dir", str(tmp_path)]

    def run(tag, *extra):
        assert main(base + ["--json", f"{tag}.json", "--plots", tag] + list(extra)) == 0
        return capsys.readouterr().out, json.loads(open(f"{tag}.json").read().splitlines()[-1])
    plain, j_plain = run("hf")
    assert "keep_heldout" not in kwargs[0] and "importance" not in j_plain
    assert not any((tmp_path / f"hf_importance.{e}").exists() for e in ("png", "svg"))
    out, j = run("hf", "--importance", "5", "--importance-seed", "11")
    assert kwargs[-1]["keep_heldout"] is True
    res = fits["res"]
    F = len(res.selected_names)
    assert res.X_sel.shape == (100, F) and res.X_sel.dtype == torch.float64
    lines = out.splitlines()
    mine = [ln for ln in lines if "ΔAUROC " in ln]
    shown = [ln.split("ΔAUROC")[0].strip() for ln in mine]
    assert len(mine) == F and sorted(shown) == sorted(res.selected_names)
    # without the flag: the same bytes
    assert [ln for ln in lines if ln not in mine and not ln.startswith(("permutation importance (", "importance plot:"))] \
        == plain.splitlines()
    assert set(j) == set(j_plain) | {"importance"} and {k: j[k] for k in j_plain} == j_plain
    rec = j["importance"]
    assert rec["n_repeats"] == 5 and rec["seed"] == 11 and len(rec["variables"]) == F
    y = torch.as_tensor(make_dev_select_labels())
    want_base, want = ops.permutation_importance(res.X_sel, y, res.model._packed_stack(torch.device("cpu")), 5, seed=11)
    assert rec["baseline"] == want_base
    means = want["auroc"].mean(1).tolist()
    order = sorted(range(F), key=lambda k: (-means[k], k))
    assert [v["name"] for v in rec["variables"]] == [res.selected_names[k] for k in order]
    assert shown == [res.selected_names[k] for k in order]
    for v, k in zip(rec["variables"], order):
        assert v["auroc"]["mean"] == means[k] and v["brier"] == want["brier"].mean(1).tolist()[k]
    assert f"ΔAUROC {means[order[0]]:+.4f} ± " in mine[0] and "ΔAP " in mine[0] and "ΔBrier " in mine[0]
    assert any((tmp_path / f"hf_importance.{e}").exists() for e in ("png", "svg"))
    # the default number of repeats; no figure with --no-plots
    only, j30 = run("nf", "--no-plots", "--importance")
    assert j30["importance"]["n_repeats"] == 30 and j30["importance"]["seed"] == 2020
    assert "importance plot:" not in only


def make_dev_select_labels():
    from hfens.io.synth import make_dev_select
    return make_dev_select(100, 12, seed=2020)[3]
