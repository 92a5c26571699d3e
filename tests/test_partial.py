"""Partial dependence, what-if curves and Friedman's H²: the f64 mirror, the validation,
StackExplainer's additions and the CLI (host)."""
import numpy as np
import pytest
import torch

from hfens import ops
from hfens.cli.predict_hf import PATIENT_PARAMS, main
from hfens.explain import StackExplainer
from hfens.io.checkpoint import load_checkpoint
from hfens.io.synth import make_hf_cohort
from hfens.ops import api
from hfens.ops import reference as ref
from hfens.ops.packing import PackedStack, pack_forest, pack_svs, stump_table


def _random_pstack(F, m, T, depth, device, seed=0, stumps=True, unused=None):
    """A random stack; ``unused`` names a column that no part of the stack reads."""
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
            while feat[t, i] == unused:
                feat[t, i] = rng.integers(0, F)
            thr[t, i] = rng.normal()
            left[t, i], right[t, i] = 2 * i + 1, 2 * i + 2
    tabs = [torch.as_tensor(a) for a in (feat, thr, left, right, val)]
    f = pack_forest(*tabs, device)
    inv_scale = 0.5 + torch.rand(F, generator=g)
    lr_w = 0.3 * torch.randn(F, generator=g)
    if unused is not None:
        inv_scale[unused] = 0.0
        lr_w[unused] = 0.0
    return PackedStack(
        F=F, sv=pack_svs(sv, coef, device),
        mean=(0.1 * torch.randn(F, generator=g)).to(device), inv_scale=inv_scale.to(device),
        gamma=0.5 / F, svc_b=0.2, probA=-1.7, probB=0.1, forest=f,
        stumps=stump_table(*tabs, -0.4, 0.1, F, device) if stumps else None, gb_init=-0.4, gb_lr=0.1,
        lr_w=lr_w.to(device), lr_b=-0.2,
        meta_w=(1.9, 0.5, 2.7), meta_b=-2.0)


class _Model:
    """The two things StackExplainer asks of a fitted stack."""

    def __init__(self, pk):
        self.pk = pk

    def to(self, device):
        return self

    def _packed_stack(self, device):
        return self.pk


def _cells(F, C, seed):
    """``C`` cells that cycle through no, one (either slot) and two substitutions."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.full((C, 2), -1, dtype=torch.int64)
    value = torch.randn(C, 2, generator=g, dtype=torch.float64)
    for c in range(C):
        kind = c % 4
        k1 = int(torch.randint(0, F, (1,), generator=g))
        k2 = (k1 + 1 + int(torch.randint(0, F - 1, (1,), generator=g))) % F
        if kind in (1, 3):
            feat[c, 0] = k1
        if kind in (2, 3):
            feat[c, 1] = k2
    return feat, value


def test_mirror_matches_plain_loop():
    F, n = 5, 3
    pk = _random_pstack(F, 64, 10, 2, "cpu", seed=5, stumps=False)
    x = torch.randn(n, F, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    feat, value = _cells(F, 9, seed=2)
    assert {tuple((feat[c] >= 0).tolist()) for c in range(9)} == {(False, False), (True, False), (False, True),
                                                                  (True, True)}
    pd, ice = ops.stack_partial(x, pk, feat, value, return_ice=True)     # host tensors run the mirror
    assert pd.dtype == ice.dtype == torch.float64 and pd.shape == (9,) and ice.shape == (n, 9)
    x32, v32 = x.float().double(), value.float().double()                # the inputs are rounded to f32 first
    want = torch.empty(n, 9, dtype=torch.float64)
    for c in range(9):
        for r in range(n):
            h = x32[r].clone()
            for s in range(2):
                if feat[c, s] >= 0:
                    h[feat[c, s]] = v32[c, s]
            want[r, c] = ref.stack_infer(h[None, :], pk)[0]
    assert float((ice - want).abs().max()) <= 1e-12
    assert float((pd - want.mean(0)).abs().max()) <= 1e-12
    assert torch.equal(ops.stack_partial(x, pk, feat, value), pd)
    assert torch.equal(ref.stack_partial(x, pk, feat, value, chunk=1), pd)   # chunking changes nothing


def test_pd_is_the_sequential_mean_of_ice():
    F, n = 5, 37
    pk = _random_pstack(F, 64, 10, 1, "cpu", seed=5)
    x = torch.randn(n, F, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    feat, value = _cells(F, 6, seed=4)
    pd, ice = ops.stack_partial(x, pk, feat, value, return_ice=True)
    for c in range(6):
        s = 0.0
        for r in range(n):
            s += float(ice[r, c])
        assert float(pd[c]) == s / n


def test_validation(monkeypatch):
    F = 4
    pk = _random_pstack(F, 32, 3, 1, "cpu")
    x = torch.zeros(2, F)
    feat, value = torch.tensor([[0, -1]]), torch.zeros(1, 2)
    ops.stack_partial(x, pk, feat, value)
    bad = [
        (torch.zeros(0, F), feat, value),                                  # n < 1
        (x, torch.zeros(0, 2, dtype=torch.int64), torch.zeros(0, 2)),      # C < 1
        (torch.zeros(F), feat, value),                                     # x not [n, F]
        (x, torch.tensor([0, -1]), value),                                 # feat not [C, 2]
        (x, torch.tensor([[0, -1, -1]]), torch.zeros(1, 3)),               # three slots
        (x, feat, torch.zeros(2, 2)),                                      # value shape differs from feat's
        (x, feat.double(), value),                                         # feat not integer
        (torch.zeros(2, F + 1), feat, value),                              # feature mismatch with pk
        (x, torch.tensor([[F, -1]]), value),                               # index >= F
        (x, torch.tensor([[-2, 0]]), value),                               # index < -1
        (x, torch.tensor([[1, 1]]), value),                                # k1 == k2 >= 0
        (x, feat, torch.tensor([[float("nan"), 0.0]])),                    # non-finite value in a used slot
        (x, torch.tensor([[-1, 2]]), torch.tensor([[0.0, float("inf")]])),
        (x, feat, torch.tensor([[1e39, 0.0]], dtype=torch.float64)),       # finite in f64, not as the kernel sees it
    ]
    for args in bad:
        with pytest.raises(ValueError, match="stack_partial"):
            ops.stack_partial(args[0], pk, args[1], args[2])
    # a non-finite value in an unused slot is not read
    ops.stack_partial(x, pk, feat, torch.tensor([[0.5, float("nan")]]))
    ops.stack_partial(x, pk, torch.tensor([[-1, -1]]), torch.tensor([[float("inf"), float("nan")]]))
    with pytest.raises(ValueError, match="stack_partial"):                 # tensors on different devices
        ops.stack_partial(x, pk, feat.to("meta"), value)
    with pytest.raises(ValueError, match="stack_partial"):
        ops.stack_partial(x.to("meta"), pk, feat.to("meta"), value.to("meta"))   # not the model's device
    assert api.PARTIAL_ICE_BYTES == 1 << 30
    monkeypatch.setattr(api, "PARTIAL_ICE_BYTES", 4 * 2 * 1 - 1)
    ops.stack_partial(x, pk, feat, value)                                  # pd alone is not limited
    with pytest.raises(ValueError, match="stack_partial"):
        ops.stack_partial(x, pk, feat, value, return_ice=True)
    monkeypatch.setattr(api, "PARTIAL_ICE_BYTES", 4 * 2 * 1)
    ops.stack_partial(x, pk, feat, value, return_ice=True)


def _explainer(F=5, B=40, seed=7, unused=None, discrete=(1,)):
    pk = _random_pstack(F, 32, 6, 1, "cpu", seed=seed, unused=unused)
    g = torch.Generator().manual_seed(seed)
    bg = torch.randn(B, F, generator=g, dtype=torch.float64)
    for k in discrete:
        bg[:, k] = torch.randint(0, 3, (B,), generator=g).double()
    return StackExplainer(_Model(pk), bg, device="cpu"), pk, bg


def test_grid_rule():
    ex, pk, bg = _explainer()
    g = ex.grid(1, points=8)                       # three distinct values: returned as they are
    assert g.dtype == torch.float64 and g.tolist() == [0.0, 1.0, 2.0]
    assert ex.grid(1, points=3).tolist() == [0.0, 1.0, 2.0]
    col = bg[:, 0].float().double()
    g = ex.grid(0, points=8)                       # continuous: 8 equally spaced values, end points included
    assert g.shape == (8,) and float(g[0]) == float(col.min()) and float(g[-1]) == float(col.max())
    assert torch.equal(g, g.float().double())
    step = (float(col.max()) - float(col.min())) / 7
    assert float((g - (float(col.min()) + step * torch.arange(8, dtype=torch.float64))).abs().max()) <= 1e-6
    g2 = ex.grid(1, points=2)                      # more distinct values than points: min..max in 2 steps
    assert g2.tolist() == [0.0, 2.0]
    assert ex.grid(0, points=40).shape[0] == torch.unique(col).numel()


def test_partial_dependence_curves():
    ex, pk, bg = _explainer()
    res = ex.partial_dependence([0, 1], points=6)
    assert res.features == [0, 1] and res.feature_names == ["x0", "x1"]
    assert [g.numel() for g in res.grids] == [6, 3] and [c.numel() for c in res.pd] == [6, 3]
    for k, grid, curve in zip(res.features, res.grids, res.pd):
        for v, got in zip(grid.tolist(), curve.tolist()):
            h = bg.float().double().clone()
            h[:, k] = v
            assert abs(got - float(ref.stack_infer(h, pk).mean())) <= 1e-12
    everything = ex.partial_dependence(points=6)
    assert everything.features == list(range(5)) and torch.equal(everything.pd[1], res.pd[1])


def test_what_if_passes_through_the_patient():
    ex, pk, bg = _explainer()
    x = torch.randn(2, 5, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    w = ex.what_if(x, points=6)
    x32 = x.float().double()
    pred = ref.stack_infer(x32, pk)
    assert torch.equal(w.x, x32) and float((w.prediction - pred).abs().max()) <= 1e-12
    for i, k in enumerate(w.features):
        grid = w.grids[i]
        assert torch.equal(grid, torch.unique(grid)) and w.risk[i].shape == (2, grid.numel())
        assert w.cohort[i].shape == grid.shape
        for p in range(2):
            at = (grid == x32[p, k]).nonzero().flatten()
            assert at.numel() == 1                                       # the patient's own value is on the grid
            assert abs(float(w.risk[i][p, at[0]]) - float(pred[p])) <= 1e-12
        # the cohort's PD on the same grid
        h = bg.float().double().clone()
        h[:, k] = grid[0]
        assert abs(float(w.cohort[i][0]) - float(ref.stack_infer(h, pk).mean())) <= 1e-12
    one = ex.what_if(x[0], features=["x3"], points=6)                   # a single patient, a named variable
    assert one.features == [3] and one.risk[0].shape[0] == 1


def _h2_oracle(pk, X, j, k):
    """Friedman's H² of (j, k) written from the formula, every PD value computed on its own."""
    n = X.shape[0]

    def pd(cols, vals):
        h = X.clone()
        for c, v in zip(cols, vals):
            h[:, c] = v
        return float(ref.stack_infer(h, pk).mean())

    a = torch.tensor([pd((j, k), (X[i, j], X[i, k])) for i in range(n)], dtype=torch.float64)
    b = torch.tensor([pd((j,), (X[i, j],)) for i in range(n)], dtype=torch.float64)
    c = torch.tensor([pd((k,), (X[i, k],)) for i in range(n)], dtype=torch.float64)
    a, b, c = a - a.mean(), b - b.mean(), c - c.mean()
    den = float((a * a).sum())
    return float(((a - b - c) ** 2).sum()) / den if den > 0 else 0.0


def test_interaction_strength_matches_brute_force():
    F, n = 4, 6
    ex, pk, bg = _explainer(F=F, B=n, seed=9, discrete=(1, 2))       # repeated values: cells collapse
    X = bg.float().double()
    it = ex.interaction_strength()
    assert it.n_rows == n and it.h2.shape == (F, F) and it.h2.dtype == torch.float64
    assert torch.equal(it.h2, it.h2.t()) and float(it.h2.diagonal().abs().max()) == 0.0
    for j in range(F):
        for k in range(j + 1, F):
            want = _h2_oracle(pk, X, j, k)
            assert abs(float(it.h2[j, k]) - want) <= 1e-10, (j, k)
    assert float(it.h2.max()) > 1e-4                                  # the stack is not additive
    # max_rows truncates to the first rows; an explicit cohort and explicit pairs
    cut = ex.interaction_strength(torch.cat([X, X + 1.0]), pairs=[(0, 3)], max_rows=n)
    assert cut.n_rows == n and float(cut.h2[0, 3]) == float(it.h2[0, 3]) and float(cut.h2[0, 1]) == 0.0
    top = it.top(2)
    assert len(top) == 2 and top[0][2] >= top[1][2] and top[0][2] == float(it.h2.max())


def test_unused_variable_has_no_interaction_and_a_flat_curve():
    F, j = 5, 2
    ex, pk, bg = _explainer(F=F, B=12, seed=13, unused=j)
    it = ex.interaction_strength()
    assert float(it.h2[j].max()) <= 1e-12 and float(it.h2[:, j].max()) <= 1e-12
    others = it.h2[[k for k in range(F) if k != j]][:, [k for k in range(F) if k != j]]
    assert float(others.max()) > 1e-4
    curve = ex.partial_dependence([j], points=8).pd[0]
    assert curve.numel() == 8 and float(curve.max() - curve.min()) <= 1e-12
    assert float(torch.stack([c.max() - c.min() for c in ex.partial_dependence(points=8).pd]).max()) > 1e-4


def _what_if_lines(out):
    rows = []
    for ln in out.splitlines():
        if ln.startswith("  ") and "  now " in ln:
            name = ln[2:26].rstrip()
            tok = ln[26:].split()
            # {current} now {p} % lowest {lo} % at {v_lo} highest {hi} % at {v_hi}
            assert tok[1] == "now" and tok[4] == "lowest" and tok[7] == "at" and tok[9] == "highest" and tok[12] == "at"
            rows.append((name, float(tok[0]), tok[2], float(tok[5]), float(tok[8]), float(tok[10]), float(tok[13])))
    return rows


def check_what_if_output(plain, out):
    """The assertions on ``--what-if``'s block that hold on every device."""
    assert out.startswith(plain) and "27.09 %" in plain
    rows = _what_if_lines(out[len(plain):])
    assert len(rows) == 17 and {r[0] for r in rows} == set(PATIENT_PARAMS)
    spans = [r[5] - r[3] for r in rows]
    assert all(a >= b - 0.0101 for a, b in zip(spans, spans[1:]))      # sorted by highest − lowest (2 decimals printed)
    assert spans[0] > 1.0
    for name, cur, now, lo, v_lo, hi, v_hi in rows:
        assert cur == float(PATIENT_PARAMS[name]) and now == "27.09"
        assert lo <= float(now) <= hi
    return rows


def test_cli_what_if_and_interactions(ckpt_path, tmp_path, capsys):
    bg = make_hf_cohort(4, 17, seed=0, nan_frac=0.0)[0]
    bgcsv, wicsv = tmp_path / "bg.csv", tmp_path / "wi.csv"
    np.savetxt(bgcsv, bg, delimiter=",")
    assert main([]) == 0
    plain = capsys.readouterr().out
    assert main(["--what-if", "--background", str(bgcsv), "--what-if-csv", str(wicsv)]) == 0
    out = capsys.readouterr().out
    check_what_if_output(plain, out)
    assert len(out[len(plain):].splitlines()) == 18                   # a heading, then the variables
    # the CSV: one line per grid point, variables in model order
    ex = StackExplainer(load_checkpoint(ckpt_path), bg, device="cpu", feature_names=list(PATIENT_PARAMS))
    w = ex.what_if([[float(v) for v in PATIENT_PARAMS.values()]])
    lines = wicsv.read_text().splitlines()
    assert lines[0] == "variable,value,risk,cohort_mean_risk"
    want = [f"{name},{v:.9g},{r:.9g},{c:.9g}"
            for i, name in enumerate(PATIENT_PARAMS)
            for v, r, c in zip(w.grids[i].tolist(), w.risk[i][0].tolist(), w.cohort[i].tolist())]
    assert lines[1:] == want and len(want) == sum(g.numel() for g in w.grids)
    # chosen variables only; after --explain's block when both are given
    assert main(["--what-if", "Max_Wall_Thick,Gender", "--background", str(bgcsv)]) == 0
    out = capsys.readouterr().out
    assert [r[0] for r in _what_if_lines(out)] == ["Max_Wall_Thick", "Gender"]
    assert main(["--what-if", "No_Such_Variable", "--background", str(bgcsv)]) == 2
    cap = capsys.readouterr()
    assert cap.out == "" and "unknown clinical variable 'No_Such_Variable'" in cap.err
    # --interactions over the background, and over a --csv cohort
    assert main(["--interactions", "3", "--background", str(bgcsv)]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain)
    rest = out[len(plain):].splitlines()
    assert "4 patients" in rest[0] and len(rest) == 4
    it = ex.interaction_strength()
    for ln, (j, k, h) in zip(rest[1:], it.top(3)):
        assert ln == f"  {ex.feature_names[j]:<24s} {ex.feature_names[k]:<24s} {h:.4f}"
    cohort = tmp_path / "cohort.csv"
    np.savetxt(cohort, make_hf_cohort(3, 17, seed=1, nan_frac=0.0)[0], delimiter=",")
    assert main(["--csv", str(cohort)]) == 0
    scored = capsys.readouterr().out
    assert main(["--csv", str(cohort), "--interactions", "--background", str(bgcsv)]) == 0
    out = capsys.readouterr().out
    assert out.startswith(scored)
    rest = out[len(scored):].splitlines()
    assert "3 patients" in rest[0] and len(rest) == 11                # N defaults to 10
