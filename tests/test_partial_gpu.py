"""Partial dependence on the GPU: the fused ``stack_partial`` kernel against the host mirror, the
properties that need no mirror (pd = sequential mean of ice, determinism, grid and stream
independence), StackExplainer's additions and the CLI on ``cuda``.

Tolerances are the bounds the project already holds the same per-row arithmetic to:
``test_stack_infer_random`` keeps the kernel within 5e-6 of the f64 reference per row and
``test_stack_infer_checkpoint`` within 2e-6 on the shipped checkpoint; ice is such a row and pd a
mean of such rows."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.cli.predict_hf import PATIENT_PARAMS, main
from hfens.explain import StackExplainer
from hfens.io.checkpoint import load_checkpoint
from hfens.io.synth import make_hf_cohort
from hfens.ops import reference as ref
from hfens.ops.packing import PackedStack, pack_forest, pack_stack, pack_svs, stump_table

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


# (F, m, T, depth, stumps, n, C): the smallest shapes that reach each path of the kernel
SHAPES = [
    (5, 64, 10, 2, False, 3, 7),      # generic tree walk, odd F, a half-empty tile
    (5, 64, 10, 1, True, 100, 65),    # C crosses a tile by one; n not a power of two
    (11, 250, 30, 1, True, 2, 130),   # several tiles per workgroup (grid=1); waves beyond the work
    (8, 6000, 20, 1, True, 5, 3),     # SVs exceed LDS: restaging barriers inside the row loop, most waves idle
    (19, 32, 4, 1, True, 1, 64),      # F > 18: the f32 MFMA path with SVs resident
]


def _inputs(F, n, C):
    """Cohort and cells that cycle through no, one (either slot) and two substitutions, as f64."""
    g = torch.Generator().manual_seed(1000 * F + C)
    x = torch.randn(n, F, generator=g, dtype=torch.float64)
    value = torch.randn(C, 2, generator=g, dtype=torch.float64)
    k1 = torch.randint(0, F, (C,), generator=g)
    k2 = (k1 + 1 + torch.randint(0, F - 1, (C,), generator=g)) % F
    kind = torch.arange(C) % 4
    feat = torch.stack([torch.where((kind == 1) | (kind == 3), k1, torch.full_like(k1, -1)),
                        torch.where((kind == 2) | (kind == 3), k2, torch.full_like(k2, -1))], 1)
    return x, feat, value


@functools.lru_cache(maxsize=None)
def _mirror(shape):
    F, m, T, depth, stumps, n, C = shape
    x, feat, value = _inputs(F, n, C)
    return ref.stack_partial(x, _random_pstack(F, m, T, depth, "cpu", seed=F, stumps=stumps), feat, value,
                             return_ice=True)


def _gpu(shape, dev, dtype=torch.float64, **kw):
    F, m, T, depth, stumps, n, C = shape
    x, feat, value = _inputs(F, n, C)
    pk = _random_pstack(F, m, T, depth, dev, seed=F, stumps=stumps)
    return ops.stack_partial(x.to(dev, dtype), pk, feat.to(dev), value.to(dev, dtype), return_ice=True, **kw)


def _sequential_mean(ice):
    """f64 mean of every ice column on the host, summed in row order."""
    ice = ice.cpu()
    s = torch.zeros(ice.shape[1], dtype=torch.float64)
    for r in range(ice.shape[0]):
        s = s + ice[r].to(torch.float64)
    return s / float(ice.shape[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_random_stacks_match_mirror(dev, shape):
    F, m, T, depth, stumps, n, C = shape
    pd, ice = _gpu(shape, dev)
    wpd, wice = _mirror(shape)
    assert pd.dtype == torch.float64 and ice.dtype == torch.float32
    assert pd.shape == (C,) and ice.shape == (n, C)
    dpd = float((pd.cpu() - wpd).abs().max())
    dice = float((ice.cpu().double() - wice).abs().max())
    print(f"max|dpd| {dpd:.3g}  max|dice| {dice:.3g}")
    assert dpd <= 5e-6
    assert dice <= 5e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_pd_is_the_sequential_mean_of_ice(dev, shape):
    pd, ice = _gpu(shape, dev)
    assert torch.equal(pd.cpu(), _sequential_mean(ice))
    F, m, T, depth, stumps, n, C = shape
    x, feat, value = _inputs(F, n, C)
    pk = _random_pstack(F, m, T, depth, dev, seed=F, stumps=stumps)
    assert torch.equal(ops.stack_partial(x.to(dev), pk, feat.to(dev), value.to(dev)), pd)   # without ice


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]])
def test_f32_inputs_equal_f64_inputs(dev, shape):
    a = _gpu(shape, dev)
    b = _gpu(shape, dev, torch.float32)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_deterministic_and_grid_independent(dev, shape):
    a = _gpu(shape, dev)
    b = _gpu(shape, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for grid in (1, 3):
        c = _gpu(shape, dev, grid=grid)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_external_stream(dev):
    shape = SHAPES[2]
    want = _gpu(shape, dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = _gpu(shape, dev, stream=side.cuda_stream)
    side.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def ckpt_case(ckpt_path):
    """Default patient plus 3 cohort rows; the plain row, one cell per variable and a few pairs."""
    pk = pack_stack(load_checkpoint(ckpt_path), "cpu")
    x = torch.tensor([[float(v) for v in PATIENT_PARAMS.values()]], dtype=torch.float64)
    x = torch.cat([x, torch.as_tensor(make_hf_cohort(3, 17, seed=0, nan_frac=0.0)[0], dtype=torch.float64)])
    alt = torch.as_tensor(make_hf_cohort(1, 17, seed=5, nan_frac=0.0)[0], dtype=torch.float64)[0]
    feat = [[-1, -1]] + [[k, -1] for k in range(17)] + [[13, 16], [16, 13], [0, 13], [-1, 15], [6, 3]]
    feat = torch.tensor(feat)
    value = torch.stack([alt[feat[:, 0].clamp(min=0)], alt[feat[:, 1].clamp(min=0)]], 1)
    return x, feat, value, ref.stack_partial(x, pk, feat, value, return_ice=True)


def test_checkpoint_matches_mirror(dev, ckpt_path, ckpt_case):
    x, feat, value, (wpd, wice) = ckpt_case
    gpu = load_checkpoint(ckpt_path, device=dev)
    pd, ice = ops.stack_partial(x.to(dev), gpu._packed_stack(dev), feat.to(dev), value.to(dev), return_ice=True)
    dpd = float((pd.cpu() - wpd).abs().max())
    dice = float((ice.cpu().double() - wice).abs().max())
    print(f"max|dpd| {dpd:.3g}  max|dice| {dice:.3g}")
    assert dpd <= 2e-6
    assert dice <= 2e-6
    assert torch.equal(pd.cpu(), _sequential_mean(ice))
    # the no-substitution cell is the plain prediction
    p1 = gpu.predict_p1(x.to(dev))
    assert float((ice[:, 0].double() - p1.double()).abs().max()) <= 2e-6
    assert f"{100 * float(ice[0, 0]):.2f}" == "27.09"


def _unused_case(dev):
    """A stack that ignores variable j (no scale, no LR weight, no tree on it), with its cohort."""
    F = 6
    pk = _random_pstack(F, 64, 4, 1, dev, seed=21)
    used = set(pk.forest.nodes.reshape(-1, 4)[:, 0].tolist())
    j = next(k for k in range(F) if k not in used)
    inv_scale, lr_w = pk.inv_scale.clone(), pk.lr_w.clone()
    inv_scale[j] = 0.0
    lr_w[j] = 0.0
    pk = dataclasses.replace(pk, inv_scale=inv_scale, lr_w=lr_w)
    bg = torch.randn(12, F, generator=torch.Generator().manual_seed(22), dtype=torch.float64)
    return pk, bg, j


class _Model:
    """The two things StackExplainer asks of a fitted stack."""

    def __init__(self, pk):
        self.pk = pk

    def to(self, device):
        return self

    def _packed_stack(self, device):
        return self.pk


def test_unused_variable_has_no_interaction_and_a_flat_curve(dev):
    pk, bg, j = _unused_case(dev)
    F = pk.F
    ex = StackExplainer(_Model(pk), bg, device=dev)
    it = ex.interaction_strength()
    print(f"max H2 with the unused variable {float(it.h2[j].max()):.3g}, among the others {float(it.h2.max()):.3g}")
    assert float(it.h2[j].max()) <= 1e-12 and float(it.h2[:, j].max()) <= 1e-12
    assert float(it.h2.max()) > 1e-4
    curve = ex.partial_dependence([j], points=8).pd[0]
    assert curve.numel() == 8 and float(curve.max() - curve.min()) <= 1e-12
    assert float(torch.stack([c.max() - c.min() for c in ex.partial_dependence(points=8).pd]).max()) > 1e-4


def _singles(cols, grids, dev):
    feat = torch.tensor([[k, -1] for k, g in zip(cols, grids) for _ in range(g.numel())], device=dev)
    v = torch.cat(grids)
    return feat, torch.stack([v, torch.zeros_like(v)], 1)


def test_explainer_cuda(dev, ckpt_path):
    gpu = load_checkpoint(ckpt_path, device=dev)
    pk = gpu._packed_stack(dev)
    bg = torch.as_tensor(make_hf_cohort(40, 17, seed=0, nan_frac=0.0)[0], dtype=torch.float64)
    X = torch.as_tensor(make_hf_cohort(3, 17, seed=1, nan_frac=0.0)[0], dtype=torch.float64)
    ex = StackExplainer(gpu, bg, device=dev, feature_names=list(PATIENT_PARAMS))
    bgd, Xd = bg.to(dev), X.float().double().to(dev)            # the patients as the kernel sees them
    # partial dependence: the grid rule, then one op call over the background
    cols = [13, 0, 16]
    res = ex.partial_dependence(cols, points=8)
    assert res.features == cols and res.feature_names == [list(PATIENT_PARAMS)[k] for k in cols]
    assert res.grids[1].tolist() == [0.0, 1.0]
    for k, g in zip(cols, res.grids):
        assert g.device.type == torch.device(dev).type and torch.equal(g, ex.grid(k, 8))
        if k != 0:
            assert g.numel() == 8 and float(g[0]) == float(bg[:, k].float().min()) and float(g[-1]) == float(bg[:, k].float().max())
    feat, value = _singles(cols, res.grids, dev)
    assert torch.equal(torch.cat(res.pd), ops.stack_partial(bgd, pk, feat, value))
    # what-if: the patients as the cohort, their own values merged into the grids
    w = ex.what_if(X, cols, points=8)
    for i, k in enumerate(cols):
        assert torch.equal(w.grids[i], torch.unique(torch.cat([res.grids[i], Xd[:, k]])))
    feat, value = _singles(cols, w.grids, dev)
    _, ice = ops.stack_partial(Xd, pk, feat, value, return_ice=True)
    assert torch.equal(torch.cat(w.risk, 1), ice.double())
    assert torch.equal(torch.cat(w.cohort), ops.stack_partial(bgd, pk, feat, value))
    _, plain = ops.stack_partial(Xd, pk, torch.tensor([[-1, -1]], device=dev), torch.zeros(1, 2, device=dev),
                                 return_ice=True)
    assert torch.equal(w.prediction, plain[:, 0].double())
    for i, k in enumerate(cols):                                       # every curve passes through the prediction
        for p in range(3):
            at = (w.grids[i] == Xd[p, k]).nonzero().flatten()
            assert at.numel() == 1 and float(w.risk[i][p, at[0]]) == float(w.prediction[p])
    # Friedman's H²: the formula on direct calls, nothing de-duplicated
    it = ex.interaction_strength(max_rows=6)
    assert it.n_rows == 6 and torch.equal(it.h2, it.h2.t()) and float(it.h2.diagonal().abs().max()) == 0.0
    C6 = bgd[:6].contiguous()
    for j, k in [(13, 16), (0, 13), (3, 7)]:
        f2 = torch.tensor([[j, k]], device=dev).expand(6, 2).contiguous()
        a = ops.stack_partial(C6, pk, f2, C6[:, [j, k]].contiguous())
        one = torch.zeros(6, device=dev, dtype=torch.float64)
        b = ops.stack_partial(C6, pk, torch.tensor([[j, -1]], device=dev).expand(6, 2).contiguous(),
                              torch.stack([C6[:, j], one], 1))
        c = ops.stack_partial(C6, pk, torch.tensor([[k, -1]], device=dev).expand(6, 2).contiguous(),
                              torch.stack([C6[:, k], one], 1))
        a, b, c = a - a.mean(), b - b.mean(), c - c.mean()
        den = float((a * a).sum())
        want = float(((a - b - c) ** 2).sum()) / den if den > 0 else 0.0
        assert abs(float(it.h2[j, k]) - want) <= 1e-12


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


def test_cli_what_if_default_background_cuda(tmp_path, capsys):
    """``--what-if`` with no ``--background``: the 128-patient default cohort through the CLI."""
    assert main(["--device", "cuda"]) == 0
    plain = capsys.readouterr().out
    wicsv = tmp_path / "wi.csv"
    assert main(["--device", "cuda", "--what-if", "--what-if-csv", str(wicsv)]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and "27.09 %" in plain
    rows = _what_if_lines(out[len(plain):])
    assert len(rows) == 17 and {r[0] for r in rows} == set(PATIENT_PARAMS)
    spans = [r[5] - r[3] for r in rows]
    assert all(a >= b - 0.0101 for a, b in zip(spans, spans[1:]))      # sorted by highest − lowest (2 decimals printed)
    assert spans[0] > 1.0
    for name, cur, now, lo, v_lo, hi, v_hi in rows:
        assert cur == float(PATIENT_PARAMS[name]) and now == "27.09"
        assert lo <= float(now) <= hi
    lines = wicsv.read_text().splitlines()
    assert lines[0] == "variable,value,risk,cohort_mean_risk"
    names = [ln.split(",")[0] for ln in lines[1:]]
    assert list(dict.fromkeys(names)) == list(PATIENT_PARAMS)          # model order
    ex = StackExplainer(load_checkpoint(None, device="cuda"), device="cuda")
    w = ex.what_if([[float(v) for v in PATIENT_PARAMS.values()]])
    assert len(names) == sum(g.numel() for g in w.grids)               # one line per grid point
    assert names.count("Max_Wall_Thick") in (32, 33) and names.count("Gender") == 2
    assert main(["--device", "cuda", "--what-if", "No_Such_Variable"]) == 2
    capsys.readouterr()


def test_cli_interactions_csv_cuda(dev, ckpt_path, tmp_path, capsys):
    X = make_hf_cohort(3, 17, seed=1, nan_frac=0.0)[0]
    csv = tmp_path / "cohort.csv"
    np.savetxt(csv, X, delimiter=",")
    assert main(["--device", "cuda", "--csv", str(csv)]) == 0
    plain = capsys.readouterr().out
    assert main(["--device", "cuda", "--csv", str(csv), "--interactions", "5"]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and len(plain.splitlines()) == 3
    rest = out[len(plain):].splitlines()
    assert "3 patients" in rest[0] and len(rest) == 6
    ex = StackExplainer(load_checkpoint(ckpt_path, device=dev), device=dev, feature_names=list(PATIENT_PARAMS))
    for ln, (j, k, h) in zip(rest[1:], ex.interaction_strength(X).top(5)):
        assert ln == f"  {ex.feature_names[j]:<24s} {ex.feature_names[k]:<24s} {h:.4f}"
