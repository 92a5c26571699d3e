"""Exact Shapley attributions on the GPU: the fused coalition kernel and the f64 reduction
against the host mirror, plus the properties that do not need one (efficiency, determinism,
grid independence, patient chunking).

Tolerances come from the bounds the project already holds the same arithmetic to:
``test_stack_infer_random`` keeps the kernel within 5e-6 of the f64 reference per row; v is a
mean of such rows (5e-6), and Σ_S |c_k(S)| = 2 makes phi at most twice that (1e-5).  On the
shipped checkpoint ``test_stack_infer_checkpoint``'s 2e-6 gives 2e-6 for v and 4e-6 for phi."""
import functools

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


# (F, m, T, depth, stumps, n, B)
SHAPES = [
    (5, 64, 10, 2, False, 3, 1),      # generic tree walk, odd F, one background, half-empty tile
    (5, 64, 10, 1, True, 1, 100),     # B not a power of two
    (11, 250, 30, 1, True, 2, 3),     # B < 64, odd F, 32 tiles per patient
    (8, 6000, 20, 1, True, 1, 5),     # SVs exceed LDS: chunked restaging (f32 MFMA path)
    (12, 434, 100, 1, True, 1, 7),
    (19, 32, 4, 1, True, 1, 1),       # widest k-step count (F > 18): f32 MFMA path, SVs resident
]


def _inputs(F, n, B):
    """f32-representable patients and background (what the kernel sees), as f64."""
    g = torch.Generator().manual_seed(100 * F + B)
    x = torch.randn(n, F, generator=g).double()
    bg = torch.randn(B, F, generator=g).double()
    return x, bg


@functools.lru_cache(maxsize=None)
def _mirror(shape):
    F, m, T, depth, stumps, n, B = shape
    x, bg = _inputs(F, n, B)
    return ref.stack_shapley(x, bg, _random_pstack(F, m, T, depth, "cpu", seed=F, stumps=stumps),
                             return_values=True)


def _gpu(shape, dev, dtype=torch.float64, **kw):
    F, m, T, depth, stumps, n, B = shape
    x, bg = _inputs(F, n, B)
    pk = _random_pstack(F, m, T, depth, dev, seed=F, stumps=stumps)
    return ops.stack_shapley(x.to(dev, dtype), bg.to(dev, dtype), pk, return_values=True, **kw)


def _check_against_mirror(got, want):
    phi, base, pred, v = (t.cpu() for t in got)
    wphi, wbase, wpred, wv = want
    assert phi.dtype == v.dtype == pred.dtype == base.dtype == torch.float64
    assert phi.shape == wphi.shape and v.shape == wv.shape and pred.shape == wpred.shape and base.dim() == 0
    dv, dphi = float((v - wv).abs().max()), float((phi - wphi).abs().max())
    dbase, dpred = abs(float(base - wbase)), float((pred - wpred).abs().max())
    print(f"max|dv| {dv:.3g}  max|dphi| {dphi:.3g}  |dbase| {dbase:.3g}  max|dpred| {dpred:.3g}")
    assert dv <= 5e-6
    assert dphi <= 1e-5
    assert dbase <= 5e-6 and dpred <= 5e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_random_stacks_match_mirror(dev, shape):
    _check_against_mirror(_gpu(shape, dev), _mirror(shape))


def test_f32_inputs_match_mirror(dev):
    _check_against_mirror(_gpu(SHAPES[0], dev, torch.float32), _mirror(SHAPES[0]))


@pytest.mark.parametrize("shape", SHAPES)
def test_efficiency_from_kernel_values(dev, shape):
    phi, base, pred, v = _gpu(shape, dev)
    gap = (phi.sum(1) - (v[:, -1] - v[:, 0])).abs()
    print(f"max efficiency gap {float(gap.max()):.3g}")
    assert float(gap.max()) <= 1e-9
    assert torch.equal(pred, v[:, -1]) and float(base) == float(v[0, 0])
    assert torch.equal(v[:, 0], v[0, 0].expand(v.shape[0]))      # v(∅) does not depend on the patient


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_deterministic_and_grid_independent(dev, shape):
    a = _gpu(shape, dev)
    b = _gpu(shape, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    for grid in (1, 3):
        c = _gpu(shape, dev, grid=grid)
        assert torch.equal(a[3], c[3]) and torch.equal(a[0], c[0])


def test_patient_chunking(dev, monkeypatch):
    F, B, n = 11, 3, 5
    pk = _random_pstack(F, 250, 30, 1, dev, seed=F)
    x, bg = _inputs(F, n, B)
    x, bg = x.to(dev), bg.to(dev)
    one = ops.stack_shapley(x, bg, pk, return_values=True)
    monkeypatch.setattr(api, "SHAPLEY_WS_BYTES", 1)               # one patient per chunk
    for rv in (True, False):
        got = ops.stack_shapley(x, bg, pk, return_values=rv)
        assert all(torch.equal(g, w) for g, w in zip(got, one))


@pytest.fixture(scope="module")
def ckpt_case(ckpt_path):
    pk = pack_stack(load_checkpoint(ckpt_path), "cpu")
    x = torch.tensor([[float(v) for v in PATIENT_PARAMS.values()]], dtype=torch.float64)
    bg = torch.as_tensor(make_hf_cohort(2, 17, seed=0, nan_frac=0.0)[0], dtype=torch.float64)
    return x, bg, ref.stack_shapley(x, bg, pk, return_values=True)


def test_checkpoint_matches_mirror(dev, ckpt_path, ckpt_case):
    x, bg, (wphi, wbase, wpred, wv) = ckpt_case
    gpu = load_checkpoint(ckpt_path, device=dev)
    phi, base, pred, v = ops.stack_shapley(x.to(dev), bg.to(dev), gpu._packed_stack(dev), return_values=True)
    dv, dphi = float((v.cpu() - wv).abs().max()), float((phi.cpu() - wphi).abs().max())
    print(f"max|dv| {dv:.3g}  max|dphi| {dphi:.3g}")
    assert dv <= 2e-6
    assert dphi <= 4e-6
    assert f"{100 * float(pred[0]):.2f}" == "27.09"
    assert abs(float(pred[0]) - float(gpu.predict_p1(x.to(dev))[0])) <= 2e-6
    assert abs(float(phi.sum()) - (float(pred[0]) - float(base))) <= 1e-9


def test_explainer_cuda(dev, ckpt_path):
    gpu = load_checkpoint(ckpt_path, device=dev)
    bg = make_hf_cohort(4, 17, seed=0, nan_frac=0.0)[0]
    X = make_hf_cohort(3, 17, seed=1, nan_frac=0.0)[0]
    ex = StackExplainer(gpu, bg, device=dev, feature_names=list(PATIENT_PARAMS))
    e = ex.shap_values(X)
    phi, base, pred = ops.stack_shapley(torch.as_tensor(X).to(dev), torch.as_tensor(bg).to(dev),
                                        gpu._packed_stack(dev))
    assert torch.equal(e.phi, phi) and torch.equal(e.prediction, pred) and e.base_value == float(base)
    assert e.feature_names == list(PATIENT_PARAMS)
    assert torch.equal(ex.mean_abs(X), phi.abs().mean(0))


def test_external_stream(dev):
    shape = SHAPES[2]
    want = _gpu(shape, dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = _gpu(shape, dev, stream=side.cuda_stream)
    side.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def _variable_lines(out):
    got = {}
    for ln in out.splitlines():
        if ln.startswith("  "):
            got[ln[2:26].rstrip()] = float(ln[26:].split()[-1])
    return got


def test_cli_explain_default_background_cuda(capsys):
    """``--explain`` with no ``--background``: the 128-patient default cohort through the CLI."""
    assert main(["--device", "cuda"]) == 0
    plain = capsys.readouterr().out
    assert main(["--device", "cuda", "--explain"]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and "27.09 %" in plain
    got = _variable_lines(out)
    assert list(got) == sorted(got, key=lambda nm: -abs(got[nm])) and set(got) == set(PATIENT_PARAMS)
    tail = out.splitlines()[-1]
    assert tail.startswith("Sum of contributions:")
    total, diff = tail.split(":")[1].split("=")
    a, b = diff.split(" - ")
    assert f"{float(a):.2f}" == "27.09"
    assert abs(float(total) - (float(a) - float(b))) <= 2.1e-4                # printed to 4 decimals
    assert abs(sum(got.values()) - float(total)) <= 17 * 5e-5 + 5.1e-5


def test_cli_csv_importance_cuda(dev, ckpt_path, tmp_path, capsys):
    X = make_hf_cohort(3, 17, seed=1, nan_frac=0.0)[0]
    csv = tmp_path / "cohort.csv"
    np.savetxt(csv, X, delimiter=",")
    assert main(["--device", "cuda", "--csv", str(csv)]) == 0
    plain = capsys.readouterr().out
    assert main(["--device", "cuda", "--csv", str(csv), "--explain"]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and len(plain.splitlines()) == 3
    got = _variable_lines(out)
    want = StackExplainer(load_checkpoint(ckpt_path, device=dev), device=dev).mean_abs(X).cpu().tolist()
    assert list(got) == sorted(got, key=lambda nm: -got[nm]) and set(got) == set(PATIENT_PARAMS)
    for k, name in enumerate(PATIENT_PARAMS):
        assert abs(got[name] - 100 * want[k]) <= 5.1e-5
