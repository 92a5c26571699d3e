"""Exact Shapley attributions: the f64 mirror, the validation, StackExplainer and the CLI (host)."""
import itertools
import math

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.cli.predict_hf import PATIENT_PARAMS, format_probability, main
from hfens.explain import StackExplainer
from hfens.io.checkpoint import load_checkpoint
from hfens.io.synth import make_hf_cohort
from hfens.ops import reference as ref
from hfens.ops.packing import PackedStack, pack_forest, pack_stack, pack_svs, stump_table


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


def test_shapley_weights_sum_to_two():
    # Σ_S |c_k(S)| = Σ_s C(F−1, s)·w(s) (k joins) + the same (k absent) = 2
    for F in (1, 4, 17, 20):
        w = ref.shapley_weights(F)
        tot = sum(math.comb(F - 1, s) * float(w[s]) for s in range(F))
        assert abs(2 * tot - 2.0) < 1e-14


def test_mirror_matches_permutation_definition():
    F, B = 4, 3
    pk = _random_pstack(F, 32, 5, 1, "cpu", seed=3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, F, generator=g, dtype=torch.float64)
    bg = torch.randn(B, F, generator=g, dtype=torch.float64)

    def value(p, present):
        h = bg.clone()
        for k in present:
            h[:, k] = x[p, k]
        return float(ref.stack_infer(h, pk).mean())

    want = torch.zeros(2, F, dtype=torch.float64)
    perms = list(itertools.permutations(range(F)))
    assert len(perms) == 24
    for p in range(2):
        for order in perms:
            present, prev = [], value(p, [])
            for k in order:
                present.append(k)
                cur = value(p, present)
                want[p, k] += cur - prev
                prev = cur
    want /= len(perms)
    phi, base, pred, v = ref.stack_shapley(x, bg, pk, return_values=True)
    assert phi.shape == (2, F) and v.shape == (2, 1 << F) and pred.shape == (2,)
    assert float((phi - want).abs().max()) <= 1e-12
    # bit convention: bit k of S set <=> feature k takes the patient's value
    # (the mirror sums ‖sv − z‖² over features in another order than stack_infer: a few ulps)
    assert abs(float(v[1, 0b0101]) - value(1, [0, 2])) <= 1e-13
    assert abs(float(base) - value(0, [])) <= 1e-13
    assert float((pred - ref.stack_infer(x, pk)).abs().max()) <= 1e-13
    # the op routes host tensors to the mirror
    phi2, base2, pred2 = ops.stack_shapley(x, bg, pk)
    assert torch.equal(phi2, phi) and torch.equal(pred2, pred) and float(base2) == float(base)


@pytest.fixture(scope="module")
def ckpt_shapley(ckpt_path):
    """Default patient against one background patient on the shipped 17-feature stack."""
    pk = pack_stack(load_checkpoint(ckpt_path), "cpu")
    x = torch.tensor([[float(v) for v in PATIENT_PARAMS.values()]], dtype=torch.float64)
    bg = torch.as_tensor(make_hf_cohort(1, 17, seed=0, nan_frac=0.0)[0], dtype=torch.float64)
    return x, bg, ref.stack_shapley(x, bg, pk)


def test_efficiency_and_dummy_on_checkpoint(ckpt_shapley):
    x, bg, (phi, base, pred) = ckpt_shapley
    assert phi.shape == (1, 17)
    assert abs(float(phi.sum()) - (float(pred[0]) - float(base))) <= 1e-12
    assert f"{100 * float(pred[0]):.2f}" == "27.09"
    same = (x[0] == bg[0]).nonzero().flatten().tolist()
    differ = (x[0] != bg[0]).nonzero().flatten().tolist()
    assert same and differ
    for k in same:   # a feature that never changes a hybrid row contributes nothing
        assert abs(float(phi[0, k])) <= 1e-12


def test_validation():
    pk = _random_pstack(4, 32, 3, 1, "cpu")
    x, bg = torch.zeros(1, 4), torch.zeros(2, 4)
    with pytest.raises(ValueError):
        ops.stack_shapley(x, torch.zeros(0, 4), pk)           # empty background
    with pytest.raises(ValueError):
        ops.stack_shapley(x, torch.zeros(2, 5), pk)           # background width
    with pytest.raises(ValueError):
        ops.stack_shapley(torch.zeros(1, 3), bg, pk)          # patient width
    pk21 = _random_pstack(21, 32, 3, 1, "cpu")
    with pytest.raises(ValueError):
        ops.stack_shapley(torch.zeros(1, 21), torch.zeros(1, 21), pk21)   # F > 20


def test_explainer_host(ckpt_path, ckpt_shapley):
    x, bg, (phi, base, pred) = ckpt_shapley
    clf = load_checkpoint(ckpt_path)
    ex = StackExplainer(clf, bg, device="cpu", feature_names=list(PATIENT_PARAMS))
    e = ex.shap_values(x[0])
    assert torch.equal(e.phi, phi) and e.base_value == float(base) and torch.equal(e.prediction, pred)
    assert e.feature_names == list(PATIENT_PARAMS)
    clf.estimators_ = clf.estimators_[:2]
    clf._pstack = None
    with pytest.raises(ValueError, match="not an HF-shaped stack"):
        StackExplainer(clf, bg, device="cpu")


def test_explainer_default_background_is_the_hf_cohort(ckpt_path):
    ex = StackExplainer(load_checkpoint(ckpt_path), device="cpu")
    want = torch.as_tensor(make_hf_cohort(128, 17, seed=0, nan_frac=0.0)[0], dtype=torch.float64)
    assert torch.equal(ex.background, want) and len(ex.feature_names) == 17


def test_cli_explain(tmp_path, capsys, ckpt_shapley):
    x, bg, (phi, base, pred) = ckpt_shapley
    assert main([]) == 0
    plain = capsys.readouterr().out
    assert plain == format_probability(float(pred[0])) + "\n" and "27.09 %" in plain
    # (the default 128-patient background costs minutes on the host mirror: one row from a CSV)
    csv = tmp_path / "bg.csv"
    np.savetxt(csv, bg.numpy(), delimiter=",")
    assert main(["--explain", "--background", str(csv)]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain)                      # the probability block comes first, unchanged
    rest = out[len(plain):].splitlines()
    assert rest[0].startswith("Base value") and f"{100 * float(base):.2f} %" in rest[0]
    var = [ln for ln in rest if ln.startswith("  ")]
    assert len(var) == 17
    got = {}
    for ln in var:
        name = ln[2:26].rstrip()
        val, contrib = ln[26:].split()
        assert float(val) == float(PATIENT_PARAMS[name])
        got[name] = float(contrib)
    assert list(got) == sorted(got, key=lambda nm: -abs(got[nm]))            # sorted by |phi|
    for k, name in enumerate(PATIENT_PARAMS):
        assert abs(got[name] - 100 * float(phi[0, k])) <= 5.1e-5
    tail = rest[-1]
    assert tail.startswith("Sum of contributions:")
    total, diff = tail.split(":")[1].split("=")
    a, b = diff.split(" - ")
    assert abs(float(total) - (float(a) - float(b))) <= 2.1e-4                # printed to 4 decimals
    assert abs(sum(got.values()) - float(total)) <= 17 * 5e-5 + 5.1e-5


def test_cli_csv_importance(tmp_path, capsys, ckpt_shapley):
    x, bg, (phi, base, pred) = ckpt_shapley
    cohort, bgcsv = tmp_path / "cohort.csv", tmp_path / "bg.csv"
    np.savetxt(cohort, x.numpy(), delimiter=",")
    np.savetxt(bgcsv, bg.numpy(), delimiter=",")
    assert main(["--csv", str(cohort)]) == 0
    plain = capsys.readouterr().out
    assert main(["--csv", str(cohort), "--explain", "--background", str(bgcsv)]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and plain == f"{float(pred[0]):.6f}\n"
    var = [ln for ln in out.splitlines() if ln.startswith("  ")]
    got = {ln[2:26].rstrip(): float(ln[26:].split()[-1]) for ln in var}
    assert len(got) == 17 and list(got) == sorted(got, key=lambda nm: -got[nm])   # sorted by mean |phi|
    for k, name in enumerate(PATIENT_PARAMS):
        assert abs(got[name] - 100 * abs(float(phi[0, k]))) <= 5.1e-5
