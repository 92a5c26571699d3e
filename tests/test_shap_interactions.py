"""Exact Shapley interaction values: the f64 mirror against the longdouble subset-sum oracle, the
closed forms, the validation, StackExplainer and ``--explain-pairs`` (host).

The mirror is a sum of 2^F products c_ij(T)·v(T) in f64, in an order left to the GEMM, so its distance
from the oracle is bounded entry by entry by ``(2^F + 4)·2^-53·Σ_T |c_ij(T)|·|v(T)|`` (2^F − 1 additions
and one product rounding per term, the weight's own rounding, and the oracle's longdouble error far
below); the diagonal ``φ_i − Σ_j Φ_ij`` adds φ's bound of the same form."""
import math

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.cli.predict_hf import PATIENT_PARAMS, main
from hfens.explain import InteractionExplanation, StackExplainer
from hfens.io.checkpoint import load_checkpoint
from hfens.io.synth import make_hf_cohort
from hfens.ops import reference as ref
from hfens.ops.packing import pack_stack

from test_explain import _random_pstack

U = 2.0 ** -53


def _game(F, n=2, seed=0):
    g = torch.Generator().manual_seed(1000 * F + seed)
    return torch.randn(n, 1 << F, generator=g, dtype=torch.float64)


def entry_bound(v, F):
    """``(2^F + 4)·2^-53·Σ_T |c_ij(T)|·|v(T)|`` per entry, plus φ's bound of the same form on the diagonal."""
    S = torch.arange(1 << F)
    inS = ((S[:, None] >> torch.arange(F)[None, :]) & 1).bool()
    size = inS.sum(1)
    w = torch.cat([ref.shapley_weights(F), torch.zeros(1, dtype=torch.float64)])
    ck = torch.where(inS, w[(size - 1).clamp(min=0)][:, None], w[size][:, None])       # |c_k(T)|
    b = ref.shapley_interaction_abs_sums(F, v) + torch.diag_embed(v.abs() @ ck)
    return ((1 << F) + 4) * U * b


@pytest.mark.parametrize("F", range(1, 9))
def test_mirror_matches_oracle(F):
    v = _game(F)
    Phi, phi = ref.shapley_interactions_from_values(v, F)
    oPhi, ophi = ref.shapley_interaction_oracle(v.numpy(), F)
    assert Phi.shape == (2, F, F) and phi.shape == (2, F) and Phi.dtype == torch.float64
    err = np.abs(Phi.numpy().astype(np.longdouble) - oPhi).astype(np.float64)
    bound = entry_bound(v, F).numpy()
    print(f"F {F}: max err {err.max():.3g}  min bound {bound.min():.3g}")
    assert (err <= bound).all()
    assert float(np.abs(phi.numpy() - ophi).max()) <= float(bound.max())
    assert torch.equal(Phi, Phi.transpose(1, 2))
    assert torch.equal(phi, ref.shapley_from_values(v, F))


def test_f1_is_phi():
    v = torch.tensor([[0.25, 0.75], [1.0, -2.0]], dtype=torch.float64)
    Phi, phi = ref.shapley_interactions_from_values(v, 1)
    assert torch.equal(Phi, phi[:, :, None]) and torch.equal(phi[:, 0], v[:, 1] - v[:, 0])
    assert ref.shapley_interaction_weights(1).numel() == 0


@pytest.mark.parametrize("F", [2, 3, 6, 8])
def test_pair_game(F):
    """v(T) = c·[i ∈ T][j ∈ T]: Φ_ij = Φ_ji = c/2 and every other entry 0."""
    i, j, c = 0, F - 1, 3.0
    T = torch.arange(1 << F)
    v = (c * (((T >> i) & 1) * ((T >> j) & 1)).double())[None, :]
    Phi, phi = ref.shapley_interactions_from_values(v, F)
    want = torch.zeros(F, F, dtype=torch.float64)
    want[i, j] = want[j, i] = c / 2
    assert ((Phi[0] - want).abs() <= entry_bound(v, F)[0]).all()


@pytest.mark.parametrize("F", [2, 5, 8])
def test_additive_game_and_ignored_feature(F):
    """v(T) = Σ_{k ∈ T} a_k with a_{F−1} = 0: the diagonal is a, the rest 0; the ignored feature's row and
    column are 0."""
    g = torch.Generator().manual_seed(F)
    a = torch.randn(F, generator=g, dtype=torch.float64)
    a[F - 1] = 0.0
    T = torch.arange(1 << F)
    inT = ((T[:, None] >> torch.arange(F)[None, :]) & 1).double()
    v = (inT @ a)[None, :]
    Phi, phi = ref.shapley_interactions_from_values(v, F)
    assert ((Phi[0] - torch.diag(a)).abs() <= entry_bound(v, F)[0]).all()
    # a random game that ignores its last feature
    h = _game(F - 1, n=1, seed=7)
    v2 = torch.cat([h, h], 1)
    Phi2, phi2 = ref.shapley_interactions_from_values(v2, F)
    b = entry_bound(v2, F)[0]
    assert (Phi2[0, F - 1].abs() <= b[F - 1]).all() and (Phi2[0, :, F - 1].abs() <= b[:, F - 1]).all()


@pytest.mark.parametrize("F", [2, 3, 7, 12, 17, 20])
def test_abs_coefficients_sum_to_two(F):
    """Σ_T |c_ij(T)| = Σ_s C(F−2, s)·u(s)·4 = 2 for i ≠ j, from the mirror's own coefficient matrix."""
    if F <= 12:
        s = ref.shapley_interaction_abs_sums(F)
        off = s[~torch.eye(F, dtype=torch.bool)]
        assert float((off - 2.0).abs().max()) <= 1e-13
    u = ref.shapley_interaction_weights(F)
    assert u.shape == (F - 1,)
    assert abs(4 * sum(math.comb(F - 2, k) * float(u[k]) for k in range(F - 1)) - 2.0) <= 1e-14


@pytest.mark.parametrize("F", [1, 2, 5, 9])
def test_row_sums_and_total(F):
    v = _game(F, n=3, seed=1)
    Phi, phi = ref.shapley_interactions_from_values(v, F)
    P = Phi.numpy().astype(np.longdouble)
    assert (np.abs(P.sum(2) - phi.numpy()) <= F * U * np.abs(P).sum(2)).all()
    total = (v[:, -1] - v[:, 0]).numpy()
    assert (np.abs(P.sum((1, 2)).astype(np.float64) - total) <= entry_bound(v, F).sum((1, 2)).numpy()).all()


@pytest.fixture(scope="module")
def stack5():
    F, B = 5, 3
    pk = _random_pstack(F, 32, 5, 1, "cpu", seed=3)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, F, generator=g, dtype=torch.float64)
    bg = torch.randn(B, F, generator=g, dtype=torch.float64)
    return pk, x, bg


def test_stack_mirror_shares_phi_with_stack_shapley(stack5):
    pk, x, bg = stack5
    Phi, phi, base, pred, v = ref.stack_shapley_interactions(x, bg, pk, return_values=True)
    wphi, wbase, wpred, wv = ref.stack_shapley(x, bg, pk, return_values=True)
    assert torch.equal(phi, wphi) and torch.equal(base, wbase) and torch.equal(pred, wpred) and torch.equal(v, wv)
    assert Phi.shape == (2, 5, 5)
    oPhi, _ = ref.shapley_interaction_oracle(v.numpy(), 5)
    assert (np.abs(Phi.numpy() - oPhi).astype(np.float64) <= entry_bound(v, 5).numpy()).all()
    # the ops route host tensors to the mirrors
    got = ops.stack_shapley_interactions(x, bg, pk)
    assert len(got) == 4 and torch.equal(got[0], Phi) and torch.equal(got[1], phi)
    P2, p2 = ops.shapley_interactions_from_values(v, 5)
    assert torch.equal(P2, Phi) and torch.equal(p2, phi)


def test_validation(stack5):
    pk, x, bg = stack5
    with pytest.raises(ValueError, match="stack_shapley_interactions"):
        ops.stack_shapley_interactions(x, torch.zeros(0, 5), pk)              # empty background
    with pytest.raises(ValueError):
        ops.stack_shapley_interactions(x, torch.zeros(2, 6), pk)              # background width
    with pytest.raises(ValueError):
        ops.stack_shapley_interactions(torch.zeros(1, 4), bg, pk)             # patient width
    with pytest.raises(ValueError):
        ops.stack_shapley_interactions(torch.zeros(5), bg, pk)                # not a matrix
    pk21 = _random_pstack(21, 32, 3, 1, "cpu")
    with pytest.raises(ValueError, match="limited to 20"):
        ops.stack_shapley_interactions(torch.zeros(1, 21), torch.zeros(1, 21), pk21)
    with pytest.raises(ValueError):
        ops.shapley_interactions_from_values(torch.zeros(1, 8, dtype=torch.float64), 21)
    with pytest.raises(ValueError):
        ops.shapley_interactions_from_values(torch.zeros(1, 8, dtype=torch.float64), 0)
    with pytest.raises(ValueError):
        ops.shapley_interactions_from_values(torch.zeros(1, 7, dtype=torch.float64), 3)   # not 2^F columns
    with pytest.raises(ValueError):
        ops.shapley_interactions_from_values(torch.zeros(8, dtype=torch.float64), 3)      # not a matrix
    with pytest.raises(ValueError):
        ops.shapley_interactions_from_values(torch.zeros(1, 8), 3)                        # f32
    with pytest.raises(ValueError):
        ref.shapley_interaction_oracle(np.zeros((1, 1 << 11)), 11)


def test_top_orders_by_pair_effect():
    Phi = torch.zeros(2, 3, 3, dtype=torch.float64)
    Phi[1, 0, 1] = Phi[1, 1, 0] = 0.1
    Phi[1, 0, 2] = Phi[1, 2, 0] = -0.3
    Phi[1, 1, 2] = Phi[1, 2, 1] = 0.2
    e = InteractionExplanation(Phi, Phi.sum(2), 0.0, torch.zeros(2, dtype=torch.float64), ["a", "b", "c"])
    assert e.top(2, p=1) == [(0, 2, -0.6), (1, 2, 0.4)]
    assert len(e.top(10, p=1)) == 3 and e.top(1) == [(0, 1, 0.0)]
    assert torch.equal(e.mean_abs_pairs(), Phi[1].abs())


@pytest.fixture(scope="module")
def ckpt_pairs(ckpt_path):
    """Default patient against two background patients on the shipped 17-feature stack."""
    pk = pack_stack(load_checkpoint(ckpt_path), "cpu")
    x = torch.tensor([[float(v) for v in PATIENT_PARAMS.values()]], dtype=torch.float64)
    bg = torch.as_tensor(make_hf_cohort(2, 17, seed=0, nan_frac=0.0)[0], dtype=torch.float64)
    return x, bg, ref.stack_shapley_interactions(x, bg, pk)


def test_explainer_host(ckpt_path, ckpt_pairs):
    x, bg, (Phi, phi, base, pred) = ckpt_pairs
    ex = StackExplainer(load_checkpoint(ckpt_path), bg, device="cpu", feature_names=list(PATIENT_PARAMS))
    e = ex.shap_interaction_values(x[0])
    assert torch.equal(e.Phi, Phi) and torch.equal(e.phi, phi) and torch.equal(e.prediction, pred)
    assert e.base_value == float(base) and e.feature_names == list(PATIENT_PARAMS)
    assert abs(float(Phi.sum()) - (float(pred[0]) - float(base))) <= 1e-12
    assert f"{100 * float(pred[0]):.2f}" == "27.09"
    top = e.top(5)
    assert [abs(t[2]) for t in top] == sorted((abs(t[2]) for t in top), reverse=True)
    assert all(i < j and eff == 2.0 * float(Phi[0, i, j]) for i, j, eff in top)


def _pair_lines(lines):
    got = []
    for ln in lines:
        if ln.startswith("  "):
            got.append((ln[2:26].rstrip(), ln[27:51].rstrip(), float(ln[51:])))
    return got


def test_cli_explain_pairs(tmp_path, capsys, ckpt_pairs):
    x, bg, (Phi, phi, base, pred) = ckpt_pairs
    csv = tmp_path / "bg.csv"
    np.savetxt(csv, bg.numpy(), delimiter=",")
    assert main(["--explain", "--background", str(csv)]) == 0
    plain = capsys.readouterr().out
    assert main(["--explain-pairs", "--background", str(csv)]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain)                      # the --explain output (implied) comes first, unchanged
    rest = out[len(plain):].splitlines()
    assert rest[0].startswith("Strongest variable pairs")
    got = _pair_lines(rest)
    names = list(PATIENT_PARAMS)
    assert len(got) == 10
    assert [abs(g[2]) for g in got] == sorted((abs(g[2]) for g in got), reverse=True)
    eff = {(names[i], names[j]): 200 * float(Phi[0, i, j]) for i in range(17) for j in range(i + 1, 17)}
    for a, b, val in got:
        assert abs(val - eff[(a, b)]) <= 5.1e-5       # printed to 4 decimals
    tenth = sorted((abs(t) for t in eff.values()), reverse=True)[9]
    assert all(abs(val) >= tenth - 1.1e-4 for _, _, val in got)
    tail = rest[-1]
    assert tail.startswith("Main effects ")
    lhs, total, diff = tail[len("Main effects "):].split(" = ")
    m, p = lhs.split(" + pair effects ")
    a, b = diff.split(" - ")
    assert abs(float(m) + float(p) - float(total)) <= 1.1e-4
    assert abs(float(total) - (float(a) - float(b))) <= 1.1e-4 + 1e-10
    assert f"{float(a):.2f}" == "27.09"


def test_cli_csv_pair_importance(tmp_path, capsys, ckpt_pairs):
    x, bg, (Phi, phi, base, pred) = ckpt_pairs
    cohort, bgcsv = tmp_path / "cohort.csv", tmp_path / "bg.csv"
    np.savetxt(cohort, x.numpy(), delimiter=",")
    np.savetxt(bgcsv, bg.numpy(), delimiter=",")
    assert main(["--csv", str(cohort), "--explain", "--background", str(bgcsv)]) == 0
    plain = capsys.readouterr().out
    assert main(["--csv", str(cohort), "--explain", "--explain-pairs", "3", "--background", str(bgcsv)]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain)
    rest = out[len(plain):].splitlines()
    assert rest[0].startswith("Mean |pair effect|")
    got = _pair_lines(rest)
    names = list(PATIENT_PARAMS)
    assert len(got) == 3 and [g[2] for g in got] == sorted((g[2] for g in got), reverse=True)
    for a, b, val in got:
        assert abs(val - 200 * abs(float(Phi[0, names.index(a), names.index(b)]))) <= 5.1e-5
