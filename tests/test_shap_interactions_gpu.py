"""Exact Shapley interaction values on the GPU: the pair-reduction kernel on arbitrary games against the
longdouble oracle (F ≤ 10) or the f64 mirror, its structure, the fused op on random stacks and the
shipped checkpoint, the call paths that must not change a bit, and ``--explain-pairs`` on ``cuda``.

Bounds.  Φ_ij is a sum of 2^F products c_ij(T)·v(T) in f64: 2^F − 1 additions, one rounding per product,
one for the weight and one spare give ``(2^F + 4)·2^-53·Σ_T |c_ij(T)|·|v(T)|`` per entry whatever the
order of the sum (``entry_bound`` of tests/test_shap_interactions.py, from the mirror's own coefficients);
the diagonal φ_i − Σ_j Φ_ij adds φ's bound of the same form.  On a stack, v itself is within 5e-6 of the
mirror's (2e-6 on the shipped checkpoint: tests/test_explain_gpu.py), so Φ_ij is within
``Σ_T |c_ij(T)|`` times that: 2 off the diagonal, the mirror's coefficient sums on it."""
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

from test_explain_gpu import SHAPES, _inputs, _mirror, _random_pstack
from test_shap_interactions import U, _pair_lines, ckpt_pairs, entry_bound  # noqa: F401  (ckpt_pairs: fixture)

pytestmark = pytest.mark.gpu


def _log2(x):
    assert x & (x - 1) == 0
    return x.bit_length() - 1


def _edge_F():
    G = api.SHAPLEY_PAIR_GROUP
    fg = max(F for F in range(2, 21) if F * (F - 1) // 2 <= G)        # the last F whose pairs fill one group
    fs, ft = _log2(api.SHAPLEY_PAIR_SLAB), _log2(api.SHAPLEY_PAIR_THREADS)
    return sorted({1, 2, 3, fg, fg + 1, ft, ft + 1, fs, fs + 1, 13})


def test_edges_are_where_the_constants_put_them():
    assert _edge_F() == [1, 2, 3, 6, 7, 8, 9, 12, 13]


def _game(F, n):
    g = torch.Generator().manual_seed(77 * F + n)
    return torch.randn(n, 1 << F, generator=g, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _want(F, n):
    """(Phi, phi) of the seeded game as longdouble arrays — the oracle up to F = 10, the mirror above —
    and the per-entry bound."""
    v = _game(F, n)
    if F <= 10:
        Phi, phi = ref.shapley_interaction_oracle(v.numpy(), F)
    else:
        Phi, phi = (t.numpy().astype(np.longdouble) for t in ref.shapley_interactions_from_values(v, F))
    return Phi, phi, entry_bound(v, F).numpy()


def _check_game(dev, F, n):
    v = _game(F, n)
    Phi, phi = ops.shapley_interactions_from_values(v.to(dev), F)
    assert Phi.shape == (n, F, F) and phi.shape == (n, F) and Phi.dtype == phi.dtype == torch.float64
    wPhi, wphi, bound = _want(F, n)
    err = np.abs(Phi.cpu().numpy().astype(np.longdouble) - wPhi).astype(np.float64)
    perr = np.abs(phi.cpu().numpy().astype(np.longdouble) - wphi).astype(np.float64)
    print(f"F {F}: max err {err.max():.3g} (largest err/bound {(err / bound).max():.3g})  max phi err {perr.max():.3g}")
    assert (err <= bound).all()
    assert (perr <= np.diagonal(bound, axis1=1, axis2=2)).all()
    assert torch.equal(Phi, Phi.transpose(1, 2))
    # row i sums to phi[i]: the kernel rounds the F − 2 additions of Σ_j and the subtraction
    P = Phi.cpu().numpy().astype(np.longdouble)
    gap = np.abs(P.sum(2) - phi.cpu().numpy()).astype(np.float64)
    assert (gap <= F * U * np.abs(P).sum(2).astype(np.float64)).all()
    again, _ = ops.shapley_interactions_from_values(v.to(dev), F)
    assert torch.equal(again, Phi)
    return Phi


@pytest.mark.parametrize("F", _edge_F())
def test_kernel_on_random_games(dev, F):
    _check_game(dev, F, 3)


def test_kernel_on_a_random_game_f20(dev):
    _check_game(dev, 20, 1)


def test_patients_do_not_mix(dev):
    """Patient p of a batch gets the bits it gets alone."""
    F = 13
    v = _game(F, 3).to(dev)
    Phi, phi = ops.shapley_interactions_from_values(v, F)
    one, one_phi = ops.shapley_interactions_from_values(v[2:3].clone(), F)
    assert torch.equal(Phi[2:3], one) and torch.equal(phi[2:3], one_phi)


@pytest.mark.parametrize("F", [2, 7, 13])
def test_closed_forms(dev, F):
    T = torch.arange(1 << F)
    i, j, c = 0, F - 1, 3.0
    pair = c * (((T >> i) & 1) * ((T >> j) & 1)).double()                 # c·[i ∈ T][j ∈ T]
    h = _game(F - 1, 1)[0]
    ignored = torch.cat([h, h])                                           # ignores feature F − 1
    v = torch.stack([pair, ignored])
    Phi, phi = ops.shapley_interactions_from_values(v.to(dev), F)
    Phi, b = Phi.cpu(), entry_bound(v, F)
    want = torch.zeros(F, F, dtype=torch.float64)
    want[i, j] = want[j, i] = c / 2
    assert ((Phi[0] - want).abs() <= b[0]).all()
    assert (Phi[1, F - 1].abs() <= b[1, F - 1]).all() and (Phi[1, :, F - 1].abs() <= b[1, :, F - 1]).all()


# ------------------------------------------------------------------ the fused op on random stacks
STACKS = [SHAPES[0], SHAPES[2], SHAPES[3]]
assert STACKS == [(5, 64, 10, 2, False, 3, 1), (11, 250, 30, 1, True, 2, 3), (8, 6000, 20, 1, True, 1, 5)]


def _gpu(shape, dev, op=ops.stack_shapley_interactions, **kw):
    F, m, T, depth, stumps, n, B = shape
    x, bg = _inputs(F, n, B)
    pk = _random_pstack(F, m, T, depth, dev, seed=F, stumps=stumps)
    return op(x.to(dev), bg.to(dev), pk, return_values=True, **kw)


@pytest.mark.parametrize("shape", STACKS)
def test_random_stacks_match_mirror(dev, shape):
    F = shape[0]
    Phi, phi, base, pred, v = _gpu(shape, dev)
    wphi, wbase, wpred, wv = _mirror(shape)
    wPhi, wphi2 = ref.shapley_interactions_from_values(wv, F)
    assert torch.equal(wphi2, wphi)
    tol = ref.shapley_interaction_abs_sums(F) * 5e-6
    err = (Phi.cpu() - wPhi).abs()
    print(f"max|dPhi| {float(err.max()):.3g}  off-diagonal tolerance {float(tol[0, -1]):.3g}  "
          f"diagonal {float(tol[0, 0]):.3g}")
    assert (err <= tol).all()
    assert torch.equal(Phi, Phi.transpose(1, 2))
    assert float((Phi.sum((1, 2)) - (pred - base)).abs().max()) <= 1e-9
    want = _gpu(shape, dev, op=ops.stack_shapley)
    assert all(torch.equal(g, w) for g, w in zip((phi, base, pred, v), want))
    # the kernel on the op's own table is the op
    P2, p2 = ops.shapley_interactions_from_values(v, F)
    assert torch.equal(P2, Phi) and torch.equal(p2, phi)


@pytest.mark.parametrize("shape", STACKS)
def test_deterministic_and_grid_independent(dev, shape):
    a = _gpu(shape, dev)
    b = _gpu(shape, dev)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    for grid in (1, 3):
        c = _gpu(shape, dev, grid=grid)
        assert all(torch.equal(s, t) for s, t in zip(a, c))


def test_patient_chunking(dev, monkeypatch):
    F, B, n = 11, 3, 5
    pk = _random_pstack(F, 250, 30, 1, dev, seed=F)
    x, bg = _inputs(F, n, B)
    x, bg = x.to(dev), bg.to(dev)
    one = ops.stack_shapley_interactions(x, bg, pk, return_values=True)
    monkeypatch.setattr(api, "SHAPLEY_WS_BYTES", 1)               # one patient per chunk
    for rv in (True, False):
        got = ops.stack_shapley_interactions(x, bg, pk, return_values=rv)
        assert len(got) == (5 if rv else 4)
        assert all(torch.equal(g, w) for g, w in zip(got, one))


def test_external_stream(dev):
    shape = STACKS[1]
    want = _gpu(shape, dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = _gpu(shape, dev, stream=side.cuda_stream)
    side.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------ shipped checkpoint, explainer, CLI
def test_checkpoint_matches_mirror(dev, ckpt_path, ckpt_pairs):  # noqa: F811
    x, bg, (wPhi, wphi, wbase, wpred) = ckpt_pairs
    gpu = load_checkpoint(ckpt_path, device=dev)
    Phi, phi, base, pred = ops.stack_shapley_interactions(x.to(dev), bg.to(dev), gpu._packed_stack(dev))
    tol = ref.shapley_interaction_abs_sums(17) * 2e-6
    err = (Phi.cpu() - wPhi).abs()
    print(f"max|dPhi| {float(err.max()):.3g}  tolerance {float(tol.min()):.3g} … {float(tol.max()):.3g}")
    assert (err[0] <= tol).all()
    assert abs(float(Phi.sum()) - (float(pred[0]) - float(base))) <= 1e-9
    assert f"{100 * float(pred[0]):.2f}" == "27.09"
    want = ops.stack_shapley(x.to(dev), bg.to(dev), gpu._packed_stack(dev))
    assert all(torch.equal(g, w) for g, w in zip((phi, base, pred), want))


def test_explainer_cuda(dev, ckpt_path):
    gpu = load_checkpoint(ckpt_path, device=dev)
    bg = make_hf_cohort(4, 17, seed=0, nan_frac=0.0)[0]
    X = make_hf_cohort(3, 17, seed=1, nan_frac=0.0)[0]
    ex = StackExplainer(gpu, bg, device=dev, feature_names=list(PATIENT_PARAMS))
    e = ex.shap_interaction_values(X)
    s = ex.shap_values(X)
    Phi, phi, base, pred = ops.stack_shapley_interactions(torch.as_tensor(X).to(dev), torch.as_tensor(bg).to(dev),
                                                          gpu._packed_stack(dev))
    assert torch.equal(e.Phi, Phi) and torch.equal(e.phi, phi) and torch.equal(e.prediction, pred)
    assert torch.equal(e.phi, s.phi) and e.base_value == s.base_value == float(base)
    top = e.top(4, p=2)
    assert all(i < j and eff == 2.0 * float(Phi[2, i, j]) for i, j, eff in top)
    assert [abs(t[2]) for t in top] == sorted((abs(t[2]) for t in top), reverse=True)


def test_cli_explain_pairs_cuda(dev, ckpt_path, capsys):
    """``--explain-pairs`` with no ``--background``: the 128-patient default cohort through the CLI."""
    assert main(["--device", "cuda", "--explain"]) == 0
    plain = capsys.readouterr().out
    assert main(["--device", "cuda", "--explain", "--explain-pairs", "6"]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and "27.09 %" in plain
    rest = out[len(plain):].splitlines()
    got = _pair_lines(rest)
    e = StackExplainer(load_checkpoint(ckpt_path, device=dev), device=dev).shap_interaction_values(
        [[float(v) for v in PATIENT_PARAMS.values()]])
    names = list(PATIENT_PARAMS)
    want = e.top(6)
    assert [(a, b) for a, b, _ in got] == [(names[i], names[j]) for i, j, _ in want]
    for (_, _, val), (_, _, eff) in zip(got, want):
        assert abs(val - 100 * eff) <= 5.1e-5
    lhs, total, diff = rest[-1][len("Main effects "):].split(" = ")
    m, p = lhs.split(" + pair effects ")
    a, b = diff.split(" - ")
    assert f"{float(a):.2f}" == "27.09"
    assert abs(float(m) + float(p) - float(total)) <= 1.1e-4
    assert abs(float(total) - (float(a) - float(b))) <= 1.1e-4 + 1e-7


def test_cli_csv_pair_importance_cuda(dev, ckpt_path, tmp_path, capsys):
    X = make_hf_cohort(3, 17, seed=1, nan_frac=0.0)[0]
    csv = tmp_path / "cohort.csv"
    np.savetxt(csv, X, delimiter=",")
    assert main(["--device", "cuda", "--csv", str(csv), "--explain"]) == 0
    plain = capsys.readouterr().out
    assert main(["--device", "cuda", "--csv", str(csv), "--explain-pairs", "5"]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain)
    got = _pair_lines(out[len(plain):].splitlines())
    e = StackExplainer(load_checkpoint(ckpt_path, device=dev), device=dev).shap_interaction_values(X)
    m = e.mean_abs_pairs().cpu()
    names = list(PATIENT_PARAMS)
    assert len(got) == 5 and [g[2] for g in got] == sorted((g[2] for g in got), reverse=True)
    for a, b, val in got:
        assert abs(val - 100 * float(m[names.index(a), names.index(b)])) <= 5.1e-5
    fifth = sorted((float(m[i, j]) for i in range(17) for j in range(i + 1, 17)), reverse=True)[4]
    assert all(val >= 100 * fifth - 1.1e-4 for _, _, val in got)
