"""The device KNN imputation (ops/csrc/knn.hip, models/imputer.py) against the longdouble brute
force ``ops.reference.knn_impute1`` — an oracle written apart from the kernels and the host mirror —
at the shapes, missing patterns, ties, near-ties and magnitudes where the kernels change path.

Unless a case says otherwise the imputer is fitted on one matrix and transforms ANOTHER one, and the
assertions are ``assert_imputed``'s: the reference's shape, donor cells bit-equal, column-mean cells
within n_c·2⁻⁵²·mean|x_c|, no NaN left, present cells untouched.  Inputs and their references come
from tests/test_knn_reference.py (built once per process; each has zero undecided cells)."""
import numpy as np
import pytest
import torch

from hfens.models import imputer as imp_mod
from hfens.models.imputer import KNNImputer

from test_knn_reference import (MISS_COUNTS, SWEEP, VARIANT_SHAPES, assert_imputed, reference, reference_of)

pytestmark = pytest.mark.gpu


def _fit(dev, fit):
    return KNNImputer(n_neighbors=1).fit(torch.tensor(fit).to(dev))


def _impute(dev, fit, X):
    return _fit(dev, fit).transform(torch.tensor(X).to(dev)).cpu().numpy()


def _check(dev, name):
    fit, X, ref, mean_mask, _ = reference(name)
    out = _impute(dev, fit, X)
    assert_imputed(out, fit, X, ref, mean_mask)
    return out


def _donor_cells(X, fit, mean_mask):
    keep = ~np.isnan(fit).all(0)
    return np.isnan(X[:, keep]) & ~mean_mask


# ----------------------------------------------------------------------------- a. shapes
@pytest.mark.parametrize("F,nd,n", SWEEP)
def test_shape_sweep(dev, F, nd, n):
    _check(dev, f"sweep-{F}-{nd}-{n}")


# ----------------------------------------------------------------------------- b. kernel variants
@pytest.mark.parametrize("plan", [True, False])
@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("kernel", [None, "direct", "lds"])
@pytest.mark.parametrize("F,nd,n", VARIANT_SHAPES)
def test_kernel_variants(dev, monkeypatch, F, nd, n, kernel, mfma, plan):
    """Direct / packed-FMA (SM where F % 4 == 0) / LDS-tile search, the matrix-core filter (skipped
    above F = 48: F = 49 must still be right), device- and host-planned."""
    if kernel is None:
        monkeypatch.delenv("HFENS_KNN_KERNEL", raising=False)
    else:
        monkeypatch.setenv("HFENS_KNN_KERNEL", kernel)
    monkeypatch.setattr(imp_mod, "MFMA_FILTER", mfma)
    monkeypatch.setattr(imp_mod, "DEVICE_PLAN", plan)
    _check(dev, f"sweep-{F}-{nd}-{n}")


# ----------------------------------------------------------------------------- c. missing patterns
@pytest.mark.parametrize("plan", [True, False])
@pytest.mark.parametrize("F", [24, 64])
def test_missing_patterns(dev, monkeypatch, F, plan):
    monkeypatch.setattr(imp_mod, "DEVICE_PLAN", plan)
    fit, X, ref, mean_mask, _ = reference(f"patterns-{F}")
    # what the case is there to cover, from the inputs and the reference's mask
    counts = np.isnan(X).sum(1)
    per_class = {k: int((counts == k).sum()) for k in MISS_COUNTS(F)}
    print("rows per missing-count class", per_class, "column-mean cells", int(mean_mask.sum()))
    assert all(v >= 6 for v in per_class.values())
    assert np.isnan(X[:, 0]).any() and np.isnan(X[:, F - 1]).any()          # (F = 64: mask bit 63)
    assert np.isnan(fit).all(1).any()                                       # an all-NaN fit row
    assert np.isnan(fit).all(0).sum() == 1 and ref.shape[1] == F - 1        # a dropped column
    assert ((~np.isnan(fit)).sum(0) == 1).any()                             # a one-donor column
    lone = [r for r in np.nonzero(counts == F - 1)[0] if not np.isnan(X[r, 11])]
    assert any(mean_mask[r, 8] and not mean_mask[r].all() for r in lone)    # no candidate shares its feature
    assert mean_mask.sum() >= 1
    imp = _fit(dev, fit)
    out = imp.transform(torch.tensor(X).to(dev)).cpu().numpy()
    assert_imputed(out, fit, X, ref, mean_mask)
    # a receiver matrix with no NaN: zero receivers, the kept columns come back untouched
    full = np.random.default_rng(F).standard_normal((20, F))
    out = imp.transform(torch.tensor(full).to(dev)).cpu().numpy()
    assert_imputed(out, fit, full, full[:, ~np.isnan(fit).all(0)], np.zeros((20, F - 1), dtype=bool))


# ----------------------------------------------------------------------------- d. exact ties
@pytest.mark.parametrize("mfma", ["auto", "1"])
@pytest.mark.parametrize("F", [5, 12])
def test_exact_ties_lowest_index(dev, monkeypatch, F, mfma):
    monkeypatch.setattr(imp_mod, "MFMA_FILTER", mfma)
    fit, X, ref, mean_mask, ties = reference(f"binary-{F}")
    cells = int(_donor_cells(X, fit, mean_mask).sum())
    print(f"binary-{F}: {ties} tie cells of {cells} donor cells, {int(mean_mask.sum())} column-mean cells")
    assert ties >= 0.9 * cells
    _check(dev, f"binary-{F}")


@pytest.mark.parametrize("kernel", [None, "direct", "lds"])
def test_f32_search_ties_lowest_index(dev, monkeypatch, kernel):
    """The cases above pass through the f64 refine, which re-decides every tie and so would hide a
    wrong tie-break of the f32 search.  Here the refine is off (EXACT off) and the input's f32
    distances are exact (binary_balanced): the search's own slot update must keep the lowest index."""
    if kernel is None:
        monkeypatch.delenv("HFENS_KNN_KERNEL", raising=False)
    else:
        monkeypatch.setenv("HFENS_KNN_KERNEL", kernel)
    monkeypatch.setattr(imp_mod, "EXACT", False)
    fit, X, ref, mean_mask, ties = reference("binary-balanced")
    cells = int(_donor_cells(X, fit, mean_mask).sum())
    print(f"binary-balanced: {ties} tie cells of {cells} donor cells")
    assert not np.isnan(fit).any() and (fit.mean(0) == 0.5).all() and ties >= 0.5 * cells
    _check(dev, "binary-balanced")


# ----------------------------------------------------------------------------- e. the f64 refine
def _pair_winners(name):
    """(cells won by the lower index 2k, by the higher index 2k+1) in the reference of a pairs case."""
    fit, X, ref, mean_mask, _ = reference(name)
    cells = _donor_cells(X, fit, mean_mask)
    lo = hi = 0
    for c in range(ref.shape[1]):
        v = ref[cells[:, c], c]
        lo += int(np.isin(v, fit[0::2, c]).sum())
        hi += int(np.isin(v, fit[1::2, c]).sum())
    assert lo + hi == int(cells.sum())
    return lo, hi


@pytest.mark.parametrize("name", ["pairs-hi", "pairs-lo"])
def test_refine_both_passes(dev, monkeypatch, name):
    """Donor pairs 1e-9 apart: the f32 search ties them (lower index first); where the higher index
    is strictly closer in f64 the refine's pass 1 must move the donor, elsewhere pass 0 keeps it."""
    monkeypatch.setattr(imp_mod, "KNN_DEBUG", True)
    imp_mod.LAST_REFINE.clear()
    lo, hi = _pair_winners(name)
    assert lo >= 1 and hi >= 1
    _check(dev, name)
    pass1 = sum(t[4] for t in imp_mod.LAST_REFINE)
    print(f"{name}: lower index wins {lo} cells, higher {hi}; refine pass-1 receivers {pass1}; "
          f"re-scanned {sum(t[1] for t in imp_mod.LAST_REFINE)}, pairs {sum(t[2] for t in imp_mod.LAST_REFINE)}")
    assert pass1 >= 1
    assert all(t[3] == 0 for t in imp_mod.LAST_REFINE)       # (no overflow here: the parallel pair list)


@pytest.mark.parametrize("name", ["pairs-hi", "pairs-lo"])
def test_refine_is_needed(dev, monkeypatch, name):
    """Negative control: the f32-only search (EXACT off) gets at least one donor cell of the same
    input wrong, so the case above passes only because of the f64 refine."""
    monkeypatch.setattr(imp_mod, "EXACT", False)
    fit, X, ref, mean_mask, _ = reference(name)
    out = _impute(dev, fit, X)
    assert out.shape == ref.shape
    differ = int((_donor_cells(X, fit, mean_mask) & (out != ref)).sum())
    print(f"{name}: {differ} donor cells differ without the refine")
    assert differ >= 1


# ----------------------------------------------------------------------------- f. refine overflow
@pytest.mark.parametrize("plan,mfma", [(True, "0"), (True, "1"), (False, "0")])
@pytest.mark.parametrize("name", ["binary-5", "pairs-hi", "pairs-lo"])
def test_refine_overflow_fallback(dev, monkeypatch, name, plan, mfma):
    """The pair list capped at 64 entries: the window pairs overflow it and the serial fallback
    (knn_cand_kernel MODE 1, and MODE 2 where pass 1 is needed) decides — same donors.  The pairs
    cases list two pairs per slot, fewer than the 16 per row the cap otherwise grows by, so the
    per-row term is switched off for them."""
    monkeypatch.setattr(imp_mod, "REFINE_CAP_MIN", 64)
    if name.startswith("pairs"):
        monkeypatch.setattr(imp_mod, "REFINE_CAP_PER_ROW", 0)
    monkeypatch.setattr(imp_mod, "KNN_DEBUG", True)
    monkeypatch.setattr(imp_mod, "MFMA_FILTER", mfma)
    monkeypatch.setattr(imp_mod, "DEVICE_PLAN", plan)
    imp_mod.LAST_REFINE.clear()
    _check(dev, name)
    overflow = sum(t[3] for t in imp_mod.LAST_REFINE)
    print(f"{name} plan={plan} mfma={mfma}: overflow in {overflow} of {len(imp_mod.LAST_REFINE)} refine calls, "
          f"pairs {[t[2] for t in imp_mod.LAST_REFINE]}, pass-1 receivers {[t[4] for t in imp_mod.LAST_REFINE]}")
    assert overflow >= 1


# ----------------------------------------------------------------------------- g. scale
@pytest.mark.parametrize("plan", [True, False])
def test_large_magnitudes(dev, monkeypatch, plan):
    """One column × 1e12, one at 1e9 + 1e-6·N(0,1): ‖m‖ ≈ 1e13 in the refine's error window, where
    the expanded ‖x‖² + ‖y‖² − 2x·y form (sklearn's) no longer finds the donors."""
    monkeypatch.setattr(imp_mod, "DEVICE_PLAN", plan)
    _check(dev, "scaled")


# ----------------------------------------------------------------------------- h. call shapes
def test_noncontiguous_receivers(dev):
    fit, X, ref, mean_mask, _ = reference("sweep-17-257-65")
    wide = torch.tensor(np.hstack([X[:, :2], X, X[:, :3]])).to(dev)
    sliced = wide[:, 2:2 + X.shape[1]]                   # a column slice of a wider tensor
    turned = torch.tensor(np.ascontiguousarray(X.T)).to(dev).t()   # dense, column-major
    assert not sliced.is_contiguous() and not turned.is_contiguous()
    imp = _fit(dev, fit)
    for view in (sliced, turned):
        before = view.clone()
        assert_imputed(imp.transform(view).cpu().numpy(), fit, X, ref, mean_mask)
        assert torch.equal(torch.isnan(view), torch.isnan(before))     # the caller's tensor is not written


def test_float32_receivers(dev):
    fit, X, _, _, _ = reference("sweep-17-257-65")
    X32 = X.astype(np.float32)
    Xp = X32.astype(np.float64)                          # what as_tensor promotes it to
    ref, mean_mask, _ = reference_of(fit, Xp)
    out = _fit(dev, fit).transform(torch.tensor(X32).to(dev))
    assert out.dtype == torch.float64
    assert_imputed(out.cpu().numpy(), fit, Xp, ref, mean_mask)


@pytest.mark.parametrize("plan", [True, False])
@pytest.mark.parametrize("defer", [False, True])
def test_transform_many_side_stream(dev, monkeypatch, defer, plan):
    monkeypatch.setattr(imp_mod, "DEVICE_PLAN", plan)
    fit, A, refA, maskA, _ = reference("sweep-17-257-65")
    B = reference("sweep-17-33-1")[1]
    B = np.vstack([B, A[::-1][:40]])                     # another matrix, another row count
    refB, maskB, _ = reference_of(fit, B)
    side = torch.cuda.Stream(device=dev)
    got = _fit(dev, fit).transform_many([torch.tensor(A).to(dev), torch.tensor(B).to(dev)],
                                        streams=[None, side], defer=defer)
    if defer:
        outs, run = got
        assert outs[1] is None
        got = run()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert_imputed(got[0].cpu().numpy(), fit, A, refA, maskA)
    assert_imputed(got[1].cpu().numpy(), fit, B, refB, maskB)
