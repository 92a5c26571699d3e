"""The longdouble brute-force 1-NN imputation (ops/reference.py knn_impute1) as an oracle that
shares nothing with the kernels: checked here against sklearn (well-scaled, tie-free inputs) and
against the host path on every input that tests/test_knn_reference_gpu.py runs on the device.

The input constructions live here and are imported by the GPU module; every one of them must
have ZERO undecided cells (a candidate with another value within relative 2⁻⁴⁵ above the
minimum) — ``reference()`` asserts it, so a seed that violates it fails loudly."""
import functools

import numpy as np
import pytest
import torch

from hfens.models.imputer import KNNImputer
from hfens.ops.reference import knn_impute1

# (F, donors, receivers): every F of the kernels' bucket edges (16/32/40/48/64, F % 4, padded F ≤ 40,
# matrix-core buckets 16/24/32/40/48), every donor count around the 32 / 224 / 256-row tiles and the
# split threshold, every receiver count around the 64-lane ballots and the 256-row plan blocks; each
# F bucket meets more than one donor split (nd > 256) at least once
SWEEP = [
    (1, 257, 63), (2, 31, 65), (4, 513, 1), (5, 2, 255), (8, 223, 257), (9, 225, 600),
    (16, 255, 63), (17, 257, 65), (24, 449, 255), (25, 1, 257), (32, 33, 600), (33, 513, 257),
    (40, 223, 63), (41, 255, 65), (48, 257, 255), (49, 513, 257), (63, 449, 600), (64, 257, 65),
    (1, 2, 600), (2, 449, 1), (4, 223, 257), (5, 225, 65), (8, 1, 63), (9, 513, 255),
    (16, 257, 600), (17, 33, 1), (24, 225, 63), (25, 255, 600), (32, 513, 65), (33, 223, 255),
    (40, 449, 600), (41, 257, 257), (48, 31, 1), (49, 2, 63), (63, 255, 1), (64, 1, 255),
]
VARIANT_SHAPES = [(16, 255, 63), (17, 257, 65), (40, 449, 600), (41, 257, 257), (48, 257, 255), (49, 513, 257)]


def _holes(rng, A, frac):
    A[rng.random(A.shape) < frac] = np.nan
    return A


def continuous(F, nd, n, seed=None):
    """N(0,1) donors with ≈ 15 % NaN, other N(0,1) receivers with ≈ 25 % NaN (at least one)."""
    rng = np.random.default_rng(1000 * F + 7 * nd + n if seed is None else seed)
    fit = _holes(rng, rng.standard_normal((nd, F)), 0.15)
    X = _holes(rng, rng.standard_normal((n, F)), 0.25)
    X[n // 2, (nd + n) % F] = np.nan
    return fit, X


MISS_COUNTS = lambda F: (0, 1, 8, 9, 16, 17, F - 1, F)   # noqa: E731  (slot groups of 8)


def patterns(F):
    """The crafted missing patterns: receivers with exactly 0/1/8/9/16/17/F−1/F missing columns (six rows
    each; the first of each class misses column 0 first, the second column F−1), a fit matrix with
    an all-NaN row (3), an all-NaN column (5), a one-donor column (7), and a column (9) whose every
    candidate lacks column 11 — the receiver that has only column 11 gets its mean."""
    rng = np.random.default_rng(40 + F)
    fit = _holes(rng, rng.standard_normal((40, F)), 0.10)
    fit[:, 5] = np.nan
    fit[:, 7] = np.nan
    fit[10, 7] = 0.625
    fit[:, 11] = np.nan
    fit[0:5, 11] = rng.standard_normal(5)
    fit[0:5, 9] = np.nan
    fit[5:9, 9] = rng.standard_normal(4)
    fit[3, :] = np.nan
    rows = []
    for k in MISS_COUNTS(F):
        for i in range(6):
            x = rng.standard_normal(F)
            first = {0: [0], 1: [F - 1]}.get(i, [])[:k]
            rest = [c for c in rng.permutation(F) if c not in first]
            x[np.array(first + rest[:k - len(first)], dtype=np.int64)] = np.nan
            rows.append(x)
    lone = np.full(F, np.nan)
    lone[11] = 0.25
    rows.append(lone)
    X = np.array(rows)
    return fit, X[rng.permutation(X.shape[0])]


def binary(F):
    """All-0/1 data (300 donors, 200 receivers): every distance is a small rational and nearly every
    cell an exact tie (at F = 12 the ones are sparse: fair bits give 4096 patterns for 300 donors and
    a tie in only 3 cells of 4)."""
    rng = np.random.default_rng(500 + F)
    p1 = 0.5 if F <= 8 else 0.12
    fit = _holes(rng, (rng.random((300, F)) < p1).astype(np.float64), 0.15)
    X = _holes(rng, (rng.random((200, F)) < p1).astype(np.float64), 0.25)
    return fit, X


def binary_balanced():
    """Complete 0/1 donors (300 × 12) with exactly 150 ones per column, 200 receivers with ≈ 25 % NaN.
    The column means are 0.5, so the centred f32 values are ±0.5 exactly, and with complete donors a
    receiver's F/|common| is the same for every donor: the f32 distances are exact multiples of one
    constant, ties are exact in f32 too, and the f32 search ALONE must find the lowest index."""
    rng = np.random.default_rng(512)
    fit = np.stack([rng.permutation(np.repeat([0.0, 1.0], 150)) for _ in range(12)], axis=1)
    X = _holes(rng, rng.integers(0, 2, (200, 12)).astype(np.float64), 0.25)
    return fit, X


def pairs(a, b):
    """Donor rows 2k / 2k+1 = Z_k + a·s_k / Z_k + b·s_k (one NaN pattern per pair): the two round to
    the same centred f32 almost everywhere, so only an f64 evaluation separates them.  Receivers
    Z_j + 0.05·s_0·|N(0,1)|."""
    rng = np.random.default_rng(17)
    Z = rng.standard_normal((150, 17))
    s = rng.choice([-1.0, 1.0], size=(150, 17))
    hole = rng.random((150, 17)) < 0.10
    fit = np.empty((300, 17))
    fit[0::2] = np.where(hole, np.nan, Z + a * s)
    fit[1::2] = np.where(hole, np.nan, Z + b * s)
    X = _holes(rng, Z + 0.05 * s[0] * np.abs(rng.standard_normal((150, 17))), 0.25)
    return fit, X


def scaled():
    """F = 17, column 3 × 1e12, column 11 = 1e9 + 1e-6·N(0,1), the rest N(0,1); 300 donors, 200 receivers."""
    rng = np.random.default_rng(1712)
    def make(n, frac):
        A = rng.standard_normal((n, 17))
        A[:, 3] *= 1e12
        A[:, 11] = 1e9 + 1e-6 * A[:, 11]
        return _holes(rng, A, frac)
    return make(300, 0.15), make(200, 0.25)


CASES = {f"sweep-{F}-{nd}-{n}": functools.partial(continuous, F, nd, n) for F, nd, n in SWEEP}
CASES.update({"patterns-24": functools.partial(patterns, 24), "patterns-64": functools.partial(patterns, 64),
              "binary-5": functools.partial(binary, 5), "binary-12": functools.partial(binary, 12),
              "binary-balanced": binary_balanced,
              "pairs-hi": functools.partial(pairs, 2e-9, 1e-9), "pairs-lo": functools.partial(pairs, 1e-9, 2e-9),
              "scaled": scaled})
WELL_SCALED = [k for k in CASES if k.startswith("sweep")]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fit, X, ref, mean_mask, n_ties) of a named case — computed once per process, read-only."""
    fit, X = CASES[name]()
    ref, mean_mask, ties, undecided = knn_impute1(fit, X)
    assert undecided == 0, f"{name}: {undecided} undecided cells — pick another seed"
    for a in (fit, X, ref, mean_mask):
        a.setflags(write=False)
    return fit, X, ref, mean_mask, ties


def reference_of(fit, X):
    ref, mean_mask, ties, undecided = knn_impute1(fit, X)
    assert undecided == 0
    return ref, mean_mask, ties


def assert_imputed(out, fit, X, ref, mean_mask):
    """``out`` against the reference: shape; donor cells bit-equal; column-mean cells within
    n_c·2⁻⁵²·mean|x_c| (recursive-summation bound of two summation orders over the n_c present
    fit values); no NaN; the cells that were present unchanged bit for bit."""
    out = np.ascontiguousarray(out, dtype=np.float64)
    assert out.shape == ref.shape
    assert not np.isnan(out).any()
    keep = ~np.isnan(fit).all(0)
    Xk = np.ascontiguousarray(np.asarray(X, dtype=np.float64)[:, keep])
    was = ~np.isnan(Xk)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)   # noqa: E731
    assert np.array_equal(bits(out)[was], bits(Xk)[was]), "present cells changed"
    donor = ~was & ~mean_mask
    bad = donor & (bits(out) != bits(ref))
    assert not bad.any(), f"{int(bad.sum())} of {int(donor.sum())} donor cells differ, first at {np.argwhere(bad)[0]}"
    fk = fit[:, keep]
    n_c = (~np.isnan(fk)).sum(0)
    bound = n_c * 2.0 ** -52 * np.nansum(np.abs(fk), 0) / np.maximum(n_c, 1)
    err = np.where(mean_mask, np.abs(out - ref), 0.0)
    assert (err <= bound[None, :]).all(), f"column-mean cells off by up to {err.max()}"


def host_impute(fit, X):
    return KNNImputer(n_neighbors=1).fit(torch.tensor(fit)).transform(torch.tensor(X)).numpy()


# ----------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", WELL_SCALED)
def test_reference_matches_sklearn(name):
    SK = pytest.importorskip("sklearn.impute").KNNImputer
    fit, X, ref, mean_mask, ties = reference(name)
    assert ties == 0
    theirs = SK(n_neighbors=1).fit(fit).transform(X)
    assert theirs.shape == ref.shape
    assert (np.abs(theirs - ref) <= 1e-12 * (1 + np.abs(ref))).all()


@pytest.mark.parametrize("name", list(CASES))
def test_host_path_matches_reference(name):
    fit, X, ref, mean_mask, _ = reference(name)
    assert_imputed(host_impute(fit, X), fit, X, ref, mean_mask)


def test_reference_by_hand():
    """Three donors, worked by hand: scaling by F/|common|, the candidate rule, the lowest index on
    an exact tie, the column mean, a dropped column."""
    nan = np.nan
    fit = np.array([[0.0, 1.0, nan, 5.0],
                    [3.0, nan, nan, 7.0],
                    [0.0, 1.0, nan, 9.0]])
    X = np.array([[0.1, 1.0, 2.0, nan],      # d² to rows 0 and 2: 4/2·0.01 (tie → row 0); row 1: 4/1·2.9²
                  [2.9, nan, nan, nan],      # row 1: 4·0.01 beats rows 0/2: 4·2.9²
                  [nan, nan, 1.0, nan],      # only column 2 present, no donor has it: column means
                  [nan, 4.0, nan, 6.0]])     # col 0: row 0 (F/2·(9+1)=20) and 2 (F/2·(9+9)) vs row 1 (4/1·1): row 1
    out, mean_mask, ties, undecided = knn_impute1(fit, X)
    assert out.tolist() == [[0.1, 1.0, 5.0], [2.9, 1.0, 7.0], [1.0, 1.0, 7.0], [3.0, 4.0, 6.0]]
    assert mean_mask.tolist() == [[False] * 3, [False] * 3, [True] * 3, [False] * 3]
    assert (ties, undecided) == (2, 0)       # (0, 3) and (1, 1): rows 0 and 2 at the same distance


def test_reference_flags_undecided():
    fit = np.array([[1.0, 10.0], [1.0 + 2.0 ** -50, 20.0], [1.0 + 2.0 ** -50, 10.0]])
    X = np.array([[0.0, np.nan]])
    assert knn_impute1(fit, X)[3] == 1                       # row 1 (another value) within 2⁻⁴⁵
    assert knn_impute1(fit[[0, 2]], X)[3] == 0               # the same value: either donor will do
    assert knn_impute1(fit * [1.0, 1.0] + [[0.0, 0.0], [0.5, 0.0], [0.5, 0.0]], X)[3] == 0


def test_patterns_preconditions():
    for F in (24, 64):
        fit, X, ref, mean_mask, _ = reference(f"patterns-{F}")
        counts = np.isnan(X).sum(1)
        assert all(int((counts == k).sum()) >= 6 for k in MISS_COUNTS(F))
        assert np.isnan(X[:, 0]).any() and np.isnan(X[:, F - 1]).any()
        assert np.isnan(fit).all(1).any() and np.isnan(fit).all(0).sum() == 1 and ref.shape[1] == F - 1
        assert ((~np.isnan(fit)).sum(0) == 1).any()
        assert mean_mask.sum() >= 1
        # the receiver with only column 11: column 9 (kept index 8) has no candidate, others do
        lone = np.nonzero(counts == F - 1)[0]
        lone = [r for r in lone if not np.isnan(X[r, 11])]
        assert any(mean_mask[r, 8] and not mean_mask[r].all() for r in lone)


@pytest.mark.parametrize("F", [5, 12])
def test_binary_preconditions(F):
    fit, X, ref, mean_mask, ties = reference(f"binary-{F}")
    assert set(np.unique(fit[~np.isnan(fit)])) == {0.0, 1.0} and fit.shape == (300, F) and X.shape == (200, F)
    assert ties >= 0.9 * int((np.isnan(X) & ~mean_mask).sum())
