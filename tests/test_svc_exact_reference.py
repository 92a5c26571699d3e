"""The exact-SMO SVC oracles (ops/reference.py: gram_kernel_error, smo_oracle, platt_oracle,
gamma_oracle) proved on the CPU: against the installed sklearn (libsvm), against the host mirrors of
models/smo.py, against wrong variants of themselves and against numpy emulations of the kernels'
f32 expressions.  The builders of the crafted problems live here and are shared with the GPU side,
tests/test_svc_exact_reference_gpu.py."""
import numpy as np
import pytest

from hfens.models import smo
from hfens.ops import reference as R

EPS = 1e-3
MAX_ITER = 10 ** 7
GRAM_LS = (1, 2, 63, 64, 65, 129)
GRAM_FS = (1, 2, 7, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 64)


# ------------------------------------------------------------------------------------ builders
def ngl2e_of(F):
    """The stored f32 scale of γ = 1/F."""
    return np.float32(-R.LOG2E / F)


def gram_rows(l, F, seed):
    """f32 rows for the Gram tests: standard normal, then (as far as l allows) row 1 = row 0 (an
    off-diagonal d² of 0), row 2 = row 0 + 40 (2^(ngl2e·d²) underflows), rows 4 and 5 with norms near
    1e3 and a difference of O(1) (clamp and cancellation), rows 6 and 7 the same 1e-3 apart (the
    computed d² is rounding noise of either sign), and four rows of small integers (every
    intermediate exact, see gram_kernel_error)."""
    rng = np.random.default_rng(seed)
    Z = rng.normal(size=(l, F)).astype(np.float32)
    if l >= 2:
        Z[1] = Z[0]
    if l >= 3:
        Z[2] = Z[0] + np.float32(40)
    if l >= 8:
        base = np.float32(1e3 / np.sqrt(F)) + rng.normal(size=F).astype(np.float32)
        Z[4] = base
        Z[5] = base + rng.normal(size=F).astype(np.float32)
        Z[6] = base
        Z[7] = base + np.float32(1e-3)
    if l >= 16:
        hi = 8 if F > 1 else 3
        Z[8:12] = rng.integers(-hi, hi + 1, size=(4, F)).astype(np.float32)
    return Z


def _fma32(a, b, c):
    """fl32(a·b + c): the product of two f32 is exact in f64, the sum is rounded to f64 and then to
    f32 (a double rounding that differs from one fma rounding only on exact f64 half-way cases)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gram_emul(Z32, ngl2e, clamp=True):
    """gram_rbf_kernel's expression in numpy f32: k-ordered fma chains for the norms and the dot
    products, d2 = fma(−2, dot, fl(na + nb)), the clamp, exp2(fl(ngl2e·d2)) flushed below 2⁻¹²⁶, and
    the diagonal forced to 1."""
    Z = np.asarray(Z32, dtype=np.float32)
    l, F = Z.shape
    n = np.zeros(l, np.float32)
    dot = np.zeros((l, l), np.float32)
    for k in range(F):
        n = _fma32(Z[:, k], Z[:, k], n)
        dot = _fma32(Z[:, k][:, None] * np.ones((1, l), np.float32), Z[:, k][None, :] * np.ones((l, 1), np.float32),
                     dot)
    s = (n[:, None] + n[None, :]).astype(np.float32)
    d2 = _fma32(np.full((l, l), -2, np.float32), dot, s)
    if clamp:
        d2 = np.maximum(d2, np.float32(0))
    e = (np.float32(ngl2e) * d2).astype(np.float32)
    with np.errstate(under="ignore", over="ignore"):
        K = np.exp2(e.astype(np.float64))
    K = np.where(K < 2.0 ** -126, 0.0, K).astype(np.float32)
    np.fill_diagonal(K, 1.0)
    return K


def _cohort(l, F, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(l, F))
    w = rng.normal(size=F)
    y = (X @ w / F ** 0.5 + 0.5 * rng.normal(size=l) - 0.5) > 0
    if y.all() or not y.any():
        y[0], y[-1] = True, False
    Z = ((X - X.mean(0)) / X.std(0)).astype(np.float32)
    order = np.argsort(~y, kind="stable")
    return Z[order], int(y.sum())


def smo_problem(kind, l, seed=0, F=5):
    """``(Z32, npos, Cp, Cn)``, positives first, Cp ≠ Cn throughout.

    gauss: a standardised Gaussian cohort with noisy linear labels.  npos1 / nposl1: one positive /
    one negative.  dup_opposite: the first points of each class are the same rows (2 + 2Q_ij = 0: τ
    in the update).  dup_equal: every class made of groups of four rows 1e-4 apart (K_ij rounds to 1,
    2 − 2K_ij = 0: τ in the selection, with several such candidates at once).  all_bound: twice as
    many negatives as positives, Cp = 2Cn = 2⁻⁹, so every α ends at its bound and Σ yα = 0 holds
    exactly there: no free vector.  clusters: two classes 8 apart, few support vectors."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "clusters":
        npos = l // 2
        Z = rng.normal(size=(l, F))
        Z[:npos] += 8.0 / np.sqrt(F)
        return Z.astype(np.float32), npos, 1.5, 0.75
    Z, npos = _cohort(l, F, seed + l)
    if kind == "npos1":
        npos = 1
    elif kind == "nposl1":
        npos = l - 1
    elif kind == "all_bound":
        npos = l // 3
        Z = np.concatenate([Z[:npos], Z[npos:npos + 2 * npos]])
        return Z, npos, 2.0 ** -9, 2.0 ** -10
    elif kind == "dup_opposite":
        k = max(1, min(8, npos, l - npos))
        Z[npos:npos + k] = Z[:k]
    elif kind == "dup_equal":
        for lo, hi in ((0, npos), (npos, l)):
            for c in range(lo, hi - 3, 4):
                for k in range(1, 4):
                    Z[c + k] = Z[c] + np.float32(1e-4) * rng.normal(size=F).astype(np.float32)
    else:
        assert kind == "gauss", kind
    return Z, npos, 1.0 * l / (2.0 * npos), 0.7 * l / (2.0 * (l - npos))


CPU_PROBLEMS = [("gauss", 300), ("gauss", 2), ("gauss", 3), ("npos1", 40), ("nposl1", 40), ("dup_opposite", 60),
                ("dup_equal", 60), ("dup_equal", 120), ("all_bound", 60), ("clusters", 80)]
SKLEARN_PROBLEMS = CPU_PROBLEMS


def problem_gram(kind, l):
    Z, npos, Cp, Cn = smo_problem(kind, l)
    return gram_emul(Z, ngl2e_of(Z.shape[1])), npos, Cp, Cn


# Platt inputs.  The kernel assembles d = −(Σ_s part[row][s] − ρ_k) from f32 partials, or takes a
# per-fold constant (source-map code < 0): a case carries those tables, platt_dec() is the same
# assembly in numpy f64 (S = 2 partials of f32: their f64 sum is exact, the subtraction rounds once).
PLATT_CONSTS = np.array([0.0, 0.7, -1.3])
PLATT_RHO = np.array([0.0, 0.125])
PLATT_LS = (1, 2, 1023, 1025, 16384, 16385)
# the one listed input that is NOT compared with platt_oracle by value: a constant decision value
# makes the Hessian singular up to the ridge, f64 does not determine the Newton direction, and
# the oracle reports the run undecided.  Every other input must be decided (platt_by_value()).
PLATT_UNDECIDED = ("const",)


def platt_case(name, seed_override=None):
    """``dict(part [l, 2] f32, rowk [l] i32, srcmap [l] i32, n0)``: positions < n0 carry label +1."""
    ls = {"allpos": 1023, "allneg": 1023, "separable": 1025, "const": 1023, "huge": 1025}
    l = ls[name] if name in ls else int(name[5:])
    seed = {"gauss1": 1, "gauss2": 2, "gauss1023": 101, "gauss1025": 101, "gauss16384": 103, "gauss16385": 103,
            "allpos": 7, "allneg": 8, "separable": 100, "const": 10, "huge": 124}[name]
    rng = np.random.default_rng(seed if seed_override is None else seed_override)
    n0 = {"allpos": l, "allneg": 0}.get(name, max(1, int(0.3 * l)) if l > 1 else 1)
    lab = np.where(np.arange(l) < n0, 1.0, -1.0)
    if name == "separable":
        v = lab * (1.0 + np.abs(rng.normal(size=l)))
    elif name == "const":
        v = np.full(l, 0.3)
    elif name == "huge":
        v = (0.8 * lab + 1.5 * rng.normal(size=l)) * np.exp(rng.uniform(0, np.log(1e4), size=l))
        v[:4] = [1e4, -1e4, 9999.5, -1e4]
    else:
        v = 0.8 * lab + 1.5 * rng.normal(size=l)
    srcmap = rng.permutation(l).astype(np.int32)
    part = np.zeros((l, 2), np.float32)
    part[srcmap, 0] = (-v).astype(np.float32)          # position i reads partial row srcmap[i]
    part[:, 1] = 0.0 if name == "const" else (1e-3 * rng.normal(size=l)).astype(np.float32)
    rowk = rng.integers(0, 2, size=l).astype(np.int32)
    if name == "const":
        rowk[:] = 0
    if l >= 1023 and name not in ("const", "separable"):
        srcmap[5], srcmap[n0 + 1 if n0 + 1 < l else 6], srcmap[l - 1] = -1, -2, -3   # the three constant codes
    return dict(name=name, part=part, rowk=rowk, srcmap=srcmap, n0=n0, l=l)


def platt_dec(c):
    sm = c["srcmap"]
    r = np.maximum(sm, 0)
    p = c["part"].astype(np.float64)
    d = -((p[r, 0] + p[r, 1]) - PLATT_RHO[c["rowk"][r]])
    dec = np.where(sm >= 0, d, PLATT_CONSTS[np.where(sm < 0, -1 - sm, 0)])
    return dec, np.where(np.arange(c["l"]) < c["n0"], 1.0, -1.0)


PLATT_NAMES = ["gauss%d" % l for l in PLATT_LS] + ["allpos", "allneg", "separable", "const", "huge"]
# the summation depth the f64 evaluation bounds assume: 16 values per thread + 6 wave levels + 16 wave
# totals + 8 workgroup totals = 46 in the deepest kernel (numpy's pairwise sum is shallower); the seeds
# above were chosen so that every by-value input is decided at this depth
PLATT_DEPTH = 48
# platt_oracle in longdouble against the same code in float64 over the by-value inputs, relative to
# max(1, |A|, |B|): measured 1.08e-15 (the separable input; the others are below 3e-16), recorded as
# 1.1e-15.  The GPU suite allows ten times the recorded figure.
PLATT_MEASURED = 1.1e-15
PLATT_MARGIN = 10 * PLATT_MEASURED


_platt_cache = {}


def platt_ref(name):
    if name not in _platt_cache:
        c = platt_case(name)
        dec, lab = platt_dec(c)
        _platt_cache[name] = (c, dec, lab, R.platt_oracle(dec, lab, depth=PLATT_DEPTH),
                              R.platt_oracle(dec, lab, dtype=np.float64, depth=PLATT_DEPTH))
    return _platt_cache[name]


def platt_by_value():
    """The inputs compared with platt_oracle by value: those the oracle itself reports decided."""
    return [n for n in PLATT_NAMES if platt_ref(n)[3].decided]


def platt_margin():
    """The reference-against-reference figure: max over the by-value inputs of the
    longdouble-vs-float64 difference of (A, B), relative to max(1, |A|, |B|)."""
    worst = 0.0
    for name in platt_by_value():
        _, _, _, o, o64 = platt_ref(name)
        sc = max(1.0, abs(float(o.A)), abs(float(o.B)))
        worst = max(worst, abs(float(o.A - o64.A)) / sc, abs(float(o.B - o64.B)) / sc)
    return worst


# ------------------------------------------------------------------------------------ smo_oracle
def _sk_fit(K, npos, Cp, Cn):
    from sklearn.svm import SVC
    l = K.shape[0]
    # sklearn's libsvm sorts the class labels, and the smaller one is libsvm's +1 class: label 0 for
    # the positives keeps libsvm's internal order equal to ours (positives first)
    lab = (np.arange(l) >= npos).astype(int)
    m = SVC(kernel="precomputed", C=1.0, class_weight={0: Cp, 1: Cn}, shrinking=False, tol=EPS)
    m.fit(K.astype(np.float64), lab)
    return m


def _sk_mismatch(o, m, npos):
    """Where an SMO result departs from sklearn's fit of the same matrix (empty: nowhere)."""
    bad = []
    sv = np.flatnonzero(o.alpha != 0)
    y = np.where(np.arange(o.alpha.size) < npos, 1.0, -1.0)
    # sklearn reports binary models from its class 1's side: dual_coef_ = −y·α, intercept_ = +ρ
    if not np.array_equal(sv, m.support_):
        bad.append("support")
    elif not np.array_equal(-(y * o.alpha)[sv], m.dual_coef_[0]):
        bad.append("dual_coef")
    if float(m.intercept_[0]) != o.rho:
        bad.append("rho")
    # libsvm counts the pair updates it made (++iter sits between the selection and the update) and
    # sklearn reports that count unchanged: the convention differs by the constant 0
    if int(m.n_iter_[0]) != o.iters:
        bad.append("n_iter")
    return bad


@pytest.mark.parametrize("kind,l", SKLEARN_PROBLEMS, ids=lambda v: str(v))
def test_smo_oracle_matches_sklearn_bit_for_bit(kind, l):
    K, npos, Cp, Cn = problem_gram(kind, l)
    o = R.smo_oracle(K, npos, Cp, Cn, EPS, MAX_ITER)
    m = _sk_fit(K, npos, Cp, Cn)
    assert _sk_mismatch(o, m, npos) == [], (kind, l, o.iters, int(m.n_iter_[0]))
    assert len(o.pairs) == o.iters and o.gap < EPS
    C = np.where(np.arange(l) < npos, Cp, Cn)
    assert ((o.alpha >= 0) & (o.alpha <= C)).all()
    # the drift bound is a bound: the incrementally updated G against Qα − 1 in longdouble
    L = np.longdouble
    y = np.where(np.arange(l) < npos, 1.0, -1.0).astype(L)
    Gs = -1 + y * (K.astype(L) @ (y * o.alpha.astype(L)))
    assert (np.abs(o.G.astype(L) - Gs) <= o.drift).all()
    assert o.drift.max() < 1e-9


@pytest.mark.parametrize("kind,l", CPU_PROBLEMS, ids=lambda v: str(v))
def test_smo_oracle_pins_the_host_mirror(kind, l):
    """models/smo.py::_smo_host — the mirror every device-against-host test leans on."""
    K, npos, Cp, Cn = problem_gram(kind, l)
    o = R.smo_oracle(K, npos, Cp, Cn, EPS, MAX_ITER)
    a, rho, it = smo._smo_host(K, npos, Cp, Cn, EPS, MAX_ITER)
    assert it == o.iters
    assert np.array_equal(a, o.alpha)
    free = (o.alpha > 0) & (o.alpha < np.where(np.arange(l) < npos, Cp, Cn))
    if free.any():
        # the mirror sums the free y·G pairwise, libsvm in index order: n·2⁻⁵³·Σ|yG| covers both
        assert abs(rho - o.rho) <= free.sum() * 2.0 ** -53 * np.abs(o.G[free]).sum()
    else:
        assert rho == o.rho


def test_smo_problems_reach_their_edges():
    """The crafted problems hit what they were built for."""
    K, npos, Cp, Cn = problem_gram("all_bound", 60)
    o = R.smo_oracle(K, npos, Cp, Cn, EPS, MAX_ITER)
    C = np.where(np.arange(K.shape[0]) < npos, Cp, Cn)
    assert (o.alpha == C).all()                                    # no free vector
    K, npos, Cp, Cn = problem_gram("dup_opposite", 60)
    assert (K[:npos, npos:] == 1).any()                            # 2 + 2Q_ij = 0
    o = R.smo_oracle(K, npos, Cp, Cn, EPS, MAX_ITER)
    assert any(K[i, j] == 1 and (i < npos) != (j < npos) for i, j in o.pairs)
    K, npos, Cp, Cn = problem_gram("dup_equal", 60)
    off = K - np.eye(K.shape[0], dtype=np.float32)
    assert (off[:npos, :npos] == 1).sum() >= 4 and (off[npos:, npos:] == 1).sum() >= 4
    K, npos, Cp, Cn = problem_gram("clusters", 80)
    o = R.smo_oracle(K, npos, Cp, Cn, EPS, MAX_ITER)
    assert 0 < (o.alpha > 0).sum() < 40


def _variant_case(variant):
    return {"ties_first": ("gauss", 300), "no_tau": ("dup_equal", 120), "clip_swapped": ("gauss", 300),
            "rho_ub": ("all_bound", 60), "stop_after_select": ("gauss", 300)}[variant]


@pytest.mark.parametrize("variant", R.SMO_VARIANTS)
def test_sklearn_comparison_rejects_wrong_variants(variant):
    """Each wrong rule, on an input built to hit it, departs from libsvm where it should."""
    kind, l = _variant_case(variant)
    K, npos, Cp, Cn = problem_gram(kind, l)
    m = _sk_fit(K, npos, Cp, Cn)
    good = R.smo_oracle(K, npos, Cp, Cn, EPS, MAX_ITER)
    assert _sk_mismatch(good, m, npos) == []
    bad = R.smo_oracle(K, npos, Cp, Cn, EPS, 20 * good.iters + 100, variant=variant)
    miss = _sk_mismatch(bad, m, npos)
    assert miss, variant
    if variant == "ties_first":
        # at α = 0 every positive ties at −yG = 1: libsvm takes the last one
        assert good.pairs[0][0] == npos - 1 and bad.pairs[0][0] == 0
    elif variant == "no_tau":
        # several zero curvatures at once: without the floor they all tie at −∞
        k = next(k for k, (p, q) in enumerate(zip(good.pairs, bad.pairs)) if p != q)
        i, j = bad.pairs[k]
        assert K[i, j] == 1 and good.pairs[k][0] == i and K[i, good.pairs[k][1]] == 1
    elif variant == "clip_swapped":
        C = np.where(np.arange(l) < npos, Cp, Cn)
        assert Cp != Cn and ("dual_coef" in miss or "support" in miss or (bad.alpha > C).any())
    elif variant == "rho_ub":
        assert np.array_equal(bad.alpha, good.alpha) and miss == ["rho"]
    else:
        assert bad.iters != good.iters and "n_iter" in miss


# ------------------------------------------------------------------------------------ platt_oracle
def test_platt_oracle_pins_the_host_mirror():
    """models/smo.py::_sigmoid_train_host (the mirror the existing Platt kernel test compares with, and
    the routine behind the sklearn probA_/probB_ parity of tests/test_parity_sklearn.py) on every
    listed input: by value where the input is decided, and through the stop rule everywhere — the
    longdouble gradient at the mirror's (A, B) is below 1e-5 within the f64 evaluation bound, unless
    the oracle itself ran to a cap."""
    for name in PLATT_NAMES:
        c, dec, lab, o, o64 = platt_ref(name)
        A, B = smo._sigmoid_train_host(dec, lab)
        if o.decided:
            sc = max(1.0, abs(float(o.A)), abs(float(o.B)))
            assert abs(A - float(o.A)) <= PLATT_MARGIN * sc and abs(B - float(o.B)) <= PLATT_MARGIN * sc, \
                (name, A, B, float(o.A), float(o.B))
        f, g1, g2, df, dg = o.evaluate(A, B)
        assert o.capped or (abs(g1) < 1e-5 + dg and abs(g2) < 1e-5 + dg), (name, float(g1), float(g2))


def test_platt_inputs_are_all_decided():
    """Every listed input but the singular one takes, in f64, the branches it takes in longdouble:
    the share of by-value inputs left undecided is 0, and membership comes from the oracle's own
    flag, so a decided input cannot go unchecked."""
    und = [n for n in PLATT_NAMES if not platt_ref(n)[3].decided]
    assert und == list(PLATT_UNDECIDED), und
    for n in platt_by_value():
        _, _, _, o, o64 = platt_ref(n)
        assert o.iters == o64.iters and o.capped == o64.capped, n


def test_platt_oracle_matches_sklearn_probA_probB():
    """sklearn's SVC(probability=True) on a precomputed kernel: libsvm shuffles the grouped points
    with sklearn's seeded generator, trains one sub-model per fold and hands the out-of-fold decision
    values to its own sigmoid_train.  The folds are regenerated here (models/smo.py _expand_py, the
    index bookkeeping tests/test_smo_host.py pins), every fold is solved by smo_oracle (bit-equal to
    libsvm on such matrices, above), the decision values are Σ yα·K − ρ in f64, oriented as libsvm
    orients them (its sub-model's first label is −1), and platt_oracle must land on probA_/probB_.
    Both are f64-or-better runs of one algorithm on decided input, so the margin is the
    reference-against-reference one, PLATT_MARGIN relative to max(1, |A|, |B|)."""
    import types
    from sklearn.svm import SVC
    l, F = 200, 5
    rng = np.random.default_rng(77)
    Z, npos = _cohort(l, F, 77)
    y = np.r_[np.zeros(npos), np.ones(l - npos)]
    mix = rng.permutation(l)
    Z, y = Z[mix], y[mix]
    K = gram_emul(Z, ngl2e_of(F)).astype(np.float64)
    n0 = int((y == 0).sum())
    w = np.array([l / (2.0 * n0), l / (2.0 * (l - n0))])
    m = SVC(kernel="precomputed", C=1.0, class_weight={0: w[0], 1: w[1]}, probability=True, shrinking=False,
            tol=EPS, random_state=2020).fit(K, y)
    probs, meta = smo._expand_py(0, y, 1.0 / F, w, types.SimpleNamespace(C=1.0, probability=True, random_state=2020))
    dec = np.zeros(l)
    folds = [p for p in probs if p.fold >= 0]
    assert len(folds) == 5 and all(p.rows is not None for p in folds)
    for p in folds:
        o = R.smo_oracle(K[np.ix_(p.rows, p.rows)], p.npos, p.Cp, p.Cn, EPS, MAX_ITER)
        ys = np.where(np.arange(p.l) < p.npos, 1.0, -1.0)
        dec[p.held] = -(K[np.ix_(p.held_rows, p.rows)] @ (ys * o.alpha) - o.rho)
    lab = np.where(np.arange(l) < meta["n0"], 1.0, -1.0)
    o = R.platt_oracle(dec, lab, depth=PLATT_DEPTH)
    assert o.decided and not o.capped and o.iters > 0
    sc = max(1.0, abs(float(o.A)), abs(float(o.B)))
    print("platt_oracle - sklearn:", float(o.A) - m.probA_[0], float(o.B) - m.probB_[0])
    assert abs(float(o.A) - float(m.probA_[0])) <= PLATT_MARGIN * sc
    assert abs(float(o.B) - float(m.probB_[0])) <= PLATT_MARGIN * sc


def test_platt_f64_margin():
    """The reference-against-reference figure behind PLATT_MARGIN, re-measured."""
    m = platt_margin()
    print("platt longdouble vs float64, relative to max(1, |A|, |B|):", m)
    assert m <= PLATT_MEASURED


# ------------------------------------------------------------------------------------ gram_kernel_error
@pytest.mark.parametrize("F", GRAM_FS)
def test_gram_emulation_stays_inside_budget(F):
    for l in GRAM_LS:
        Z = gram_rows(l, F, 100 * F + l)
        K, dK = R.gram_kernel_error(Z, ngl2e_of(F))
        Kh = gram_emul(Z, ngl2e_of(F))
        assert R.gram_inside(Kh, K, dK).all(), (l, F)
        assert (np.diagonal(Kh) == 1).all() and np.array_equal(Kh, Kh.T)
        if l >= 3:
            assert Kh[0, 1] == 1 and Kh[0, 2] == 0          # d² = 0 off the diagonal; underflow


@pytest.mark.parametrize("F", GRAM_FS)
def test_gram_budget_rejects_wrong_scale_and_missing_clamp(F):
    """One f32 ulp on the scale: 2⁻²³ relative in the exponent when the scale is a power of two and
    the ulp goes up, against a budget of 2⁻²⁴ (the product's rounding) plus exp2's on the integer
    rows, whose distances are exact — so the scale here is the power of two next to −log2 e / F.
    Without the clamp the near-coincident large rows give 2^(+noise) > 1."""
    e2 = np.float32(-2.0 ** np.round(np.log2(R.LOG2E / F)))
    up = np.nextafter(e2, np.float32(-np.inf))
    hit_scale = hit_clamp = False
    for l in GRAM_LS:
        Z = gram_rows(l, F, 100 * F + l)
        K, dK = R.gram_kernel_error(Z, e2)
        assert R.gram_inside(gram_emul(Z, e2), K, dK).all()
        hit_scale |= not R.gram_inside(gram_emul(Z, up), K, dK).all()
    for seed in range(8):
        Z = gram_rows(65, F, seed)
        K, dK = R.gram_kernel_error(Z, ngl2e_of(F))
        assert R.gram_inside(gram_emul(Z, ngl2e_of(F)), K, dK).all()
        hit_clamp |= not R.gram_inside(gram_emul(Z, ngl2e_of(F), clamp=False), K, dK).all()
    assert hit_scale and hit_clamp, (hit_scale, hit_clamp)


# ------------------------------------------------------------------------------------ gamma_oracle
def test_gamma_oracle_matches_numpy_and_beats_one_pass():
    rng = np.random.default_rng(5)
    F = 17
    Z = rng.normal(size=(1500, F))
    offs = np.array([0, 1, 500, 1500])
    g, e2 = R.gamma_oracle(Z, offs, F)
    for f in range(3):
        z = Z[offs[f]:offs[f + 1]]
        assert abs(float(g[f]) - 1.0 / (F * z.var())) <= 1e-12 / (F * z.var())
        assert e2[f] == np.float32(-float(g[f]) * R.LOG2E)
    Zb = 1e8 + rng.normal(size=(1000, F))
    gb, _ = R.gamma_oracle(Zb, [0, 1000], F)
    one_pass = (Zb * Zb).mean() - Zb.mean() ** 2
    two_pass = ((Zb.astype(np.longdouble) - Zb.astype(np.longdouble).mean()) ** 2).mean()
    assert abs(float(gb[0]) * F * float(two_pass) - 1) < 1e-15
    assert abs(float(gb[0]) * F * one_pass - 1) > 1e-3             # the one-pass variance is lost to cancellation
    z0 = np.zeros((4, F))
    assert R.gamma_oracle(z0, [0, 4], F)[0][0] == 1
    zn = rng.normal(size=(4, F))
    zn[1, 2] = np.nan
    zi = rng.normal(size=(4, F))
    zi[0, 0] = np.inf
    assert np.isnan(R.gamma_oracle(zn, [0, 4], F)[0][0]) and np.isnan(R.gamma_oracle(zi, [0, 4], F)[0][0])
