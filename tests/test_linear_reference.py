"""The linear-model certificates of ops/reference.py (logreg_objective, logreg_kkt,
logreg_newton_step, l1qp_kkt, lasso_gap_oracle, moments_oracle) proved on the CPU before
tests/test_linear_reference_gpu.py lets them judge a kernel: each accepts real solutions (the host
loop's, its mirrors' and scikit-learn's) and rejects every wrong variant it is there to catch."""
import numpy as np
import pytest
import torch

from hfens.models import lasso, logreg_solver
from hfens.ops import reference as R

L = np.longdouble
EPS = float(np.finfo(np.float64).eps)
# what the GPU file allows a kernel (its KKT_BOUND for L1 and L2): a wrong variant must land above it
KKT_ACCEPT = {True: 4.40e-7, False: 1.61e-8}


def _lr_problem(n=400, F=6, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)) * np.array([0.3, 1.0, 3.0, 1.0, 0.1, 2.0])[:F]
    u = np.array([1.5, -1.0, 0.0, 0.0, 4.0, 0.3])[:F]
    y = np.where(X @ u + rng.logistic(size=n) >= 0, 1.0, -1.0)
    Xa = np.concatenate([X, np.ones((n, 1))], 1)
    n1, n0 = (y > 0).sum(), (y < 0).sum()
    s = np.where(y > 0, n / (2.0 * n1), n / (2.0 * n0))      # balanced class weights
    return Xa, s, y


def _host(Xa, s, y, pen, l1, C=1.0):
    W, _ = logreg_solver._solve_loop(torch.as_tensor(Xa), torch.as_tensor(s[None]), torch.as_tensor(y),
                                     torch.as_tensor(pen), C, l1, 100)
    return W[0].numpy()


@pytest.fixture(scope="module")
def lr():
    Xa, s, y = _lr_problem()
    F1 = Xa.shape[1]
    ones = np.ones(F1, np.uint8)
    last = ones.copy()
    last[-1] = 0
    C1 = 0.05            # strong enough an L1 penalty that some coefficients are exactly zero
    return dict(Xa=Xa, s=s, y=y, ones=ones, last=last, C1=C1, w1=_host(Xa, s, y, ones, True, C1),
                w2=_host(Xa, s, y, last, False))


def test_logreg_kkt_accepts_host_solution(lr):
    """At the host loop's solutions the certificate is at or below the loop's own stop rules."""
    k1 = R.logreg_kkt(lr["Xa"], lr["s"], lr["y"], lr["w1"], lr["C1"], True, lr["ones"])
    k2 = R.logreg_kkt(lr["Xa"], lr["s"], lr["y"], lr["w2"], 1.0, False, lr["last"])
    assert (lr["w1"] == 0).any() and (lr["w1"] != 0).sum() >= 3
    assert 0 <= k1["ratio"] <= 1e-9, float(k1["ratio"])
    assert 0 <= k2["ratio"] <= 1e-10, float(k2["ratio"])
    assert k1["norm0"] > 0 and k2["norm0"] > 0


def test_logreg_kkt_accepts_sklearn_solution(lr):
    """liblinear (L1, intercept penalised as an augmented feature) and lbfgs (L2, free intercept)
    minimise the same objectives: their solutions pass at their own, looser accuracy."""
    from sklearn.linear_model import LogisticRegression as SK
    Xa, s, y = lr["Xa"], lr["s"], lr["y"]
    a = SK(penalty="l1", solver="liblinear", tol=1e-10, C=lr["C1"], intercept_scaling=1.0, max_iter=10000,
           random_state=0).fit(Xa[:, :-1], y, sample_weight=s)
    w = np.concatenate([a.coef_[0], a.intercept_])
    k = R.logreg_kkt(Xa, s, y, w, lr["C1"], True, lr["ones"])
    assert k["ratio"] <= 1e-6, float(k["ratio"])
    assert np.abs(w - lr["w1"]).max() < 1e-6
    b = SK(penalty="l2", solver="lbfgs", tol=1e-12, C=1.0, max_iter=10000).fit(Xa[:, :-1], y, sample_weight=s)
    w = np.concatenate([b.coef_[0], b.intercept_])
    k = R.logreg_kkt(Xa, s, y, w, 1.0, False, lr["last"])
    assert k["ratio"] <= 1e-4, float(k["ratio"])
    assert np.abs(w - lr["w2"]).max() < 1e-4
    F = R.logreg_objective(Xa, s, y, lr["w2"], 1.0, False, lr["last"])
    assert F <= R.logreg_objective(Xa, s, y, w, 1.0, False, lr["last"]) + L(1e-12) * abs(F)


def test_logreg_kkt_rejects_wrong_variants(lr):
    Xa, s, y, w1, w2, C1 = lr["Xa"], lr["s"], lr["y"], lr["w1"], lr["w2"], lr["C1"]
    r1 = lambda w, s_=s, pen=lr["ones"]: float(R.logreg_kkt(Xa, s_, y, w, C1, True, pen)["ratio"])      # noqa: E731
    r2 = lambda w, s_=s, pen=lr["last"]: float(R.logreg_kkt(Xa, s_, y, w, 1.0, False, pen)["ratio"])    # noqa: E731
    nz = np.flatnonzero(w1 != 0)
    # a coefficient moved by 1e-6
    for j in (nz[0], nz[-1]):
        w = w1.copy()
        w[j] += 1e-6
        assert r1(w) > KKT_ACCEPT[True], (j, r1(w))
    for j in (0, len(w2) - 1):
        w = w2.copy()
        w[j] -= 1e-6
        assert r2(w) > KKT_ACCEPT[False], (j, r2(w))
    # the sign of the smallest non-zero coefficient flipped
    j = nz[np.argmin(np.abs(w1[nz]))]
    w = w1.copy()
    w[j] = -w[j]
    assert r1(w) > 100 * KKT_ACCEPT[True], r1(w)
    # a zero coefficient made non-zero, by less than any tolerance on w would notice
    j = np.flatnonzero(w1 == 0)[0]
    w = w1.copy()
    w[j] = 1e-12
    assert r1(w) > 100 * KKT_ACCEPT[True], r1(w)
    # the free intercept judged as penalised, and a penalised one judged as free
    assert r2(w2, pen=lr["ones"]) > 100 * KKT_ACCEPT[False]
    assert r1(w1, pen=lr["last"]) > 100 * KKT_ACCEPT[True]
    # class weights swapped
    sw = np.where(y > 0, s[y < 0][0], s[y > 0][0])
    assert sw.sum() != s.sum() or not np.array_equal(sw, s)
    assert r1(w1, s_=sw) > 100 * KKT_ACCEPT[True] and r2(w2, s_=sw) > 100 * KKT_ACCEPT[False]
    # and the objective tells the better of two points apart at 1e-12 relative
    F = R.logreg_objective(Xa, s, y, w2, 1.0, False, lr["last"])
    w = w2.copy()
    w[0] += 1e-4
    assert R.logreg_objective(Xa, s, y, w, 1.0, False, lr["last"]) > F + L(1e-12) * abs(F)


def test_logreg_objective_is_overflow_free():
    Xa = np.array([[1e4, 1.0], [-1e4, 1.0]])
    y = np.array([1.0, -1.0])
    w = np.array([1.0, 0.0])
    F = R.logreg_objective(Xa, np.ones(2), y, -w, 2.0, True, np.array([1, 0], np.uint8))
    assert np.isfinite(F) and abs(F - (2.0 * 2e4 + 1.0)) < 1e-9
    k = R.logreg_kkt(Xa, np.ones(2), y, w, 2.0, True, np.array([1, 1], np.uint8))
    assert np.isfinite(k["norm"]) and k["norm"] == 1.0          # saturated rows: g = 0, sub = sign(w_0)


def test_newton_step_against_finite_differences():
    """F1 = 3: d = −(H + P)⁻¹g with H and g from central differences of logreg_objective itself."""
    rng = np.random.default_rng(11)
    Xa = np.concatenate([rng.normal(size=(40, 2)), np.ones((40, 1))], 1)
    y = np.where(rng.random(40) < 0.5, 1.0, -1.0)
    s = rng.uniform(0.5, 2.0, 40)
    pen = np.array([1, 1, 0], np.uint8)
    C = 0.7
    st = R.logreg_newton_step(Xa, s, y, C, pen)
    f = lambda w: R.logreg_objective(Xa, s, y, w, C, False, pen)     # noqa: E731
    h = L(1e-4)
    I = np.eye(3, dtype=L) * h
    z = np.zeros(3, dtype=L)
    g = np.array([(f(z + I[i]) - f(z - I[i])) / (2 * h) for i in range(3)], dtype=L)
    A = np.array([[(f(z + I[i] + I[j]) - f(z + I[i] - I[j]) - f(z - I[i] + I[j]) + f(z - I[i] - I[j])) / (4 * h * h)
                   for j in range(3)] for i in range(3)], dtype=L)
    d = -np.linalg.solve(A.astype(np.float64), g.astype(np.float64))
    assert np.abs(g - st["g"]).max() < 1e-7 and np.abs(A - st["A"]).max() < 1e-6
    assert np.abs(d - st["d"].astype(np.float64)).max() < 1e-6 * np.abs(d).max()
    assert abs(st["delta"] - st["g"] @ st["d"]) < 1e-15 and st["delta"] < 0
    for k in range(8):
        assert st["FK"][k] == f(st["d"] * L(2.0) ** -k)
    assert st["F0"] == f(z)
    # the Armijo choice: the first admissible step, and the margin is its distance to the threshold
    thr = st["F0"] + L(0.01) * L(2.0) ** -np.arange(8) * st["delta"]
    assert st["k"] == int(np.argmax(st["FK"] <= thr)) and st["margin"] > 0


def _qp(F1=9, seed=5):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(3 * F1, F1))
    H = A.T @ A / F1 + 1e-12 * np.eye(F1)
    w = rng.normal(size=F1) * (rng.random(F1) < 0.6)
    g = rng.normal(size=F1) * 2
    pen = np.ones(F1, np.uint8)
    pen[[1, F1 - 1]] = 0
    return H, g, w, pen


def test_l1qp_kkt_accepts_mirror_and_rejects_wrong(monkeypatch):
    H, g, w, pen = _qp()
    t = lambda a: torch.as_tensor(a[None])      # noqa: E731
    for finish in (True, False):
        if not finish:     # plain coordinate descent to the step rule: what the bound is derived from
            monkeypatch.setattr(logreg_solver, "_newton_finish", lambda *a: None)
        capped = []
        d = logreg_solver._host_l1_qp(t(H), t(g), t(w), torch.as_tensor(pen), 1.0, 200 if finish else 5000, 1e-12,
                                      capped=capped)[0].numpy()
        assert capped == [False]
        res, bound = R.l1qp_kkt(H, g, w, pen, 1.0, d, tol=1e-12)
        assert (np.abs(res) <= bound).all(), float((np.abs(res) / bound).max())
    u = w + d
    assert (u[pen == 1] == 0).any() and (u[pen == 1] != 0).any()

    def worst(d_, pen_=pen, lam=1.0):
        r, b = R.l1qp_kkt(H, g, w, pen_, lam, d_, tol=1e-12)
        return float((np.abs(r) / b).max())
    j = np.flatnonzero((u != 0) & (pen == 1))[0]
    z = np.flatnonzero((u == 0) & (pen == 1))[0]
    d1 = d.copy()
    d1[j] += 1e-6
    assert worst(d1) > 1e3                       # a coordinate moved by 1e-6
    d1 = d.copy()
    d1[j] = -u[j] - w[j]
    assert worst(d1) > 1e3                       # the sign of w_j + d_j flipped
    d1 = d.copy()
    d1[z] += 1e-12
    assert worst(d1) > 1e3                       # a zero made non-zero
    assert worst(d, pen_=np.ones_like(pen)) > 1e3      # unpenalised coordinates judged as penalised
    assert worst(d, lam=1.001) > 1e3


def _lasso(seed=2, n=120, F=8):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)) * 10.0 ** rng.uniform(-0.5, 0.5, F)
    X -= X.mean(0)
    y = X @ (rng.normal(size=F) * (rng.random(F) < 0.5)) + rng.normal(size=n)
    y -= y.mean()
    return X.T @ X, X.T @ y, float(y @ y), float(n)


@pytest.mark.parametrize("tol", [1e-4, 1e-13])
def test_lasso_gap_accepts_mirror_and_rejects_neighbour(tol):
    G, q, yy, n = _lasso()
    amax = np.abs(q).max() / n
    alphas = np.geomspace(2 * amax, 1e-2 * amax, 10)
    W = lasso._cd_path_host(G, q, yy, n, alphas, 20000, tol)
    assert not W[0].any()                                  # alpha ≥ alpha_max
    for a in range(10):
        gap, bud = R.lasso_gap_oracle(G, q, yy, n, alphas[a], W[a])
        assert gap > -bud
        assert gap < L(tol) * L(yy) + bud, (a, float(gap))
    for a in range(3, 9):
        # the neighbouring alphas' solutions are not this alpha's (below alpha_max: w ≠ 0)
        for o in (a - 1, a + 1):
            gap, bud = R.lasso_gap_oracle(G, q, yy, n, alphas[a], W[o])
            assert gap > L(tol) * L(yy) + bud, (a, o, float(gap))
    if tol < 1e-12:
        a = 5
        j = np.flatnonzero(W[a] != 0)[0]
        w = W[a].copy()
        w[j] += 1e-6 * max(1.0, abs(w[j]))                 # a coefficient moved by 1e-6
        gap, bud = R.lasso_gap_oracle(G, q, yy, n, alphas[a], w)
        assert gap > L(tol) * L(yy) + bud, float(gap)


def test_lasso_gap_matches_sklearn():
    """The same number sklearn reports for its own solution (dual_gap_ is divided by n there)."""
    from sklearn.linear_model import Lasso
    rng = np.random.default_rng(4)
    X = rng.normal(size=(80, 5))
    X -= X.mean(0)
    y = X @ np.array([1.0, 0, -2.0, 0, 0.5]) + rng.normal(size=80)
    y -= y.mean()
    m = Lasso(alpha=0.1, fit_intercept=False, tol=1e-6, precompute=True).fit(X, y)
    gap, _ = R.lasso_gap_oracle(X.T @ X, X.T @ y, y @ y, 80, 0.1, m.coef_)
    assert abs(float(gap) / 80 - m.dual_gap_) <= 1e-9 * max(1.0, abs(m.dual_gap_))


def test_moments_oracle():
    rng = np.random.default_rng(9)
    X, W, V = rng.normal(size=(5, 3)), rng.uniform(0, 2, size=(2, 5)), rng.normal(size=(2, 5))
    G, a, v, Gm, am, vm = R.moments_oracle(X, W, V)
    for p in range(2):
        for i in range(3):
            sa = sv = sam = svm = L(0)
            for r in range(5):
                sa += L(W[p, r]) * L(X[r, i])
                sv += L(V[p, r]) * L(X[r, i])
                sam += abs(L(W[p, r]) * L(X[r, i]))
                svm += abs(L(V[p, r]) * L(X[r, i]))
            assert abs(a[p, i] - sa) < 1e-17 and abs(v[p, i] - sv) < 1e-17
            assert abs(am[p, i] - sam) < 1e-17 and abs(vm[p, i] - svm) < 1e-17
            for j in range(3):
                sg = sgm = L(0)
                for r in range(5):
                    sg += L(W[p, r]) * L(X[r, i]) * L(X[r, j])
                    sgm += abs(L(W[p, r]) * L(X[r, i]) * L(X[r, j]))
                assert abs(G[p, i, j] - sg) < 1e-17 and abs(Gm[p, i, j] - sgm) < 1e-17
    assert R.moments_oracle(X, W)[2] is None
    # the project's host path passes the (n + 2)·eps bound; the same with one row dropped does not
    from hfens import ops
    Gt, at, vt = ops.weighted_moments(torch.as_tensor(X), torch.as_tensor(W), torch.as_tensor(V))
    k = 7 * L(EPS)
    assert (np.abs(Gt.numpy() - G) <= k * Gm).all() and (np.abs(at.numpy() - a) <= k * am).all()
    assert (np.abs(vt.numpy() - v) <= k * vm).all()
    Gd, ad, vd = ops.weighted_moments(torch.as_tensor(X[:-1]), torch.as_tensor(W[:, :-1]), torch.as_tensor(V[:, :-1]))
    assert (np.abs(Gd.numpy() - G) > k * Gm).any() and (np.abs(ad.numpy() - a) > k * am).all()
    assert (np.abs(vd.numpy() - v) > k * vm).all()
