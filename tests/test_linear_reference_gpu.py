"""logreg.hip (logreg_fused, logreg_coop) and linear.hip (l1_qp_cd, lasso_cd_path, weighted_moments)
against the longdouble certificates of ops/reference.py: the min-norm subgradient of the logistic
objective, the KKT residual of the L1 quadratic subproblem, sklearn's duality gap and the exact
moments.  A certificate judges the kernel's own answer from the raw inputs, so it holds however the
kernel got there; tests/test_linear_reference.py proves the certificates first.

Every shape is the smallest that reaches its branch of the kernels:

* logreg_fused's task layouts, T = F1(F1+1)/2 + F1 against 1024 threads: G > 1 row groups (F1 ≤ 30),
  G = 1 with idle threads (F1 = 31, 43), up to three tasks per thread (F1 = 44, 63, 64);
* its row chunks: n at CR − 1, CR, CR + 1 and 2·CR + 3 for each F1's CR (``_cr``), the scratch
  override of CR at F1 = 64, and n = 5 (fewer rows than row groups);
* logreg_coop with a ragged last slab and with empty slabs;
* lasso_cd_path's ``live`` mask, alpha ≥ alpha_max, the sweep cap, A = 1 and unequal row counts;
* weighted_moments at F = 1, its limit F = 128 and n = 128k ± 1.

Host figures and the largest values seen on an MI355X stand next to each constant."""
import numpy as np
import pytest
import torch

from hfens.models import logreg_solver
from hfens.ops import reference as R

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
L = np.longdouble
C_LR = 1.0

# The certificate bound of the logistic kernels: the largest logreg_kkt ratio (‖sub(w)‖₁ / ‖sub(0)‖₁)
# a solve may leave.  It is 10 × the worst ratio of the HOST loop (logreg_solver._solve_loop on CPU
# tensors, not the code under test) over this file's whole problem list, and never below the
# solvers' own stop rules (1e-9 for L1, 1e-10 for L2).  Most solves end orders of magnitude below
# their stop rule (Newton's last step); the worst ones leave by the line-search or step-size exits,
# when the decrease left is below the f64 resolution of the objective, and where that happens
# depends on the host's summation order: the same loop on the same list left
#   L1  4.42e-9  (F1 = 64, n = 259, all penalised, chunk model) on the development host,
#       4.40e-8  (F1 = 2, n = 1025, last unpenalised, all-rows model) on the MI355X machine's CPU;
#   L2  1.004e-10 (F1 = 30, n = 128, last unpenalised, chunk model) on the development host,
#       1.61e-9  (F1 = 64, n = 259, first and middle unpenalised, chunk model) on the MI355X machine's.
# The bound takes the larger figure of each.  Largest kernel ratio on an MI355X over the list:
#   L1  2.48e-8 (F1 = 2, n = 1025, last unpenalised, all-rows model),
#   L2  2.45e-9 (F1 = 63, n = 131, all penalised, chunk model: the line search gave up at an objective
#       within 4.6e-16 of the host loop's).
# Other largest values seen there: one Newton step err / tolerance 2.6e-3; l1_qp_cd residual / bound
# 3.4e-4 and |d − mirror| 1.8e-15; lasso |kernel gap − oracle gap| / budget 0.90; moments error / bound 0.18.
HOST_WORST = {True: 4.40e-8, False: 1.61e-9}
KKT_BOUND = {True: max(10 * HOST_WORST[True], 1e-9), False: max(10 * HOST_WORST[False], 1e-10)}

SEEN = {}     # name → largest observed value / bound in this process (printed, never asserted)


def _seen(name, v):
    SEEN[name] = max(SEEN.get(name, 0.0), float(v))
    return SEEN[name]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ----------------------------------------------------------------------------- logistic problems
def _cr(F1):
    """Rows per LDS chunk, restated from logreg_lds_plan (logreg.hip): at most 32 KiB of staged rows,
    a multiple of 64 between 64 and 1024, raised when CR·F1 doubles cannot hold the F1² + F1 doubles
    of the Newton-finish scratch (only F1 = 64: 64·64 < 64·64 + 64 → 128; F1 = 63 fits exactly)."""
    CR = (32 * 1024) // (F1 * 8)
    CR = 1024 if CR > 1024 else CR // 64 * 64
    CR = max(CR, 64)
    if CR * F1 < F1 * F1 + F1:
        CR = (F1 + 1 + 63) // 64 * 64
    return CR


assert [_cr(f) for f in (1, 2, 4, 18, 30, 31, 43, 44, 63, 64)] == [1024, 1024, 1024, 192, 128, 128, 64, 64, 64, 128]

LR_F1 = (1, 2, 18, 30, 31, 43, 44, 63, 64)
LR_CASES = [(F1, n) for F1 in LR_F1 for n in (_cr(F1) - 1, _cr(F1), _cr(F1) + 1, 2 * _cr(F1) + 3)] + [(1, 5), (64, 5)]
N_FAR = 2


class _LrData:
    """One row matrix with unequal column scales (three decades; the last column is the intercept's
    ones for F1 ≥ 2), labels from a noisy linear rule, and the row sets of the models:

    * ``sep``: the rows the rule labels correctly — a separable problem — plus N_FAR rows 300 times
      further out on their own side, whose σ saturates to exactly 1 (D = 0) once w has moved;
    * ``chunk``: every ordinary row except the first LDS chunk (the first half when n ≤ CR);
    * ``five``: about 5 rows of both labels with weights so small that |g_j(0)| ≤ ¼: under an
      all-ones L1 mask w = 0 is optimal and the solve stops in its first iteration;
    * ``full`` / ``half``: all ordinary rows / every other one (non-separable, for the masks with
      unpenalised coordinates, where a separable or tiny problem has no finite optimum)."""

    def __init__(self, F1, n):
        rng = np.random.default_rng(1000 * F1 + n)
        scales = 10.0 ** rng.uniform(-1.5, 1.5, F1)
        X = rng.normal(size=(n, F1)) * scales
        if F1 >= 2:
            X[:, -1] = 1.0
        u = rng.normal(size=F1) / scales / np.sqrt(F1)
        if F1 >= 2:
            tf = X[:, :-1] @ u[:-1]
            u[-1] = 0.1 * tf.std() - np.median(tf)      # a small offset: both labels stay frequent
        nfar = N_FAR if n >= 60 else 0
        t = X @ u
        if nfar:
            far = np.argsort(-np.abs(t))[:nfar]
            X[far, :F1 - 1 if F1 >= 2 else F1] *= 300.0
            t = X @ u
        y = np.where(t + 0.7 * rng.logistic(size=n) >= 0, 1.0, -1.0)
        ordinary = np.ones(n, bool)
        if nfar:
            y[far] = np.where(t[far] >= 0, 1.0, -1.0)
            ordinary[far] = False
        if n <= 8:
            y[:2] = (1.0, -1.0)        # both labels present
        self.F1, self.n, self.X, self.y, self.CR = F1, n, X, y, _cr(F1)
        clean = (y == np.where(t >= 0, 1.0, -1.0)) & (np.abs(t) > 0.05)
        self.rows = {}
        self.rows["sep"] = self._balanced(clean | ~ordinary)
        ch = ordinary.copy()
        ch[:self.CR if n > self.CR else n // 2] = False
        self.rows["chunk"] = self._balanced(ch)
        idx = np.flatnonzero(ordinary)
        pick = np.concatenate([idx[y[idx] > 0][:3], idx[y[idx] < 0][:2]])
        five = np.zeros(n)
        five[pick] = 0.5 / (C_LR * np.abs(X[pick]).sum(0).max())
        self.rows["five"] = five
        self.rows["full"] = ordinary.astype(np.float64)
        hf = ordinary.copy()
        hf[1::2] = False
        self.rows["half"] = self._balanced(hf)

    def _balanced(self, m):
        n1, n0 = float((m & (self.y > 0)).sum()), float((m & (self.y < 0)).sum())
        tot = n1 + n0
        return m * np.where(self.y > 0, tot / (2 * max(n1, 1.0)), tot / (2 * max(n0, 1.0)))

    def _posed(self, name):
        """With unpenalised coordinates a model has a finite optimum only if those coordinates alone
        cannot separate it: both labels, and more than a handful of rows."""
        m = self.rows[name] != 0
        return m.sum() >= 16 and (m & (self.y > 0)).any() and (m & (self.y < 0)).any()

    def masks(self, l1):
        """(name, penal, model names) per penalty mask of this shape.  Under a mask with unpenalised
        coordinates the chunk model gives way to the all-rows model where it is not well posed (at
        n = CR + 1 it keeps a single row)."""
        F1, n = self.F1, self.n
        out = [("ones", np.ones(F1, np.uint8), ("sep", "chunk", "five"))]
        chunk = "chunk" if self._posed("chunk") else "full"
        if F1 >= 2 and n >= 16:
            p = np.ones(F1, np.uint8)
            p[-1] = 0
            assert self._posed("sep") or n < 60
            out.append(("last", p, ("sep", chunk, "five")))
        if F1 >= 3 and n >= 60:
            # unpenalised first and middle coordinates; the 5-row model could be separable on two
            # unpenalised coordinates alone, so the every-other-row model stands in for it
            p = np.ones(F1, np.uint8)
            p[[0, F1 // 2]] = 0
            assert self._posed("sep") and self._posed("half")
            out.append(("firstmid", p, ("sep", chunk, "half")))
        if not l1 and n >= 16 * F1:
            # nothing penalised: only non-separable problems, so that H is positive definite
            out.append(("none", np.zeros(F1, np.uint8), ("full", "half")))
        return out

    def S(self, names):
        return np.stack([self.rows[k] for k in names])


_LR_DATA, _LR_HOST = {}, {}


def _lr_data(F1, n):
    if (F1, n) not in _LR_DATA:
        _LR_DATA[(F1, n)] = _LrData(F1, n)
    return _LR_DATA[(F1, n)]


def _lr_host(F1, n, l1, mask):
    """The host loop's solution of one batch (computed once, shared)."""
    key = (F1, n, l1, mask)
    if key not in _LR_HOST:
        D = _lr_data(F1, n)
        name, pen, models = next(m for m in D.masks(l1) if m[0] == mask)
        W, _ = logreg_solver._solve_loop(torch.as_tensor(D.X), torch.as_tensor(D.S(models)), torch.as_tensor(D.y),
                                         torch.as_tensor(pen), C_LR, l1, 100)
        _LR_HOST[key] = W.numpy().copy()
    return _LR_HOST[key]


def _solve(dev, monkeypatch, X, S, y, pen, l1, max_outer=100, members=1):
    """One launch through logreg_solver._launch_fused / _finish_fused → (W, iters, err word)."""
    monkeypatch.setattr(logreg_solver, "MEMBERS", members)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    h = logreg_solver._launch_fused(t(X), t(S), t(y), t(pen), C_LR, l1, max_outer)
    W, iters = logreg_solver._finish_fused(h)
    err = int(h["err"].cpu()) if h["err"] is not None else 0
    assert logreg_solver.LAST_PATH["members"] == members
    return W.cpu().numpy(), iters.cpu().numpy(), err


def _certify(D, models, pen, l1, W, Wh, tag):
    """logreg_kkt ratio of every model within KKT_BOUND, and the kernel's objective no worse than
    the host loop's (1e-12 relative)."""
    S = D.S(models)
    for b in range(len(models)):
        assert np.isfinite(W[b]).all(), (tag, models[b])
        k = R.logreg_kkt(D.X, S[b], D.y, W[b], C_LR, l1, pen)
        kh = R.logreg_kkt(D.X, S[b], D.y, Wh[b], C_LR, l1, pen)
        Fk = R.logreg_objective(D.X, S[b], D.y, W[b], C_LR, l1, pen)
        Fh = R.logreg_objective(D.X, S[b], D.y, Wh[b], C_LR, l1, pen)
        big = _seen(f"logreg kkt ratio {'L1' if l1 else 'L2'}", k["ratio"])
        print(f"{tag} {models[b]}: ratio kernel {float(k['ratio']):.3e} host {float(kh['ratio']):.3e} "
              f"F kernel-host {float(Fk - Fh):.3e} of {float(Fh):.6e} (largest ratio so far {big:.3e})")
        assert k["ratio"] <= KKT_BOUND[l1], (tag, models[b], float(k["ratio"]), float(kh["ratio"]))
        assert Fk <= Fh + L(1e-12) * abs(Fh), (tag, models[b], float(Fk - Fh), float(Fh))


@pytest.mark.parametrize("F1,n", LR_CASES)
@pytest.mark.parametrize("pen", ["l1", "l2"])
def test_logreg_fused_certificate(dev, monkeypatch, pen, F1, n):
    """members = 1: every penalty mask of the shape (``_LrData.masks``), three models a launch."""
    l1 = pen == "l1"
    D = _lr_data(F1, n)
    for name, penal, models in D.masks(l1):
        W, iters, _ = _solve(dev, monkeypatch, D.X, D.S(models), D.y, penal, l1)
        tag = f"{pen} F1={F1} n={n} mask={name}"
        print(tag, "iters", iters.tolist())
        assert (iters >= 1).all() and (iters < 100).all(), (tag, iters)
        if l1 and name == "ones":
            # the 5-row model: w = 0 is optimal, found in the first iteration
            assert iters[2] == 1 and not W[2].any(), (tag, iters, W[2])
        _certify(D, models, penal, l1, W, _lr_host(F1, n, l1, name), tag)


def test_logreg_saturated_rows():
    """The separable model's far rows do saturate: at the host loop's solution their σ is exactly 1
    in f64, so D = s·σ(1 − σ) = 0 (what the certificate tests run through pass A)."""
    hit = 0
    for F1, n in ((18, 387), (44, 131), (64, 259)):
        D = _lr_data(F1, n)
        w = _lr_host(F1, n, False, "ones")[0]
        far = np.flatnonzero((D.rows["sep"] != 0) & (D.rows["full"] == 0))
        assert far.size == N_FAR
        sig = 1.0 / (1.0 + np.exp(-(D.y[far] * (D.X[far] @ w))))
        hit += int((sig * (1.0 - sig) == 0.0).sum())
    assert hit >= 3, hit


@pytest.mark.parametrize("F1,n", [(2, 1025), (18, 387), (31, 129), (44, 131), (64, 259)])
@pytest.mark.parametrize("pen", ["l1", "l2"])
def test_logreg_launch_independence(dev, monkeypatch, pen, F1, n):
    """A model's bits do not depend on which models share its launch, nor on the launch: B = 3
    together, each alone and a repeat are bit-identical in W and iters; the 5-row model stops before
    the others (per-model stopping)."""
    l1 = pen == "l1"
    D = _lr_data(F1, n)
    penal = np.ones(F1, np.uint8)
    models = ("sep", "chunk", "five")
    S = D.S(models)
    W, it, _ = _solve(dev, monkeypatch, D.X, S, D.y, penal, l1)
    W2, it2, _ = _solve(dev, monkeypatch, D.X, S, D.y, penal, l1)
    assert np.array_equal(_bits(W), _bits(W2)) and np.array_equal(it, it2)
    for b in range(3):
        Wb, itb, _ = _solve(dev, monkeypatch, D.X, S[b:b + 1], D.y, penal, l1)
        assert np.array_equal(_bits(W[b]), _bits(Wb[0])), (models[b], np.abs(W[b] - Wb[0]).max())
        assert it[b] == itb[0], (models[b], it, itb)
    assert it[2] < max(it[0], it[1]), it


NEWTON_CASES = [(18, 387, "ones"), (18, 193, "last"), (44, 131, "ones"), (44, 65, "last"), (64, 259, "ones"),
                (64, 129, "last")]


def _newton_case(F1, n, mask):
    D = _lr_data(F1, n)
    _, penal, models = next(m for m in D.masks(False) if m[0] == mask)
    return D, penal, models, [R.logreg_newton_step(D.X, s, D.y, C_LR, penal) for s in D.S(models)]


def test_logreg_one_newton_step(dev, monkeypatch):
    """max_outer = 1, L2: W = 2^-k·d with d the exact first Newton direction and k the oracle's
    Armijo choice, within cond(H + P)·(n + 2)·eps of max|2^-k·d| — pass A (H, g, the loss), the
    in-kernel Cholesky and the line search against the exact answer.  A model whose Armijo margin is
    within 1e-12·|F| of the threshold is ambiguous and left out (at most one; none on these seeds)."""
    left_out = 0
    for F1, n, mask in NEWTON_CASES:
        D, penal, models, steps = _newton_case(F1, n, mask)
        W, iters, _ = _solve(dev, monkeypatch, D.X, D.S(models), D.y, penal, False, max_outer=1)
        assert (iters == 1).all(), iters
        for b, st in enumerate(steps):
            if st["k"] is None or st["margin"] <= L(1e-12) * abs(st["F0"]):
                left_out += 1
                continue
            want = (st["d"] * L(2.0) ** -st["k"])
            cond = float(np.linalg.cond(st["A"].astype(np.float64)))
            tol = cond * (n + 2) * EPS * float(np.abs(want).max())
            err = float(np.abs(W[b].astype(L) - want).max())
            big = _seen("newton step err / tol", err / tol)
            print(f"newton F1={F1} n={n} {mask} {models[b]}: k={st['k']} cond={cond:.3e} err={err:.3e} tol={tol:.3e} "
                  f"(largest err/tol so far {big:.3e})")
            assert err <= tol, (F1, n, mask, models[b], st["k"], err, tol)
    assert left_out <= 1, left_out


@pytest.mark.parametrize("pen,n,F1,members", [("l1", 1030, 18, 16), ("l2", 40, 44, 3), ("l1", 20, 64, 16)])
def test_logreg_coop_certificate(dev, monkeypatch, pen, n, F1, members):
    """logreg_coop: a ragged last slab (1030 rows over 16 members: 65 each, the last 55), and 20 rows
    over 16 members (slabs of 2: members 10 … 15 own no row and still take part in every
    exchange).  The same certificate as members = 1, W within 1e-7 of it, no exchange timeout."""
    l1 = pen == "l1"
    D = _lr_data(F1, n)
    penal = np.ones(F1, np.uint8)
    if not l1:
        penal[-1] = 0
    models = ("sep", "chunk", "five")
    S = D.S(models)
    logreg_solver.LAST_PATH.pop("coop_fallback", None)
    W1, it1, _ = _solve(dev, monkeypatch, D.X, S, D.y, penal, l1)
    Wm, itm, err = _solve(dev, monkeypatch, D.X, S, D.y, penal, l1, members=members)
    assert err == 0
    assert not logreg_solver.LAST_PATH.get("coop_fallback")
    Wh, _ = logreg_solver._solve_loop(torch.as_tensor(D.X), torch.as_tensor(S), torch.as_tensor(D.y),
                                      torch.as_tensor(penal), C_LR, l1, 100)
    _certify(D, models, penal, l1, Wm, Wh.numpy(), f"coop {pen} F1={F1} n={n} members={members}")
    d = float(np.abs(Wm - W1).max())
    print("coop vs members=1", d, it1.tolist(), itm.tolist())
    assert d < 1e-7, d


# ----------------------------------------------------------------------------- l1_qp_cd
def _qp_problems(F1):
    """H = C·X̃ᵀDX̃ + 1e-12·I, g and w of three models after two outer iterations of the host loop (real
    prox-Newton iterates: some coordinates already at zero)."""
    rng = np.random.default_rng(77 + F1)
    n = 40 + 6 * F1
    X = rng.normal(size=(n, F1)) * 10.0 ** rng.uniform(-0.5, 0.5, F1)
    if F1 >= 2:
        X[:, -1] = 1.0
    y = np.where(X @ (rng.normal(size=F1) / np.sqrt(F1)) + rng.logistic(size=n) >= 0, 1.0, -1.0)
    S = np.ones((3, n))
    S[1, ::3] = 0.0
    S[2] = np.where(y > 0, 2.0, 0.5)
    W, _ = logreg_solver._solve_loop(torch.as_tensor(X), torch.as_tensor(S), torch.as_tensor(y),
                                     torch.ones(F1, dtype=torch.uint8), C_LR, True, 2)
    W = W.numpy()
    M = y[None] * (W @ X.T)
    sig = 1.0 / (1.0 + np.exp(-M))
    H = C_LR * np.einsum("bn,ni,nj->bij", S * sig * (1 - sig), X, X) + 1e-12 * np.eye(F1)
    g = C_LR * (S * (sig - 1.0) * y[None]) @ X
    return H, g, W


@pytest.mark.parametrize("F1", [1, 2, 17, 63, 64])
def test_l1_qp_cd_certificate(dev, F1):
    """l1_qp_cd (max_sweeps 200, tol 1e-12) on three launches: λ = 1 all penalised; a λ so large that
    every coordinate ends at w + d = 0; λ = 1 with unpenalised coordinates.  The host mirror leaves
    before the sweep cap on every problem (a capped solve carries no bound); the residual of
    reference.l1qp_kkt is within its derived bound and d within 1e-10 of the mirror."""
    from hfens import ops
    E = ops.ext()
    H, g, w = _qp_problems(F1)
    ones = np.ones(F1, np.uint8)
    some = ones.copy()
    some[[0, F1 // 2, F1 - 1]] = 0
    lam_big = 2.0 * float(np.abs(g - np.einsum("bij,bj->bi", H, w)).max()) + 1.0
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    for tag, lam, pen in (("ones", 1.0, ones), ("big", lam_big, ones), ("some", 1.0, some)):
        capped = []
        dm = logreg_solver._host_l1_qp(torch.as_tensor(H), torch.as_tensor(g), torch.as_tensor(w),
                                       torch.as_tensor(pen), lam, 200, 1e-12, capped=capped).numpy()
        assert capped == [False] * 3, (F1, tag, capped)
        Hd, gd, wd, pd = t(H), t(g), t(w), t(pen)
        d = torch.empty(3, F1, dtype=torch.float64, device=dev)
        E.l1_qp_cd(3, F1, Hd.data_ptr(), gd.data_ptr(), wd.data_ptr(), pd.data_ptr(), float(lam), 200, 1e-12,
                   d.data_ptr(), ops.stream_ptr(dev))
        d = d.cpu().numpy()
        for b in range(3):
            res, bound = R.l1qp_kkt(H[b], g[b], w[b], pen, lam, d[b], tol=1e-12)
            big = _seen("l1qp residual / bound", (np.abs(res) / bound).max())
            dd = float(np.abs(d[b] - dm[b]).max())
            print(f"l1qp F1={F1} {tag} b={b}: res/bound {float((np.abs(res) / bound).max()):.3e} "
                  f"|d - mirror| {dd:.3e} (largest res/bound so far {big:.3e})")
            assert (np.abs(res) <= bound).all(), (F1, tag, b, float((np.abs(res) / bound).max()))
            assert dd <= 1e-10, (F1, tag, b, dd)
            if tag == "big":
                assert not (w[b] + d[b]).any()
            if tag == "some":
                assert (d[b][pen == 0] != 0).all()


# ----------------------------------------------------------------------------- lasso_cd_path
def _lasso_problem(F, P, A, first_factor=1.0):
    """P problems on row subsets of different sizes of one centred design: column 1 has zero variance
    (F ≥ 3: an exact zero column after centring, G_kk = 0), the last column duplicates column 0 exactly
    (F ≥ 2).  The grid of each problem runs from first_factor·alpha_max down two decades."""
    rng = np.random.default_rng(5 * F + P)
    n = 300
    X = rng.normal(size=(n, F)) * 10.0 ** rng.uniform(-1, 1, F)
    beta = rng.normal(size=F) * (rng.random(F) < 0.5)
    G, q, yy, ns, al = [], [], [], [], []
    for p in range(P):
        rows = np.arange(n)[: n - 37 * p]
        Xp = X[rows] - X[rows].mean(0)
        if F >= 3:
            Xp[:, 1] = 0.0
        if F >= 2:
            Xp[:, -1] = Xp[:, 0]
        yp = Xp @ beta + rng.normal(size=rows.size)
        yp = yp - yp.mean()
        G.append(Xp.T @ Xp)
        q.append(Xp.T @ yp)
        yy.append(yp @ yp)
        ns.append(float(rows.size))
        amax = np.abs(q[-1]).max() / rows.size
        al.append(np.geomspace(first_factor * amax, 1e-2 * amax, A) if A > 1 else np.array([first_factor * amax * 0.1]))
    return np.stack(G), np.stack(q), np.array(yy), np.array(ns), np.stack(al)


def _lasso_run(dev, G, q, yy, ns, al, max_iter, tol):
    from hfens import ops
    P, F = q.shape
    A = al.shape[1]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    Gd, qd, yd, nd, ad = t(G), t(q), t(yy), t(ns), t(al)
    coefs = torch.full((P, A, F), float("nan"), dtype=torch.float64, device=dev)
    gaps = torch.full((P, A), float("nan"), dtype=torch.float64, device=dev)
    iters = torch.full((P, A), -1, dtype=torch.int32, device=dev)
    ops.ext().lasso_cd_path(P, F, A, Gd.data_ptr(), qd.data_ptr(), yd.data_ptr(), nd.data_ptr(), ad.data_ptr(),
                            int(max_iter), float(tol), coefs.data_ptr(), gaps.data_ptr(), iters.data_ptr(),
                            ops.stream_ptr(dev))
    return coefs.cpu().numpy(), gaps.cpu().numpy(), iters.cpu().numpy()


LASSO_RULES = [(1e-4, 1000), (1e-13, 20000), (1e-4, 1)]


@pytest.mark.parametrize("tol,max_iter", LASSO_RULES)
@pytest.mark.parametrize("P,A", [(1, 1), (3, 10), (3, 1), (1, 10)])
@pytest.mark.parametrize("F", [1, 2, 40, 63, 64])
def test_lasso_cd_path_certificate(dev, F, P, A, tol, max_iter):
    """coefs, gaps and iters of a direct call.  A path point that the kernel reports converged
    (its gap below tol·yy) has an oracle gap below tol·yy + budget; the kernel's gap is within the
    budget of the oracle's everywhere; iters is the number of sweeps run, max_iter when they ran
    out; zero-variance coordinates stay exactly 0; at 2×alpha_max the solution is exactly 0; at the
    tight tolerance the zeros satisfy |q_j − (Gw)_j| ≤ αn·(1 + 1e-9)."""
    first = 2.0 if A > 1 else 1.0
    G, q, yy, ns, al = _lasso_problem(F, P, A, first)
    coefs, gaps, iters = _lasso_run(dev, G, q, yy, ns, al, max_iter, tol)
    assert np.isfinite(coefs).all() and np.isfinite(gaps).all()
    assert (iters >= 1).all() and (iters <= max_iter).all(), iters
    for p in range(P):
        for a in range(A):
            w = coefs[p, a]
            gap, bud = R.lasso_gap_oracle(G[p], q[p], yy[p], ns[p], al[p, a], w)
            tol_s = L(tol) * L(yy[p])
            _seen("lasso |gap kernel - oracle| / budget", abs(L(gaps[p, a]) - gap) / bud)
            print(f"lasso F={F} P={P} A={A} tol={tol} p={p} a={a}: iters {iters[p, a]} gap kernel {gaps[p, a]:.3e} "
                  f"oracle {float(gap):.3e} budget {float(bud):.3e} tol·yy {float(tol_s):.3e}")
            assert abs(L(gaps[p, a]) - gap) <= bud, (p, a, gaps[p, a], float(gap), float(bud))
            if gaps[p, a] < tol * yy[p]:
                assert gap < tol_s + bud, (p, a, float(gap), float(tol_s), float(bud))
            else:
                assert iters[p, a] == max_iter, (p, a, iters[p, a])      # the sweeps ran out
            if max_iter == 1:
                assert iters[p, a] == 1
            if F >= 3:
                assert w[1] == 0.0
            if A > 1 and a == 0:
                assert not w.any() and iters[p, a] == 1                    # alpha = 2·alpha_max
            if tol < 1e-12 and gaps[p, a] < tol * yy[p]:
                r = np.abs(L(1) * q[p] - G[p].astype(L) @ w.astype(L))
                l1 = L(al[p, a]) * L(ns[p])
                assert (r[w == 0] <= l1 * (1 + L(1e-9))).all(), (p, a, float((r[w == 0] / l1).max()))
    if max_iter == 1 and A > 1 and F >= 40:
        # one sweep cannot converge the small alphas: the exhausted branch was taken
        assert (gaps >= tol * yy[:, None]).any()


# ----------------------------------------------------------------------------- weighted_moments
_MOM = {}


def _mom_case(n, F, P):
    if (n, F, P) not in _MOM:
        rng = np.random.default_rng(n * 131 + F * 7 + P)
        X = rng.normal(size=(n, F)) * 10.0 ** rng.uniform(-1, 1, F)
        W = 10.0 ** rng.uniform(-6, 6, size=(P, n))          # twelve decades
        W[rng.random((P, n)) < 0.2] = 0.0                    # exact zeros
        if n > 1:
            W[:, 0] = 0.0
        V = rng.normal(size=(P, n)) * 10.0 ** rng.uniform(-3, 3, size=(P, n))   # mixed sign
        _MOM[(n, F, P)] = (X, W, V, R.moments_oracle(X, W, V))
    return _MOM[(n, F, P)]


@pytest.mark.parametrize("with_v", [True, False])
@pytest.mark.parametrize("P", [1, 7])
@pytest.mark.parametrize("n,F", [(1, 1), (127, 2), (128, 63), (129, 64), (257, 65), (1000, 128)])
def test_weighted_moments_oracle(dev, n, F, P, with_v):
    """Every entry within (n + 2)·eps of its magnitude sum (an f64 sum of n terms in any order, each
    term two roundings); G exactly symmetric; a repeated call bit-identical; V = None → no v."""
    from hfens import ops
    X, W, V, (G0, a0, v0, Gm, am, vm) = _mom_case(n, F, P)
    Xd, Wd = torch.as_tensor(X).to(dev), torch.as_tensor(W).to(dev)
    Vd = torch.as_tensor(V).to(dev) if with_v else None
    G, a, v = ops.weighted_moments(Xd, Wd, Vd)
    G2, a2, v2 = ops.weighted_moments(Xd, Wd, Vd)
    assert torch.equal(G, G2) and torch.equal(a, a2)
    assert torch.equal(G, G.transpose(1, 2))
    G, a = G.cpu().numpy(), a.cpu().numpy()
    k = (n + 2) * L(EPS)
    tiny = L(np.finfo(np.float64).tiny)
    rg = np.abs(G.astype(L) - G0) / (k * Gm + tiny)
    ra = np.abs(a.astype(L) - a0) / (k * am + tiny)
    print(f"moments n={n} F={F} P={P}: G err/bound {float(rg.max()):.3e} a {float(ra.max()):.3e} "
          f"(largest so far {_seen('moments err / bound', max(rg.max(), ra.max())):.3e})")
    assert (rg <= 1).all(), float(rg.max())
    assert (ra <= 1).all(), float(ra.max())
    if with_v:
        assert torch.equal(v, v2)
        rv = np.abs(v.cpu().numpy().astype(L) - v0) / (k * vm + tiny)
        _seen("moments err / bound", rv.max())
        assert (rv <= 1).all(), float(rv.max())
    else:
        assert v is None
