"""The working-set SVC oracles (ops/reference.py: svc_dual_oracle, svc_kkt, ws_select_oracle,
ws_gupdate_budget) checked on the CPU: at libsvm's own solutions, against wrong variants of
themselves, against a brute-force selection, and the f32 → f64 write-back of svm_ws.hip emulated in
numpy.  The GPU side is tests/test_svm_ws_reference_gpu.py."""
import numpy as np
import pytest

from hfens.models import smo
from hfens.ops import reference as R

U = 2.0 ** -24
EPS = 1e-3


def _draw(n, F, seed):
    """Standardised rows (f32-representable), labels, positives first."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F))
    w = rng.normal(size=F)
    y = (X @ w / F ** 0.5 + 0.5 * rng.normal(size=n) - 1.0) > 0
    Z = ((X - X.mean(0)) / X.std(0)).astype(np.float32)
    order = np.argsort(~y, kind="stable")
    return Z[order], int(y.sum())


def _dual(Z, coef_sv, sv_idx, gamma):
    """The formula of tests/test_svm_ws_gpu.py::_dual."""
    Zs = Z[sv_idx]
    d2 = ((Zs[:, None, :] - Zs[None, :, :]) ** 2).sum(-1)
    K = np.exp(-gamma * d2)
    return 0.5 * coef_sv @ K @ coef_sv - np.abs(coef_sv).sum()


class _Case:
    def __init__(self, n, F, seed):
        from sklearn.svm import SVC
        self.Z, self.npos = _draw(n, F, seed)
        self.l, self.F = n, F
        Z64 = self.Z.astype(np.float64)
        gamma = 1.0 / (F * Z64.var())
        self.ngl2e = np.float32(-gamma * R.LOG2E)
        self.gamma64 = gamma                                      # unrounded (the γ mutant)
        self.gamma = -float(self.ngl2e) / R.LOG2E                 # the problem's γ
        self.Cp, self.Cn = n / (2.0 * self.npos), n / (2.0 * (n - self.npos))
        self.y = np.where(np.arange(n) < self.npos, 1.0, -1.0)
        lab = (self.y > 0).astype(int)
        sk = SVC(class_weight="balanced", gamma=self.gamma).fit(Z64, lab)
        a = np.zeros(n)
        a[sk.support_] = np.abs(sk.dual_coef_[0])
        assert (np.sign(sk.dual_coef_[0]) == self.y[sk.support_]).all()
        self.alpha_sk, self.rho_sk = a, -float(sk.intercept_[0])
        K = smo._gram_host(Z64, self.gamma)
        self.alpha_host, self.rho_host, _ = smo._smo_host(K, self.npos, self.Cp, self.Cn, EPS, 10 ** 7)

    def oracle(self, alpha):
        return R.svc_dual_oracle(self.Z, self.npos, self.Cp, self.Cn, self.ngl2e, alpha)

    def violations(self, o, alpha, rho_ref, slack):
        """Names of the oracle checks that ``o`` misses at ``alpha``.  ``slack``: the solver's own
        gradient error U·Σα (libsvm caches Q as float; _smo_host reads an f32 Gram), which moves
        each of the two maxima of its gap and its ρ by at most that much; γ's quantisation moves K
        by ≤ K·γd²·U ≤ U/e, inside the factor 2."""
        sv = np.flatnonzero(alpha > 0)
        ref_obj = _dual(self.Z.astype(np.float64), (self.y * alpha)[sv], sv, self.gamma)
        sumC = self.npos * self.Cp + (self.l - self.npos) * self.Cn
        bad = []
        if not o["gap"] < EPS + 2 * slack:
            bad.append("gap")
        if not abs(o["sya"]) <= 1e-12 * sumC:
            bad.append("sya")
        if not abs(o["rho"] - rho_ref) <= 2 * slack:
            bad.append("rho")
        if not abs(o["obj"] - ref_obj) <= 1e-10 * abs(ref_obj):
            bad.append("obj")
        return bad


@pytest.fixture(scope="module", params=[(400, 5, 11), (1200, 17, 12)], ids=["400x5", "1200x17"])
def case(request):
    return _Case(*request.param)


def test_oracle_at_libsvm_solution(case):
    """sklearn's SVC stops at m − M < 1e-3 on ITS gradient (float Q entries, f64 sums); the oracle's
    true gap, Σ yα, ρ and objective must agree with that solution.  The gap itself needs no slack."""
    a = case.alpha_sk
    o = case.oracle(a)
    assert o["gap"] < EPS, o["gap"]
    assert case.violations(o, a, case.rho_sk, U * a.sum()) == []
    assert o["G"].dtype == np.longdouble and abs(o["sya"] - (case.y * a).sum()) < 1e-12


def test_oracle_at_host_smo_solution(case):
    a = case.alpha_host
    assert ((a >= 0) & (a <= np.where(case.y > 0, case.Cp, case.Cn))).all()
    assert case.violations(case.oracle(a), a, case.rho_host, U * a.sum()) == []


def _mutants(c, a):
    """Wrong variants of the oracle, each composed from the same building blocks."""
    L = np.longdouble
    y, e2 = c.y.astype(L), c.ngl2e
    good = c.oracle(a)
    G = good["G"]

    def pack(Gm, kkt=None, **kw):
        aL = a.astype(L)
        o = dict(kkt if kkt is not None else R.svc_kkt(aL, Gm, c.npos, c.Cp, c.Cn))
        o.update(G=Gm, obj=(aL * (Gm - 1)).sum() / 2, sya=(y * aL).sum())
        o.update(kw)
        return o
    Kya = R.ws_kernel_matvec(c.Z, e2, c.y * a)
    C = np.where(c.y > 0, c.Cp, c.Cn)
    yield "no_minus_one", pack(y * Kya)
    yield "y_dropped", pack(-1 + Kya)
    yield "membership_swapped", pack(G, R.svc_kkt((C - a).astype(L), G, c.npos, c.Cp, c.Cn))
    yield "C_swapped", pack(G, R.svc_kkt(a.astype(L), G, c.npos, c.Cn, c.Cp))
    yield "gamma_unrounded", pack(-1 + y * R.ws_kernel_matvec(c.Z, L(-c.gamma64 * R.LOG2E), c.y * a))
    yield "rho_all_points", pack(G, rho=(y * G).mean())


def test_oracle_rejects_mutants(case):
    a = case.alpha_sk
    assert case.violations(case.oracle(a), a, case.rho_sk, U * a.sum()) == []
    seen = {}
    for name, o in _mutants(case, a):
        seen[name] = case.violations(o, a, case.rho_sk, U * a.sum())
    assert len(seen) == 6 and all(seen.values()), seen


def test_large_path_matches_longdouble(case, monkeypatch):
    """The f64 row-chunk path (above WS_LONGDOUBLE_MAX points) against the longdouble one."""
    a = case.alpha_sk
    o = case.oracle(a)
    monkeypatch.setattr(R, "WS_LONGDOUBLE_MAX", 0)
    o64 = case.oracle(a)
    nsv = (a > 0).sum()
    assert np.abs(o64["G"] - o["G"]).max() <= 4 * nsv * 2.0 ** -53 * a.sum()
    assert abs(o64["gap"] - o["gap"]) <= 8 * nsv * 2.0 ** -53 * a.sum()


def _fma32(a, b, c):
    """f32 fma: the product of two f32 is exact in f64; one f64 add, then the f32 rounding."""
    f = np.float32
    return (np.asarray(a, f).astype(np.float64) * np.asarray(b, f).astype(np.float64)
            + np.asarray(c, f).astype(np.float64)).astype(f)


def test_gupdate_budget_covers_f32_emulation(case):
    """One gradient update emulated in numpy f32 the way the kernel evaluates it (k-ordered fma
    chains, ‖a‖² + ‖b‖² − 2a·b, exp2 rounded to f32, the two half-chains of a lane pair and their
    final add) stays inside ws_gupdate_budget in both forms, the summation-tree form is the tighter
    one, and neither is vacuous."""
    rng = np.random.default_rng(3)
    Z, l, F = case.Z, case.l, case.F
    d = np.zeros(l)
    cols = rng.choice(l, 96, replace=False)
    d[cols] = rng.normal(size=96) * 0.3
    f = np.float32
    sn = np.zeros(l, f)
    for k in range(F):
        sn = _fma32(Z[:, k], Z[:, k], sn)
    sn = case.ngl2e * sn
    k2 = f(-2) * case.ngl2e
    part = [np.zeros(l, f), np.zeros(l, f)]
    for p, c in enumerate(cols):
        dot = np.zeros(l, f)
        for k in range(F):
            dot = _fma32(Z[c, k], Z[:, k], dot)
        e = np.minimum(_fma32(k2, dot, sn + sn[c]), f(0))
        h = (p // 4) % 2
        part[h] = _fma32(f(case.y[c] * d[c]), np.exp2(e.astype(np.float64)).astype(f), part[h])
    acc = part[0] + part[1]
    exact = R.ws_kernel_matvec(Z, case.ngl2e, case.y * d)
    err = np.abs(acc.astype(np.longdouble) - exact)
    worst = R.ws_gupdate_budget(Z, case.ngl2e, d, 96)
    tree = R.ws_gupdate_budget(Z, case.ngl2e, d, 96, order=cols, npos=case.npos)
    assert (err <= tree).all(), float((err / tree).max())
    assert (tree <= worst).all() and tree.max() < 1e-4 * np.abs(d).sum()
    some = [3, 77, l - 1]
    assert np.allclose(R.ws_gupdate_budget(Z, case.ngl2e, d, 96, order=cols, npos=case.npos, rows=some), tree[some],
                       rtol=1e-12, atol=0)     # (BLAS blocks differently for three rows)
    print("emulated / tree budget", float((err / tree).max()))


# ------------------------------------------------------------------------------- selection
def _select_brute(alpha, G, npos, Cp, Cn, Q, prev, bits=R.WS_KEY_BITS):
    l = len(alpha)
    taken, lists = set(), []
    for side in (0, 1):
        cand = []
        for t in range(l):
            yv = 1 if t < npos else -1
            C = Cp if yv > 0 else Cn
            member = (alpha[t] < C if yv > 0 else alpha[t] > 0) if side == 0 else \
                     (alpha[t] > 0 if yv > 0 else alpha[t] < C)
            if member:
                v = np.float32(-yv * G[t] if side == 0 else yv * G[t])
                cand.append((t, v))
        k = min(Q // 4, len(cand))
        cand = [(t, int(R.ws_okey(v)) >> (32 - bits)) for t, v in cand]
        ranked = sorted(cand, key=lambda c: (-c[1], c[0]))
        T = ranked[k - 1][1] if k else None
        need = k - sum(1 for _, key in cand if key > T) if k else 0
        picks = [t for t, key in cand if key > T and t not in taken] if k else []
        for t, key in sorted(cand):
            if need > 0 and key == T and t not in taken:
                picks.append(t)
                need -= 1
        taken |= set(picks)
        lists.append(sorted(picks))
    return lists[0], lists[1], [p for p in prev if p not in taken]


def _sel_cases():
    rng = np.random.default_rng(9)
    # first round: every pick by position
    yield "first_round", np.zeros(40), -np.ones(40), 15, 1.0, 0.7, 16, []
    # n_up < Q/4: only two points can go up
    a = np.zeros(30)
    a[:10] = 1.0
    a[3] = 0.4
    a[12] = 0.2
    yield "few_up", a, rng.normal(size=30), 10, 1.0, 0.7, 32, [3, 29]
    # free points are eligible for both lists; previous picks partly picked again
    a = rng.random(60) * 0.7
    a[rng.random(60) < 0.3] = 0.0
    yield "both_lists", a, rng.normal(size=60), 25, 1.0, 0.7, 16, [0, 5, 17, 33, 59, 2]
    # ties inside the 22-bit window, and exact ties
    G = np.round(rng.normal(size=80), 1) * (1 + 2.0 ** -15 * rng.integers(0, 3, 80))
    a = rng.random(80) * 0.5
    yield "ties", a, G, 33, 1.0, 0.7, 24, list(range(0, 80, 7))
    # twelve free points, lists of eight: the lists' tops overlap
    yield "overlap", np.full(12, 0.3), rng.normal(size=12), 6, 1.0, 0.7, 32, [1, 2]
    yield "empty_low", np.concatenate([np.zeros(5), np.full(5, 0.7)]), rng.normal(size=10), 5, 1.0, 0.7, 8, []


@pytest.mark.parametrize("name,alpha,G,npos,Cp,Cn,Q,prev", list(_sel_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_select_oracle_matches_brute_force(name, alpha, G, npos, Cp, Cn, Q, prev):
    up, low, carried = R.ws_select_oracle(alpha, G, npos, Cp, Cn, Q, prev)
    if name == "empty_low":
        assert up.size == low.size == carried.size == 0
        return
    bu, bl, bc = _select_brute(alpha, G, npos, Cp, Cn, Q, prev)
    assert list(up) == bu and list(low) == bl and list(carried) == bc
    assert not set(up) & set(low)
    # the 22-bit ranking never leaves out a member more than 2⁻¹³ (relative) above a picked one
    pos = np.arange(len(alpha)) < npos
    yG = np.where(pos, G, -G).astype(np.float32)
    C = np.where(pos, Cp, Cn)
    member = np.where(pos, alpha < C, alpha > 0)
    if len(up) and len(up) < member.sum():
        out = member.copy()
        out[up] = False
        assert (-yG[out]).max() <= (-yG[up]).min() + 2.0 ** -13 * np.abs(yG).max()
    if name == "overlap":
        assert len(up) == 8 and len(low) < 8            # up picks left out of the low list, not replaced
    if name == "first_round":
        assert list(up) == [0, 1, 2, 3] and list(low) == [15, 16, 17, 18]
    if name == "few_up":
        assert len(up) < Q // 4
    if name == "both_lists":
        assert set(prev) & (set(up) | set(low)) and len(carried) < len(prev)


# ------------------------------------------------------------------------------- write-back
def _writeback(a32, a0, C, clamp):
    """ws_solve_kernel / ws_kc_round_kernel's publication of one slot: f32 α ``a32`` after the
    inner solve, f64 α ``a0`` before it."""
    a32 = np.float32(a32)
    anew = a0
    if a32 != np.float32(a0):
        if a32 <= np.float32(0):
            anew = 0.0
        elif a32 >= np.float32(C):
            anew = C
        else:
            anew = a0 + (float(a32) - float(np.float32(a0)))
        if clamp:
            anew = min(max(anew, 0.0), C)
    return anew


def _near_bounds(C):
    f = np.float32
    out = [f(2.0) ** f(-k) for k in range(20, 150)]           # tiny positive f32 down to the subnormals
    x = f(0)
    for _ in range(64):
        x = np.nextafter(x, f(1))
        out.append(x)
    x = f(C)
    for _ in range(64):
        x = np.nextafter(x, f(0))
        out.append(x)
    return out


def test_writeback_stays_in_the_box():
    """``anew = a0 + ((double)a − (double)(float)a0)`` leaves [0, C] WITHOUT the f64 clamp: with
    (float)a0 above a0 (a0 = 0.3: by 1.19e-8) every positive f32 a below that difference gives
    anew < 0 — e.g. a0 = 0.3, a = 2⁻³⁰: anew = −1.1e-8.  (Reaching such an a needs a pair step that
    stops within half an f32 ulp of a0 above zero without being clipped to it: rare, not
    impossible, since the step is an arbitrary f32.)  Above C it is not reachable: a < (float)C means
    a ≤ (float)C − ulp, (float)C − C ≤ ulp/2 and a0 − (float)a0 ≤ ulp/2, so anew ≤ C.  The kernels
    now clamp anew in f64; this emulation is the regression test: the clamped form never leaves
    the box and changes no bit of a result that was inside it."""
    below, above = [], []
    for C in (0.9, 1.3, 0.1):            # (float)C rounds down, down, up
        for a0 in (0.3, 0.1, np.nextafter(C, 0.0)):
            if a0 > C:
                continue
            for a in _near_bounds(C):
                raw = _writeback(a, a0, C, False)
                fix = _writeback(a, a0, C, True)
                assert 0.0 <= fix <= C
                if 0.0 <= raw <= C:
                    assert raw == fix
                elif raw < 0.0:
                    below.append((C, a0, float(a), raw))
                else:
                    above.append((C, a0, float(a), raw))
    assert below and all(float(np.float32(a0)) > a0 for _, a0, _, _ in below), below[:3]
    assert not above, above[:3]
