"""The oracles and certificates of the Nyström interior-point SVC (ops/reference.py: wgram_oracle,
phi_mv_oracle, phit_oracle, rbf_oracle_f64, chol_certificate, chol_solve_certificate,
ipm_rows_oracle, svc_dual_certificate) checked on the CPU: each against an answer known in closed
form, and each certificate against planted faults of the kind a kernel could produce.

Of the planted faults below, the flat tolerances that tests/test_linalg_gpu.py used before
(``max|err| / max|want| < 1e-12`` on the Gram, ``atol=1e-5`` on L Lᵀ after a jitter retry) would have ACCEPTED: a zeroed or transposed output tile whose entries are small beside the
largest entry of S, a dropped row tail whose weights are small, and a jitter of the wrong rung; the
tests named ``*_flat_tolerance_accepted`` show each with the old formula next to the certificate's
verdict."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

from hfens.ops import reference as R

LD = np.longdouble


def _rng(seed):
    return np.random.default_rng(seed)


# ---------------------------------------------------------------------------------- known answers
def _hadamard(k):
    H = np.array([[1.0]])
    for _ in range(k):
        H = np.block([[H, H], [H, -H]])
    return H


def test_wgram_of_an_orthonormal_map_is_the_identity():
    Phi = _hadamard(4)[:, :8] / 4.0          # 16 × 8, exactly orthonormal columns (entries ±¼)
    S, M = R.wgram_oracle(Phi, np.ones(16))
    assert (S == np.eye(8)).all()
    assert (M == np.full((8, 8), 1.0)).all()
    # weights: S_jk = Σ_i d_i φ_ij φ_ik in exact rationals
    d = _rng(0).integers(-5, 9, 16).astype(np.float64) / 8
    S, M = R.wgram_oracle(Phi, d)
    for j, k in ((0, 0), (1, 5), (7, 2)):
        want = sum(Fraction(d[i]) * Fraction(Phi[i, j]) * Fraction(Phi[i, k]) for i in range(16))
        assert Fraction(float(S[j, k])) == want
        assert Fraction(float(M[j, k])) == sum(abs(Fraction(d[i])) for i in range(16)) / 16


def test_skinny_oracles_against_rationals():
    g = _rng(1)
    Phi = g.integers(-8, 8, (7, 5)).astype(np.float64) / 4
    W = g.integers(-8, 8, (5, 3)).astype(np.float64) / 2
    V = g.integers(-8, 8, (7, 2)).astype(np.float64) / 2
    Y, Ym = R.phi_mv_oracle(Phi, W)
    O, Om = R.phit_oracle(Phi, V)
    assert (Y == (Phi @ W)).all() and (Ym == np.abs(Phi) @ np.abs(W)).all()      # small dyadics: exact in f64
    assert (O == (Phi.T @ V)).all() and (Om == np.abs(Phi).T @ np.abs(V)).all()


def test_rbf_of_identical_rows_is_one_and_far_rows_underflow():
    A = _rng(2).standard_normal((4, 7))
    K, dK = R.rbf_oracle_f64(A, A, 0.3)
    assert (np.diagonal(K) == 1).all()
    assert (np.diagonal(dK) == LD(R.LR_EXP_ULP) * 2 * LD(R.LR_U)).all()   # d² = 0: only exp's own error
    # a closed form: ‖a − b‖² = 4, γ = ¼: e⁻¹
    K, dK = R.rbf_oracle_f64(np.array([[1.0, 0.0]]), np.array([[-1.0, 0.0]]), 0.25)
    assert abs(K[0, 0] - np.exp(LD(-1))) < 1e-18
    assert 0 < dK[0, 0] < 1e-14
    K, dK = R.rbf_oracle_f64(np.array([[0.0]]), np.array([[40.0]]), 1.0)   # e⁻¹⁶⁰⁰ < 2⁻¹⁰⁷⁴
    assert K[0, 0] < LD(2.0) ** -1074 and dK[0, 0] >= LD(2.0) ** -1022
    # the difference form keeps what the GEMM form loses: rows near 1e6, 1e-3 apart
    a = np.array([[1e6, -1e6, 1e6]])
    b = a + 1e-3
    K, dK = R.rbf_oracle_f64(a, b, 1.0)
    t = (_ld(b) - _ld(a))[0]
    assert abs(K[0, 0] - np.exp(-(t * t).sum())) < 1e-18 and dK[0, 0] < 1e-14


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _known_factor(r, seed, spread=0):
    """(S, L, sc): S = L0 L0ᵀ from an integer lower-triangular L0 (exact), sc = fl(diag(S)^-½) and
    L = fl(sc_i·L0_ij), the factor of sc·S·sc up to one rounding per entry.  ``spread``: rows and
    columns of S scaled by powers of two spanning that many binary orders (exact)."""
    g = _rng(seed)
    L0 = np.tril(g.integers(-3, 4, (r, r))).astype(np.float64)
    L0[np.arange(r), np.arange(r)] = g.integers(2, 6, r)
    if spread:
        L0 = L0 * np.exp2(g.integers(-spread, spread + 1, r))[:, None]
    S = L0 @ L0.T
    sc = 1.0 / np.sqrt(np.diagonal(S))
    return S, sc[:, None] * L0, sc


def _plain_chol(S):
    """Unblocked right-looking Cholesky of the equilibrated S in plain f64: (L, sc)."""
    r = S.shape[0]
    sc = 1.0 / np.sqrt(np.diagonal(S))
    A = np.tril(S * sc[:, None] * sc[None, :])
    for j in range(r):
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        for k in range(j + 1, r):
            A[k:, k] -= A[k:, j] * A[k, j]
    return A, sc


def _plain_solve(L, sc, B):
    """sc ∘ (L Lᵀ)⁻¹ (sc ∘ B) by plain f64 substitution."""
    r = L.shape[0]
    X = B * sc[:, None]
    for i in range(r):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    for i in range(r - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X * sc[:, None]


@pytest.mark.parametrize("r", [2, 5, 33])
def test_chol_certificate_accepts_a_factor_built_from_a_known_L(r):
    S, L, sc = _known_factor(r, r)
    cert = R.chol_certificate(S, L, sc, 0)
    assert cert.ok, cert
    assert R.chol_jitter(0) == 0.0 and R.chol_jitter(1) == 1e-14 and R.chol_jitter(3) == 1e-14 * 100.0 * 100.0
    # and a plain f64 factorisation of a badly scaled SPD matrix, with its substitutions
    g = _rng(r)
    A = g.standard_normal((r, 2 * r))
    dsc = np.exp(g.uniform(-9, 9, r))
    S = dsc[:, None] * (A @ A.T) * dsc[None, :]
    L, sc = _plain_chol(S)
    assert R.chol_certificate(S, L, sc, 0).ok
    B = g.standard_normal((r, 4))
    assert R.chol_solve_certificate(L, sc, B, _plain_solve(L, sc, B)).ok


def _enumerate_svc(Phi, y, c):
    """The C-SVC dual's optimum by enumerating the active sets: every split of the points into
    (at 0, free, at c); the free block from the KKT equations; the first split whose solution is
    feasible with the right multiplier signs.  Returns (α, ρ)."""
    l = len(y)
    Q = (y[:, None] * Phi) @ (y[:, None] * Phi).T
    for st in itertools.product((0, 1, 2), repeat=l):
        st = np.array(st)
        F = np.nonzero(st == 1)[0]
        if F.size == 0 or F.size > Phi.shape[1] + 1:
            continue
        a = np.where(st == 2, c, 0.0)
        A = np.zeros((F.size + 1, F.size + 1))
        A[:-1, :-1] = Q[np.ix_(F, F)]
        A[:-1, -1] = y[F]
        A[-1, :-1] = y[F]
        rhs = np.concatenate([1.0 - Q[F] @ a, [-(y @ a)]])
        if abs(np.linalg.det(A)) < 1e-9:
            continue
        sol = np.linalg.solve(A, rhs)
        a[F] = sol[:-1]
        b = sol[-1]
        q = Q @ a + b * y - 1.0
        if ((a[F] > 1e-9) & (a[F] < c[F] - 1e-9)).all() and (q[st == 0] >= -1e-12).all() and (q[st == 2] <= 1e-12).all():
            return a, -b
    raise AssertionError("no optimal active set")


def test_svc_certificate_on_the_two_point_problem():
    # φ = ±1, y = ±1: α = (½, ½), w = 1, ρ = 0, objective Σα − ½w² = ½
    Phi, y, c = np.array([[1.0], [-1.0]]), np.array([1.0, -1.0]), np.array([10.0, 10.0])
    cert = R.svc_dual_certificate(Phi, y, c, np.array([0.5, 0.5]), 0.0, rd_tol=1e-8)
    assert cert.ok, cert
    assert cert.extra["w"][0] == 1 and cert.extra["D"] == 0.5 and cert.extra["P"] == 0.5 and cert.extra["gap"] == 0
    assert not R.svc_dual_certificate(Phi, y, c, np.array([0.5, 0.5]), 1e-4, rd_tol=1e-8).ok
    assert not R.svc_dual_certificate(Phi, y, c, np.array([0.4, 0.4]), 0.0, rd_tol=1e-8).ok


SIX = (np.array([[2.0, 1.0], [1.5, 2.5], [3.0, 0.5], [-1.0, -1.5], [-2.0, 0.5], [0.25, -2.0]]),
       np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0]))


@pytest.mark.parametrize("cval", [100.0, 0.05])
def test_svc_certificate_on_six_points_by_enumeration(cval):
    """Separable (large C: no point at its upper bound) and soft (small C: bounded points)."""
    Phi, y = SIX
    c = np.full(6, cval)
    a, rho = _enumerate_svc(Phi, y, c)
    if cval > 1:
        assert (a < cval).all() and (y * (Phi @ (Phi.T @ (y * a)) - rho) >= 1 - 1e-12).all()
    else:
        assert (a == cval).any()
    cert = R.svc_dual_certificate(Phi, y, c, a, rho, rd_tol=1e-8)
    assert cert.ok, cert
    assert abs(cert.extra["gap"]) < 1e-12 * (1 + abs(cert.extra["D"]))
    # another optimal α cannot exist here (Q restricted to the free points is regular), but a
    # non-optimal feasible one must fail on the gap alone
    bad = a.copy()
    i, j = np.nonzero((a > 0) & (y > 0))[0][0], np.nonzero((a > 0) & (y < 0))[0][0]
    bad[i] += 1e-3 * cval
    bad[j] += 1e-3 * cval                                   # keeps yᵀα = 0 and the box
    if (bad <= c).all():
        cert = R.svc_dual_certificate(Phi, y, c, bad, rho, rd_tol=1e-8)
        assert cert.why == ["gap"], cert


def test_ipm_rows_oracle_on_hand_values():
    o = R.ipm_rows_oracle
    one = lambda v: np.array([v], dtype=np.float64)   # noqa: E731
    s, rd = o.resid(one(3.0), one(1.0), one(-1.0), one(0.5), 0.25, one(2.0), one(4.0))
    assert s[0] == 2.0 and rd[0] == (((-1.0 * 0.5 - 1.0) + 0.25 * -1.0) - 2.0) + 4.0
    di, di2, rn, rm, H2 = o.pred(one(1.0), one(2.0), one(3.0), one(4.0), one(0.5), one(-1.0))
    assert di[0] == 1.0 / 5.0 and (di2 == 0.2).all() and rn[0] == 3.0 and rm[0] == 8.0
    assert H2[0, 0] == (-0.5 - 3.0) + 4.0 and H2[0, 1] == -1.0
    assert o.max_step([(one(1.0), one(2.0))] * 4, (1, 1, 1, 1)) == 1.0          # no negative direction
    assert o.max_step([(one(3.0), one(-2.0))] * 4, (1, 1, 1, 1)) == 1.0         # ratio 1.5 > 1
    z = o.max_step([(one(0.0), one(-2.0))] + [(one(1.0), one(1.0))] * 3, (1, 1, 1, 1))
    assert z == 0.0 and not np.signbit(z)
    assert o.max_step([(one(1.0), one(4.0))] * 4, (1, -1, 1, 1)) == 0.25        # the slack pair: −Δα
    a, b, c3 = o.select3(False, (one(1.0),) * 3, (one(np.nan),) * 3)
    assert np.isnan(a[0]) and np.isnan(c3[0])
    assert (o.fill(3, 0.5) == 0.5).all()
    assert (o.scale_rows(np.array([[1.5, 2.0]], dtype=np.float32), one(3.0)) == [[4.5, 6.0]]).all()


# ---------------------------------------------------------------------------------- planted faults
def _gram_case(n, r, seed, colscale=None, d=None):
    g = _rng(seed)
    Phi = g.standard_normal((n, r)).astype(np.float32).astype(np.float64)
    if colscale is not None:
        Phi = Phi * colscale[None, :]
    d = np.exp(g.uniform(-2, 2, n)) if d is None else d
    return Phi, d


def _f64_gram(Phi, d):
    S = (Phi * d[:, None]).T @ Phi             # an f64 sum of the n terms in the library's order
    return np.triu(S) + np.triu(S, 1).T        # mirrored, as the kernels' reduction does


def _flat(got, want):
    """The former test's measure: max|err| / max|want|."""
    return float(np.abs(got - np.asarray(want, dtype=np.float64)).max() / np.abs(np.asarray(want, dtype=np.float64)).max())


def _gram_ok(got, S, M, n, f32=False):
    bound = R.wgram_bound_f32(M, n) if f32 else R.wgram_bound_f64(M, n)
    return R.entries_within("gram", got, S, bound).ok and (got == got.T).all()


def test_gram_bound_accepts_an_f64_product_and_rejects_tile_faults():
    n, r = 300, 192
    Phi, d = _gram_case(n, r, 3)
    S, M = R.wgram_oracle(Phi, d)
    good = _f64_gram(Phi, d)
    assert _gram_ok(good, S, M, n)
    for I, J in ((0, 1), (1, 1), (2, 0)):
        z = good.copy()
        z[64 * I:64 * I + 64, 64 * J:64 * J + 64] = 0.0                       # one 64 × 64 tile zeroed
        assert not _gram_ok(z, S, M, n), (I, J)
        t = good.copy()
        t[64 * I:64 * I + 64, 64 * J:64 * J + 64] = good[64 * I:64 * I + 64, 64 * J:64 * J + 64].T.copy()
        if I != J:                                                            # (a diagonal tile is symmetric)
            assert not _gram_ok(t, S, M, n), (I, J)
    low = np.triu(good)                                                       # lower triangle not mirrored
    assert not _gram_ok(low, S, M, n)
    assert not R.entries_within("gram", low, S, R.wgram_bound_f64(M, n)).ok
    assert not _gram_ok(_f64_gram(Phi, d * d), S, M, n)                       # d applied twice
    z = good.copy()
    z[:128, :128] = 0.0                                                       # one 128 × 128 tile
    assert not _gram_ok(z, S, M, n)


def test_tile_fault_flat_tolerance_accepted():
    """Columns 128… scaled by 1e-7: tile (2, 2) holds entries 1e-14 of the largest.  Zeroing or
    transposing it moves max|err| / max|want| by 1e-14 — the old 1e-12 passes; the per-entry bound
    does not."""
    n, r = 300, 192
    cs = np.where(np.arange(r) >= 128, 1e-7, 1.0)
    Phi, d = _gram_case(n, r, 4, colscale=cs)
    S, M = R.wgram_oracle(Phi, d)
    good = _f64_gram(Phi, d)
    assert _gram_ok(good, S, M, n)
    z = good.copy()
    z[128:, 128:] = 0.0
    assert _flat(z, S) < 1e-12 and not _gram_ok(z, S, M, n)
    t = good.copy()
    t[130:150, 160:180] = good[130:150, 160:180].T.copy()      # part of the tile transposed in place
    t[160:180, 130:150] = t[130:150, 160:180].T
    assert _flat(t, S) < 1e-12 and (t == t.T).all() and not _gram_ok(t, S, M, n)


def test_dropped_row_tail_rejected_and_flat_tolerance_accepted():
    n, r = 35, 68                                  # slab 32: a tail of 3 rows
    Phi, d = _gram_case(n, r, 5)
    S, M = R.wgram_oracle(Phi, d)
    assert _gram_ok(_f64_gram(Phi, d), S, M, n)
    assert not _gram_ok(_f64_gram(Phi[:32], d[:32]), S, M, n)
    # d non-zero only in the last row: the dropped tail leaves S = 0
    d1 = np.zeros(n)
    d1[-1] = 2.5
    S1, M1 = R.wgram_oracle(Phi, d1)
    assert _gram_ok(_f64_gram(Phi, d1), S1, M1, n) and not _gram_ok(np.zeros((r, r)), S1, M1, n)
    # tail weights 3e-13 of the rest: 1e-14 of every entry's terms, under the flat 1e-12, over γ_{n+2}
    d2 = d.copy()
    d2[32:] *= 3e-13
    S2, M2 = R.wgram_oracle(Phi, d2)
    cut = _f64_gram(Phi[:32], d2[:32])
    assert _gram_ok(_f64_gram(Phi, d2), S2, M2, n)
    assert _flat(cut, S2) < 1e-12 and not _gram_ok(cut, S2, M2, n)


def _f32_gram(Phi, d, skip=None):
    """wsyrk_f32's arithmetic: B = f32(d·φ), f32 products and sums over 256-row flushes, f64 beyond."""
    n, r = Phi.shape
    A = Phi.astype(np.float32)
    B = (Phi * d[:, None]).astype(np.float32)
    S = np.zeros((r, r))
    for k, s in enumerate(range(0, n, R.LR_WF_FLUSH)):
        if k == skip:
            continue
        S += (A[s:s + 256].T @ B[s:s + 256]).astype(np.float64)
    return np.triu(S) + np.triu(S, 1).T


def test_f32_gram_bound_accepts_the_flush_arithmetic_and_rejects_a_lost_flush():
    n, r = 1100, 68
    Phi, d = _gram_case(n, r, 6)
    S, M = R.wgram_oracle(Phi, d)
    assert _gram_ok(_f32_gram(Phi, d), S, M, n, f32=True)
    assert not _gram_ok(_f32_gram(Phi, d), S, M, n)                    # f32 sums are not f64 sums
    for k in (0, 2, 4):
        assert not _gram_ok(_f32_gram(Phi, d, skip=k), S, M, n, f32=True), k
    # the constant is the formula, not a number: it scales with the rows in one flush
    one = np.ones((1, 1), dtype=LD)
    assert R.wgram_bound_f32(one, 1)[0, 0] < 2e-7 and 1.5e-5 < R.wgram_bound_f32(one, 4099)[0, 0] < 1.6e-5
    assert R.wgram_bound_f32(one, 256)[0, 0] == R.wgram_bound_f32(one, 256 + 0)[0, 0]
    assert float(R.wgram_bound_f64(one, 4099)[0, 0]) == pytest.approx(4101 * 2.0 ** -53, rel=1e-9)


def test_skinny_bounds_reject_a_dropped_row_and_column():
    g = _rng(7)
    Phi = g.standard_normal((130, 36)).astype(np.float32).astype(np.float64)
    W, V = g.standard_normal((36, 3)), g.standard_normal((130, 3))
    Y, Ym = R.phi_mv_oracle(Phi, W)
    O, Om = R.phit_oracle(Phi, V)
    assert R.entries_within("y", Phi @ W, Y, R.lr_gamma(37) * Ym).ok
    assert R.entries_within("o", Phi.T @ V, O, R.lr_gamma(131) * Om).ok
    assert not R.entries_within("y", Phi[:, :32] @ W[:32], Y, R.lr_gamma(37) * Ym).ok      # last 4 columns
    assert not R.entries_within("o", Phi[:128].T @ V[:128], O, R.lr_gamma(131) * Om).ok    # last 2 rows
    sw = (Phi.T @ V)[:, [1, 0, 2]]                                                          # columns of V swapped
    assert not R.entries_within("o", sw, O, R.lr_gamma(131) * Om).ok


def test_chol_certificate_rejects_planted_faults():
    r = 48
    S, L, sc = _known_factor(r, 11)
    assert R.chol_certificate(S, L, sc, 0).ok
    sh = L.copy()
    sh[16:, 5] = L[:-16, 5]                        # one column offset by a 16-row MFMA block
    sh[:16, 5] = 0.0
    assert "factor" in R.chol_certificate(S, sh, sc, 0).why
    up = L.copy()
    up[3, 40] = 1e-300
    assert R.chol_certificate(S, up, sc, 0).why == ["upper"]
    neg = L.copy()
    neg[:, 7] = -neg[:, 7]                         # L Lᵀ unchanged, but not the Cholesky factor
    assert R.chol_certificate(S, neg, sc, 0).why == ["diag"]
    s2 = sc.copy()
    s2[9] *= 1 + 2.0 ** -50                        # 4 ulp
    assert "sc" in R.chol_certificate(S, L, s2, 0).why
    assert "info" in R.chol_certificate(S, L, sc, -1).why
    # jitter: the factor of sc·S·sc + 1e-12·I is certified at rung 2 and at no other
    Ss = _ld(S) * _ld(sc)[:, None] * _ld(sc)[None, :]
    Lj, _ = _plain_chol(np.asarray(Ss + LD(R.chol_jitter(2)) * np.eye(r), dtype=np.float64) / 1.0)
    # (_plain_chol re-equilibrates a unit-diagonal matrix by 1 ± 1e-12: undo it exactly in longdouble)
    dj = np.sqrt(np.diagonal(Ss) + LD(R.chol_jitter(2)))
    Lj = np.asarray(_ld(Lj) * dj[:, None], dtype=np.float64)
    assert R.chol_certificate(S, Lj, sc, 2).ok
    for wrong in (0, 1, 3):
        assert "factor" in R.chol_certificate(S, Lj, sc, wrong).why, wrong


def test_jitter_rung_flat_tolerance_accepted():
    """``allclose(L Lᵀ, Ss, atol=1e-5)`` (the former jitter test) cannot tell a jitter of 1e-10 from
    none: the factor of Ss passes it against Ss + 1e-10·I; the certificate rejects every wrong rung."""
    r = 48
    S, L, sc = _known_factor(r, 12, spread=20)
    assert R.chol_certificate(S, L, sc, 0).ok
    Ss = S * sc[:, None] * sc[None, :]
    assert np.allclose(L @ L.T, Ss + 1e-10 * np.eye(r), atol=1e-5, rtol=0)        # wrong matrix, old check passes
    for wrong in (1, 2, 3, 4):
        assert not R.chol_certificate(S, L, sc, wrong).ok, wrong


def test_chol_solve_certificate_rejects_planted_faults():
    r = 40
    g = _rng(13)
    A = g.standard_normal((r, 2 * r))
    dsc = np.exp(g.uniform(-7, 7, r))
    S = dsc[:, None] * (A @ A.T) * dsc[None, :]
    L, sc = _plain_chol(S)
    B = g.standard_normal((r, 4))
    X = _plain_solve(L, sc, B)
    assert R.chol_solve_certificate(L, sc, B, X).ok
    one_sided = X / sc[:, None]                                   # sc applied on one side only
    assert not R.chol_solve_certificate(L, sc, B, one_sided).ok
    un = X.copy()
    un[:, 2] = B[:, 2]                                            # one right-hand side of four left unsolved
    assert R.chol_solve_certificate(L, sc, B, un).why == ["rhs2"]
    sw = X[:, [1, 0, 2, 3]]
    assert R.chol_solve_certificate(L, sc, B, sw).why == ["rhs0", "rhs1"]
    fw = X.copy()
    fw[r - 1] *= 1 + 1e-9                                         # the last back-substitution row off
    assert not R.chol_solve_certificate(L, sc, B, fw).ok


def test_svc_certificate_rejects_planted_faults():
    Phi, y = SIX
    c = np.full(6, 0.05)
    a, rho = _enumerate_svc(Phi, y, c)
    assert R.svc_dual_certificate(Phi, y, c, a, rho, rd_tol=1e-8).ok
    out = a.copy()
    i = int(np.argmax(a == c))
    out[i] = c[i] + 1e-6                                          # one component 1e-6 outside its box
    assert "box" in R.svc_dual_certificate(Phi, y, c, out, rho, rd_tol=1e-8).why
    neg = a.copy()
    neg[int(np.argmin(a))] = -1e-6
    assert "box" in R.svc_dual_certificate(Phi, y, c, neg, rho, rd_tol=1e-8).why
    assert R.svc_dual_certificate(Phi, y, c, a, rho + 1e-4, rd_tol=1e-8).why == ["gap"]     # ρ shifted
    assert R.svc_dual_certificate(Phi, y, c, a, rho - 1e-4, rd_tol=1e-8).why == ["gap"]
    un = a.copy()
    un[int(np.nonzero((a > 0) & (a < c))[0][0])] += 1e-5          # yᵀα = ±1e-5 ≫ 1.1e-8·Σc
    assert "eq" in R.svc_dual_certificate(Phi, y, c, un, rho, rd_tol=1e-8).why
    # the constants the certificate restates are the solver's
    from hfens.models import svc_lowrank
    assert (svc_lowrank.IPM_TOL, svc_lowrank.RD_LOOSE) == (R.LR_IPM_TOL, R.LR_RD_LOOSE)


def test_rbf_bound_rejects_the_gemm_form_and_a_wrong_gamma():
    g = _rng(17)
    A = 1e6 + 1e-3 * g.standard_normal((5, 9))
    B = 1e6 + 1e-3 * g.standard_normal((6, 9))
    K, dK = R.rbf_oracle_f64(A, B, 1e5)
    diff = np.exp(-1e5 * ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))
    assert R.entries_within("k", diff, K, dK).ok
    gemm = np.exp(-1e5 * np.clip((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2 * A @ B.T, 0, None))
    assert not R.entries_within("k", gemm, K, dK).ok
    A, B = g.standard_normal((5, 9)), g.standard_normal((6, 9))
    K, dK = R.rbf_oracle_f64(A, B, 0.11)
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    assert R.entries_within("k", np.exp(-0.11 * d2), K, dK).ok
    assert not R.entries_within("k", np.exp(-0.11 * (1 + 1e-13) * d2), K, dK).ok
    assert not R.entries_within("k", np.exp(-0.11 * d2).T[:5, :5], K[:5, :5], dK[:5, :5]).ok
