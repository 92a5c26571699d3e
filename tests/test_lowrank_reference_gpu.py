"""The Nyström interior-point SVC's kernels (ops/csrc/lowrank.hip, linalg.hip, nystrom.hip) against the
oracles and certificates of ops/reference.py, called through the extension directly at the smallest
shapes that cross each boundary in the code.  Every assertion is a derived per-entry bound
(u = 2⁻⁵³, γ_k = k·u/(1 − k·u); the derivations stand next to the oracles), a certificate, or a bit
equality; nothing is compared with torch on the device.  Each test prints the largest error it saw
as a fraction of its bound (``-s`` shows them; profiles/lowrank_oracles.md records them)."""
import functools

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.ops import reference as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
F64 = torch.float64


def _t(x, dev):
    return torch.from_numpy(np.array(x, order="C")).to(dev)          # (a copy: cached problems are read-only)


def _len(fn, *args):
    out = np.zeros(1, dtype=np.int64)
    getattr(ops.ext(), fn)(*[int(a) for a in args], out.ctypes.data)
    return int(out[0])


def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _report(name, cert):
    print(f"[lowrank-oracle] {name} " + " ".join(f"{k}={v:.3g}" for k, v in cert.worst.items()))


# ------------------------------------------------------------------------------------ weighted Gram
def _weights(kind, n, g):
    if kind == "decades":                       # 12 decades
        return g.uniform(0.1, 1.0, n) * 10.0 ** g.integers(-6, 6, n)
    if kind == "zeros":                         # exact zeros among them
        d = g.uniform(0.5, 2.0, n)
        d[g.random(n) < 0.4] = 0.0
        d[0] = 0.0
        return d
    d = np.zeros(n)                             # "last": only the last row counts — a dropped tail gives S = 0
    d[-1] = 1.75
    return d


@functools.lru_cache(maxsize=None)
def _gram_problem(n, r, kind, f32):
    g = np.random.default_rng(1000003 * n + 131 * r + len(kind) + 7 * f32)
    Phi = g.standard_normal((n, r))
    if f32:
        Phi = Phi.astype(np.float32).astype(np.float64)
    d = _weights(kind, n, g)
    S, M = R.wgram_oracle(Phi, d)
    for a in (Phi, d, S, M):
        a.setflags(write=False)
    return Phi, d, S, M


def _wsyrk(kern, Phi, d, dev):
    n, r = Phi.shape
    E = ops.ext()
    P = _t(Phi if kern == "f64" else Phi.astype(np.float32), dev)
    dd = _t(d, dev)
    plen = _len("wsyrk_part_len", n, r)
    part = torch.empty(plen, dtype=F64, device=dev)
    S = torch.full((r, r), float("nan"), dtype=F64, device=dev)
    getattr(E, "wsyrk_" + kern)(P.data_ptr(), dd.data_ptr(), n, r, part.data_ptr(), plen, S.data_ptr(),
                                ops.stream_ptr(dev))
    return S.cpu().numpy()


def _check_gram(kern, n, r, kind, dev):
    Phi, d, S, M = _gram_problem(n, r, kind, kern != "f64")
    got = _wsyrk(kern, Phi, d, dev)
    bound = R.wgram_bound_f32(M, n) if kern == "f32" else R.wgram_bound_f64(M, n)
    cert = R.entries_within("gram", got, S, bound)
    _report(f"wsyrk_{kern} n={n} r={r} d={kind}", cert)
    assert cert.ok, cert
    assert (got == got.T).all()                                     # exact symmetry
    assert (got == _wsyrk(kern, Phi, d, dev)).all()                 # run-to-run bit equality
    if kind == "last":
        assert np.abs(got).max() > 0


def _g64_n(dev, r):
    """4·16·G for the G wsyrk_groups picks once its row cap no longer binds: the first n with G groups."""
    nt = (r + 127) // 128
    T = nt * (nt + 1) // 2
    return 64 * ((2 * _ncu(dev) + T - 1) // T)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
@pytest.mark.parametrize("r", [1, 3, 127, 128, 129, 260])
def test_wsyrk_f64(dev, n, r):
    _check_gram("f64", n, r, "decades", dev)


@pytest.mark.parametrize("r", [3, 129])
@pytest.mark.parametrize("side", [-1, 1])
def test_wsyrk_f64_at_the_group_cap(dev, r, side):
    """n = 4·16·G ± 1 (above 4,200 rows: G is ≈ 2 workgroups per CU over the tiles, so this boundary,
    where the ≥ 4-slabs-per-group cap stops binding, sits at 64·G rows)."""
    _check_gram("f64", _g64_n(dev, r) + side, r, "decades", dev)


@pytest.mark.parametrize("kern", ["f64x", "f32"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 4099])
@pytest.mark.parametrize("r", [4, 60, 64, 68, 128, 132, 260])
def test_wsyrk_from_f32(dev, kern, n, r):
    _check_gram(kern, n, r, "decades", dev)


@pytest.mark.parametrize("kern", ["f64", "f64x", "f32"])
@pytest.mark.parametrize("kind", ["zeros", "last"])
@pytest.mark.parametrize("n,r", [(17, 128), (33, 68), (257, 132), (4099, 260)])
def test_wsyrk_zero_and_last_row_weights(dev, kern, kind, n, r):
    _check_gram(kern, n, r, kind, dev)


@pytest.mark.parametrize("kern", ["f64x", "f32"])
def test_wsyrk_largest_tile_count(dev, kern):
    _check_gram(kern, 64, 2048, "decades", dev)


@pytest.mark.parametrize("kern,tile", [("f64", 128), ("f32", 128), ("f64x", 64)])
def test_wsyrk_tile_index(dev, kern, tile):
    """Φ with one non-zero column pair (i, j) in each position of a 3 × 3 tile grid: a tile-index
    mistake moves the entry; everything else must be exactly 0."""
    n, r = 40, 3 * tile
    g = np.random.default_rng(tile)
    d = g.uniform(0.5, 2.0, n)
    for I in range(3):
        for J in range(3):
            i, j = I * tile + 5 + I, J * tile + tile - 3 - J
            Phi = np.zeros((n, r))
            Phi[:, i] = g.standard_normal(n).astype(np.float32)
            Phi[:, j] = g.standard_normal(n).astype(np.float32)
            got = _wsyrk(kern, Phi, d, dev)
            pi, pj, dl = Phi[:, i].astype(LD), Phi[:, j].astype(LD), d.astype(LD)
            want = np.zeros((r, r), dtype=LD)
            mag = np.zeros((r, r), dtype=LD)
            for a, b, va, vb in ((i, i, pi, pi), (i, j, pi, pj), (j, i, pj, pi), (j, j, pj, pj)):
                want[a, b] = (dl * va * vb).sum()
                mag[a, b] = (dl * np.abs(va) * np.abs(vb)).sum()
            bound = R.wgram_bound_f32(mag, n) if kern == "f32" else R.wgram_bound_f64(mag, n)
            cert = R.entries_within("gram", got, want, bound)     # bound 0 off the four entries: exact zeros
            assert cert.ok, (I, J, cert)
            assert np.count_nonzero(got) == 4, (I, J)


def test_wsyrk_f64x_requires_r_multiple_of_4(dev):
    Phi = torch.zeros(8, 6, dtype=torch.float32, device=dev)
    d = torch.ones(8, dtype=F64, device=dev)
    plen = _len("wsyrk_part_len", 8, 8)
    part = torch.empty(plen, dtype=F64, device=dev)
    S = torch.empty(8, 8, dtype=F64, device=dev)
    with pytest.raises(ValueError):
        ops.ext().wsyrk_f64x(Phi.data_ptr(), d.data_ptr(), 8, 6, part.data_ptr(), plen, S.data_ptr(),
                             ops.stream_ptr(dev))


# ------------------------------------------------------------------------------------ skinny passes
NS = [1, 3, 63, 64, 65, 1025]


def _gemv(Phi, W, f32, dev):
    n, r = Phi.shape
    k = W.shape[1]
    P = _t(Phi.astype(np.float32) if f32 else Phi, dev)
    Wt = _t(W, dev)
    Y = torch.full((n, k), float("nan"), dtype=F64, device=dev)
    fn = ops.ext().phi_gemv_f32 if f32 else ops.ext().phi_gemv
    fn(P.data_ptr(), Wt.data_ptr(), n, r, k, Y.data_ptr(), ops.stream_ptr(dev))
    return Y.cpu().numpy()


def _phit(Phi, V, dev):
    n, r = Phi.shape
    k = V.shape[1]
    P, Vt = _t(Phi.astype(np.float32), dev), _t(V, dev)
    plen = _len("phit_part_len", n, r, k)
    part = torch.empty(plen, dtype=F64, device=dev)
    out = torch.full((r, k), float("nan"), dtype=F64, device=dev)
    ops.ext().phit_f32(P.data_ptr(), Vt.data_ptr(), n, r, k, part.data_ptr(), plen, out.data_ptr(),
                       ops.stream_ptr(dev))
    return out.cpu().numpy()


@pytest.mark.parametrize("r,f32", [(1, False)] + [(r, f) for r in (4, 252, 256, 260, 508, 512) for f in (False, True)])
def test_phi_gemv(dev, r, f32):
    worst = 0.0
    for n in NS:
        g = np.random.default_rng(n * 521 + r)
        Phi = g.standard_normal((n, r))
        if f32:
            Phi = Phi.astype(np.float32).astype(np.float64)
        for k in (1, 2, 3, 4):
            W = g.standard_normal((r, k)) * 10.0 ** g.integers(-3, 4, (r, 1))
            Y, Ym = R.phi_mv_oracle(Phi, W)
            cert = R.entries_within("y", _gemv(Phi, W, f32, dev), Y, R.lr_gamma(r + 1) * Ym)
            assert cert.ok, (n, k, cert)
            worst = max(worst, cert.worst["y"])
    print(f"[lowrank-oracle] phi_gemv{'_f32' if f32 else ''} r={r} y={worst:.3g}")


@pytest.mark.parametrize("r", [4, 252, 256, 260, 508, 512])
def test_phit_f32(dev, r):
    worst = 0.0
    for n in NS:
        g = np.random.default_rng(n * 523 + r)
        Phi = g.standard_normal((n, r)).astype(np.float32).astype(np.float64)
        for k in (1, 2, 3, 4):
            V = g.standard_normal((n, k)) * 10.0 ** g.integers(-3, 4, (n, 1))
            O, Om = R.phit_oracle(Phi, V)
            got = _phit(Phi, V, dev)
            cert = R.entries_within("o", got, O, R.lr_gamma(n + 1) * Om)
            assert cert.ok, (n, k, cert)
            assert (got == _phit(Phi, V, dev)).all(), (n, k)        # deterministic
            worst = max(worst, cert.worst["o"])
    print(f"[lowrank-oracle] phit_f32 r={r} o={worst:.3g}")


def test_phit_f32_past_the_group_switch(dev):
    """n = 65,536 + 1 at r = 4, k = 1 (under 2 MB): past the row count at which phit_groups changes
    its rule."""
    n, r = 65537, 4
    g = np.random.default_rng(9)
    Phi = g.standard_normal((n, r)).astype(np.float32).astype(np.float64)
    V = g.standard_normal((n, 1))
    O, Om = R.phit_oracle(Phi, V)
    got = _phit(Phi, V, dev)
    cert = R.entries_within("o", got, O, R.lr_gamma(n + 1) * Om)
    _report("phit_f32 n=65537 r=4", cert)
    assert cert.ok, cert
    assert (got == _phit(Phi, V, dev)).all()


# ------------------------------------------------------------------------------------ RBF
def _rbf(A, B, gamma, dev):
    l, F = A.shape
    m = B.shape[0]
    At, Bt = _t(A, dev), _t(B, dev)
    out = torch.full((l, m), float("nan"), dtype=F64, device=dev)
    ops.ext().rbf_f64(At.data_ptr(), l, Bt.data_ptr(), m, F, float(gamma), out.data_ptr(), ops.stream_ptr(dev))
    return out.cpu().numpy()


def _exp_ulps(got, K):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(K > LD(2.0) ** -1000, np.abs(got.astype(LD) - K) / np.spacing(np.asarray(K, dtype=np.float64)), 0)))


@pytest.mark.parametrize("l,m,F", [(0, 1, 1), (1, 1, 1), (63, 65, 32), (64, 64, 31), (65, 63, 17), (130, 513, 1)])
def test_rbf_f64(dev, l, m, F):
    g = np.random.default_rng(l + 3 * m + 7 * F)
    A, B = g.standard_normal((l, F)), g.standard_normal((m, F))
    gamma = 1.0 / F
    got = _rbf(A, B, gamma, dev)
    assert got.shape == (l, m)
    if l == 0:
        return
    K, dK = R.rbf_oracle_f64(A, B, gamma)
    cert = R.entries_within("k", got, K, dK)
    print(f"[lowrank-oracle] rbf_f64 l={l} m={m} F={F} k={cert.worst['k']:.3g} ulp={_exp_ulps(got, K):.3g}")
    assert cert.ok, cert


def test_rbf_f64_edges(dev):
    g = np.random.default_rng(3)
    A = g.standard_normal((70, 9))
    got = _rbf(A, A, 0.4, dev)
    assert (np.diagonal(got) == 1.0).all()                          # identical rows: exactly 1
    far = np.zeros((2, 3))
    far[1] = [30.0, -25.0, 20.0]                                     # γd² = 1925·0.39 > 745: 0 or a subnormal
    got = _rbf(far[:1], far[1:], 0.39, dev)
    assert 0.0 <= got[0, 0] < 2.0 ** -1022
    K, dK = R.rbf_oracle_f64(far[:1], far[1:], 0.39)
    assert R.entries_within("k", got, K, dK).ok
    A = 1e6 * g.choice([-1.0, 1.0], (66, 12)) + 1e-3 * g.standard_normal((66, 12))
    B = A[:40] + 1e-3 * g.standard_normal((40, 12))
    B[7] = A[7]
    got = _rbf(A, B, 2e4, dev)
    K, dK = R.rbf_oracle_f64(A, B, 2e4)
    cert = R.entries_within("k", got, K, dK)
    _report("rbf_f64 1e6-magnitude features", cert)
    assert cert.ok, cert
    assert got[7, 7] == 1.0 and (np.diagonal(got[:40]) > 0.3).all()  # the GEMM form gives 0 or 1 here


def test_rbf_f64_requires_at_most_32_features(dev):
    A = torch.zeros(4, 33, dtype=F64, device=dev)
    out = torch.empty(4, 4, dtype=F64, device=dev)
    with pytest.raises(ValueError):
        ops.ext().rbf_f64(A.data_ptr(), 4, A.data_ptr(), 4, 33, 0.1, out.data_ptr(), ops.stream_ptr(dev))


# ------------------------------------------------------------------------------------ Cholesky
def _spd(r, cond_decades, seed):
    """The badly scaled family of tests/test_linalg_gpu.py, in numpy."""
    g = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(g.standard_normal((r, r)))
    ev = np.logspace(0, cond_decades, r)
    S = (Q * ev) @ Q.T
    S = (S + S.T) / 2
    dsc = np.logspace(-4, 4, r)[g.permutation(r)]
    return dsc[:, None] * S * dsc[None, :]


def _woodbury(r, seed):
    """I + Φᵀ D⁻¹ Φ from a small Φ with D⁻¹ spanning 14 decades, as the solve produces late on."""
    g = np.random.default_rng(seed)
    n = max(8, 2 * r)
    Phi = g.standard_normal((n, r)).astype(np.float32).astype(np.float64)
    Dinv = 10.0 ** g.uniform(-7, 7, n)
    S = np.eye(r) + (Phi * Dinv[:, None]).T @ Phi
    return (S + S.T) / 2


def _chol(S, dev, mw=False):
    r = S.shape[0]
    E = ops.ext()
    St = _t(S, dev)
    L = torch.full((r, r), float("nan"), dtype=F64, device=dev)
    sc = torch.full((r,), float("nan"), dtype=F64, device=dev)
    info = torch.full((1,), 99, dtype=torch.int32, device=dev)
    if mw:
        work = torch.zeros(4, dtype=torch.int32, device=dev)
        PT = torch.empty(32 * r, dtype=F64, device=dev)
        E.chol_spd_mw(St.data_ptr(), r, L.data_ptr(), sc.data_ptr(), info.data_ptr(), work.data_ptr(), PT.data_ptr(),
                      ops.stream_ptr(dev))
    else:
        E.chol_spd(St.data_ptr(), r, L.data_ptr(), sc.data_ptr(), info.data_ptr(), ops.stream_ptr(dev))
    return L, sc, int(info.cpu()[0])


CHOL_R = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 511, 512, 513, 1024]


@pytest.mark.parametrize("family", ["spd", "woodbury"])
@pytest.mark.parametrize("r", CHOL_R)
def test_chol_spd_and_solve_certified(dev, r, family):
    S = _spd(r, 8, r) if family == "spd" else _woodbury(r, r)
    L, sc, info = _chol(S, dev)
    Ln, scn = L.cpu().numpy(), sc.cpu().numpy()
    assert info == 0
    cert = R.chol_certificate(S, Ln, scn, info)
    _report(f"chol_spd {family} r={r}", cert)
    assert cert.ok, cert
    if r <= 512:                                                    # the multi-workgroup factor: the same bits
        L2, sc2, info2 = _chol(S, dev, mw=True)
        assert info2 == 0 and torch.equal(L, L2) and torch.equal(sc, sc2)
    g = np.random.default_rng(r)
    for k in (1, 2, 3, 4):
        B = g.standard_normal((r, k)) * 10.0 ** g.integers(-3, 4, (1, k))
        X = _t(B, dev)
        ops.ext().chol_solve(L.data_ptr(), sc.data_ptr(), r, k, X.data_ptr(), ops.stream_ptr(dev))
        cs = R.chol_solve_certificate(Ln, scn, B, X.cpu().numpy())
        _report(f"chol_solve {family} r={r} k={k}", cs)
        assert cs.ok, (k, cs)


def test_chol_solve_requires_at_most_4_right_hand_sides(dev):
    L = torch.eye(8, dtype=F64, device=dev)
    sc = torch.ones(8, dtype=F64, device=dev)
    B = torch.ones(8, 5, dtype=F64, device=dev)
    with pytest.raises(ValueError):
        ops.ext().chol_solve(L.data_ptr(), sc.data_ptr(), 8, 5, B.data_ptr(), ops.stream_ptr(dev))


def _unit_diag_with_lmin(r, lmin, seed):
    """A symmetric matrix with an exactly unit diagonal (so the kernel's equilibration is the
    identity) whose smallest eigenvalue is ``lmin`` up to eigvalsh's rounding: a correlation matrix
    C shifted, S = (C − s·I)/(1 − s), s chosen from C's smallest eigenvalue."""
    g = np.random.default_rng(seed)
    A = g.standard_normal((r, 3 * r))
    C = A @ A.T
    dd = 1.0 / np.sqrt(np.diagonal(C))
    C = C * dd[:, None] * dd[None, :]
    C = (C + C.T) / 2
    np.fill_diagonal(C, 1.0)
    l0 = float(np.linalg.eigvalsh(C)[0])
    s = (l0 - lmin) / (1.0 - lmin)                                  # (l0 − s)/(1 − s) = lmin
    S = (C - s * np.eye(r)) / (1.0 - s)
    np.fill_diagonal(S, 1.0)
    return S


@pytest.mark.parametrize("mw", [False, True])
def test_chol_jitter_ladder_rung(dev, mw):
    """λ_min = −3e-9 after equilibration, mid-way between the 1e-10 and 1e-8 rungs: exactly the rung
    whose jitter first exceeds 3e-9, and the factor certified against Ss + jit·I."""
    r = 96
    S = _unit_diag_with_lmin(r, -3e-9, 5)
    lmin = float(np.linalg.eigvalsh(S)[0])                          # on the CPU; sc = 1 exactly
    assert -4e-9 < lmin < -2e-9
    rung = next(i for i in range(0, 9) if R.chol_jitter(i) > -lmin)
    assert rung == 4 and R.chol_jitter(rung - 1) < 0.1 * -lmin      # 1e-10 ≪ 3e-9 ≪ 1e-8: rounding cannot decide
    L, sc, info = _chol(S, dev, mw=mw)
    assert info == rung
    assert (sc.cpu().numpy() == 1.0).all()
    cert = R.chol_certificate(S, L.cpu().numpy(), sc.cpu().numpy(), info)
    _report(f"chol jitter rung mw={mw}", cert)
    assert cert.ok, cert


def test_chol_strongly_indefinite_reports_failure(dev):
    """λ_min = −10: no rung up to 1 repairs it; the kernel must come back with info = −1."""
    r = 64
    S = _unit_diag_with_lmin(r, -10.0, 6)
    assert np.linalg.eigvalsh(S)[0] < -1.0 - 1e-6
    for mw in (False, True):
        _, _, info = _chol(S, dev, mw=mw)
        assert info == -1


# ------------------------------------------------------------------------------------ row kernels
ROW_N = [1, 255, 256, 257, 1000]


def _rows(n, seed, k=None):
    """Positive α, s, ν, μ spanning decades, signed directions, ±1 labels."""
    g = np.random.default_rng(seed * 7919 + n % 1009)
    pos = lambda: g.uniform(0.1, 1.0, n) * 10.0 ** g.integers(-9, 3, n)   # noqa: E731
    sgn = lambda: g.standard_normal(n) * 10.0 ** g.integers(-6, 3, n)     # noqa: E731
    return g, pos, sgn


def _dv(x, dev):
    return _t(np.asarray(x, dtype=np.float64), dev)


class _Pin:
    """Device copies that stay alive until the test ends (a temporary freed right after ``data_ptr()``
    hands its block to the next allocation): ``pin(x)`` is the pointer of a kept f64 copy of ``x``."""

    def __init__(self, dev):
        self.dev, self.kept = dev, []

    def __call__(self, x, dtype=np.float64):
        t = _t(np.asarray(x, dtype=dtype), self.dev)
        self.kept.append(t)
        return t.data_ptr()


def _out(n, dev, *shape):
    return torch.full((n, *shape), float("nan"), dtype=F64, device=dev)


def _same(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape
    assert (got.view(np.int64) == np.ascontiguousarray(want).view(np.int64)).all()


def _cap(dev, which):
    return {"grid": 256 * 4096, "blocks": 256 * 8 * _ncu(dev), "fill": 256 * 2048, "step": 256 * 4 * _ncu(dev)}[which]


def _strided(col, stride, dev):
    """``col`` as column 1 of an [n, stride] device matrix (NaN elsewhere): (tensor kept alive, pointer)."""
    M = np.full((col.shape[0], stride), np.nan)
    c = 1 if stride > 1 else 0
    M[:, c] = col
    Mt = _t(M, dev)
    return Mt, Mt[:, c].data_ptr()


@pytest.mark.parametrize("n", ROW_N + ["cap"])
def test_ipm_resid_pred_corr_update(dev, n):
    E, sp, pin = ops.ext(), ops.stream_ptr(dev), _Pin(dev)
    n = _cap(dev, "grid") + 1 if n == "cap" else n                  # a second trip of the grid-stride loop
    g, pos, sgn = _rows(n, 1)
    o = R.ipm_rows_oracle
    a, s, nu, mu, c = pos(), pos(), pos(), pos(), pos()
    y = g.choice([-1.0, 1.0], n)
    P, rd, da, dnu, dmu = sgn(), sgn(), sgn(), sgn(), sgn()
    b, tau, t = -0.37251, 3.1e-5, 0.61803
    for stride in (1, 2, 4):
        keep, pp = _strided(P, stride, dev)
        so, ro = _out(n, dev), _out(n, dev)
        E.ipm_resid(pin(c), pin(a), pin(y), pp, stride,
                    pin([b]), pin(nu), pin(mu), n, so.data_ptr(),
                    ro.data_ptr(), sp)
        ws, wr = o.resid(c, a, y, P, b, nu, mu)
        _same(so, ws), _same(ro, wr)
    ta, ts, tn, tm, trd, ty = (_dv(v, dev) for v in (a, s, nu, mu, rd, y))
    Dinv, rnu, rmu, Dinv2, H2 = _out(n, dev), _out(n, dev), _out(n, dev), _out(n, dev, 2), _out(n, dev, 2)
    E.ipm_pred(ta.data_ptr(), ts.data_ptr(), tn.data_ptr(), tm.data_ptr(), trd.data_ptr(), ty.data_ptr(), n,
               Dinv.data_ptr(), Dinv2.data_ptr(), rnu.data_ptr(), rmu.data_ptr(), H2.data_ptr(), sp)
    for got, want in zip((Dinv, Dinv2, rnu, rmu, H2), o.pred(a, s, nu, mu, rd, y)):
        _same(got, want)
    tda, tdn, tdm = (_dv(v, dev) for v in (da, dnu, dmu))
    h = _out(n, dev)
    rnu, rmu = _out(n, dev), _out(n, dev)
    E.ipm_corr(ta.data_ptr(), ts.data_ptr(), tn.data_ptr(), tm.data_ptr(), tda.data_ptr(), tdn.data_ptr(),
               tdm.data_ptr(), trd.data_ptr(), pin([tau]), n, rnu.data_ptr(), rmu.data_ptr(),
               h.data_ptr(), sp)
    for got, want in zip((rnu, rmu, h), o.corr(a, s, nu, mu, da, dnu, dmu, rd, tau)):
        _same(got, want)
    a2, n2, m2 = _out(n, dev), _out(n, dev), _out(n, dev)
    E.ipm_update(ta.data_ptr(), tn.data_ptr(), tm.data_ptr(), tda.data_ptr(), tdn.data_ptr(), tdm.data_ptr(),
                 pin([t]), n, a2.data_ptr(), n2.data_ptr(), m2.data_ptr(), sp)
    for got, want in zip((a2, n2, m2), o.update(a, nu, mu, da, dnu, dmu, t)):
        _same(got, want)


@pytest.mark.parametrize("n", ROW_N + ["cap"])
def test_ipm_dirs_gondzio_select(dev, n):
    E, sp, pin = ops.ext(), ops.stream_ptr(dev), _Pin(dev)
    n = _cap(dev, "blocks") + 1 if n == "cap" else n
    g, pos, sgn = _rows(n, 2)
    o = R.ipm_rows_oracle
    a, s, nu, mu = pos(), pos(), pos(), pos()
    Mh, My, rnu, rmu, da, dnu, dmu = (sgn() for _ in range(7))
    db, alpha, tau = 0.123456789, 0.4375, 2.5e-4
    ta, ts, tn, tm = (_dv(v, dev) for v in (a, s, nu, mu))
    trn, trm, tda, tdn, tdm = (_dv(v, dev) for v in (rnu, rmu, da, dnu, dmu))
    for stride in (1, 2, 4):
        k1, ph = _strided(Mh, stride, dev)
        k2, py = _strided(My, stride, dev)
        outs = [_out(n, dev) for _ in range(3)]
        E.ipm_dirs(ph, stride, py, stride, pin([db]), trn.data_ptr(), trm.data_ptr(), tn.data_ptr(),
                   tm.data_ptr(), ta.data_ptr(), ts.data_ptr(), n, *[t.data_ptr() for t in outs], sp)
        for got, want in zip(outs, o.dirs(Mh, My, db, rnu, rmu, nu, mu, a, s)):
            _same(got, want)
    for al in (alpha, 0.9):                                         # 1.5·0.9 + 0.1 > 1: the min(·, 1) arm
        outs = [_out(n, dev) for _ in range(3)]
        E.ipm_gondzio_rhs(ta.data_ptr(), ts.data_ptr(), tn.data_ptr(), tm.data_ptr(), tda.data_ptr(), tdn.data_ptr(),
                          tdm.data_ptr(), pin([al]), pin([tau]), n,
                          *[t.data_ptr() for t in outs], sp)
        want = o.gondzio_rhs(a, s, nu, mu, da, dnu, dmu, al, tau)
        for got, w in zip(outs, want):
            _same(got, w)
    tca, tcs = want[0], want[1]
    for stride in (1, 2, 4):
        k1, ph = _strided(Mh, stride, dev)
        k2, py = _strided(My, stride, dev)
        outs = [_out(n, dev) for _ in range(3)]
        E.ipm_gondzio_apply(ph, stride, py, stride, pin([db]), tda.data_ptr(), tdn.data_ptr(),
                            tdm.data_ptr(), pin(tca), pin(tcs), tn.data_ptr(),
                            tm.data_ptr(), ta.data_ptr(), ts.data_ptr(), n, *[t.data_ptr() for t in outs], sp)
        for got, w in zip(outs, o.gondzio_apply(Mh, My, db, da, dnu, dmu, tca, tcs, nu, mu, a, s)):
            _same(got, w)
    for flag in (False, True):
        ok = torch.tensor(flag, dtype=torch.bool, device=dev)
        outs = [_out(n, dev) for _ in range(3)]                     # NaN-prefilled
        E.ipm_select3(ok.data_ptr(), tda.data_ptr(), tdn.data_ptr(), tdm.data_ptr(), n, *[t.data_ptr() for t in outs], sp)
        nan = np.full(n, np.nan)
        for got, w in zip(outs, o.select3(flag, (da, dnu, dmu), (nan, nan, nan))):
            _same(got, w)                                           # flag 0: the NaN bits untouched


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("n", ROW_N + ["cap"])
def test_ipm_minv_pre_post(dev, n, k):
    E, sp, pin = ops.ext(), ops.stream_ptr(dev), _Pin(dev)
    n = _cap(dev, "grid") // k + 1 if n == "cap" else n             # n·k just past the grid cap
    g, pos, sgn = _rows(n, 3 + k)
    o = R.ipm_rows_oracle
    Dinv, y = pos(), g.choice([-1.0, 1.0], n)
    U = g.standard_normal((n, k)) * 10.0 ** g.integers(-4, 4, (n, k))
    P = g.standard_normal((n, k))
    td, ty = _dv(Dinv, dev), _dv(y, dev)
    du, V = _out(n, dev, k), _out(n, dev, k)
    E.ipm_minv_pre(td.data_ptr(), ty.data_ptr(), pin(U), k, n, du.data_ptr(), V.data_ptr(), sp)
    wdu, wV = o.minv_pre(Dinv, y, U)
    _same(du, wdu), _same(V, wV)
    out = _out(n, dev, k)
    E.ipm_minv_post(td.data_ptr(), ty.data_ptr(), du.data_ptr(), pin(P), k, n, out.data_ptr(), sp)
    _same(out, o.minv_post(Dinv, y, wdu, P))


@pytest.mark.parametrize("n", ROW_N + ["cap"])
def test_fill_dev_and_scale_rows(dev, n):
    E, sp, pin = ops.ext(), ops.stream_ptr(dev), _Pin(dev)
    o = R.ipm_rows_oracle
    nf = _cap(dev, "fill") + 1 if n == "cap" else n
    for v in (0.1, -0.0, 5e-324):
        out = _out(nf, dev)
        E.fill_dev(out.data_ptr(), nf, pin([v]), sp)
        _same(out, o.fill(nf, v))
    r = 4 if n == "cap" else 12
    ns = 16 * _ncu(dev) * 256 + 1 if n == "cap" else n              # n·r/4 just past scale_rows_f32's grid
    g = np.random.default_rng(ns)
    P32 = g.standard_normal((ns, r)).astype(np.float32)
    d = g.uniform(0.1, 1.0, ns) * 10.0 ** g.integers(-6, 6, ns)
    out = _out(ns, dev, r)
    E.scale_rows_f32(pin(P32, np.float32), pin(d), ns, r, out.data_ptr(), sp)
    _same(out, o.scale_rows(P32, d))


def _max_step(pairs, signs, dev):
    n = pairs[0][0].shape[0]
    ts = [(_dv(v, dev), _dv(dv, dev)) for v, dv in pairs]
    out = torch.ones((), dtype=F64, device=dev)
    args = [p for pr in ts for p in (pr[0].data_ptr(), pr[1].data_ptr())]
    ops.ext().ipm_max_step(*args, *[float(s) for s in signs], n, out.data_ptr(), ops.stream_ptr(dev))
    return out.cpu().numpy().reshape(1)


@pytest.mark.parametrize("signs", [(1, -1, 1, 1), (-1, 1, -1, -1)])
@pytest.mark.parametrize("n", ROW_N + ["cap"])
def test_ipm_max_step(dev, n, signs):
    n = _cap(dev, "step") + 1 if n == "cap" else n
    g, pos, sgn = _rows(n, 11)
    o = R.ipm_rows_oracle
    one = lambda x: np.array([x])   # noqa: E731
    pairs = [(pos(), sgn()) for _ in range(4)]
    _same(torch.from_numpy(_max_step(pairs, signs, dev)), one(o.max_step(pairs, signs)))
    # no negative direction: exactly 1.0
    up = [(v, np.abs(dv) * s) for (v, dv), s in zip(pairs, signs)]
    assert o.max_step(up, signs) == 1.0
    _same(torch.from_numpy(_max_step(up, signs, dev)), one(1.0))
    # all ratios above 1: exactly 1.0
    slow = [(v, -s * v / (1.5 + g.random(n))) for (v, _), s in zip(pairs, signs)]
    assert o.max_step(slow, signs) == 1.0
    _same(torch.from_numpy(_max_step(slow, signs, dev)), one(1.0))
    # the minimum in the last element, in each of the four pairs
    for q in range(4):
        last = [(v.copy(), dv.copy()) for v, dv in slow]
        last[q][1][-1] = -signs[q] * last[q][0][-1] * 64.0        # ratio 1/64 there
        want = o.max_step(last, signs)
        assert want == 1.0 / 64.0
        _same(torch.from_numpy(_max_step(last, signs, dev)), one(want))
    # one v = 0 with a negative direction: exactly +0.0 (the unsigned ordering of the atomic min)
    zero = [(v.copy(), dv.copy()) for v, dv in pairs]
    zero[2][0][n // 2] = 0.0
    zero[2][1][n // 2] = -signs[2] * 3.0
    want = o.max_step(zero, signs)
    assert want == 0.0 and not np.signbit(want)
    _same(torch.from_numpy(_max_step(zero, signs, dev)), one(0.0))


# ------------------------------------------------------------------------------------ the solve, end to end
def _svc_problem(l, r, kind, seed):
    g = np.random.default_rng(seed)
    y = np.where(g.random(l) < 0.35, -1.0, 1.0)
    if kind == "single" or l == 2:
        y[:] = 1.0
        y[l // 2] = -1.0                                            # one class with a single member
    Phi = g.standard_normal((l, r)) / np.sqrt(r)
    if kind == "sep":
        Phi[:, 0] = y * (1.5 + g.random(l))                         # separable along the first feature
    else:
        Phi[:, 0] += 0.4 * y
    Phi = Phi.astype(np.float32).astype(np.float64)                 # a Φ rounded to f32
    if kind == "w20":
        c = np.where(y > 0, 0.25, 5.0)                              # 20 : 1 class weights
    elif kind == "sep":
        c = np.full(l, 50.0)
    else:
        npos = max(1, int((y > 0).sum()))
        c = np.where(y > 0, l / (2.0 * npos), l / (2.0 * max(1, l - npos)))   # balanced
    return Phi, y, c


@pytest.mark.parametrize("gram", ["f64x", "f64"])
@pytest.mark.parametrize("mw", [True, False])
@pytest.mark.parametrize("l,r,kind", [(2, 4, "sep"), (2, 16, "bal"), (64, 4, "bal"), (64, 16, "w20"), (64, 64, "single"),
                                      (64, 64, "sep"), (1500, 4, "single"), (1500, 16, "sep"), (1500, 64, "w20"),
                                      (1500, 64, "bal")])
def test_ipm_svc_dual_certified(dev, monkeypatch, l, r, kind, gram, mw):
    from hfens.models import svc_lowrank as sl
    monkeypatch.setattr(sl, "GRAM", gram)
    monkeypatch.setattr(sl, "CHOL_MW", mw)
    Phi, y, c = _svc_problem(l, r, kind, 100 * l + r)
    loose0 = sl.LAST_INFO.get("loose_rd_stops", 0)
    a, rho, it = sl.ipm_svc_dual(_t(Phi, dev), _t(y, dev), _t(c, dev))
    loose = sl.LAST_INFO.get("loose_rd_stops", 0) - loose0
    rd_tol = R.LR_RD_LOOSE if loose else R.LR_IPM_TOL               # the rule the solver says it stopped on
    cert = R.svc_dual_certificate(Phi, y, c, a.cpu().numpy(), rho, rd_tol=rd_tol)
    print(f"[lowrank-oracle] ipm l={l} r={r} {kind} {gram} mw={mw} it={it} loose={loose} "
          f"gap={float(cert.extra['gap']):.3g}/{float(cert.extra['gap_bound']):.3g} eq={cert.worst.get('eq', 0):.3g} "
          f"relgap={float(cert.extra['rel_gap']):.3g}")
    assert it <= sl.IPM_MAX_ITER
    assert cert.ok, cert                                            # the stopping test met, not the cap hit
    if kind == "sep":
        # separable with margin ≥ 1.5 along the first feature: Σα = ‖w*‖² ≤ 1/1.5² < c, so no point is
        # at its upper bound
        assert (a.cpu().numpy() < c).all()
