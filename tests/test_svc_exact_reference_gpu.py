"""The exact-SMO SVC kernels (ops/csrc/svm.hip, svm_coop.hip, stackdev.hip svm_gamma) one by one
against the oracles of ops/reference.py, through the extension's entry points with hand-built
problem tables.  The oracles themselves are proved in tests/test_svc_exact_reference.py, whose
problem builders are used here."""
import numpy as np
import pytest
import torch

from hfens.models import smo
from hfens.ops import reference as R

import test_svc_exact_reference as C

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U64 = 2.0 ** -53
L = np.longdouble


def _E():
    from hfens import ops
    return ops.ext()


def _s(dev):
    from hfens import ops
    return ops.stream_ptr(dev)


_LIVE = []


@pytest.fixture(autouse=True)
def _release_inputs():
    """Device inputs are handed to the extension as raw pointers: _d() keeps every tensor it makes
    alive until the test ends (a dropped temporary's block would be reused by the next upload)."""
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def _d(a, dev):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    _LIVE.append(t)
    return t


def _tab(arr, dev):
    return _d(arr.view(np.uint8), dev)


def _ld(l):
    return (l + 63) // 64 * 64


# ------------------------------------------------------------------------------------ gram_rbf_batch
def _gram_launch(dev, Zs, e2s, gap=0):
    """One gram_rbf_batch launch over the problems ``Zs`` (rows concatenated after a 3-row lead, so
    every zoff is non-zero; Gram blocks ``gap`` floats apart after a 64-float lead) into a NaN-filled
    buffer.  Returns the fetched buffer and the table."""
    F = Zs[0].shape[1]
    g = np.zeros(len(Zs), smo._GRAM_DT)
    zoff, koff = 3, 64
    for k, Z in enumerate(Zs):
        l = Z.shape[0]
        g[k] = (zoff, koff, l, _ld(l), e2s[k], 0)
        zoff += l
        koff += l * _ld(l) + gap
    zcat = np.concatenate([np.full((3, F), 7.0, np.float32)] + list(Zs))
    K = torch.full((koff + 64,), float("nan"), dtype=torch.float32, device=dev)
    _E().gram_rbf_batch(_d(zcat, dev).data_ptr(), F, _tab(g, dev).data_ptr(), len(Zs), max(Z.shape[0] for Z in Zs),
                        K.data_ptr(), _s(dev))
    return K.cpu().numpy(), g


@pytest.mark.parametrize("F", C.GRAM_FS)
def test_gram_rbf_batch(dev, F):
    """Every l of GRAM_LS as one batch (different l, non-zero zoff and koff: the small problems' tiles
    return early), per feature width on both sides of every GRAM_CASE bucket."""
    Zs = [C.gram_rows(l, F, 100 * F + l) for l in C.GRAM_LS]
    buf, g = _gram_launch(dev, Zs, [C.ngl2e_of(F)] * len(Zs), gap=36)
    written = np.zeros(buf.size, bool)
    for k, Z in enumerate(Zs):
        l, ld, koff = Z.shape[0], int(g[k]["ld"]), int(g[k]["koff"])
        blk = buf[koff:koff + l * ld].reshape(l, ld)
        Kh = blk[:, :l]
        K, dK = R.gram_kernel_error(Z, C.ngl2e_of(F))
        inside = R.gram_inside(Kh, K, dK)
        assert inside.all(), (l, F, np.argwhere(~inside)[:4])
        assert (np.diagonal(Kh) == np.float32(1)).all()
        assert np.array_equal(Kh.view(np.uint32), Kh.T.copy().view(np.uint32))
        if l >= 3:
            assert Kh[0, 1] == 1 and Kh[0, 2] == 0
        w = np.zeros((l, ld), bool)
        w[:, :l] = True
        written[koff:koff + l * ld] = w.ravel()
    assert np.isnan(buf[~written]).all() and not np.isnan(buf[written]).any()


# ------------------------------------------------------------------------------------ SMO problems
SMO_CASES = [("gauss", 2), ("gauss", 3), ("gauss", 255), ("gauss", 257), ("gauss", 1023), ("gauss", 1025),
             ("npos1", 257), ("nposl1", 257), ("dup_opposite", 257), ("dup_equal", 257), ("all_bound", 258),
             ("clusters", 257), ("clusters", 4096), ("clusters", 4097)]
_cache = {}


def _problem(dev, kind, l):
    """The problem, its Gram computed on the device (NaN padding kept) and the oracle's replay of
    it — computed once per module and left unchanged."""
    key = (kind, l)
    if key not in _cache:
        Z, npos, Cp, Cn = C.smo_problem(kind, l)
        l = Z.shape[0]
        e2 = C.ngl2e_of(Z.shape[1])
        ld = _ld(l)
        g = np.zeros(1, smo._GRAM_DT)
        g[0] = (0, 0, l, ld, e2, 0)
        K = torch.full((l * ld,), float("nan"), dtype=torch.float32, device=dev)
        _E().gram_rbf_batch(_d(Z, dev).data_ptr(), Z.shape[1], _tab(g, dev).data_ptr(), 1, l, K.data_ptr(), _s(dev))
        Kh = K.cpu().numpy().reshape(l, ld)
        assert np.isnan(Kh[:, l:]).all()
        o = R.smo_oracle(Kh[:, :l], npos, Cp, Cn, C.EPS, C.MAX_ITER)
        _cache[key] = dict(Z=Z, npos=npos, Cp=Cp, Cn=Cn, l=l, ld=ld, e2=e2, K=K, Kh=Kh[:, :l].copy(), o=o)
    return _cache[key]


def _check_solution(p, alpha, rho, iters, gap, Kh=None, o=None, npos=None):
    """The assertions every stored-Gram solver shares:

    * iteration count and α bit-equal to the oracle's replay of the same matrix;
    * ρ within n·2⁻⁵³·Σ|yG| of the longdouble mean of y·G over the n free points (any summation
      order of n f64 terms is within (n − 1)·2⁻⁵³·Σ|x| of the exact sum, and the division rounds once
      more); with no free point, (ub + lb)/2 bit-equal;
    * the reported gap bit-equal to the oracle's last m − M;
    * 0 ≤ α ≤ C exactly;
    * |Σ yα| ≤ 8·2⁻⁵³·Cmax per update: a pair keeps y_iα_i + y_jα_j up to the roundings of diff (or
      sum), of the two additions of δ when nothing is clipped, or of the clipped C − diff — at most
      four roundings of values within [−2Cmax, 2Cmax];
    * the gap recomputed in longdouble from the stored Gram below eps + 2·max drift: each of its two
      maxima reads one gradient entry.  This one holds whether or not the replay is right."""
    o = p["o"] if o is None else o
    Kh = p["Kh"] if Kh is None else Kh
    npos = p["npos"] if npos is None else npos
    l = Kh.shape[0]
    Cp, Cn = p["Cp"], p["Cn"]
    pos = np.arange(l) < npos
    Cv = np.where(pos, Cp, Cn)
    assert iters == o.iters, (iters, o.iters)
    assert np.array_equal(alpha.view(np.uint64), o.alpha.view(np.uint64)), int((alpha != o.alpha).sum())
    assert ((alpha >= 0) & (alpha <= Cv)).all()
    assert np.float64(gap).view(np.uint64) == np.float64(o.gap).view(np.uint64), (gap, o.gap)
    free = (alpha > 0) & (alpha < Cv)
    if free.any():
        yG = np.where(pos, o.G, -o.G)[free].astype(L)
        assert abs(L(rho) - yG.sum() / free.sum()) <= free.sum() * U64 * np.abs(yG).sum(), (rho, o.rho)
    else:
        assert rho == o.rho, (rho, o.rho)
    y = np.where(pos, 1.0, -1.0).astype(L)
    assert abs((y * alpha.astype(L)).sum()) <= 8 * U64 * max(Cp, Cn) * max(1, iters)
    Gs = -1 + y * (Kh.astype(L) @ (y * alpha.astype(L)))
    kkt = R.svc_kkt(alpha.astype(L), Gs, npos, Cp, Cn)
    assert kkt["gap"] < C.EPS + 2 * o.drift.max(), (float(kkt["gap"]), o.drift.max())


def _smo_launch(dev, p, max_l=None):
    """One smo_batch launch on the problem's device Gram; ``max_l`` (default: the problem's own size)
    picks the smo_kernel<K4> instantiation.  α with its 64 guard entries, ρ, iterations, gap."""
    l = p["l"]
    sm = np.zeros(1, smo._SMO_DT)
    sm[0] = (0, 0, l, p["ld"], p["npos"], 0, p["Cp"], p["Cn"])
    alpha = torch.full((l + 64,), -7.0, dtype=torch.float64, device=dev)
    rho = torch.zeros(1, dtype=torch.float64, device=dev)
    iters = torch.zeros(1, dtype=torch.int32, device=dev)
    gap = torch.zeros(1, dtype=torch.float64, device=dev)
    _E().smo_batch(_tab(sm, dev).data_ptr(), 1, l if max_l is None else max_l, p["K"].data_ptr(), alpha.data_ptr(),
                   C.EPS, C.MAX_ITER, rho.data_ptr(), iters.data_ptr(), gap.data_ptr(), 0, _s(dev))
    return alpha.cpu().numpy(), float(rho.item()), int(iters.item()), float(gap.item())


@pytest.mark.parametrize("kind,l", SMO_CASES, ids=lambda v: str(v))
def test_smo_batch(dev, kind, l):
    p = _problem(dev, kind, l)
    l = p["l"]
    a, rho, iters, gap = _smo_launch(dev, p)
    assert (a[l:] == -7.0).all()
    _check_solution(p, a[:l].copy(), rho, iters, gap)
    if kind == "all_bound":
        assert (a[:l] == np.where(np.arange(l) < p["npos"], p["Cp"], p["Cn"])).all()     # the no-free-vector ρ


@pytest.mark.parametrize("max_l", [4096, 8192, 12288, 16384, 24576, 32768])
def test_smo_batch_every_bucket(dev, max_l):
    """smo_batch picks smo_kernel<K4> from max_l, not from the problem: K4 = 1, 2, 3, 4, 6, 8 (the last
    three spill) on one 257-point problem, where all but the first register group of every thread is
    empty."""
    p = _problem(dev, "gauss", 257)
    l = p["l"]
    a, rho, iters, gap = _smo_launch(dev, p, max_l=max_l)
    assert (a[l:] == -7.0).all()
    _check_solution(p, a[:l].copy(), rho, iters, gap)


def _coop_launch(dev, K, l, ld, npos, Cp, Cn, W, S, lphys=None, cmap=None, max_S=None):
    cp = np.zeros(1, smo._COOP_DT)
    lphys = l if lphys is None else lphys
    cp[0] = (0, 0, 0 if cmap is not None else -1, l, ld, npos, S, lphys, 0, Cp, Cn)
    alpha = torch.full((lphys + 64,), -7.0, dtype=torch.float64, device=dev)
    rho = torch.zeros(1, dtype=torch.float64, device=dev)
    iters = torch.zeros(1, dtype=torch.int32, device=dev)
    gap = torch.zeros(1, dtype=torch.float64, device=dev)
    xchg = torch.empty(smo._COOP_GRANULES, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    mdev = _d(cmap.astype(np.int32), dev) if cmap is not None else None
    assert 1 * W <= 16                       # P·W ≤ 16: co-resident by construction
    _E().smo_coop_batch(_tab(cp, dev).data_ptr(), 1, W, S if max_S is None else max_S, K.data_ptr(),
                        mdev.data_ptr() if mdev is not None else 0,
                        alpha.data_ptr(), xchg.data_ptr(), C.EPS, C.MAX_ITER, rho.data_ptr(), iters.data_ptr(),
                        gap.data_ptr(), err.data_ptr(), 0, _s(dev))
    e = int(err.item())
    assert e == 0, f"smo_coop_batch raised err = {e}: a member exchange timed out or a key overflowed (not retried)"
    return alpha.cpu().numpy()[:l].copy(), float(rho.item()), int(iters.item()), float(gap.item())


@pytest.mark.parametrize("W", [2, 3, 5])
@pytest.mark.parametrize("kind,l", [c for c in SMO_CASES if c[1] >= 255], ids=lambda v: str(v))
def test_smo_coop_batch(dev, kind, l, W):
    p = _problem(dev, kind, l)
    l = p["l"]
    S = -(-(-(-l // W)) // 4) * 4
    _check_solution(p, *_coop_launch(dev, p["K"], l, p["ld"], p["npos"], p["Cp"], p["Cn"], W, S))


def test_smo_coop_empty_member(dev):
    """l = 9, W = 4, S = 4: the members own 4, 4, 1 and 0 points."""
    p = _problem(dev, "gauss", 9)
    _check_solution(p, *_coop_launch(dev, p["K"], 9, p["ld"], p["npos"], p["Cp"], p["Cn"], 4, 4))


def _mapped_submatrix(dev, max_S=None):
    p = _problem(dev, "gauss", 48)
    keep = np.r_[0:16, 32:48]
    cmap = np.full(48, -1, np.int32)
    cmap[keep] = np.arange(keep.size)
    npos = int((keep < p["npos"]).sum())
    assert 0 < npos < keep.size
    Ksub = p["Kh"][np.ix_(keep, keep)]
    if "o_sub" not in p:
        p["o_sub"] = R.smo_oracle(Ksub, npos, p["Cp"], p["Cn"], C.EPS, C.MAX_ITER)
    got = _coop_launch(dev, p["K"], keep.size, p["ld"], npos, p["Cp"], p["Cn"], 3, 16, lphys=48, cmap=cmap,
                       max_S=max_S)
    _check_solution(p, *got, Kh=Ksub, o=p["o_sub"], npos=npos)


def test_smo_coop_mapped_submatrix(dev):
    """A sub-problem reads its parent's Gram through a column map; W = 3, S = 16 over 48 parent
    columns, and the sub-problem leaves out columns 16..31: member 1's whole slice maps to −1."""
    _mapped_submatrix(dev)


@pytest.mark.parametrize("mapped", [False, True], ids=["unmapped", "mapped"])
@pytest.mark.parametrize("max_S", [2048, 4096, 8192, 16384])
def test_smo_coop_every_bucket(dev, max_S, mapped):
    """smo_coop_batch picks smo_coop_kernel<K4, Mapped> from max_S: K4 = 1, 2, 4, 8 (the last spills),
    unmapped on 257 points over 3 members and mapped on the 48-column sub-problem above."""
    if mapped:
        _mapped_submatrix(dev, max_S=max_S)
        return
    p = _problem(dev, "gauss", 257)
    l = p["l"]
    S = -(-(-(-l // 3)) // 4) * 4
    _check_solution(p, *_coop_launch(dev, p["K"], l, p["ld"], p["npos"], p["Cp"], p["Cn"], 3, S, max_S=max_S))


def _otf_launch(dev, Z, l, npos, Cp, Cn, e2, W, S, max_S=None):
    """One smo_coop_otf_batch launch on the rows Z; ``max_S`` (default S) picks the points-per-thread
    bucket of smo_coop_otf_kernel<KM, FP>, the width of Z the feature bucket."""
    F = Z.shape[1]
    op = np.zeros(1, smo._OTF_DT)
    op[0] = (0, 0, l, npos, S, e2, Cp, Cn)
    alpha = torch.full((l + 64,), -7.0, dtype=torch.float64, device=dev)
    rho = torch.zeros(1, dtype=torch.float64, device=dev)
    iters = torch.zeros(1, dtype=torch.int32, device=dev)
    gap = torch.zeros(1, dtype=torch.float64, device=dev)
    xchg = torch.empty(smo._OTF_GRANULES, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _E().smo_coop_otf_batch(_tab(op, dev).data_ptr(), 1, W, F, S if max_S is None else max_S, _d(Z, dev).data_ptr(),
                            alpha.data_ptr(), xchg.data_ptr(), C.EPS, C.MAX_ITER, rho.data_ptr(), iters.data_ptr(),
                            gap.data_ptr(), err.data_ptr(), _s(dev))
    e = int(err.item())
    assert e == 0, f"smo_coop_otf_batch raised err = {e}: a member exchange timed out (not retried)"
    a = alpha.cpu().numpy()
    assert (a[l:] == -7.0).all()
    return a[:l].copy(), float(rho.item()), int(iters.item()), float(gap.item())


@pytest.mark.parametrize("F", [5, 17])
@pytest.mark.parametrize("max_S", [512, 1024, 2048])
def test_smo_coop_otf_follows_stored_gram(dev, max_S, F):
    """The on-the-fly kernel's contract: it re-evaluates gram_rbf_kernel's expression, so it takes the
    pairs of the stored-Gram solvers on the device Gram of the same rows — the same iteration count
    and bit-equal α as smo_batch.  255 points of F features over W = 2 members (S = 128), in every
    instantiation: max_S gives KM = 1, 2, 4 points per thread, F = 5 / 17 the feature tiles 8 / 20."""
    key = ("otf_rows", F)
    if key not in _cache:
        Z, npos, Cp, Cn = C.smo_problem("gauss", 255, F=F)
        l = Z.shape[0]
        e2 = C.ngl2e_of(F)
        ld = _ld(l)
        g = np.zeros(1, smo._GRAM_DT)
        g[0] = (0, 0, l, ld, e2, 0)
        K = torch.full((l * ld,), float("nan"), dtype=torch.float32, device=dev)
        _E().gram_rbf_batch(_d(Z, dev).data_ptr(), F, _tab(g, dev).data_ptr(), 1, l, K.data_ptr(), _s(dev))
        p = dict(Z=Z, npos=npos, Cp=Cp, Cn=Cn, l=l, ld=ld, e2=e2, K=K)
        a, rho, iters, gap = _smo_launch(dev, p)
        _cache[key] = dict(p, ref=(a[:l].copy(), iters))
    p = _cache[key]
    a, rho, iters, gap = _otf_launch(dev, p["Z"], p["l"], p["npos"], p["Cp"], p["Cn"], p["e2"], 2, 128, max_S=max_S)
    ra, riters = p["ref"]
    assert riters > 0
    assert iters == riters, (iters, riters)
    assert np.array_equal(a.view(np.uint64), ra.view(np.uint64)), int((a != ra).sum())


@pytest.mark.parametrize("kind,l,W", [("gauss", 255, 2), ("gauss", 1025, 3)])
def test_smo_coop_otf_true_kernel_certificate(dev, kind, l, W):
    """smo_coop_otf_batch recomputes its kernel values: checked against the TRUE kernel only
    (svc_dual_oracle on the f32 rows).  Its gradient stands for −1 + y_t·Σ_c y_c α_c K̂_tc with K̂ within
    dK of K, so each of the two maxima of the gap moves by at most B = max_t Σ_c α_c dK_tc + drift,
    and ρ — a mean of such gradient entries over the free points, or the mean of two of them — by
    at most B as well.  The drift of the incremental updates is bounded from this run's OWN
    iteration count: one update rounds five times (smo_oracle's docstring), with |K̂| ≤ 1,
    |Δα| ≤ Cmax and |G_t| ≤ 1 + Σ_c C_c, by at most 2⁻⁵³·(1 + 2⁻⁵⁰)·(6·Cmax + 1 + Σ_c C_c)."""
    p = _problem(dev, kind, l)
    Z = p["Z"]
    a, rho_v, it, _ = _otf_launch(dev, Z, l, p["npos"], p["Cp"], p["Cn"], p["e2"], W, -(-l // W))
    Cv = np.where(np.arange(l) < p["npos"], p["Cp"], p["Cn"])
    assert ((a >= 0) & (a <= Cv)).all()
    o = R.svc_dual_oracle(Z, p["npos"], p["Cp"], p["Cn"], p["e2"], a)
    _, dK = R.gram_kernel_error(Z, p["e2"])
    drift = it * U64 * (1 + 2.0 ** -50) * (6 * max(p["Cp"], p["Cn"]) + 1 + Cv.sum())
    budget = float((dK @ a.astype(L)).max()) + drift
    print(f"otf {kind} {l} W={W}: true gap {float(o['gap']):.4e} budget {budget:.3e} "
          f"drift {drift:.2e} iters {it} rho diff {float(abs(L(rho_v) - o['rho'])):.3e}")
    assert o["gap"] < C.EPS + 2 * budget, (float(o["gap"]), budget)
    assert abs(L(rho_v) - o["rho"]) <= budget, (rho_v, float(o["rho"]), budget)


# ------------------------------------------------------------------------------------ svm_sv_compact
@pytest.mark.parametrize("l", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_svm_sv_compact(dev, l):
    """Three problems per launch (none / all / a random half non-zero, −0.0 among the zeros), rows
    after a 5-row lead; outputs pre-filled with a sentinel."""
    F = 5
    rng = np.random.default_rng(l)
    lead = 5
    n = lead + 3 * l
    z = rng.normal(size=(n, F)).astype(np.float32)
    coef = np.full(n, 9.0, np.float32)
    coef[lead:lead + l] = 0.0
    coef[lead + l:lead + 2 * l] = rng.normal(size=l).astype(np.float32) + np.float32(3)
    half = rng.normal(size=l).astype(np.float32)
    zero = rng.random(l) < 0.5
    half[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    coef[lead + 2 * l:] = half
    tab = np.zeros(3, smo._DEC_DT)
    for k in range(3):
        tab[k] = (lead + k * l, 0, l, 0, -1.0, 32)
    zc = torch.full((n, F), -55.0, dtype=torch.float32, device=dev)
    cc = torch.full((n,), -55.0, dtype=torch.float32, device=dev)
    counts = torch.full((3,), -55, dtype=torch.int32, device=dev)
    _E().svm_sv_compact(_d(z, dev).data_ptr(), _d(coef, dev).data_ptr(), F, _tab(tab, dev).data_ptr(), 3,
                        zc.data_ptr(), cc.data_ptr(), counts.data_ptr(), _s(dev))
    zc, cc, counts = zc.cpu().numpy(), cc.cpu().numpy(), counts.cpu().numpy()
    ez, ec = np.full((n, F), -55.0, np.float32), np.full(n, -55.0, np.float32)
    for k in range(3):
        b = lead + k * l
        keep = np.flatnonzero(coef[b:b + l] != 0)
        assert counts[k] == keep.size
        ez[b:b + keep.size] = z[b + keep]
        ec[b:b + keep.size] = coef[b + keep]
    assert counts[0] == 0 and counts[1] == l
    assert np.array_equal(zc.view(np.uint32), ez.view(np.uint32)) and np.array_equal(cc.view(np.uint32), ec.view(np.uint32))


# ------------------------------------------------------------------------------------ svm_dec_batch
def _dec_run(dev, F, shapes, S, seed):
    """One launch of svm_dec_batch over problems ``shapes`` = [(SVs, held rows)], uncompacted
    (counts null: about half the coefficients are zero) and compacted (svm_sv_compact, counts given;
    one problem more whose coefficients are all zero: its count is 0)."""
    rng = np.random.default_rng(seed)
    shapes = list(shapes) + [(40, 3)]
    P = len(shapes)
    tab = np.zeros(P, smo._DEC_DT)
    zs, hs, cs = [], [], []
    zoff = hoff = 0
    e2 = C.ngl2e_of(F)
    for k, (l, h) in enumerate(shapes):
        per = -(-(-(-l // S)) // 32) * 32
        tab[k] = (zoff, hoff, l, h, e2, per)
        z = rng.normal(size=(l, F)).astype(np.float32)
        hrow = rng.normal(size=(h, F)).astype(np.float32)
        hrow[0] = z[0]                                            # a held row that IS a support vector: d² = 0
        c = rng.normal(size=l).astype(np.float32)
        c[rng.random(l) < 0.5] = 0.0
        if k == P - 1:
            c[:] = 0.0
        elif l > 1:
            c[0] = 1.5
        zs.append(z)
        hs.append(hrow)
        cs.append(c)
        zoff += l
        hoff += h
    zcat, hcat, coef = np.concatenate(zs), np.concatenate(hs), np.concatenate(cs)
    E, s = _E(), _s(dev)
    zd, hd, cd, td = _d(zcat, dev), _d(hcat, dev), _d(coef, dev), _tab(tab, dev)
    max_h = max(h for _, h in shapes)
    part = torch.zeros((hoff, S), dtype=torch.float32, device=dev)
    E.svm_dec_batch(zd.data_ptr(), cd.data_ptr(), hd.data_ptr(), F, td.data_ptr(), P, max_h, S, part.data_ptr(), 0, s)
    zc, cc = torch.zeros_like(zd), torch.zeros_like(cd)
    counts = torch.zeros(P, dtype=torch.int32, device=dev)
    E.svm_sv_compact(zd.data_ptr(), cd.data_ptr(), F, td.data_ptr(), P, zc.data_ptr(), cc.data_ptr(), counts.data_ptr(), s)
    part2 = torch.zeros((hoff, S), dtype=torch.float32, device=dev)
    E.svm_dec_batch(zc.data_ptr(), cc.data_ptr(), hd.data_ptr(), F, td.data_ptr(), P, max_h, S, part2.data_ptr(),
                    counts.data_ptr(), s)
    part, part2, counts = part.cpu().numpy(), part2.cpu().numpy(), counts.cpu().numpy()
    for k, (l, h) in enumerate(shapes):
        z, hrow, c = zs[k], hs[k], cs[k]
        ho, per = int(tab[k]["hoff"]), int(tab[k]["per"])
        ref = R.ws_kernel_matvec(np.concatenate([hrow, z]), e2, np.concatenate([np.zeros(h), c.astype(np.float64)]),
                                 rows=np.arange(h))
        K, dK = R.gram_kernel_error(np.concatenate([hrow, z]), e2)
        K, dK = K[:h, h:], dK[:h, h:]
        ac = np.abs(c).astype(L)
        n = per + S                                                # fmas of one partial's chain, the partials' sum
        bud = dK @ ac + n * U32 / (1 - n * U32) * ((K + dK) @ ac)
        nsv = int((c != 0).sum())
        assert counts[k] == nsv
        for name, pt, cnt in (("full", part, l), ("compact", part2, nsv)):
            got = pt[ho:ho + h].astype(L).sum(1)
            assert (np.abs(got - ref) <= bud).all(), (name, F, l, h, S, float(np.abs(got - ref).max()), float(bud.max()))
            used = -(-cnt // per)
            assert (pt[ho:ho + h, used:] == 0).all(), (name, l, h, S)      # splits past the count stay zero
        assert (np.abs(part[ho:ho + h].astype(L).sum(1) - part2[ho:ho + h].astype(L).sum(1)) <= 2 * bud).all()
        if nsv == 0:
            assert (part2[ho:ho + h] == 0).all()


@pytest.mark.parametrize("F", [8, 9, 16, 17, 18, 19, 24, 25, 32, 33, 40, 41, 48, 49, 64])
def test_svm_dec_batch_feature_buckets(dev, F):
    """Both sides of every DEC_CASE bucket, three problems per launch, S = 3.  Budget per row, derived
    as _rbf_core derives its own: Σ_c |coef_c|·dK_tc (gram_kernel_error: the decision kernel evaluates
    gram_rbf_kernel's expression, its row norm as two half-width chains added once, within the same
    γ_F) plus the f32 accumulation γ_n·Σ_c |coef_c|·K̂_tc with n the fmas a partial's chain can hold
    (per) plus the partials summed (S); the partials themselves are added in longdouble here."""
    _dec_run(dev, F, [(33, 5), (70, 129), (257, 2)], 3, F)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("nsv,h", [(1, 1), (31, 127), (32, 128), (33, 129), (255, 1), (256, 127), (257, 128),
                                   (511, 129)])
def test_svm_dec_batch_chunk_edges(dev, nsv, h, S):
    """256-SV chunk and 32-SV MFMA remainders against 128-row held tiles, with and without counts;
    compacting about half of 511 or 257 ends the count inside a chunk."""
    _dec_run(dev, 17, [(nsv, h), (2 * nsv + 1, 2)], S, 1000 * nsv + h)


# ------------------------------------------------------------------------------------ platt_batch
@pytest.mark.parametrize("coop", [False, True], ids=["platt_kernel", "platt_coop_kernel"])
def test_platt_batch(dev, coop):
    """Every listed input as one launch: l ∈ {1, 2, 1023, 1025, 16384, 16385} (16385 is past the
    register path), one-class labels both ways, separable and constant decision values, |dec| to 1e4,
    the three negative source-map codes."""
    cases = [C.platt_ref(n) for n in C.PLATT_NAMES]
    tab = np.zeros(len(cases), smo._PLATT_DT)
    parts, rowks, maps, off = [], [], [], 0
    for k, (c, dec, lab, o, o64) in enumerate(cases):
        tab[k] = (off, c["l"], c["n0"])
        parts.append(c["part"])
        rowks.append(c["rowk"])
        maps.append(np.where(c["srcmap"] >= 0, c["srcmap"] + off, c["srcmap"]).astype(np.int32))
        off += c["l"]
    P = len(cases)
    part_d, rowk_d, map_d = _d(np.concatenate(parts), dev), _d(np.concatenate(rowks), dev), _d(np.concatenate(maps), dev)
    rho_d, c_d = _d(C.PLATT_RHO, dev), _d(C.PLATT_CONSTS, dev)
    dscr = torch.zeros(off, dtype=torch.float64, device=dev)
    AB = torch.full((2 * P,), float("nan"), dtype=torch.float64, device=dev)
    cbar = torch.zeros(P, dtype=torch.int32, device=dev)
    cpart = torch.zeros(P * 2 * 8 * 6, dtype=torch.float64, device=dev)
    _E().platt_batch(_tab(tab, dev).data_ptr(), P, part_d.data_ptr(), 2, rowk_d.data_ptr(), rho_d.data_ptr(),
                     c_d.data_ptr(), map_d.data_ptr(), dscr.data_ptr(), AB.data_ptr(),
                     cbar.data_ptr() if coop else 0, cpart.data_ptr() if coop else 0, _s(dev))
    got = AB.cpu().numpy()
    for k, (c, dec, lab, o, o64) in enumerate(cases):
        A, B = got[2 * k], got[2 * k + 1]
        assert np.isfinite(A) and np.isfinite(B), (c["name"], A, B)
        f, g1, g2, df, dg = o.evaluate(A, B)
        print(f"{c['name']}: A {A!r} B {B!r} oracle {float(o.A)!r} {float(o.B)!r} grad {float(g1):.3e} {float(g2):.3e}")
        # the stop rule at the returned point, in longdouble, within the f64 evaluation bound
        assert (abs(g1) < 1e-5 + dg and abs(g2) < 1e-5 + dg) or o.capped, (c["name"], float(g1), float(g2), float(dg))
        assert o.decided == (c["name"] not in C.PLATT_UNDECIDED), c["name"]
        if o.decided:
            # measured: platt_oracle longdouble vs the same code in float64, 1.1e-15 relative to
            # max(1, |A|, |B|) (C.PLATT_MEASURED, re-measured by the CPU suite); allowed: ten times
            # that, 1.1e-14, for the kernel's fused multiply-adds and reduction order
            tol = C.PLATT_MARGIN * max(1.0, abs(float(o.A)), abs(float(o.B)))
            assert abs(A - float(o.A)) <= tol and abs(B - float(o.B)) <= tol, \
                (c["name"], A - float(o.A), B - float(o.B), tol)


# ------------------------------------------------------------------------------------ svm_gamma
def _gamma_mean_term(z):
    """δ²/Var with δ = (D + 1)·2⁻⁵³·mean|z|, D = ⌈n/1024⌉ + 22: the depth-based bound of the device
    mean's error, as a relative error of the variance (see test_svm_gamma)."""
    z = np.asarray(z, dtype=L).ravel()
    D = -(-z.size // 1024) + 22
    delta = (D + 1) * U64 * np.abs(z).mean()
    return float(delta * delta / z.var())


@pytest.mark.parametrize("F", [1, 17])
def test_svm_gamma(dev, F):
    """Fits of 1, 1,023, 1,025 and 5,000 standardised rows, a fit with mean 1e8 and unit spread, an
    all-zero fit, a fit with one NaN, one with one Inf, and a standardised fit after them, in one
    launch.  γ within 4·n·2⁻⁵³ relative of the longdouble two-pass value, n = rows·F, u = 2⁻⁵³:

    * the sum of squared deviations has positive terms: any order is within n·u relative; each
      deviation and its square round once (3u relative on the term); the division by n, the product
      with F and the reciprocal round once each (3u): together below (n + 6)·u;
    * the mean m̂ = m + δ enters exactly as Σ(z − m̂)²/n = Var + δ²: a relative error δ²/Var.  A
      worst-case sum of n terms would give δ ≤ n·u·mean|z|, which for the mean-1e8 fit is far too
      much (2e-4, squared 4e-8); what bounds δ is the DEPTH of svm_gamma_kernel's sum — a term
      passes through ≤ ⌈n/1024⌉ additions in its thread, 6 wave levels and 16 wave totals — so
      δ ≤ (D + 1)·u·mean|z| with D = ⌈n/1024⌉ + 22.  _gamma_mean_term() evaluates δ²/Var for every fit
      and the test asserts that it and the first part together stay within the 4·n·u allowed (on
      the mean-1e8 fits: 1.9e-13 of 7.7e-12 at F = 17, 6.5e-14 of 4.5e-13 at F = 1; one row of one
      feature has zero variance and is exact)."""
    rng = np.random.default_rng(F)
    rows = [1, 1023, 1025, 5000, 1023, 1025, 1023, 1023, 1025]
    fits = [rng.normal(size=(r, F)) for r in rows]
    fits[4] = 1e8 + fits[4]
    fits[5] = np.zeros((1025, F))
    fits[6][500, F - 1] = np.nan
    fits[7][7, 0] = np.inf
    Z = np.concatenate(fits)
    offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    K = len(rows)
    gam = torch.zeros(K, dtype=torch.float64, device=dev)
    e2 = torch.zeros(K, dtype=torch.float32, device=dev)
    _E().svm_gamma(_d(Z, dev).data_ptr(), _d(offs, dev).data_ptr(), K, F, gam.data_ptr(), e2.data_ptr(), _s(dev))
    g, e = gam.cpu().numpy(), e2.cpu().numpy()
    ref, _ = R.gamma_oracle(Z, offs, F)
    for k in range(K):
        if k in (6, 7):
            assert np.isnan(g[k]) and np.isnan(e[k]) and np.isnan(ref[k])
            continue
        if k == 5 or (k == 0 and F == 1):
            assert g[k] == 1.0 and ref[k] == 1                     # variance exactly 0
        else:
            n = rows[k] * F
            assert (n + 6) * U64 + _gamma_mean_term(fits[k]) <= 4 * n * U64, (k, n)      # the derivation closes
            assert abs(L(g[k]) - ref[k]) <= 4 * n * U64 * ref[k], (k, g[k], float(ref[k]))
        assert e[k] == np.float32(-g[k] * 1.4426950408889634)
