"""The longdouble inference oracle (ops/reference.py stack_oracle, rbf_oracle, proba_oracle,
forest_oracle) — written on the UNPACKED model, apart from the kernels and from ops.packing — checked
here against sklearn, against the host paths, and for its power: nine deliberately wrong variants of
the host reference must each be rejected by ``assert_stack`` on a named case.

The input constructions live here and are imported by tests/test_infer_reference_gpu.py; each is
built once per process together with its oracle.  Every input has at most 1 % ``undecided`` rows (the
coupling's iteration count changes within the row's decision-value budget: p jumps there and no
tolerance can referee it) — a condition on the INPUT, asserted here, never relaxed."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from hfens.ops import reference as ref
from hfens.ops.packing import PackedStack, pack_forest, pack_stack, pack_svs, stump_table
from hfens.ops.reference import (StackSpec, couple_oracle, forest_oracle, proba_oracle, rbf_oracle,
                                 stack_oracle)

U = 2.0 ** -24
WIDTHS = [1, 2, 7, 8, 9, 17, 18, 19, 24, 25, 32, 33, 40, 63, 64]
WIDTH_ROWS = [1, 63, 64, 65, 127, 513]
RESID_MP = [544, 576, 1600, 1632, 2784, 3232]             # 2784 = 2·1376 + 32: the 12-wave plan's 32-SV tail
RBF_WIDTHS = [1, 4, 5, 8, 16, 17, 24, 32, 33, 48, 49, 64]
RBF_CHUNK_EDGES = [(24, 960), (48, 512), (64, 384)]       # mp = launch_rbf's chunk + 32 (KS 12, 24, 32)
PLATT_AB = [(-1.25857732, -1.18972403), (-1.7, 0.1), (-0.6, 0.8)]


# ----------------------------------------------------------------------------- models
def make_trees(rng, F, T, depth, feats=None):
    K = 2 ** (depth + 1) - 1
    feat = np.full((T, K), -2)
    thr = np.full((T, K), -2.0)
    left = np.full((T, K), -1)
    right = np.full((T, K), -1)
    val = rng.normal(size=(T, K))
    for t in range(T):
        for i in range(2 ** depth - 1):
            feat[t, i] = rng.integers(0, F) if feats is None else feats[rng.integers(0, len(feats))]
            thr[t, i] = rng.normal()
            left[t, i], right[t, i] = 2 * i + 1, 2 * i + 2
    return dict(feature=feat, threshold=thr, left=left, right=right, value=val)


def make_spec(F, m, T, depth, seed, **over):
    rng = np.random.default_rng(seed)
    kw = dict(mean=0.1 * rng.standard_normal(F), scale=1.0 / (0.5 + rng.random(F)),
              sv=rng.standard_normal((m, F)), coef=rng.standard_normal(m) / m ** 0.5, gamma=0.5 / F,
              intercept=0.2, A=-1.7, B=0.1, init=-0.4, lr=0.1, lr_w=0.3 * rng.standard_normal(F), lr_b=-0.2,
              meta_w=(1.9, 0.5, 2.7), meta_b=-2.0, **make_trees(rng, F, T, depth))
    kw.update(over)
    return StackSpec(**kw)


def pack_spec(M, device, stumps=True):
    """``M`` through the real packing (pack_svs, pack_forest, stump_table) — the side under test."""
    t = torch.as_tensor
    tabs = [t(M.feature), t(M.threshold), t(M.left), t(M.right), t(M.value)]
    return PackedStack(
        F=M.F, sv=pack_svs(t(M.sv), t(M.coef), device),
        mean=t(M.mean).to(device=device, dtype=torch.float32).contiguous(),
        inv_scale=(1.0 / t(M.scale)).to(device=device, dtype=torch.float32).contiguous(),
        gamma=M.gamma, svc_b=M.intercept, probA=M.A, probB=M.B, forest=pack_forest(*tabs, device),
        stumps=stump_table(*tabs, M.init, M.lr, M.F, device) if stumps else None, gb_init=M.init, gb_lr=M.lr,
        lr_w=t(M.lr_w).to(device=device, dtype=torch.float32).contiguous(), lr_b=M.lr_b,
        meta_w=M.meta_w, meta_b=M.meta_b)


def spec_from_clf(clf):
    """The unpacked parameters of a fitted HF stack (what pack_stack reads, before any packing)."""
    from hfens.models.gbdt import GradientBoostingClassifier
    from hfens.models.linear import LogisticRegression
    from hfens.models.stacking import Pipeline
    idx = {}
    for i, e in enumerate(clf.estimators_):
        idx["svc" if isinstance(e, Pipeline) else "gbc" if isinstance(e, GradientBoostingClassifier) else "lg"] = i
    assert isinstance(clf.estimators_[idx["lg"]], LogisticRegression)
    sc, svc = (s[1] for s in clf.estimators_[idx["svc"]].steps)
    gbc, lg, fin = clf.estimators_[idx["gbc"]], clf.estimators_[idx["lg"]], clf.final_estimator_
    n = lambda a: a.detach().cpu().to(torch.float64).numpy()   # noqa: E731
    mc = n(fin.coef_[0])
    return StackSpec(mean=n(sc.mean_), scale=n(sc.scale_), sv=n(svc.support_vectors_), coef=n(svc._dual_coef_[0]),
                     gamma=float(svc._gamma), intercept=float(svc._intercept_[0]), A=float(svc._probA[0]),
                     B=float(svc._probB[0]), feature=n(gbc.tree_feature_), threshold=n(gbc.tree_threshold_),
                     left=n(gbc.tree_left_), right=n(gbc.tree_right_), value=n(gbc.tree_value_),
                     init=float(gbc.init_raw_), lr=float(gbc.learning_rate), lr_w=n(lg.coef_[0]),
                     lr_b=float(lg.intercept_[0]), meta_w=(mc[idx["svc"]], mc[idx["gbc"]], mc[idx["lg"]]),
                     meta_b=float(fin.intercept_[0]))


def patients(n, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 2, size=(n, 17)).astype(np.float64)
    X[:, 6] += 1
    X[:, 13] = rng.normal(18.6, 4.4, n).round()
    X[:, 15] = rng.integers(0, 5, n)
    X[:, 16] = rng.normal(63, 5, n).round()
    return X


# ----------------------------------------------------------------------------- threshold edges
def f32_next(v, k):
    """The f32 ``k`` ulps after (before, k < 0) f32 value ``v``, through −0.0/0.0 and the subnormals."""
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


def edge_thresholds():
    """f64 thresholds: exact f32 values (positive, negative, 0.0, the f32-subnormal 2⁻¹³⁰) and points
    strictly between adjacent f32 values (the midpoint and the ¾ point, which round to nearest
    UPWARDS) — not representable in f32."""
    out = []
    for v in (0.37, -1.25, 1.0, -0.015625, 3.0e-3):
        a = np.float32(v)
        b = f32_next(a, 1)
        out += [float(a), (float(a) + float(b)) / 2, float(a) + 0.75 * (float(b) - float(a))]
    return out + [0.0, 2.0 ** -130, -(2.0 ** -130) * 1.5]


def edge_values(thr):
    """Row values for a split at ``thr``: the f32 at or below it, its neighbours, ∓0.0, ±3e38 —
    as exact f32 values and as f64 values a quarter ulp to either side (they round to the same f32)."""
    lo = np.float32(thr)
    if float(lo) > thr:
        lo = f32_next(lo, -1)
    base = [lo, f32_next(lo, 1), f32_next(lo, -1), f32_next(lo, 2), np.float32(-0.0), np.float32(0.0),
            np.float32(3e38), np.float32(-3e38)]
    out = []
    for v in base:
        q = (float(f32_next(v, 1)) - float(v)) / 4
        out += [float(v), float(v) + q, float(v) - q]
    return out


def edge_model(F, stumps):
    """Every edge threshold at the root of a tree (depth 1: the stump table; depth 2: the tree walk,
    the children splitting on other edge thresholds); leaves of one tree ≥ 0.3 apart with lr = 1, so a
    wrong leaf moves raw_gbc by ≥ 0.3 against a budget of 1e-6.  The scaler divides by 2⁷⁰ (|z| stays
    finite at x = ±3e38) and the LR weights are 0 (x·w cannot overflow): the case is about the trees."""
    rng = np.random.default_rng(60 + F)
    thrs = edge_thresholds()
    T = len(thrs)
    depth = 1 if stumps else 2
    K = 2 ** (depth + 1) - 1
    tr = make_trees(rng, F, T, depth)
    for t in range(T):
        tr["feature"][t, 0] = t % F
        tr["threshold"][t, 0] = thrs[t]
        s = 1.0 if t % 2 else -1.0
        if stumps:
            tr["value"][t] = [0.0, -0.15 * s, 0.15 * s]
        else:
            tr["feature"][t, 1], tr["feature"][t, 2] = (t + 1) % F, (t + 2) % F
            tr["threshold"][t, 1], tr["threshold"][t, 2] = thrs[(t + 1) % T], thrs[(t + 2) % T]
            tr["value"][t] = [0.0, 0.0, 0.0, -0.45 * s, -0.15 * s, 0.15 * s, 0.45 * s]
    M = make_spec(F, 40, T, depth, 61 + F, scale=np.full(F, 2.0 ** 70), lr_w=np.zeros(F), lr=1.0, init=0.05, **tr)
    rows = []
    for t in range(T):
        split = [(t % F, thrs[t])]
        if not stumps:
            split += [((t + 1) % F, thrs[(t + 1) % T]), ((t + 2) % F, thrs[(t + 2) % T])]
        for f, th in split:
            for v in edge_values(th):
                x = rng.standard_normal(F)
                x[f] = v
                rows.append(x)
    return M, np.array(rows)


# ----------------------------------------------------------------------------- the cases
Case = namedtuple("Case", "M X rows orc stumps")


def _sample(n, k, seed, extra=()):
    rng = np.random.default_rng(seed)
    r = set(rng.choice(n, size=min(k, n), replace=False).tolist()) | {i for i in extra if 0 <= i < n}
    return np.array(sorted(r))


def _build(name):
    """-> (M, X f64, rows the oracle is evaluated on or None for all, stump table wanted)."""
    p = name.split("-")
    if p[0] == "width":                               # width-F-stumps|forest
        F, st = int(p[1]), p[2] == "stumps"
        M = make_spec(F, 70, 12, 1 if st else 3, 100 + F)
        return M, np.random.default_rng(F).standard_normal((513, F)), None, st
    if p[0] == "resid":                               # resid-mp: F = 17, m = mp − 3 (3 pad slots)
        mp = int(p[1])
        # (coefficients ~ 1/m: the m·u·Σ|c|k accumulation budget stays far below the spacing of the
        # coupling jumps, or a percent of the rows would be undecided at m = 3229)
        M = make_spec(17, mp - 3, 20, 1, mp, coef=np.random.default_rng(mp + 1).standard_normal(mp - 3) / (mp - 3))
        X = np.random.default_rng(mp).standard_normal((2048, 17))
        return M, X, _sample(2048, 160, mp, (0, 31, 32, 63, 64, 511, 512, 1023, 1024, 1535, 1536, 2047)), True
    if name == "trees-global":                        # 100 × 31 nodes × 20 B > 24 KiB
        return make_spec(17, 70, 100, 4, 7), np.random.default_rng(7).standard_normal((300, 17)), None, False
    if p[0] == "evict":                               # evict-mp: F = 64, 60 depth-3 trees
        mp = int(p[1])
        return make_spec(64, mp - 2, 60, 3, mp), np.random.default_rng(mp).standard_normal((300, 64)), None, False
    if name == "t0":
        M = make_spec(17, 70, 0, 1, 9)
        return M, np.random.default_rng(9).standard_normal((200, 17)), None, False
    if name == "sparse-stumps":                       # odd features carry no stump; one pair 5 times
        rng = np.random.default_rng(11)
        tr = make_trees(rng, 17, 40, 1, feats=list(range(0, 17, 2)))
        tr["feature"][:5, 0], tr["threshold"][:5, 0] = 4, 0.3
        return make_spec(17, 70, 40, 1, 11, **tr), rng.standard_normal((300, 17)), None, True
    if p[0] == "thr":                                 # thr-F-stumps|walk
        M, X = edge_model(int(p[1]), p[2] == "stumps")
        return M, X, None, p[2] == "stumps"
    if p[0] == "dist":                                # dist | dist-underflow: identity scaler, z = x
        rng = np.random.default_rng(13)
        F, m = 17, 70
        coef = rng.standard_normal(m) / m ** 0.5
        coef[3] = 1e4 * np.abs(coef).mean()
        M = make_spec(F, m, 12, 1, 13, mean=np.zeros(F), scale=np.ones(F), coef=coef,
                      gamma=50.0 if name == "dist-underflow" else 0.5 / F)
        sv32 = M.sv.astype(np.float32).astype(np.float64)
        far = rng.standard_normal((20, F))
        far *= 50.0 / np.linalg.norm(far, axis=1, keepdims=True)
        X = np.concatenate([sv32[:20], sv32[20:40] + 1e-6 * rng.choice([-1.0, 1.0], (20, F)), far,
                            rng.standard_normal((140, F))])
        return M, X, None, True
    if p[0] == "platt":                               # platt-i: F = 1, dec = 16·exp(−x²/4) − 8 ∈ (−8, 8]
        A, B = PLATT_AB[int(p[1])]
        M = make_spec(1, 1, 4, 1, 17, mean=np.zeros(1), scale=np.ones(1), sv=np.zeros((1, 1)), coef=[16.0],
                      gamma=0.25, intercept=-8.0, A=A, B=B)
        return M, _platt_rows(M), None, True
    if p[0] == "sat":                                 # sat-i-(p|n|cp|cn): every coef 0, dec = intercept
        A, B = PLATT_AB[int(p[1])]
        clip = 16.11809565095832                      # ln((1 − 1e-7)/1e-7): r01 meets its clip
        dec = {"p": 1e4, "n": -1e4, "cp": (clip - B) / A, "cn": (-clip - B) / A}[p[2]]
        M = make_spec(5, 40, 6, 1, 19, coef=np.zeros(40), intercept=dec, A=A, B=B)
        return M, np.random.default_rng(19).standard_normal((70, 5)), None, True
    raise KeyError(name)


def coupling_jumps(A, B, lo=-8.0, hi=8.0, grid=4001):
    """Decision values in [lo, hi] where the oracle's iteration count changes: (f32 just below, f32
    just above) pairs, bisected down to adjacent f32 values."""
    d = np.linspace(lo, hi, grid)
    it = couple_oracle(d, A, B)[1]
    out = []
    for i in np.nonzero(it[1:] != it[:-1])[0]:
        a, b = np.float32(d[i]), np.float32(d[i + 1])
        ia = couple_oracle(np.array([a]), A, B)[1][0]
        while np.nextafter(a, np.float32(np.inf)) < b:
            c = np.float32((float(a) + float(b)) / 2)
            if couple_oracle(np.array([c]), A, B)[1][0] == ia:
                a = c
            else:
                b = c
        out.append((a, b))
    return out


@functools.lru_cache(maxsize=None)
def platt_decs(A, B):
    """f32 decision values at every jump ± 64 ulps, at the clip points of r01 ± 64 ulps, and ±1e4."""
    clip = 16.11809565095832
    pts = [f32_next(a, -64) for a, _ in coupling_jumps(A, B, -40, 40, 8001)]
    pts += [f32_next(b, 64) for _, b in coupling_jumps(A, B, -40, 40, 8001)]
    for c in ((clip - B) / A, (-clip - B) / A):
        pts += [np.float32(c), f32_next(c, 64), f32_next(c, -64)]
    return np.array(pts + [np.float32(1e4), np.float32(-1e4), np.float32(0.0)], dtype=np.float32)


def _platt_rows(M):
    """Rows x of the F = 1 model whose decision value 16·exp(−x²/4) − 8 lies 64 budgets to either
    side of each coupling jump in (−8, 8), plus a sweep."""
    xs = list(np.linspace(0.0, 6.0, 120))
    for a, b in coupling_jumps(M.A, M.B, -7.9, 7.9):
        for edge, sgn in ((float(a), -1.0), (float(b), 1.0)):
            x = np.sqrt(-4.0 * np.log((edge + 8.0) / 16.0))
            for _ in range(3):                        # budget at the row, then 64 of them off the jump
                dd = float(stack_oracle(M, np.array([[x]]))["d_dec"][0])
                x = np.sqrt(-4.0 * np.log((edge + sgn * 64 * dd + 8.0) / 16.0))
            xs.append(x)
    return np.array(xs)[:, None]


@functools.lru_cache(maxsize=None)
def case(name, x3=True):
    M, X, rows, stumps = _build(name)
    orc = stack_oracle(M, X if rows is None else X[rows], x3=x3)
    return Case(M, X, rows, orc, stumps)


WIDTH_CASES = [f"width-{F}-{k}" for F in WIDTHS for k in ("stumps", "forest")]
RESID_CASES = [f"resid-{mp}" for mp in RESID_MP]
TREE_CASES = ["trees-global", "evict-96", "evict-128", "t0", "sparse-stumps"]
THR_CASES = [f"thr-{F}-{k}" for F in (6, 7) for k in ("stumps", "walk")]
DIST_CASES = ["dist", "dist-underflow"]
PLATT_CASES = [f"platt-{i}" for i in range(3)]
SAT_CASES = [f"sat-{i}-{k}" for i in range(3) for k in ("p", "n", "cp", "cn")]
STACK_CASES = WIDTH_CASES + RESID_CASES + TREE_CASES + THR_CASES + DIST_CASES + PLATT_CASES + SAT_CASES
HOST_CASES = [c for c in STACK_CASES if c not in ("resid-1632", "resid-2784", "resid-3232")]   # (the largest: GPU only)


def assert_stack(got, orc, name="", key="P", decided=None, quiet=False):
    """``got`` against the oracle's ``key`` on the oracle's rows: the shape, no NaN, and every decided
    row within its own budget ``d_<key>``; prints the largest observed/budget ratio and the undecided
    count.  Returns the ratio."""
    got = np.asarray(got, dtype=np.float64)
    want, bud = orc[key], orc["d_" + key]
    assert got.shape == want.shape, f"{name}: shape {got.shape}, want {want.shape}"
    assert not np.isnan(got).any(), f"{name}: {int(np.isnan(got).sum())} NaN"
    if decided is None:
        decided = ~orc["undecided"] if key in ("P", "p_svc") else np.ones(want.shape, dtype=bool)
    ratio = (np.abs(got.astype(np.longdouble) - want) / bud)[decided]
    worst = float(ratio.max()) if ratio.size else 0.0
    if not quiet:
        print(f"{name} [{key}]: rows {want.size}, largest observed/budget {worst:.3f}, "
              f"undecided {int((~decided).sum())}")
    assert worst <= 1.0, f"{name}: {int((ratio > 1).sum())} rows over budget, worst {worst:.3g}x"
    return worst


def host_stack(c, pk=None):
    """ref.stack_infer on the packed model, rows rounded to f32 first (what the kernel is given)."""
    pk = pack_spec(c.M, "cpu", c.stumps) if pk is None else pk
    X = c.X if c.rows is None else c.X[c.rows]
    with np.errstate(over="ignore"):
        x32 = torch.as_tensor(X.astype(np.float32))
    return ref.stack_infer(x32, pk).numpy()


# ----------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("x3", [True, False], ids=["x3", "f32"])
@pytest.mark.parametrize("name", STACK_CASES)
def test_undecided_cap(name, x3):
    c = case(name, x3)                                # both budgets the GPU module referees with
    und = c.orc["undecided"]
    assert und.mean() <= 0.01, f"{name}: {int(und.sum())} of {und.size} rows undecided"
    assert np.isfinite(c.orc["P"].astype(np.float64)).all()
    if name.startswith("platt"):
        assert not und[120:].any()                    # the rows placed 64 budgets beside the jumps
        its = c.orc["it"][120:]
        assert (its[0::2] != its[1::2]).all()         # … and they straddle them


@pytest.mark.parametrize("A,B", PLATT_AB)
def test_platt_decs_are_decided(A, B):
    """The decision values handed to svc_proba1 / svc_oof (jump ± 64 f32 ulps, clip points, ±1e4):
    none undecided, several iteration counts, and both sides of every jump present."""
    dec = platt_decs(A, B)
    p, it, dp, und = proba_oracle(dec, A, B)
    assert not und.any() and len(set(it.tolist())) >= 3
    k = len(coupling_jumps(A, B, -40, 40, 8001))
    assert k >= 3 and (it[:k] != it[k:2 * k]).all()   # below[i], above[i] straddle jump i
    assert float(dp.max()) < 1e-6                     # … each on a flat stretch of p(dec)


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_reference_matches_oracle(name):
    c = case(name)
    assert_stack(host_stack(c), c.orc, name)
    if c.stumps:                                      # the same model through the tree walk
        assert_stack(host_stack(c, pack_spec(c.M, "cpu", False)), c.orc, name + " (walk)")


def test_checkpoint_matches_oracle(ckpt_path):
    from hfens.io.checkpoint import load_checkpoint
    clf = load_checkpoint(ckpt_path)
    X = patients(1500)
    orc = stack_oracle(spec_from_clf(clf), X)
    assert orc["undecided"].mean() <= 0.01
    assert_stack(ref.stack_infer(torch.as_tensor(X), pack_stack(clf, "cpu")).numpy(), orc, "checkpoint, fused")
    assert_stack(clf.predict_proba(torch.as_tensor(X))[:, 1].numpy(), orc, "checkpoint, per model")


def _sk_data(n, F, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F))
    y = (X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.3 * rng.standard_normal(n) > 0).astype(int)
    return X, y, rng.standard_normal((200, F))


def test_oracle_matches_sklearn_svc():
    SVC = pytest.importorskip("sklearn.svm").SVC
    X, y, Xt = _sk_data(300, 6, 0)
    sk = SVC(kernel="rbf", gamma=0.2, probability=True, random_state=0).fit(X, y)
    dec, dd = rbf_oracle(Xt, sk.support_vectors_, sk.dual_coef_[0], 0.2, sk.intercept_[0])
    assert_stack(sk.decision_function(Xt), dict(dec=dec, d_dec=dd), "sklearn decision_function", key="dec")
    # predict_proba runs libsvm on its own sign convention (_dual_coef_, _intercept_, _probA, _probB)
    dec, dd = rbf_oracle(Xt, sk.support_vectors_, sk._dual_coef_[0], 0.2, sk._intercept_[0])
    p, it, dp, und = proba_oracle(dec, sk._probA[0], sk._probB[0], dd)
    assert und.mean() <= 0.01 and len(set(it.tolist())) > 1
    assert_stack(sk.predict_proba(Xt)[:, 1], dict(p_svc=p, d_p_svc=dp, undecided=und), "sklearn predict_proba",
                 key="p_svc")


def test_oracle_matches_sklearn_gbc():
    GBC = pytest.importorskip("sklearn.ensemble").GradientBoostingClassifier
    X, y, Xt = _sk_data(300, 6, 1)
    sk = GBC(n_estimators=25, max_depth=3, random_state=0).fit(X, y)
    trees = [e[0].tree_ for e in sk.estimators_]
    K = max(t.node_count for t in trees)
    tab = {k: np.full((len(trees), K), fill) for k, fill in
           (("feature", -2), ("threshold", -2.0), ("left", -1), ("right", -1), ("value", 0.0))}
    for i, t in enumerate(trees):
        k = t.node_count
        tab["feature"][i, :k], tab["threshold"][i, :k] = t.feature, t.threshold
        tab["left"][i, :k], tab["right"][i, :k], tab["value"][i, :k] = t.children_left, t.children_right, t.value[:, 0, 0]
    p1 = sk.init_.class_prior_[1]
    raw, dr = forest_oracle(Xt, tab["feature"], tab["threshold"], tab["left"], tab["right"], tab["value"],
                            np.log(p1 / (1 - p1)), sk.learning_rate)
    assert_stack(sk.decision_function(Xt), dict(raw_gbc=raw, d_raw_gbc=dr), "sklearn GBC", key="raw_gbc")


def test_coupling_jumps_are_real():
    """The discontinuity the ``undecided`` flag exists for: p_svc(dec) steps by up to ~5e-3 where the
    iteration count changes, so adjacent f32 decision values can differ by 1000× any rounding budget."""
    A, B = PLATT_AB[0]
    jumps = coupling_jumps(A, B)
    assert len(jumps) >= 4
    steps = [abs(float(np.subtract(*couple_oracle(np.array([a, b]), A, B)[0]))) for a, b in jumps]
    assert 1e-3 < max(steps) < 1e-2
    a, b = jumps[0]
    _, _, _, und = proba_oracle(np.array([a], dtype=np.float64), A, B, np.array([float(b) - float(a)]))
    assert und[0]
    _, _, dp, und = proba_oracle(np.array([f32_next(a, -64)], dtype=np.float64), A, B, np.array([float(b) - float(a)]))
    assert not und[0] and dp[0] < 1e-6


# ----------------------------------------------------------------------------- mutants
def _mut_lt(c):
    pk = pack_spec(c.M, "cpu", c.stumps)              # x <= prev(t)  ⇔  x < t
    down = lambda t: torch.nextafter(t, torch.tensor(float("-inf")))   # noqa: E731
    pk.stumps.pairs[:, 0] = down(pk.stumps.pairs[:, 0])
    return host_stack(c, pk)


def _mut_nearest(c, monkeypatch):
    from hfens.ops import packing
    monkeypatch.setattr(packing, "f32_round_down", lambda thr: thr.to(torch.float32))
    return host_stack(c)


def _mut_nodup(c):
    pk = pack_spec(c.M, "cpu", True)
    lo, hi = int(pk.stumps.off[4]), int(pk.stumps.off[5])    # feature 4's pair at 0.3 occurs 5 times
    off = lo + int((pk.stumps.pairs[lo:hi, 0] - 0.3).abs().argmin())
    assert abs(float(pk.stumps.pairs[off, 0]) - 0.3) < 1e-6
    pk.stumps.pairs[off, 1] = float(c.M.lr * (c.M.value[4, 2] - c.M.value[4, 1]))
    return host_stack(c, pk)


def _mut_noinit(c):
    pk = pack_spec(c.M, "cpu", True)
    pk.stumps.base -= c.M.init
    return host_stack(c, pk)


def _mut_drop32(c):
    pk = pack_spec(c.M, "cpu", c.stumps)
    m = c.M.sv.shape[0]                               # the last 32 REAL SVs (the pad slots behind them are 0 anyway)
    assert m >= 64 and float(pk.sv.coef[m - 32:m].abs().min()) > 0 and not pk.sv.coef[m:].any()
    pk.sv.coef[m - 32:m] = 0
    return host_stack(c, pk)


def _mut_znorm(c, monkeypatch):
    def rbf(z, sv, coef, gamma, b, chunk=65536):       # the expanded form, ‖z‖² without its last feature
        zn = (z[:, :-1] ** 2).sum(1)
        d2 = (sv ** 2).sum(1)[None, :] + zn[:, None] - 2 * z @ sv.t()
        return torch.exp(-gamma * d2) @ coef + b
    monkeypatch.setattr(ref, "rbf_decision", rbf)
    return host_stack(c)


def _mut_swap(c):
    out = host_stack(c).copy()
    full = out[:out.size // 64 * 64].reshape(-1, 2, 32)
    full[:] = full[:, ::-1].copy()
    return out


def _mut_iter(c, monkeypatch):
    def couple(r01, max_iter=100):                     # stop one sweep early
        r = r01.numpy().astype(np.longdouble)
        f = np.log((1 - r) / r)                        # couple_oracle(dec = f, A = 1, B = 0) has r01 = r
        it = torch.as_tensor(couple_oracle(f, 1.0, 0.0)[1])
        out = torch.full_like(r01, 0.5)
        for v in it.unique().tolist():
            if v >= 1:
                out[it == v] = orig(r01[it == v], max_iter=v - 1) if v > 1 else 0.5
        return out
    orig = ref.couple2
    monkeypatch.setattr(ref, "couple2", couple)
    return host_stack(c)


def _mut_noclip(c, monkeypatch):
    monkeypatch.setattr(ref, "svc_proba1", lambda dec, A, B: ref.couple2(ref.sigmoid_predict(dec, A, B)))
    return host_stack(c)


MUTANTS = {
    "< for <=": (_mut_lt, False, ["thr-6-stumps", "thr-7-stumps"]),
    "threshold rounded to nearest": (_mut_nearest, True, ["thr-6-stumps", "thr-7-walk"]),
    "duplicate stumps not summed": (_mut_nodup, False, ["sparse-stumps"]),
    "base without init": (_mut_noinit, False, ["width-17-stumps"]),
    "last 32 SVs dropped": (_mut_drop32, False, ["width-17-stumps"]),
    "feature F-1 out of |z|^2": (_mut_znorm, True, ["width-17-stumps", "width-7-forest"]),
    "row halves of a tile exchanged": (_mut_swap, False, ["width-17-stumps"]),
    "one coupling iteration fewer": (_mut_iter, True, ["width-17-stumps"]),
    "clip at 1e-7 omitted": (_mut_noclip, True, ["sat-0-p", "sat-0-n"]),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_is_rejected(mutant, monkeypatch):
    fn, patches, names = MUTANTS[mutant]
    rejected = []
    for name in names:
        c = case(name)
        with monkeypatch.context() as mp:
            out = fn(c, mp) if patches else fn(c)
        assert_stack(host_stack(c), c.orc, name + " (unmutated)")
        try:
            assert_stack(out, c.orc, f"{name} ({mutant})")
        except AssertionError:
            rejected.append(name)
    assert rejected == names, f"{mutant}: not rejected on {sorted(set(names) - set(rejected))}"
