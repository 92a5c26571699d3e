"""The launch-path GBDT training kernels (ops/csrc/gbdt.hip gbdt_hist, gbdt_split, gbdt_route,
gbdt_apply_prep), each called on its own as ``hist_gbdt._run_device`` calls it, against the exact
oracles of ops/reference.py on the crafted cases of tests/test_gbdt_reference.py (which proves on the
CPU that the cases are decided and reach the branches they name).  Histograms, routing, bagging
weights, node statistics, thresholds and the w ∈ {0, 1} Σw·r² are bit-equal; the chosen cut carries the
f64 gain certificate; values, g, h, raw and the fixed-point sums stay within their derived budgets."""
import numpy as np
import pytest
import torch

from hfens import ops

from test_gbdt_reference import (HIST_CASES, PREP_CASES, ROUTE_CASES, check_prep,
                                 check_route, check_split, hist_case, prep_case, route_case, split_launches)

pytestmark = pytest.mark.gpu


def _d(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


@pytest.mark.parametrize("case", HIST_CASES, ids=str)
def test_hist_bit_equal(dev, case):
    c = hist_case(*case)
    bins, nbins = _d(c.bins, dev), _d(c.nbins, dev)
    g, h, w, node = _d(c.g, dev), _d(c.h, dev), _d(c.w, dev), _d(c.node, dev, torch.int32)
    H = torch.zeros(c.B, c.NL, c.F, 256, 3, dtype=torch.int64, device=dev)
    ops.ext().gbdt_hist(c.B, c.n, c.F, bins.data_ptr(), nbins.data_ptr(), 256, g.data_ptr(), h.data_ptr(),
                        w.data_ptr(), node.data_ptr(), c.node0, c.NL, H.data_ptr(), float(2 ** c.shift),
                        ops.stream_ptr(dev))
    want = torch.from_numpy(c.expect)
    got = H.cpu()
    assert torch.equal(got, want), (got != want).nonzero()[:4].tolist()


@pytest.mark.parametrize("idx", range(17))
def test_split_certified(dev, idx):
    L = split_launches()[idx]
    o = {k: _d(v, dev) for k, v in L.blank().items()}
    hist, nbins, lo, hi, r2 = (_d(a, dev) for a in (L.hist, L.nbins, L.lo, L.hi, L.r2))
    ops.ext().gbdt_split(L.B, L.F, L.NN, hist.data_ptr(), nbins.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                         L.node0, L.NL, L.last, float(L.min_leaf_q), float(L.min_split_q), float(2 ** L.shift),
                         o["feat"].data_ptr(), o["blo"].data_ptr(), o["thr"].data_ptr(), o["value"].data_ptr(),
                         o["stats"].data_ptr(), r2.data_ptr(), ops.stream_ptr(dev))
    undecided = check_split(L, {k: v.cpu().numpy() for k, v in o.items()})
    print(f"{L.name}: {len(L.oracles)} nodes, {undecided} undecided")
    assert undecided == 0


@pytest.mark.parametrize("case", ROUTE_CASES, ids=str)
def test_route_bit_equal(dev, case):
    c = route_case(*case)
    bins, g, w = _d(c.bins, dev), _d(c.g, dev), _d(c.w, dev)
    node, feat, blo, r2 = _d(c.node, dev, torch.int32), _d(c.feat, dev), _d(c.blo, dev), _d(c.r2_start, dev)
    ops.ext().gbdt_route(c.B, c.n, c.NN, bins.data_ptr(), g.data_ptr(), w.data_ptr(), node.data_ptr(),
                         feat.data_ptr(), blo.data_ptr(), r2.data_ptr(), c.node0, c.NL, float(2 ** c.shift),
                         ops.stream_ptr(dev))
    check_route(c, node.cpu().numpy(), r2.cpu().numpy())


@pytest.mark.parametrize("case", PREP_CASES, ids=str)
def test_apply_prep_sums(dev, case):
    """Routing, bagging weights, raw, g, h and the three fixed-point sums of one ``gbdt_apply_prep`` call.

    The budget of the sums is Σ_rows (1 + ε·|x|·scale) with ε = ``reference.GBDT_EPS_F64`` = 64u: twice the
    largest per-row relative discrepancy measured on an MI355X against the longdouble oracle (one row
    per model, 8192 rows; deviance at scale 2^48 on rows with |x| ≥ 1, w·r² at 2^50 on rows with x ≥ ¼:
    measured 31.93u — no row off by more than one unit, the resolution — allowed 64u).  At the
    scales in use (2^26 deviance, 2^40 Σw·r²) ε·|x|·scale stays below 2^-6 per row; the absolute error of
    the cancelling ``y·raw − log(1 + e^raw)`` at |raw| = 700, u·700·2^26 < 2^-17 units, sits in the half
    unit between rint's own ½ and the 1 the budget grants each row."""
    c = prep_case(*case)
    bins, y, w, raw = _d(c.bins, dev), _d(c.y, dev), _d(c.w, dev), _d(c.raw, dev)
    node = _d(c.node, dev, torch.int32)
    g, h, wt = torch.empty_like(w), torch.empty_like(w), torch.full_like(w, -1.0)
    prev_r2, cur_r2 = _d(c.start[0], dev), _d(c.start[1], dev)
    acc = _d(c.start[2][:, 0], dev)
    seeds = _d(c.seeds.view(np.int64), dev)
    prev = (0, 0, 0, 0, 0)
    if c.prev is not None:
        feat, blo, value = _d(c.feat, dev), _d(c.blo, dev), _d(c.value, dev)
        prev = (feat.data_ptr(), blo.data_ptr(), value.data_ptr(), prev_r2.data_ptr(), acc.data_ptr())
    bag = c.subsample < 1.0
    ops.ext().gbdt_apply_prep(c.B, c.n, c.F, c.NN, bins.data_ptr(), y.data_ptr(), w.data_ptr(), raw.data_ptr(),
                              g.data_ptr(), h.data_ptr(), node.data_ptr(), *prev, cur_r2.data_ptr(), c.lr,
                              float(2 ** c.shift), float(2 ** 26), wt.data_ptr() if bag else 0, c.subsample,
                              seeds.data_ptr() if bag else 0, c.row_off, c.stage, ops.stream_ptr(dev))
    n = lambda t: t.cpu().numpy()   # noqa: E731
    check_prep(c, dict(raw=n(raw), g=n(g), h=n(h), node=n(node), wt=n(wt) if bag else None, prev_r2=n(prev_r2),
                       cur_r2=n(cur_r2), dev=n(acc)))


def test_apply_prep_row_error_within_measured(dev):
    """The measurement behind ``reference.GBDT_EPS_MEASURED``, repeated: one row per model (8192 rows), the
    deviance at scale 2^48 and w·r² at 2^50, against the longdouble oracle's rounded term.  On rows with
    |x| ≥ 1 (deviance) or x ≥ ¼ (w·r²) the relative discrepancy stays within the recorded 32u."""
    from hfens.ops import reference as ref
    B, n, NN, F = 4096, 1, 3, 1
    rng = np.random.default_rng(3)
    worst = 0.0
    for yv in (0.0, 1.0):
        raw = rng.uniform(-3, 3, (B, n))
        bins, y = np.zeros((F, n), np.uint8), np.full(n, yv, np.float32)
        w, node = np.ones((B, n), np.float32), np.zeros((B, n), np.int32)
        feat, blo, value = np.full((B, NN), -2, np.int32), np.zeros((B, NN), np.int32), np.zeros((B, NN))
        o = ref.gbdt_apply_prep_oracle(bins, y, w, raw, node, (feat, blo, value), 0.1, 50, 48)
        d = [_d(a, dev) for a in (bins, y, w, raw, node, feat, blo, value)]
        g, h = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
        pr2 = torch.zeros(B, NN, dtype=torch.int64, device=dev)
        cr2, acc = torch.zeros_like(pr2), torch.zeros(B, dtype=torch.int64, device=dev)
        ops.ext().gbdt_apply_prep(B, n, F, NN, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                  g.data_ptr(), h.data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(),
                                  d[7].data_ptr(), pr2.data_ptr(), acc.data_ptr(), cr2.data_ptr(), 0.1,
                                  float(2 ** 50), float(2 ** 48), 0, 1.0, 0, 0, 1, ops.stream_ptr(dev))
        for got, want in ((acc, o.dev), (pr2[:, 0], np.array(o.prev_r2)[:, 0]), (cr2[:, 0], o.cur_r2)):
            got, want = got.cpu().numpy(), np.asarray(want)
            big = np.abs(want) >= 2.0 ** 48
            worst = max(worst, float((np.abs(got[big] - want[big]) / np.abs(want[big]).astype(np.float64)).max()))
    print(f"largest per-row relative discrepancy: {worst / 2.0 ** -53:.2f} u")
    assert worst <= ref.GBDT_EPS_MEASURED


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("path", ["launch", "fused", "stage"])
@pytest.mark.parametrize("F", [5, 9])
def test_stump_paths_certified(dev, monkeypatch, F, path, ties):
    """Three stages of three masked stump models through each depth-1 device path — the stage and fused
    kernels carry their own split code — replayed and certified by ``check_stumps``: stage 0 decided and
    bit-equal in feature, bin, threshold and node sums; the duplicated / mirrored columns resolve to the
    lowest index, or to sklearn's visit order on the stage path with SKLEARN_TIES on."""
    from hfens.models import hist_gbdt
    from test_gbdt_reference import assert_stump_cases, check_stumps, fit_stumps
    monkeypatch.setattr(hist_gbdt, "SKLEARN_TIES", ties)
    monkeypatch.setattr(hist_gbdt, "STUMP_PATH", path)
    monkeypatch.setattr(hist_gbdt, "FUSED_STUMPS", path == "fused")
    s = fit_stumps(F, dev, ties)
    assert hist_gbdt.LAST_PATH["path"] == path
    assert_stump_cases(s, check_stumps(s))


# ---- the edges of the boosting steps that the three depth-1 paths share (ops/csrc/gbdt.hip) ----
EDGE_ROWS = 2100          # two full 1,024-row sub-tiles and one of 52 rows
EDGE_DISTINCT = (1, 2, 3, 4, 5, 8, 9, 64, 256)
EDGE_ATTRS = ("tree_feature_", "tree_threshold_", "tree_value_", "tree_impurity_",
              "tree_weighted_n_node_samples_", "train_score_")
# variant -> (STUMP_PATH, HFENS_GBDT_MFMA, HFENS_SG_THREADS, HFENS_SG_ATOMIC_GROUPS, PERSIST)
EDGE_VARIANTS = {
    "launch": ("launch", None, None, None, "0"),
    "fused": ("fused", None, None, None, "0"),
    "stage_valu": ("stage", "0", "512", None, "0"),
    "stage_mfma": ("stage", "1", "512", None, "0"),
    "stage_mfma_1024": ("stage", "1", "1024", None, "0"),
    "stage_partials": ("stage", "1", "512", "1", "0"),
    "stage_persist_valu": ("stage", "0", "512", None, "1"),
    "stage_persist_mfma": ("stage", "1", "512", None, "1"),
}
_EDGE_DATA = []


def _edge_data():
    """Nine columns with 1, 2, 3, 4, 5, 8, 9, 64 and 256 distinct values (every value present: the last has
    bin 4*63 + 3), labels that depend on three of them, and four row masks: all rows, every third row out,
    only rows below 1,024 (two sub-tiles of zero weights), and 420 rows (below min_samples_split = 500)."""
    if not _EDGE_DATA:
        n = EDGE_ROWS
        g = torch.Generator().manual_seed(77)
        cols = [(torch.arange(n) % k)[torch.randperm(n, generator=g)].double() * 0.5 for k in EDGE_DISTINCT]
        X = torch.stack(cols, 1).contiguous()
        z = 0.9 * (X[:, 1] - 0.25) + 0.4 * (X[:, 4] - 1.0) + (X[:, 8] - 64.0) / 32.0
        y = (torch.rand(n, generator=g, dtype=torch.float64) < torch.sigmoid(z)).double()
        masks = torch.ones(4, n, dtype=torch.bool)
        masks[1, ::3] = False
        masks[2, 1024:] = False
        masks[3] = False
        masks[3, ::5] = True
        _EDGE_DATA.append((X, y, masks))
    return _EDGE_DATA[0]


def _edge_fit(dev, monkeypatch, variant, subsample):
    from hfens.models import hist_gbdt
    from hfens.models.gbdt import GradientBoostingClassifier
    path, mf, nt, atomic, persist = EDGE_VARIANTS[variant]
    monkeypatch.setattr(hist_gbdt, "STUMP_PATH", path)
    monkeypatch.setattr(hist_gbdt, "FUSED_STUMPS", path == "fused")
    monkeypatch.setattr(hist_gbdt, "PERSIST", persist)
    for name, val in (("HFENS_GBDT_MFMA", mf), ("HFENS_SG_THREADS", nt), ("HFENS_SG_ATOMIC_GROUPS", atomic)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    X, y, masks = _edge_data()
    ms = [GradientBoostingClassifier(n_estimators=4, max_depth=1, subsample=subsample, min_samples_split=500,
                                     random_state=s) for s in (2020, 7, 8, 9)]
    hist_gbdt.fit_gbdt_batch(ms, X.to(dev), y.to(dev), masks.to(dev))
    assert hist_gbdt.LAST_PATH["path"] == path
    if path == "stage":
        assert hist_gbdt.GRAPH_INFO["persist"] == (persist == "1")
    return ms


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("subsample", [1.0, 0.7])
def test_stump_paths_equal_at_step_edges(dev, monkeypatch, subsample, ties):
    """Four stages of four stump models on 2,100 rows (sub-tiles of 1,024, 1,024 and 52 rows) and nine
    columns whose bin counts sit on both sides of every threshold of the shared steps — constant, binary,
    3, 4 | 5 (small-feature scan), 8 | 9 (register / matrix-core histogram against LDS atomics), 64 and 256
    (the last lane's last bin) — with one model whose last two sub-tiles carry no weight and one whose root
    stays below min_samples_split in every stage.  Every path and every stage-kernel instantiation (VALU
    and MFMA at 512 threads, MFMA at 1,024, partial slots with the reduce launch, both persistent loops)
    gives the launch path's trees bit for bit; with sklearn's tie ranks on, which the launch and fused
    paths ignore, the stage variants agree among themselves."""
    from hfens.models import hist_gbdt
    monkeypatch.setattr(hist_gbdt, "SKLEARN_TIES", ties)
    names = [v for v in EDGE_VARIANTS if not ties or EDGE_VARIANTS[v][0] == "stage"]
    out = {v: _edge_fit(dev, monkeypatch, v, subsample) for v in names}
    base = out[names[0]]
    assert all(int(t) == -2 for t in base[3].tree_feature_[:, 0]), "model 3's roots must stay leaves"
    assert any(int(t) >= 0 for t in base[0].tree_feature_[:, 0]), "model 0 must split"
    for v in names[1:]:
        for a, b in zip(base, out[v]):
            for attr in EDGE_ATTRS:
                assert torch.equal(getattr(a, attr), getattr(b, attr)), (v, attr)
