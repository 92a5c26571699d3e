"""The GBDT training oracles of ops/reference.py (gbdt_hist_oracle, gbdt_split_oracle, gbdt_route_oracle,
gbdt_apply_prep_oracle: Python ints, Fractions and longdouble, nothing shared with models/hist_gbdt.py)
checked against sklearn's friedman_mse stump and against the host mirror ``_HostKernels`` on crafted
inputs: one kernel at a time, bit-equal where the answer is an integer, within a derived budget elsewhere.

The input builders and the ``check_*`` functions live here and are imported by
tests/test_gbdt_reference_gpu.py, which feeds the same cases to the HIP kernels.  Conditions on the
INPUTS are asserted here on the oracle alone: every split case outside the named large-magnitude
entries is decided (the exact best beats every other candidate by more than the f64 error margin), and
fewer than 1 % of the apply_prep rows sit on an f32 rounding boundary."""
import functools
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from hfens.ops import reference as ref

U = 2.0 ** -53
SENT = -7            # prefill of feat / blo / stats: an entry the kernel must leave alone keeps it
SENT_F = 12345.0     # same for thr / value


# ============================================================================ 1. histograms
HIST_NBINS = [1, 2, 3, 4, 5, 8, 9, 255, 256]
# (rows, models, nodes in the level, first node, fixed-point shift)
HIST_CASES = [(1, 1, 1, 0, 40), (255, 3, 1, 0, 40), (1024, 1, 2, 1, 40), (1025, 3, 16, 15, 40),
              (1025, 3, 1, 15, 40), (2049, 3, 1, 0, 32), (2049, 1, 16, 15, 32), (255, 1, 2, 1, 32),
              (16385, 1, 1, 0, 40), (16385, 1, 2, 1, 32)]


def _crafted_g(shift):
    """|g| whose fixed-point image is an exact half in both parities (0.5, 1.5, 2.5 → 0, 2, 2; 0.75 → 1;
    1.25 → 1), zeros of both signs and the smallest subnormal, each with both signs."""
    s = 2.0 ** (40 - shift)
    mags = [2.0 ** -41 * s, 3 * 2.0 ** -42 * s, (2.0 ** -40 + 2.0 ** -41) * s, 5 * 2.0 ** -42 * s,
            5 * 2.0 ** -41 * s, 0.0, 2.0 ** -149]
    return np.array([v for m in mags for v in (m, -m)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def hist_case(n, B, NL, node0, shift):
    rng = np.random.default_rng(1000 * n + 10 * NL + B + shift)
    F = len(HIST_NBINS)
    nbins = np.array(HIST_NBINS, dtype=np.int32)
    bins = np.stack([rng.integers(0, nb, n) for nb in HIST_NBINS]).astype(np.uint8)
    if n > 512:
        bins[8, :2] = (255, 0)
    g = rng.uniform(-1, 1, (B, n)).astype(np.float32)
    h = rng.uniform(0, 0.25, (B, n)).astype(np.float32)
    cg = _crafted_g(shift)
    k = min(n, len(cg))
    g[:, :k] = cg[:k]
    h[:, :k] = np.float32(2.0 ** -41 * 2.0 ** (40 - shift))
    neg = (bins[2] == 1) | (bins[6] == 4)          # one all-negative bin on a register and an LDS feature
    g[:, neg] = -np.abs(g[:, neg])
    w = (rng.random((B, n)) > 0.15).astype(np.float32)
    w[:, :k] = 1
    node = rng.integers(max(node0 - 1, 0), node0 + NL + 1, (B, n)).astype(np.int32)
    node[:, :k] = node0 + (np.arange(k) % NL)
    if B > 1:
        node[1] = node0 + NL                          # a model with no row in the level
    c = types.SimpleNamespace(n=n, B=B, F=F, NL=NL, node0=node0, shift=shift, nbins=nbins, bins=bins, g=g,
                              h=h, w=w, node=node)
    c.expect = ref.gbdt_hist_oracle(bins, nbins, g, h, w, node, node0, NL, shift)
    return c


class _St:
    """The attributes ``_HostKernels`` reads, set by hand."""
    wt = None
    frank = None
    subsample = 1.0
    row_off = 0

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def wcur(self):
        return self.wt if self.wt is not None else self.w


def host_hist(c):
    from hfens.models.hist_gbdt import _HostKernels
    t = torch.from_numpy
    st = _St(B=c.B, n=c.n, F=c.F, qscale=float(2 ** c.shift), g=t(c.g), h=t(c.h), w=t(c.w),
             node=t(c.node).long(), bins=t(c.bins), raw=torch.zeros(1))
    return _HostKernels.hist(st, c.node0, c.NL).numpy()


# ============================================================================ 2. splits
def _spread(rng, total, parts):
    """``parts`` non-negative ints summing to ``total``."""
    cut = np.sort(rng.integers(0, total + 1, parts - 1))
    return np.diff(np.concatenate([[0], cut, [total]])).astype(object)


def make_node(rng, nbins, shift, rows, best=None, dup=(), tg_per_row=0.0, min_cnt=1, empty=None, noise=1e-3,
              signal=0.25):
    """One node's histogram ``[F][256][3]`` of Python ints, every feature a partition of the same
    ``rows`` rows (Σw = rows·2^shift, equal Σg and Σh).  ``best`` = (f, j) plants a step in feature f
    after bin j: rows left of it carry residual −signal, right of it +signal (shifted so the mean is
    ``tg_per_row``), which makes that cut the unique maximiser by a wide margin; other features spread
    the node's Σg in proportion to their bin counts plus ``noise``.  ``dup`` = (src, dst) pairs copy a
    feature.  ``empty`` = (f, first, last) empties those bins of f into the last bin before they are
    filled."""
    unit = 1 << shift
    F = len(nbins)
    H = [[[0, 0, 0] for _ in range(256)] for _ in range(F)]
    TG = int(tg_per_row * rows * unit)
    TH = rows * (unit // 5)
    for f in range(F):
        nb = int(nbins[f])
        live = [j for j in range(nb) if not (empty and empty[0] == f and empty[1] <= j <= empty[2])]
        cnt = {j: min_cnt for j in live}
        for j, e in zip(live, _spread(rng, rows - min_cnt * len(live), len(live))):
            cnt[j] += int(e)
        if best is not None and best[0] == f:
            lw = sum(cnt[j] for j in live if j <= best[1])
            rw = rows - lw
            # left rows −s·rw/rows, right rows +s·lw/rows around the mean: sums to TG
            per = {j: (-signal * rw / rows if j <= best[1] else signal * lw / rows) for j in live}
        else:
            per = {j: 0.0 for j in live}
        gs = {j: int((per[j] + tg_per_row + noise * rng.standard_normal()) * cnt[j] * unit) for j in live}
        gs[live[-1]] += TG - sum(gs.values())
        hs = {j: cnt[j] * (unit // 5) for j in live}
        for j in live:
            H[f][j] = [gs[j], hs[j], cnt[j] * unit]
    for src, dst in dup:
        H[dst] = [list(x) for x in H[src]]
    r2 = int((signal * signal / 4 + tg_per_row ** 2 + 0.01) * rows * unit)
    return H, r2, TG, TH


def _vals(nbins):
    """lo/hi bin values: bin j of every feature spans [j, j + 0.25]."""
    F = len(nbins)
    lo = np.tile(np.arange(256, dtype=np.float64), (F, 1))
    return lo, lo + 0.25


class SplitLaunch:
    """One ``gbdt_split`` launch: ``B × NL`` nodes over shared bin tables."""

    def __init__(self, name, nbins, shift, nodes, NL=1, node0=0, NN=3, last=1, min_leaf=1, min_split=2,
                 vals=None):
        self.name, self.shift, self.NL, self.node0, self.NN, self.last = name, shift, NL, node0, NN, last
        self.nbins = np.asarray(nbins, dtype=np.int32)
        self.F = len(nbins)
        assert len(nodes) % NL == 0
        self.B = len(nodes) // NL
        self.min_leaf_q, self.min_split_q = min_leaf << shift, min_split << shift
        self.lo, self.hi = vals if vals is not None else _vals(nbins)
        self.hist = np.zeros((self.B, NL, self.F, 256, 3), dtype=np.int64)
        self.r2 = np.zeros((self.B, NN), dtype=np.int64)
        self.labels = []
        for k, (label, H, r2) in enumerate(nodes):
            b, nd = divmod(k, NL)
            self.hist[b, nd] = np.array(H, dtype=np.int64)
            self.r2[b, node0 + nd] = r2
            self.labels.append(label)

    @functools.cached_property
    def oracles(self):
        return [ref.gbdt_split_oracle(self.hist[b, nd].tolist(), self.nbins, self.lo, self.hi,
                                      int(self.r2[b, self.node0 + nd]), self.shift, self.min_leaf_q,
                                      self.min_split_q)
                for b in range(self.B) for nd in range(self.NL)]

    def blank(self):
        B, NN = self.B, self.NN
        return dict(feat=np.full((B, NN), SENT, np.int32), blo=np.full((B, NN), SENT, np.int32),
                    thr=np.full((B, NN), SENT_F), value=np.full((B, NN), SENT_F),
                    stats=np.full((B, NN, 4), SENT, np.int64))


def _launch_scan():
    """(a) scan geometry: every (bin count, best bin) at the lane and wave-shuffle boundaries."""
    nbins = [2, 3, 4, 5, 64, 255, 256]
    rng = np.random.default_rng(11)
    nodes = []
    for f, nb in enumerate(nbins):
        for j in sorted({0, 3, 4, 63, 127, 253, nb - 2}):
            if j < nb - 1:
                H, r2, _, _ = make_node(rng, nbins, 40, 4000, best=(f, j))
                nodes.append((f"nb{nb}@{j}", H, r2))
    return SplitLaunch("scan", nbins, 40, nodes)


def _launch_wave(F):
    """(b) wave geometry: the best feature at the wave-stride positions, and duplicated columns in the
    same wave (1, 5) and in different waves (2, 7), (6, 3) — the lower index must win."""
    nbins = [12] * F
    rng = np.random.default_rng(20 + F)
    nodes = []
    for f in sorted({0, 3, 4, F - 1}):
        if f < F:
            H, r2, _, _ = make_node(rng, nbins, 40, 900, best=(f, int(rng.integers(0, 11))))
            nodes.append((f"F{F}best{f}", H, r2))
    for lo_f, hi_f in ((1, 5), (2, 7), (3, 6)):
        if hi_f < F:
            for src, dst in ((lo_f, hi_f), (hi_f, lo_f)):
                H, r2, _, _ = make_node(rng, nbins, 40, 900, best=(src, 5), dup=[(src, dst)])
                nodes.append((f"F{F}dup{src}->{dst}", H, r2))
    for src, dst in ((1, 4), (6, 2)):                                # x → −x: the cut's sides swap
        if max(src, dst) < F:
            for cut in (2, 5, 8):
                H, r2, _, _ = make_node(rng, nbins, 40, 900, best=(src, cut))
                H[dst] = [list(x) for x in H[src][11::-1]] + H[dst][12:]
                nodes.append((f"F{F}mirror{src}->{dst}@{cut}", H, r2))
    if F > 8:                                                        # a three-way tie over three waves
        H, r2, _, _ = make_node(rng, nbins, 40, 900, best=(8, 2), dup=[(8, 6), (8, 3)])
        nodes.append((f"F{F}dup8->6,3", H, r2))
    return SplitLaunch(f"wave{F}", nbins, 40, nodes)


def _launch_minleaf():
    """(c) min_samples_leaf = 5, min_samples_split = 20: the planted cut leaves 4 / 5 rows on either
    side, or exactly one fixed-point unit less than 5 rows; the node weighs one unit less than 20 rows,
    or exactly 20; one node has Σh = 0."""
    nbins = [6, 9, 3]
    shift, unit = 40, 1 << 40
    rng = np.random.default_rng(31)
    nodes = []

    def planted(side, cnt, minus_one):
        # feature 1, cut after bin 0 (left) or bin 7 (right): that side holds exactly ``cnt`` rows
        while True:
            H, r2, _, _ = make_node(rng, nbins, shift, 60, best=(1, 0 if side == "l" else 7), min_cnt=cnt)
            lone = H[1][0] if side == "l" else H[1][8]
            if lone[2] == cnt * unit:
                break
        if minus_one:
            other = H[1][1] if side == "l" else H[1][7]
            lone[2] -= 1
            other[2] += 1
        return H, r2

    for side in "lr":
        for cnt, m1 in ((4, False), (5, False), (5, True), (6, False)):
            H, r2 = planted(side, cnt, m1)
            nodes.append((f"leaf_{side}{cnt}{'-1q' if m1 else ''}", H, r2))
    for rows, m1 in ((20, True), (20, False), (19, False)):
        H, r2, _, _ = make_node(rng, nbins, shift, rows, best=(0, 2), min_cnt=1)
        if m1:
            for f in range(3):
                H[f][0][2] -= 1
        nodes.append((f"split_{rows}{'-1q' if m1 else ''}", H, r2))
    H, r2, _, _ = make_node(rng, nbins, shift, 19, best=(0, 2))
    for f in range(3):
        for j in range(256):
            H[f][j][1] = 0
    nodes.append(("split_19_h0", H, r2))
    H, r2, _, _ = make_node(rng, nbins, shift, 60, best=(0, 2), min_cnt=5, tg_per_row=0.1)
    nodes.append(("pure", H, 0))                      # Σw r² = 0: impurity −mean² < 0, a leaf
    H, r2, _, _ = make_node(rng, nbins, shift, 1 << 16, best=(0, 2), min_cnt=5, signal=0.0, noise=0.0)
    nodes.append(("eps_below", H, 1))                 # impurity 2^-56 = eps / 16 with candidates: a leaf
    H, r2, _, _ = make_node(rng, nbins, shift, 60, min_cnt=2, signal=0.0, noise=0.0)
    nodes.append(("flat", H, 60 * unit // 4))         # every gain an exact 0: lowest feature, lowest bin
    nodes.append(("empty", [[[0, 0, 0] for _ in range(256)] for _ in range(3)], 0))
    return SplitLaunch("minleaf", nbins, shift, nodes, min_leaf=5, min_split=20)


def _launch_gaps():
    """(d) runs of empty bins after the chosen cut (1, 5, up to nb − 2 bins) and (e) thresholds between
    adjacent doubles, next to the largest doubles and below an infinite bin value."""
    nbins = [4, 64, 256, 9]
    rng = np.random.default_rng(41)
    lo, hi = _vals(nbins)
    x = 1.0 + 2.0 ** -30
    hi[3, 0], lo[3, 1] = x, np.nextafter(x, 2)                    # midpoint rounds to one of the two
    hi[3, 1], lo[3, 2] = np.nextafter(x, 2), np.nextafter(np.nextafter(x, 2), 2)
    hi[3, 2], lo[3, 3] = 1.7e308, 1.75e308
    hi[3, 3], lo[3, 4] = -1.7e308, 1.7e308
    hi[3, 4], lo[3, 5] = 1.7e308, np.inf
    hi[3, 5], lo[3, 6] = -np.inf, 5.0
    nodes = []
    for f, j, last in ((1, 10, 11), (1, 10, 15), (1, 0, 62), (1, 30, 62), (2, 3, 254), (2, 127, 132),
                       (2, 252, 254), (0, 0, 2), (0, 1, 2)):
        H, r2, _, _ = make_node(rng, nbins, 40, 3000, best=(f, j), empty=(f, j + 1, last))
        nodes.append((f"gap_f{f}_{j}+{last - j}", H, r2))
    for j in range(6):
        H, r2, _, _ = make_node(rng, nbins, 40, 3000, best=(3, j))
        nodes.append((f"thr_{j}", H, r2))
    return SplitLaunch("gaps", nbins, 40, nodes, vals=(lo, hi))


def _launch_magnitudes(shift):
    """(f) Σw up to 2^62: 2^22 rows at shift 40, 2^29 at shift 32; Σg ≈ 0 (late boosting) and Σg far
    from 0 (a deep node: the two products of the gain nearly cancel, κ is large)."""
    nbins = [8, 64, 256, 2]
    rng = np.random.default_rng(50 + shift)
    top = 22 if shift == 40 else 29
    nodes = []
    for lg_rows in (10, 15, top):
        for name, tgr, sig in (("tg0", 0.0, 0.25), ("mid", 0.05, 0.25), ("deep", 0.45, 0.02)):
            H, r2, _, _ = make_node(rng, nbins, shift, 1 << lg_rows, best=(int(rng.integers(0, 3)), 5),
                                    tg_per_row=tgr, signal=sig, noise=1e-3 if lg_rows < top else 1e-4)
            nodes.append((f"s{shift}_2^{lg_rows}_{name}", H, r2))
    return SplitLaunch(f"magnitude{shift}", nbins, shift, nodes)


def _launch_levels(node0, NL, last):
    """(g) heap placement: NN = 63, the level's nodes write themselves and children 2k+1, 2k+2."""
    nbins = [5, 17, 3]
    rng = np.random.default_rng(60 + node0 + last)
    nodes = []
    for k in range(2 * NL):
        H, r2, _, _ = make_node(rng, nbins, 40, 500, best=(k % 3, k % 2))
        if k == 1:
            for j in range(256):
                H[k % 3][j][1] *= int(j > k % 2)      # left child Σh = 0: Newton value 0
            tot = sum(H[k % 3][j][1] for j in range(256))
            for f in range(3):
                if f != k % 3:
                    for j in range(256):
                        H[f][j][1] = 0
                    H[f][0][1] = tot
        nodes.append((f"lvl{node0}_{k}", H, r2))
    if NL > 1:
        nodes[NL + 1] = ("empty", [[[0, 0, 0] for _ in range(256)] for _ in range(3)], 0)
    return SplitLaunch(f"level{node0}_{last}", nbins, 40, nodes, NL=NL, node0=node0, NN=63, last=last)


def _launch_random():
    """(h) 200 random histograms in one launch; draws the oracle does not decide are redrawn."""
    nbins = [2, 7, 33, 256, 4, 100]
    rng = np.random.default_rng(71)
    lo, hi = _vals(nbins)
    nodes = []
    while len(nodes) < 200:
        f = int(rng.integers(0, 6))
        j = int(rng.integers(0, nbins[f] - 1))
        rows = int(rng.integers(600, 5000))
        H, r2, _, _ = make_node(rng, nbins, 40, rows, best=(f, j), tg_per_row=float(rng.uniform(-0.3, 0.3)),
                                signal=float(rng.uniform(0.02, 0.3)), noise=0.02,
                                min_cnt=int(rng.integers(0, 2)))
        o = ref.gbdt_split_oracle(H, nbins, lo, hi, r2, 40, 3 << 40, 2 << 40)
        if o.kind == "split" and o.decided:
            nodes.append((f"rnd{len(nodes)}", H, r2))
    return SplitLaunch("random", nbins, 40, nodes, min_leaf=3)


@functools.lru_cache(maxsize=None)
def split_launches():
    out = [_launch_scan()] + [_launch_wave(F) for F in (1, 4, 5, 9, 128)]
    out += [_launch_minleaf(), _launch_gaps(), _launch_magnitudes(40), _launch_magnitudes(32)]
    out += [_launch_levels(n0, NL, last) for n0, NL in ((0, 1), (1, 2), (15, 16)) for last in (0, 1)]
    return out + [_launch_random()]


def _close(got, want: Fraction, rel):
    if want == 0:
        return got == 0.0
    return abs(Fraction(float(got)) - want) <= rel * abs(want)


def check_split(L: SplitLaunch, out):
    """Every output of one launch against the oracle.  ``out``: feat, blo, thr, value, stats as numpy
    arrays that started as ``L.blank()``.  Returns the number of undecided nodes."""
    exp = L.blank()
    undecided = 0
    for k, o in enumerate(L.oracles):
        b, nd = divmod(k, L.NL)
        hn = L.node0 + nd
        tag = f"{L.name}/{L.labels[k]}"
        if o.kind == "empty":
            exp["feat"][b, hn] = -3
            continue
        exp["stats"][b, hn, :3] = (o.tw, o.tg, o.th)
        if o.kind == "leaf":
            exp["feat"][b, hn], exp["blo"][b, hn], exp["thr"][b, hn] = -2, 0, -2.0
            want = Fraction(0) if o.th == 0 else Fraction(o.tg, o.th)
            assert _close(out["value"][b, hn], want, 4 * U), (tag, "leaf value")
            exp["value"][b, hn] = out["value"][b, hn]
            assert out["feat"][b, hn] == -2, (tag, "a leaf", int(out["feat"][b, hn]))
            continue
        f, j = int(out["feat"][b, hn]), int(out["blo"][b, hn])
        assert f >= 0, (tag, "must split", f)
        why = o.certify(f, j)
        assert why is None, (tag, why)
        undecided += not o.decided
        (lw, lg, lh), (rw, rg, rh), thr = ref.gbdt_split_children(o, f, j)
        exp["feat"][b, hn], exp["blo"][b, hn], exp["thr"][b, hn] = f, j, thr
        assert _close(out["value"][b, hn], Fraction(o.tg, o.tw), 4 * U), (tag, "node value")
        exp["value"][b, hn] = out["value"][b, hn]
        for c, (cw, cg, ch) in ((2 * hn + 1, (lw, lg, lh)), (2 * hn + 2, (rw, rg, rh))):
            exp["stats"][b, c, :3] = (cw, cg, ch)
            if L.last:
                exp["feat"][b, c], exp["blo"][b, c], exp["thr"][b, c] = -2, 0, -2.0
                want = Fraction(0) if ch == 0 else Fraction(cg, ch)
                assert _close(out["value"][b, c], want, 4 * U), (tag, "child value", c)
                exp["value"][b, c] = out["value"][b, c]
    for key in ("feat", "blo", "stats", "value"):
        bad = np.argwhere(out[key] != exp[key])
        assert bad.size == 0, (L.name, key, bad[:4].tolist())
    same = out["thr"].view(np.int64) == exp["thr"].view(np.int64)       # bit-equal, −0.0 and inf included
    assert same.all(), (L.name, "thr", np.argwhere(~same)[:4].tolist())
    return undecided


def host_split(L: SplitLaunch):
    from hfens.models.hist_gbdt import _HostKernels
    t = torch.from_numpy
    o = {k: t(v)[None].clone() for k, v in L.blank().items()}
    bm = types.SimpleNamespace(nbins=t(L.nbins), lo_val=t(L.lo), hi_val=t(L.hi))
    st = _St(B=L.B, F=L.F, qscale=float(2 ** L.shift), min_leaf_q=float(L.min_leaf_q),
             min_split_q=float(L.min_split_q), bm=bm, r2=t(L.r2)[None], **o)
    _HostKernels.split(st, t(L.hist), L.node0, L.NL, bool(L.last), 0)
    return {k: v[0].numpy() for k, v in o.items()}


# ============================================================================ 3. route and apply_prep
def _tables(rng, B, NN, F, leaf_level_only=True):
    """Hand-made tree tables: internal nodes split a random feature at a low bin; a few nodes of every
    level are leaves (feat −2) or unreachable (−3); one leaf value is exactly 0."""
    feat = rng.integers(0, F, (B, NN)).astype(np.int32)
    blo = rng.integers(0, 3, (B, NN)).astype(np.int32)
    value = rng.uniform(-2, 2, (B, NN))
    kill = rng.random((B, NN)) < 0.2
    feat[kill] = np.where(rng.random(kill.sum()) < 0.5, -2, -3)
    first_leaf = NN // 2
    feat[:, first_leaf:] = -2
    if NN >= 63:
        feat[:, 30] = 1                                # rows of node 30 reach children 61 and 62
    value[:, NN - 1] = 0.0
    return feat, blo, value


ROUTE_CASES = [(1, 3, 0, 1), (257, 15, 1, 2), (1024, 63, 15, 16), (1024, 63, 3, 4), (262145, 63, 15, 16)]


@functools.lru_cache(maxsize=None)
def route_case(n, NN, node0, NL):
    rng = np.random.default_rng(n + NN)
    B, F = (1, 3) if n > 100000 else (2, 5)
    bins = rng.integers(0, 4, (F, n)).astype(np.uint8)
    feat, blo, _ = _tables(rng, B, NN, F)
    if NN >= 63 and node0 == 15:
        feat[:, 15:31] = rng.integers(0, F, (B, 16))
        feat[:, 17] = -2
    node = rng.integers(max(node0 - 2, 0), min(node0 + NL + 2, NN // 2 + 1), (B, n)).astype(np.int32)
    g = rng.uniform(-1, 1, (B, n)).astype(np.float32)
    w = (rng.random((B, n)) > 0.2).astype(np.float32)
    g *= w
    shift = 40
    c = types.SimpleNamespace(n=n, B=B, F=F, NN=NN, node0=node0, NL=NL, bins=bins, feat=feat, blo=blo, node=node,
                              g=g, w=w, shift=shift)
    c.new, moved = ref.gbdt_route_oracle(bins, node, feat, blo, node0, NL)
    c.r2 = np.array(ref.gbdt_route_r2_oracle(g, w, c.new, moved, NN, shift), dtype=np.int64)
    c.r2_start = rng.integers(0, 1000, (B, NN)).astype(np.int64)      # the kernel adds to what is there
    return c


def check_route(c, node, r2):
    assert np.array_equal(np.asarray(node, dtype=np.int64), c.new), "routing"
    assert np.array_equal(r2, c.r2_start + c.r2), "child sums of w·r²"


def host_route(c):
    from hfens.models.hist_gbdt import _HostKernels
    t = torch.from_numpy
    st = _St(n=c.n, qscale=float(2 ** c.shift), bins=t(c.bins), g=t(c.g), w=t(c.w), node=t(c.node).long(),
             feat=t(c.feat).long()[None], blo=t(c.blo).long()[None], r2=t(c.r2_start.copy())[None],
             raw=torch.zeros(c.B, c.n, dtype=torch.float64))
    _HostKernels.route(st, c.node0, c.NL, 0)
    return st.node.numpy(), st.r2[0].numpy()


RAW_EDGES = [0.0, 1e-8, 20.0, 36.7, 40.0, 700.0]
# (rows, heap nodes, subsample, global row offset, stage); stage 0 has no previous tree
PREP_CASES = [(1, 3, 1.0, 0, 1), (257, 15, 1.0, 0, 1), (1024, 63, 1.0, 0, 1), (1024, 3, 1.0, 0, 0),
              (1024, 63, 0.5, 0, 1), (1024, 15, 0.7, (1 << 33) + 5, 99), (257, 3, 0.7, (1 << 33) + 5, 0),
              (262145, 63, 0.5, (1 << 33) + 5, 1), (262145, 15, 0.7, 0, 99)]
PREP_SEEDS = [0xD1B54A32D192ED03, 0x9E3779B97F4A7C15 ^ 0xFFFF, 12345]


@functools.lru_cache(maxsize=None)
def prep_case(n, NN, subsample, row_off, stage):
    rng = np.random.default_rng(n + NN + stage)
    B, F = (1, 3) if n > 100000 else (2, 5)
    lr, shift = 0.1, 40
    bins = rng.integers(0, 4, (F, n)).astype(np.uint8)
    feat, blo, value = _tables(rng, B, NN, F)
    last0 = NN // 4                                     # first node of the tree's last split level
    node = rng.integers(last0, NN // 2, (B, n)).astype(np.int32) if NN > 3 else np.zeros((B, n), np.int32)
    if NN > 3:
        feat[:, last0:NN // 2][feat[:, last0:NN // 2] == -3] = -2
    else:
        feat[:, 0] = 0
    y = (rng.random(n) < 0.4).astype(np.float32)
    w = (rng.random((B, n)) > 0.2).astype(np.float32)
    raw = rng.normal(0, 2, (B, n))
    edges = np.array([s * v for v in RAW_EDGES for s in (1, -1)])
    # every edge with both labels from 4096 rows on; below, one label each (alternating by magnitude), and
    # below 1024 rows no edge beyond ±20: the saturated rows, whose tiny g and h no f64 expression can
    # decide, stay under 1 % of the rows in EVERY case
    if n < 1024:
        edges = edges[:6]
    k = min(n, 2 * len(edges) if n >= 4096 else len(edges))
    raw[:, :k] = np.tile(edges, 2)[:k]
    y[:k] = ((np.arange(k) >= len(edges)) ^ (np.arange(k) // 2 % 2 == 1)).astype(np.float32)
    w[:, :k] = 1
    prev = (feat, blo, value) if stage > 0 else None
    if prev is not None:
        # raw + lr·value within 2u needs |result| ≥ |lr·value| (no cancellation): mirror the raws that fail
        leaf, _ = ref.gbdt_route_oracle(bins, node, feat, blo, 0, NN)
        step = lr * np.take_along_axis(value, leaf, 1)
        bad = np.abs(raw + step) < np.abs(step)
        raw[bad] = -raw[bad]
        bad = np.abs(raw + step) < np.abs(step)
        raw[bad] += 2 * step[bad]
    seeds = np.array(PREP_SEEDS[:B], dtype=np.uint64)
    c = types.SimpleNamespace(n=n, B=B, F=F, NN=NN, lr=lr, shift=shift, bins=bins, feat=feat, blo=blo,
                              value=value, node=node, y=y, w=w, raw=raw, subsample=subsample, row_off=row_off,
                              stage=stage, seeds=seeds, prev=prev)
    c.o = ref.gbdt_apply_prep_oracle(bins, y, w, raw, node, prev, lr, shift, 26, subsample,
                                     [int(s) for s in seeds], row_off, stage)
    c.start = rng.integers(0, 1000, (3, B, NN)).astype(np.int64)     # prev_r2, cur_r2, dev[.., 0] before
    return c


def check_prep(c, out):
    """``out``: raw, g, h, node, wt (None without bagging), prev_r2 [B, NN], cur_r2 [B, NN], dev [B] after
    the call, started from ``c.start``.  Prints the largest deviations in units of their budgets."""
    o = c.o
    ld = np.longdouble
    assert not np.asarray(out["node"]).any(), "every row back at the root"
    if c.subsample < 1.0:
        assert np.array_equal(out["wt"].view(np.int32), o.wt.view(np.int32)), "in-bag weights"
    rawd = np.abs(out["raw"].astype(ld) - o.raw)
    if c.prev is not None:
        assert (np.abs(o.raw) >= np.abs(o.step)).all(), "input condition: no cancellation in raw + lr·value"
        assert (rawd <= 2 * ld(U) * np.abs(o.raw)).all(), ("raw", float((rawd / np.abs(o.raw).clip(1e-300)).max() / U))
    else:
        assert not rawd.any(), "stage 0 leaves raw alone"
    for name in ("g", "h"):
        got, want = out[name], getattr(o, name + "32")
        und = getattr(o, name + "_und")
        err = np.abs(got.astype(ld) - getattr(o, name))
        assert (err <= getattr(o, name + "_tol")).all(), (name, "beyond one f32 ulp")
        bits = got.view(np.int32) == want.view(np.int32)
        bits |= (got == 0) & (want == 0)                             # ±0: w·r with w = 0
        assert (bits | und).all(), (name, "decided rows differ", int((~(bits | und)).sum()))
    ratios = {}
    for name, got, start, want, bud in (
            ("cur_r2", out["cur_r2"][:, 0], c.start[1][:, 0], o.cur_r2, o.cur_r2_budget),) + ((
            ("prev_r2", out["prev_r2"], c.start[0], o.prev_r2, o.prev_r2_budget),
            ("dev", out["dev"], c.start[2][:, 0], o.dev, o.dev_budget)) if c.prev is not None else ()):
        diff = np.abs((np.asarray(got) - start).astype(np.float64) - np.array(want, dtype=np.float64))
        bud = np.array(bud)
        assert (diff <= bud).all(), (name, diff.max(), bud.max())
        ratios[name] = float((diff / bud.clip(1)).max())
    if c.prev is None:
        assert np.array_equal(out["prev_r2"], c.start[0]) and np.array_equal(out["dev"], c.start[2][:, 0])
    assert np.array_equal(out["cur_r2"][:, 1:], c.start[1][:, 1:]), "only the root slot of cur_r2"
    print(f"prep n={c.n} NN={c.NN} sub={c.subsample} t={c.stage}: sum deviation / budget {ratios}")


def host_prep(c):
    from hfens.models.hist_gbdt import _HostKernels
    t = torch.from_numpy
    T = c.stage + 1
    r2 = torch.zeros(T, c.B, c.NN, dtype=torch.int64)
    dev = torch.zeros(T, c.B, dtype=torch.int64)
    r2[c.stage] = t(c.start[1])
    if c.stage > 0:
        r2[c.stage - 1] = t(c.start[0])
        dev[c.stage - 1] = t(c.start[2][:, 0])
    st = _St(n=c.n, T=T, lr=c.lr, qscale=float(2 ** c.shift), dscale=float(2 ** 26), bins=t(c.bins),
             y=t(c.y), w=t(c.w), raw=t(c.raw.copy()), node=t(c.node).long(), r2=r2, dev=dev,
             subsample=c.subsample, row_off=c.row_off, seeds=t(c.seeds.view(np.int64)),
             bagw=torch.zeros(T, c.B, dtype=torch.float64))
    prev = None if c.prev is None else tuple(t(a).long() if a.dtype != np.float64 else t(a) for a in c.prev)
    _HostKernels.apply_prep(st, prev, c.stage)
    z = torch.zeros(c.B, c.NN, dtype=torch.int64)
    return dict(raw=st.raw.numpy(), g=st.g.numpy(), h=st.h.numpy(), node=st.node.numpy(),
                wt=None if st.wt is None else st.wt.to(torch.float32).numpy(), cur_r2=r2[c.stage].numpy(),
                prev_r2=(r2[c.stage - 1] if c.stage > 0 else t(c.start[0])).numpy(),
                dev=(dev[c.stage - 1] if c.stage > 0 else t(c.start[2][:, 0])).numpy())


# ============================================================================ the CPU tests
@pytest.mark.parametrize("case", HIST_CASES, ids=str)
def test_hist_mirror_matches_oracle(case):
    c = hist_case(*case)
    assert np.array_equal(host_hist(c), c.expect)
    assert c.expect[..., 2].any() or c.n == 1


def test_hist_crafted_values_round_half_even():
    q = [ref.gbdt_q(v, 40) for v in _crafted_g(40)]
    assert q == [0, 0, 1, -1, 2, -2, 1, -1, 2, -2, 0, 0, 0, 0]
    assert [ref.gbdt_q(v, 32) for v in _crafted_g(32)] == q
    c = hist_case(2049, 3, 1, 0, 32)
    assert (c.expect[0, 0, 2, 1, 0] < 0) and (c.expect[0, 0, 6, 4, 0] < 0)     # the all-negative bins


@pytest.mark.parametrize("idx", range(17))
def test_split_mirror_matches_oracle(idx):
    L = split_launches()[idx]
    undecided = check_split(L, host_split(L))
    und = [lab for lab, o in zip(L.labels, L.oracles) if o.kind == "split" and not o.decided]
    print(f"{L.name}: {len(L.oracles)} nodes, undecided {und}")
    assert not und and undecided == 0


def test_split_cases_reach_what_they_name():
    by = {L.name: L for L in split_launches()}
    assert len(split_launches()) == 17
    kinds = dict(zip(by["minleaf"].labels, by["minleaf"].oracles))
    for side, cut in (("l", 0), ("r", 7)):
        assert kinds[f"leaf_{side}4"].best != (1, cut) and (1, cut) not in kinds[f"leaf_{side}4"].cands
        assert (1, cut) not in kinds[f"leaf_{side}5-1q"].cands
        assert kinds[f"leaf_{side}5"].best == (1, cut) and kinds[f"leaf_{side}6"].best == (1, cut)
    assert kinds["split_20-1q"].kind == "leaf" and not kinds["split_20-1q"].cands
    assert kinds["split_20"].kind == "split"
    assert kinds["split_19_h0"].kind == "leaf" and kinds["split_19_h0"].th == 0
    assert kinds["pure"].kind == "leaf" and kinds["pure"].cands and kinds["pure"].imp < -1e-6
    assert kinds["eps_below"].kind == "leaf" and 0 < kinds["eps_below"].imp < Fraction(ref.GBDT_LEAF_EPS) / 10
    assert kinds["eps_below"].cands
    assert kinds["empty"].kind == "empty"
    flat = kinds["flat"]
    assert flat.kind == "split" and flat.decided and len(flat.cands) > 6 and flat.best == min(flat.cands)
    assert all(g == 0 for g, _ in flat.cands.values())
    for L in split_launches():
        for lab, o in zip(L.labels, L.oracles):
            if o.kind == "split" and lab not in ("pure",):
                assert o.imp > 100 * Fraction(ref.GBDT_LEAF_EPS), (L.name, lab)
    # every planted best is the oracle's best; duplicated columns resolve to the lower index
    for lab, o in zip(by["wave9"].labels, by["wave9"].oracles):
        if "dup" in lab:
            src, dst = int(lab.split("dup")[1].split("->")[0]), int(lab.split("->")[1].split(",")[0])
            assert o.best[0] == min(src, dst, 3 if "," in lab else 99), lab
        if "mirror" in lab:
            src, dst = int(lab.split("mirror")[1].split("->")[0]), int(lab.split("->")[1].split("@")[0])
            cut = int(lab.split("@")[1])
            assert o.decided and o.key[(src, cut)] == o.key[(dst, 10 - cut)]
            assert o.best == min((src, cut), (dst, 10 - cut)), lab
    gaps = dict(zip(by["gaps"].labels, by["gaps"].oracles))
    t = {j: ref.gbdt_split_children(gaps[f"thr_{j}"], 3, j)[2] for j in range(6)}
    lo, hi = by["gaps"].lo, by["gaps"].hi
    assert {t[0] == hi[3, 0], t[1] == hi[3, 1]} == {True}            # both adjacent pairs fall back to a
    assert t[2] == 1.7e308 / 2 + 1.75e308 / 2 and t[3] == 0.0 and t[4] == 1.7e308 and t[5] == -np.inf
    kappa_big = [o for o in by["magnitude40"].oracles if o.kind == "split" and o.cands[o.best][1] > 100 * U]
    assert kappa_big, "a large-κ best candidate"


@pytest.mark.parametrize("case", ROUTE_CASES, ids=str)
def test_route_mirror_matches_oracle(case):
    c = route_case(*case)
    check_route(c, *host_route(c))
    assert (c.new != c.node).any() or c.n == 1
    if c.NN == 63 and c.node0 == 15:
        assert (c.new == 62).any() and c.r2[:, 62].all()


@pytest.mark.parametrize("case", PREP_CASES, ids=str)
def test_prep_mirror_matches_oracle(case, capsys):
    c = prep_case(*case)
    und = max(c.o.g_und.mean(), c.o.h_und.mean())
    assert und < 0.01, f"{und:.3%} of the rows sit on an f32 rounding boundary"
    check_prep(c, host_prep(c))
    if c.subsample < 1.0 and c.n > 100000:
        share = float((c.o.wt[0] > 0).sum() / (c.w[0] > 0).sum())
        sigma = (c.subsample * (1 - c.subsample) / (c.w[0] > 0).sum()) ** 0.5
        assert abs(share - c.subsample) < 5 * sigma, (share, sigma)


def test_bag_oracle_equals_bag_mask():
    from hfens.models.hist_gbdt import bag_mask
    gidx = torch.arange(10000) + (1 << 33) + 5
    seeds = torch.from_numpy(np.array(PREP_SEEDS, dtype=np.uint64).view(np.int64))
    for stage in (0, 1, 99):
        got = bag_mask(seeds, stage, gidx, 0.7).numpy()
        want = np.array([[ref.gbdt_bag_oracle(s, stage, int(i), 0.7) for i in gidx] for s in PREP_SEEDS])
        assert np.array_equal(got, want), stage


@pytest.mark.parametrize("min_leaf", [1, 5])
def test_split_oracle_equals_sklearn_stump(min_leaf):
    """30 small problems with integer targets and a planted winner: the oracle's cut gives sklearn's
    friedman_mse row partition, threshold and child means."""
    from sklearn.tree import DecisionTreeRegressor
    rng = np.random.default_rng(5 + min_leaf)
    for trial in range(30):
        n, F = int(rng.integers(40, 120)), 4
        X = rng.integers(0, 9, (n, F)).astype(np.float64)
        fb, cut = int(rng.integers(0, F)), int(rng.integers(2, 6))
        yv = np.where(X[:, fb] <= cut, -8, 8) + rng.integers(-2, 3, n)
        shift = 40
        vals = [np.unique(X[:, f]) for f in range(F)]
        nbins = [len(v) for v in vals]
        H = [[[0, 0, 0] for _ in range(256)] for _ in range(F)]
        lo, hi = np.zeros((F, 256)), np.zeros((F, 256))
        for f in range(F):
            lo[f, :nbins[f]] = hi[f, :nbins[f]] = vals[f]
            for i in range(n):
                j = int(np.searchsorted(vals[f], X[i, f]))
                H[f][j][0] += int(yv[i]) << shift
                H[f][j][1] += 1 << shift
                H[f][j][2] += 1 << shift
        r2 = int((yv.astype(object) ** 2).sum()) << shift
        o = ref.gbdt_split_oracle(H, nbins, lo, hi, r2, shift, min_leaf << shift, 2 << shift)
        assert o.kind == "split" and o.decided, trial
        (lw, lg, _), (rw, rg, _), thr = ref.gbdt_split_children(o, *o.best)
        tr = DecisionTreeRegressor(criterion="friedman_mse", max_depth=1, min_samples_leaf=min_leaf).fit(X, yv)
        t_ = tr.tree_
        assert t_.feature[0] == o.best[0] and t_.threshold[0] == thr, trial
        assert np.array_equal(X[:, o.best[0]] <= thr, X[:, t_.feature[0]] <= t_.threshold[0])
        assert abs(t_.value[1, 0, 0] - lg / lw) < 1e-12 and abs(t_.value[2, 0, 0] - rg / rw) < 1e-12
        assert (t_.n_node_samples[1], t_.n_node_samples[2]) == (lw >> shift, rw >> shift)


# ============================================================================ 4. three-stage stump fits
STUMP_MIN_LEAF = 5
STUMP_T = 3


@functools.lru_cache(maxsize=None)
def stump_data(F):
    """600 rows, three fold masks.  F = 5: the informative column 1, its duplicate 3 and its mirror 4
    (x → −x) tie exactly.  F = 9 adds a constant column 5, column 6 whose only cut leaves exactly
    ``STUMP_MIN_LEAF`` rows (fewer under the masks that drop one of them), and the strongest column 7,
    whose values 3..6 occur only on rows that model 1 does not see: a run of four empty bins after its cut."""
    rng = np.random.default_rng(90 + F)
    n = 600
    X = np.zeros((n, F))
    base = rng.integers(0, 6, n).astype(np.float64)
    X[:, 0] = rng.integers(0, 40, n)
    X[:, 1] = base
    X[:, 2] = rng.integers(0, 3, n)
    X[:, 3] = base
    X[:, 4] = -base
    prob = 0.1 + 0.12 * base
    if F == 9:
        X[:, 5] = 1.0
        X[[0, 1, 2, 3, 5], 6] = 1.0                     # rows 0, 3 leave model 0's mask, row 1 model 1's
        fold1 = np.arange(n) % 3 == 1
        X[:, 7] = np.where(fold1, rng.integers(3, 7, n), rng.choice([0, 1, 2, 7, 8, 9], n))
        X[:, 8] = rng.integers(0, 200, n)
        prob = 0.1 + 0.05 * base + 0.5 * (X[:, 7] >= 7) + 0.25 * (X[:, 7] >= 5) * (X[:, 7] < 7)
    y = (rng.random(n) < prob).astype(np.float64)
    masks = np.ones((3, n), dtype=bool)
    for b in range(3):
        masks[b, b::3] = False
    return X, y, masks


def fit_stumps(F, device, ties):
    """``fit_gbdt_batch`` of three 3-stage stump models on ``stump_data(F)``; returns what
    ``check_stumps`` reads, as numpy.  The caller has set the path switches."""
    from hfens.models import hist_gbdt
    from hfens.models.gbdt import GradientBoostingClassifier
    X, y, masks = stump_data(F)
    ms = [GradientBoostingClassifier(n_estimators=STUMP_T, max_depth=1, min_samples_leaf=STUMP_MIN_LEAF,
                                     random_state=s) for s in range(3)]
    out = {}
    t = torch.from_numpy
    hist_gbdt.fit_gbdt_batch(ms, t(X).to(device), t(y).to(device), t(masks).to(device), state_out=out)
    st = out["st"]
    n_ = lambda a: a.detach().cpu().numpy()   # noqa: E731
    rank = None
    if ties and hist_gbdt.LAST_PATH["path"] in ("stage", None):
        # the launch and fused kernels break ties by the lowest index whatever the switch says
        rank = n_(hist_gbdt.sklearn_stump_ranks(ms, st.bins.cpu(), t(masks), STUMP_T))
    return dict(F=F, rank=rank, bins=n_(st.bins), nbins=n_(st.bm.nbins), lo=n_(st.bm.lo_val), hi=n_(st.bm.hi_val),
                raw0=n_(out["raw0"]), lr=out["lr"], feat=n_(st.feat), blo=n_(st.blo), thr=n_(st.thr),
                value=n_(st.value), stats=n_(st.stats), r2=n_(st.r2), dev=n_(st.dev),
                train_score=[n_(m.train_score_) for m in ms])


def check_stumps(s):
    """Replays each stage in longdouble from the fit's OWN tables of the stages before it, rebuilds the
    root histogram in Python ints and certifies the recorded stump.

    The rebuilt histogram is exact — not merely within a budget — when no in-model row's g or h lies
    within 2^-44 of an f32 rounding boundary: the replayed raw differs from the f64 one by at most
    3 stages × 2u·|raw| < 2^-49, σ' ≤ ¼, and y − p adds 4u.  That condition is asserted on the replayed
    numbers; with it Σw, Σg, Σh of the root and both leaves, the threshold and (in a decided case) the
    cut are bit-equal, leaf values are within 4u of the exact quotient and the training deviance within
    its fixed-point budget.  Returns the cuts [T][B]."""
    X, y, masks = stump_data(s["F"])
    ld = np.longdouble
    shift, unit = 40, 1 << 40
    n = len(y)
    cuts = [[None] * 3 for _ in range(STUMP_T)]
    for b in range(3):
        w = masks[b].astype(ld)
        raw = np.full(n, ld(s["raw0"][b]))
        rows = np.nonzero(masks[b])[0]
        for t in range(STUMP_T):
            p = ref._lm_sigmoid(raw)
            g, h = w * (y - p), w * p * ref._lm_sigmoid(-raw)
            q = []
            for v in (g, h, w):
                f32, dist, _ = ref._f32_round_info(v)
                assert (dist[rows] > ld(2.0 ** -44)).all() or t == 0 and (dist[rows] > ld(2.0 ** -50)).all(), \
                    "input condition: a row sits on an f32 rounding boundary"
                q.append([ref.gbdt_q(x, shift) for x in f32])
            H = [[[0, 0, 0] for _ in range(256)] for _ in range(s["F"])]
            for i in rows:
                for f in range(s["F"]):
                    c = H[f][int(s["bins"][f, i])]
                    c[0] += q[0][i]
                    c[1] += q[1][i]
                    c[2] += q[2][i]
            o = ref.gbdt_split_oracle(H, s["nbins"], s["lo"], s["hi"], int(s["r2"][t, b, 0]), shift,
                                      STUMP_MIN_LEAF * unit, 2 * unit,
                                      rank=None if s["rank"] is None else s["rank"][t, b])
            f, j = int(s["feat"][t, b, 0]), int(s["blo"][t, b, 0])
            tag = (s["F"], "model", b, "stage", t)
            assert o.kind == "split" and f >= 0, tag
            why = o.certify(f, j)
            assert why is None, (tag, why)
            if t == 0:
                assert o.decided and (f, j) == o.best, (tag, (f, j), o.best)
            left, right, thr = ref.gbdt_split_children(o, f, j)
            assert np.float64(thr).view(np.int64) == s["thr"][t, b, 0].view(np.int64), (tag, "thr")
            want = [(o.tw, o.tg, o.th), left, right]
            assert s["stats"][t, b, :, :3].tolist() == [list(x) for x in want], (tag, "node sums")
            for c, (_, cg, ch) in ((1, left), (2, right)):
                assert _close(s["value"][t, b, c], Fraction(cg, ch), 4 * U), (tag, "leaf value", c)
            go_left = s["bins"][f] <= j
            raw = raw + ld(s["lr"]) * np.where(go_left, s["value"][t, b, 1], s["value"][t, b, 2]).astype(ld)
            x = w * -2 * (y * raw - ref._lm_softplus(raw))
            dev = int(np.rint(x * ld(2.0 ** 26))[rows].astype(np.int64).sum())
            bud = float((1 + ld(ref.GBDT_EPS_F64) * np.abs(x[rows]) * 2.0 ** 26).sum())
            assert abs(int(s["dev"][t, b]) - dev) <= bud, (tag, "deviance", int(s["dev"][t, b]) - dev, bud)
            score = s["dev"][t, b] / 2.0 ** 26 / len(rows)
            assert abs(float(s["train_score"][b][t]) - score) <= 4 * U * abs(score), (tag, "train_score_")
            cuts[t][b] = (f, j)
    return cuts


def assert_stump_cases(s, cuts):
    """What the data was crafted for, read off the certified fit."""
    if s["F"] == 5:
        # columns 1, 3 (duplicate) and 4 (mirror) tie exactly at stage 0
        for b in range(3):
            f, j = cuts[0][b]
            assert f in (1, 3, 4), cuts[0]
            if s["rank"] is None:
                assert f == 1, ("lowest index among the tied columns", cuts[0])
            else:
                assert f == min((1, 3, 4), key=lambda c: s["rank"][0, b][c]), ("sklearn's visit order", cuts[0])
    else:
        assert cuts[0][1][0] == 7 and s["nbins"][5] == 1
        f, j = cuts[0][1]
        assert s["lo"][7, j + 1] < s["thr"][0, 1, 0] * 2 - s["hi"][7, j], "model 1's threshold skips its empty bins"


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("F", [5, 9])
def test_stump_fit_host_certified(monkeypatch, F, ties):
    from hfens.models import hist_gbdt
    monkeypatch.setattr(hist_gbdt, "SKLEARN_TIES", ties)
    monkeypatch.setitem(hist_gbdt.LAST_PATH, "path", None)
    s = fit_stumps(F, torch.device("cpu"), ties)
    assert_stump_cases(s, check_stumps(s))
