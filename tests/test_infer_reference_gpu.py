"""The inference kernels (ops/csrc/stack.hip stack_infer; ops/csrc/infer.hip rbf_decision, svc_proba1,
svc_oof, forest_raw) against the longdouble oracle of ops/reference.py, at the widths, SV counts, tree
sizes, thresholds, distances and decision values where the kernels change path or lose accuracy.

Inputs, oracles and ``assert_stack`` (shape, no NaN, every decided row within its OWN budget, the
largest observed/budget ratio printed) come from tests/test_infer_reference.py, which also proves on
the CPU that these cases reject nine wrong variants.  Each test prints the path its launch takes,
recomputed from ops/csrc/stack_model.h's formulas (``stack_path``)."""
import ast
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

from hfens import ops
from hfens.ops.reference import proba_oracle, rbf_oracle

from test_infer_reference import (PLATT_AB, PLATT_CASES, RBF_CHUNK_EDGES, RBF_WIDTHS, RESID_CASES, SAT_CASES,
                                  THR_CASES, WIDTH_ROWS, WIDTHS, assert_stack, case, pack_spec, platt_decs)

pytestmark = pytest.mark.gpu

LDS_CAP = 160 * 1024


# ----------------------------------------------------------------------------- stack_model.h's plan
def stack_ks(F):
    ks = (F + 1) // 2
    return 4 if ks <= 4 else 9 if ks <= 9 else 12 if ks <= 12 else 16 if ks <= 16 else 32


def _sv_floats(ks, x3):
    return (3 * 2 * ks + 7) // 8 * 8 + 2 if x3 else 2 * ks + 2


def _lds_bytes(W, F, CH, ks, node_bytes, x3):
    xs = (W * 64 * (F | 1) + 3) & ~3
    return (_sv_floats(ks, x3) * CH + 4 * ks + xs) * 4 + node_bytes


def stack_chunk(W, F, mp, ks, node_bytes, x3):
    fixed = _lds_bytes(W, F, 0, ks, node_bytes, x3)
    if fixed >= LDS_CAP:
        return 0
    return min((LDS_CAP - fixed) // (_sv_floats(ks, x3) * 4) // 32 * 32, mp)


def _plan(W, F, mp, ks, node_bytes, x3):
    in_lds = 0 < node_bytes <= 24 * 1024
    CH = stack_chunk(W, F, mp, ks, node_bytes if in_lds else 0, x3)
    if in_lds and CH < mp:
        ch2 = stack_chunk(W, F, mp, ks, 0, x3)
        if ch2 > CH:
            in_lds, CH = False, ch2
    return CH, in_lds


Path = namedtuple("Path", "ks kind waves chunks trees")


def stack_path(pk):
    """The launch stack_pick (stack.hip) makes for ``pk`` under the current environment: KS, 'X3' or
    'f32', waves per workgroup, the SV chunk sizes, and trees 'lds' | 'global' | 'stumps'.

    X3 (KS ≤ 9, unless HFENS_STACK_X3=0) runs only when its plan keeps every SV resident.  The f32
    path scores its plans ``1000·(resident) + waves·blocks_per_cu``, 8 waves against 12 for KS ≤ 9:
      * only the 8-wave plan resident                     -> 8 waves, one chunk;
      * neither resident: each plan fills LDS to within one 32-SV step of the 160 KiB cap, more than
        half of it, so each has ONE block per CU and 12 waves beat 8 -> 12 waves, the 12-wave chunk;
      * both resident: blocks_per_cu depends on the register count, which is not modelled here ->
        waves '8|12' (one chunk and the same tree placement either way, asserted).
    HFENS_STACK_WAVES=8|12|16 forces the shape (16: f32 path only)."""
    F, mp = pk.F, pk.sv.mp
    ks = stack_ks(F)
    narrow = ks <= 9
    node_bytes = 0 if pk.stumps is not None else pk.forest.n_trees * pk.forest.max_nodes * 20
    trees = lambda in_lds: "stumps" if pk.stumps is not None else "lds" if in_lds else "global"   # noqa: E731
    split = lambda CH: tuple(min(CH, mp - s) for s in range(0, mp, CH))   # noqa: E731
    forced = int(os.environ.get("HFENS_STACK_WAVES", "0"))
    if narrow and int(os.environ.get("HFENS_STACK_X3", "1")) != 0:
        xw = forced if forced in (8, 12) else int(os.environ.get("HFENS_STACK_X3_WAVES", "8"))
        W = 12 if xw == 12 else 8
        CH, in_lds = _plan(W, F, mp, ks, node_bytes, True)
        if CH >= mp:
            return Path(ks, "X3", W, (mp,), trees(in_lds))
    plans = {W: _plan(W, F, mp, ks, node_bytes, False) for W in ((8, 12, 16) if narrow else (8,))}
    assert all(CH >= 32 for CH, _ in plans.values())
    if narrow and forced in (12, 16):
        W = forced
    elif not narrow or forced == 8 or plans[12][0] < mp <= plans[8][0]:
        W = 8
    elif plans[8][0] < mp:
        W = 12
    else:
        assert plans[8] == plans[12] == (mp, plans[8][1])
        return Path(ks, "f32", "8|12", (mp,), trees(plans[8][1]))
    CH, in_lds = plans[W]
    return Path(ks, "f32", W, split(CH), trees(in_lds))


_PACKED = {}


def packed(dev, name, stumps=None):
    c = case(name)
    st = c.stumps if stumps is None else stumps
    if (name, st) not in _PACKED:
        _PACKED[name, st] = pack_spec(c.M, dev, st)
    return _PACKED[name, st]


def run_stack(dev, name, dtype=torch.float64, n=None, grid=0, stumps=None, X=None):
    c = case(name)
    with np.errstate(over="ignore"):
        x = torch.as_tensor((c.X if X is None else X)[:n]).to(dev).to(dtype)
    return ops.stack_infer(x, packed(dev, name, stumps), grid=grid).cpu().numpy()


def sub(orc, idx):
    return {k: v[idx] for k, v in orc.items()}


def referee(name, out, path, label=""):
    """``out`` (all rows of the case) against the oracle whose d² budget is the launched path's: the
    X3 dropped-product term only where X3 ran."""
    c = case(name, path.kind == "X3")
    assert out.shape == (c.X.shape[0],)
    assert not np.isnan(out).any()
    return assert_stack(out if c.rows is None else out[c.rows], c.orc, f"{name} {label} path={tuple(path)}")


def check(dev, name, label="", **kw):
    return referee(name, run_stack(dev, name, **kw), stack_path(packed(dev, name, kw.get("stumps"))), label)


# ----------------------------------------------------------------------------- a. width sweep
@pytest.mark.parametrize("kind", ["stumps", "forest"])
@pytest.mark.parametrize("F", WIDTHS)
def test_width_sweep(dev, monkeypatch, F, kind):
    name = f"width-{F}-{kind}"
    envs = [("1", "8"), ("1", "12"), ("0", "8")] if F <= 18 else [("1", "8")]
    seen = set()
    for x3, xw in envs:
        monkeypatch.setenv("HFENS_STACK_X3", x3)
        monkeypatch.setenv("HFENS_STACK_X3_WAVES", xw)
        path = stack_path(packed(dev, name))
        seen.add(path.kind)
        assert path.ks == stack_ks(F) and path.chunks == (96,)
        c = case(name, path.kind == "X3")
        for dtype in (torch.float32, torch.float64):
            worst = 0.0
            for n in WIDTH_ROWS:
                out = run_stack(dev, name, dtype=dtype, n=n)
                worst = max(worst, assert_stack(out, sub(c.orc, slice(0, n)), name, quiet=True))
            print(f"{name} X3={x3} waves={xw} {str(dtype)[6:]} path={tuple(path)}: largest observed/budget {worst:.3f}, "
                  f"undecided {int(c.orc['undecided'].sum())} of {c.X.shape[0]}")
    assert seen == ({"X3", "f32"} if F <= 18 else {"f32"})


# ----------------------------------------------------------------------------- b. residency edges
@pytest.mark.parametrize("name", RESID_CASES)
def test_residency_edges(dev, name):
    """The default launch.  Above 1600 SVs neither f32 plan is resident and stack_pick takes 12 waves
    (chunk 1376), so the 32-SV tail of the launched plan is at mp = 2·1376 + 32; the 8-wave plan's
    edges (1600 + 32, 1600 + 1600 + 32) run in test_residency_edges_8_waves."""
    mp = int(name.split("-")[1])
    path = stack_path(packed(dev, name))
    assert path[1:4] == {544: ("X3", 8, (544,)), 576: ("f32", "8|12", (576,)), 1600: ("f32", 8, (1600,)),
                         1632: ("f32", 12, (1376, 256)), 2784: ("f32", 12, (1376, 1376, 32)),
                         3232: ("f32", 12, (1376, 1376, 480))}[mp]
    assert packed(dev, name).sv.mp == mp
    for grid in (0, 1, 3):                            # grid 1, 3: a workgroup restages chunk 0 between tiles
        check(dev, name, f"grid={grid}", grid=grid)


# ----------------------------------------------------------------------------- c. trees out of LDS
@pytest.mark.parametrize("name,want", [("trees-global", ("f32", 1, "global")), ("evict-96", ("f32", 1, "global")),
                                       ("evict-128", ("f32", 2, "global")), ("t0", ("X3", 1, "global")),
                                       ("sparse-stumps", ("X3", 1, "stumps")), ("width-17-forest", ("X3", 1, "lds"))])
def test_tree_residency(dev, monkeypatch, name, want):
    if name == "trees-global":
        monkeypatch.setenv("HFENS_STACK_X3", "0")
    if name == "sparse-stumps":
        off = packed(dev, name).stumps.off.cpu().numpy()
        assert (np.diff(off)[1::2] == 0).all() and (np.diff(off)[0::2] > 0).all()
    path = stack_path(packed(dev, name))
    assert (path.kind, len(path.chunks), path.trees) == want
    for dtype in (torch.float32, torch.float64):
        check(dev, name, str(dtype)[6:], dtype=dtype)
    if name == "trees-global":
        monkeypatch.setenv("HFENS_STACK_X3", "1")
        check(dev, name, "X3")


# ----------------------------------------------------------------------------- d. threshold edges
@pytest.mark.parametrize("name", THR_CASES)
def test_threshold_edges(dev, monkeypatch, name):
    """Leaf selection is exact: raw_gbc (forest_raw) within the accumulation budget of the oracle's
    leaf sum — the wrong leaf is ≥ 0.3 away — for f32 rows and for f64 rows that round to them."""
    c = case(name)
    M = c.M
    tabs = [torch.as_tensor(a) for a in (M.feature, M.threshold, M.left, M.right, M.value)]
    with np.errstate(over="ignore"):
        for x in (torch.as_tensor(c.X.astype(np.float32)), torch.as_tensor(c.X)):
            raw = ops.tree_raw(x.to(dev), *tabs, M.init, M.lr).cpu().numpy()
            assert_stack(raw, c.orc, f"{name} forest_raw {str(x.dtype)[6:]}", key="raw_gbc")
    assert float(c.orc["d_raw_gbc"].max()) < 1e-3
    for x3 in ("1", "0"):
        monkeypatch.setenv("HFENS_STACK_X3", x3)
        for dtype in (torch.float32, torch.float64):
            check(dev, name, f"X3={x3} {str(dtype)[6:]}", dtype=dtype)
    if c.stumps:                                      # the stump model through the tree walk as well
        check(dev, name, "walk", stumps=False)


# ----------------------------------------------------------------------------- e. distance edges
@pytest.mark.parametrize("name", ["dist", "dist-underflow"])
def test_distance_edges(dev, monkeypatch, name):
    c = case(name)
    M = c.M
    for x3 in ("1", "0"):
        monkeypatch.setenv("HFENS_STACK_X3", x3)
        for dtype in (torch.float32, torch.float64):
            check(dev, name, f"X3={x3} {str(dtype)[6:]}", dtype=dtype)
    dec, dd = rbf_oracle(c.X, M.sv, M.coef, M.gamma, M.intercept)
    t = torch.as_tensor
    got = ops.rbf_decision(t(c.X).to(dev), t(M.sv).to(dev), t(M.coef).to(dev), M.gamma, M.intercept).cpu().numpy()
    assert_stack(got, dict(dec=dec, d_dec=dd), f"{name} rbf_decision", key="dec")
    if name == "dist-underflow":                      # every kernel value underflows away from the SVs
        assert (np.abs(dec[40:] - np.float32(M.intercept)) < 1e-30).all()
        assert (got[40:] == np.float32(M.intercept)).all()


# ----------------------------------------------------------------------------- f. rbf_decision
def _rbf_case(F, m, n, seed, rows=None):
    rng = np.random.default_rng(seed)
    z, sv, coef = rng.standard_normal((n, F)), rng.standard_normal((m, F)), rng.standard_normal(m)
    dec, dd = rbf_oracle(z if rows is None else z[rows], sv, coef, 1.0 / F, 0.25)
    return z, sv, coef, dec, dd


def _rbf_run(dev, z, sv, coef, F):
    t = torch.as_tensor
    return ops.rbf_decision(t(z).to(dev), t(sv).to(dev), t(coef).to(dev), 1.0 / F, 0.25).cpu().numpy()


def _rbf_ks(F):
    ks = (F + 1) // 2
    return next(k for k in (2, 4, 8, 12, 16, 24, 32) if ks <= k)


def _rbf_chunk(F, mp):
    return min(96 * 1024 // ((2 * _rbf_ks(F) + 2) * 4) // 32 * 32, mp)


@pytest.mark.parametrize("F", RBF_WIDTHS)
def test_rbf_width_sweep(dev, F):
    z, sv, coef, dec, dd = _rbf_case(F, 70, 200, 300 + F)
    got = _rbf_run(dev, z, sv, coef, F)
    assert_stack(got, dict(dec=dec, d_dec=dd), f"rbf F={F} KS={_rbf_ks(F)} chunks=1", key="dec")


@pytest.mark.parametrize("F,mp", RBF_CHUNK_EDGES)
def test_rbf_chunk_edges(dev, F, mp):
    assert _rbf_chunk(F, mp) == mp - 32
    rows = np.arange(0, 200, 3)
    z, sv, coef, dec, dd = _rbf_case(F, mp - 1, 200, 400 + F, rows)
    got = _rbf_run(dev, z, sv, coef, F)
    assert got.shape == (200,) and not np.isnan(got).any()
    assert_stack(got[rows], dict(dec=dec, d_dec=dd), f"rbf F={F} KS={_rbf_ks(F)} chunks=2 ({mp - 32} + 32)", key="dec")


def test_rbf_grid_stride_wrap(dev):
    """n > 2048 workgroups × 4 waves × 32 rows with two SV chunks: the workgroups that wrap restage chunk
    0 for their second row tile.  The oracle referees the last 33 rows and 256 sampled ones."""
    F, mp, n = 64, 384, 262144 + 33
    assert _rbf_chunk(F, mp) == 352
    rng = np.random.default_rng(5)
    sv, coef = rng.standard_normal((mp - 1, F)), rng.standard_normal(mp - 1)
    z = torch.randn(n, F, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    rows = np.concatenate([np.sort(rng.choice(n - 33, 256, replace=False)), np.arange(n - 33, n)])
    dec, dd = rbf_oracle(z[rows].numpy(), sv, coef, 1.0 / F, 0.25)
    got = _rbf_run(dev, z, sv, coef, F)
    assert got.shape == (n,) and not np.isnan(got).any()
    assert_stack(got[rows], dict(dec=dec, d_dec=dd), "rbf wrap F=64 KS=32 chunks=2 (352 + 32)", key="dec")


# ----------------------------------------------------------------------------- g. Platt and coupling
@pytest.mark.parametrize("A,B", PLATT_AB)
def test_platt_kernels_beside_the_jumps(dev, A, B):
    """svc_proba1 and svc_oof at every coupling jump ± 64 f32 ulps, at r01's clip points and at ±1e4:
    p within the same-iteration-count budget shows the kernel took the oracle's iteration count."""
    dec = platt_decs(A, B)
    p, it, dp, und = proba_oracle(dec, A, B)
    assert not und.any() and len(set(it.tolist())) >= 3
    orc = dict(p_svc=p, d_p_svc=dp, undecided=und)
    got = ops.svc_proba1(torch.as_tensor(dec).to(dev), A, B).cpu().numpy()
    assert_stack(got, orc, f"svc_proba1 A={A} B={B} iteration counts {sorted(set(it.tolist()))}", key="p_svc")
    # svc_oof: model 0 (rho 0) and model 1 (rho 1: dec + 1 − 1 is exact) with the same (A, B)
    n = dec.size
    model = (np.arange(n) % 2).astype(np.int32)
    d64 = dec.astype(np.float64) + model
    rows = np.random.default_rng(0).permutation(n).astype(np.int64)
    meta = torch.full((n, 3), -1.0, dtype=torch.float64, device=dev)
    t = lambda a: torch.as_tensor(a).to(dev)   # noqa: E731
    args = [t(d64), t(model), t(np.array([0.0, 1.0])), t(np.array([A, B, A, B])), t(rows)]
    ops.ext().svc_oof(*(a.data_ptr() for a in args), meta.data_ptr(), 3, 1, n, ops.stream_ptr(dev))
    meta = meta.cpu().numpy()
    assert (meta[:, 0] == -1).all() and (meta[:, 2] == -1).all()
    assert_stack(meta[rows, 1], orc, f"svc_oof A={A} B={B}", key="p_svc")


@pytest.mark.parametrize("name", PLATT_CASES + SAT_CASES)
def test_stack_coupling_beside_the_jumps(dev, name):
    c = case(name)
    assert not c.orc["undecided"][120:].any()
    for dtype in (torch.float32, torch.float64):
        check(dev, name, f"{str(dtype)[6:]} iteration counts {sorted(set(c.orc['it'].tolist()))}", dtype=dtype)


# ----------------------------------------------------------------------------- h. row isolation
@pytest.mark.parametrize("name", ["width-17-stumps", "width-17-forest", "width-40-forest"])
def test_row_isolation(dev, name):
    c = case(name)
    n = 200
    pk = packed(dev, name)

    def run(X):
        out = torch.full((n + 64,), -1.0, device=dev)
        with np.errstate(over="ignore"):
            ops.stack_infer(torch.as_tensor(X.astype(np.float32)).to(dev), pk, out=out)
        return out.cpu().numpy()
    base = run(c.X[:n])
    path = stack_path(pk)
    assert_stack(base[:n], sub(case(name, path.kind == "X3").orc, slice(0, n)), f"{name} path={tuple(path)}")
    for pos in (0, 31, 32, 63, 64, n - 1):
        for bad in (3e38, -3e38, np.nan):
            X = c.X[:n].copy()
            X[pos] = bad
            out = run(X)
            keep = np.arange(n) != pos
            assert np.array_equal(out[:n][keep].view(np.int32), base[:n][keep].view(np.int32)), (pos, bad)
            assert (out[n:] == -1.0).all(), (pos, bad)


# ----------------------------------------------------------------------------- i. forced wave shapes
_CHILD = """
import sys
import numpy as np
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import test_infer_reference_gpu as g
dev = torch.device("cuda:0")
out = {{}}
grids = [int(v) for v in sys.argv[2].split(",")]
for name in sys.argv[3:]:
    out[name + "|path"] = np.array(repr(tuple(g.stack_path(g.packed(dev, name)))))
    for dtype in (torch.float32, torch.float64):
        for grid in grids:
            out[name + "|" + str(dtype)[6:] + " grid=" + str(grid)] = g.run_stack(dev, name, dtype=dtype, grid=grid)
np.savez(sys.argv[1], **out)
"""


def run_child(tmp_path, env, names, grids=(0,)):
    """One fresh Python process (HFENS_STACK_WAVES is read once per process) under its own timeout:
    stack_infer on the named cases, f32 and f64 rows; every output refereed here against the
    oracle of the path the child reports.  -> {name: Path}."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=os.path.dirname(here), tests=here))
    res = tmp_path / "out.npz"
    r = subprocess.run([sys.executable, str(script), str(res), ",".join(map(str, grids)), *names],
                       env=dict(os.environ, **env), timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(res)
    paths = {name: Path(*ast.literal_eval(str(got[name + "|path"]))) for name in names}
    for key in got.files:
        name, what = key.split("|")
        if what != "path":
            referee(name, got[key], paths[name], f"{env} {what}")
    return paths


@pytest.mark.parametrize("waves,x3", [("8", "1"), ("12", "1"), ("16", "1"), ("8", "0"), ("12", "0"), ("16", "0")])
def test_forced_wave_shapes(dev, tmp_path, waves, x3):
    """One child per forced shape (one at a time) runs the F = 17 and F = 8 width cases."""
    names = ["width-17-stumps", "width-17-forest", "width-8-stumps", "width-8-forest"]
    paths = run_child(tmp_path, dict(HFENS_STACK_WAVES=waves, HFENS_STACK_X3=x3), names)
    for path in paths.values():                       # (16 waves: no X3 shape, X3 keeps its 8)
        want = ("X3", 8 if waves == "16" else int(waves)) if x3 == "1" else ("f32", int(waves))
        assert (path.kind, path.waves, path.chunks) == want + ((96,),)


def test_residency_edges_8_waves(dev, tmp_path):
    """The 8-wave f32 plan's chunk edge at F = 17 (chunk 1600), forced with HFENS_STACK_WAVES=8 in a
    child process: two chunks, the second of 32 SVs; three chunks; grid 1 and 3 restage chunk 0."""
    paths = run_child(tmp_path, dict(HFENS_STACK_WAVES="8"), ["resid-1600", "resid-1632", "resid-3232"], (0, 1, 3))
    assert [tuple(paths[f"resid-{mp}"][1:4]) for mp in (1600, 1632, 3232)] == [
        ("f32", 8, (1600,)), ("f32", 8, (1600, 32)), ("f32", 8, (1600, 1600, 32))]
