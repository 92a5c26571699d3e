"""Batched logistic-regression solvers.

All B fits (CV folds / refit) advance together; each outer iteration is a few
device GEMM/reduction ops over the rows plus one tiny subproblem launch:

* L1 (liblinear ``solve_l1r_lr`` objective, intercept as an L1-penalised augmented
  feature with ``intercept_scaling``): proximal Newton.  Quadratic model
  (g, H = C·X̃ᵀDX̃) → L1-QP solved by the ``l1_qp_cd`` kernel (one wave per model, H in
  LDS) → Armijo line search on 8 step sizes evaluated in one pass.
* L2 (the lbfgs meta-learner's objective ½‖w‖² + C·Σ s·logloss, intercept not
  penalised): damped Newton with a batched dense solve.

Both converge to the unique optimum well below liblinear's / lbfgs's tolerance,
so coefficients agree with sklearn to its own stopping accuracy.
With ``group`` (rows sharded over ranks) the per-iteration g, H and line-search
losses are all-reduced (F² + F + 8 doubles per model).

On one GPU the whole solve runs as ONE launch (``ops/csrc/logreg.hip``): ``logreg_coop`` spreads
every model over up to 16 workgroups (row slabs; the per-iteration H/g/loss and line-search sums
are exchanged between them in a fixed member order), ``logreg_fused`` is the one-workgroup form
(used when a cooperative SMO shares the device and too few CUs are free for the members, or
``HFENS_LOGREG_MEMBERS=1``).  The loop below is the host / data-parallel path and the reference
the fused kernels are tested against.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .. import ops
from .base import balanced_class_weight


def _check_same(models, attrs):
    for a in attrs:
        if len({repr(getattr(m, a)) for m in models}) != 1:
            raise ValueError(f"batched logistic fit needs identical '{a}' across models")


def _newton_finish(Hb, gb, wb, pn, lam, d, eps_diag):
    """Exact minimiser of the L1-QP on the current sign pattern of w + d, or None when it is not
    optimal (mirror of ops/csrc/l1qp.h: the same reduced system, the same acceptance test)."""
    F1 = gb.shape[0]
    Hp = Hb + eps_diag * np.eye(F1)
    u = wb + d
    S = (~pn) | (u != 0)
    sig = np.where(pn, np.sign(u), 0.0)
    A = np.where(S[:, None] & S[None, :], Hp, 0.0) + np.diag((~S).astype(float))
    rhs = np.where(S, Hp @ wb - gb - lam * sig, 0.0)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    un = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    ok = np.all(np.where(S & pn, ((sig > 0) & (un > 0)) | ((sig < 0) & (un < 0)), True))
    r = gb + Hp @ (un - wb)
    ok = ok and np.all(np.where(~S, np.abs(r) <= lam * (1 + 1e-12), True))
    return un - wb if ok else None


def _host_l1_qp(H, g, w, penal, lam, max_sweeps=200, tol=1e-12, eps_diag=0.0, capped=None):
    """``capped``: an optional list that receives, per model, whether the solve ran into
    ``max_sweeps`` (left by neither the step rule nor the exact finish)."""
    Hn, gn, wn = H.cpu().numpy(), g.cpu().numpy(), w.cpu().numpy()
    pn = penal.cpu().numpy().astype(bool)
    B, F1 = gn.shape
    out = np.zeros_like(gn)
    for b in range(B):
        Hb, gb, wb = Hn[b], gn[b], wn[b]
        d = np.zeros(F1)
        Hd = np.zeros(F1)
        if capped is not None:
            capped.append(True)
        for sweep in range(max_sweeps):
            mx = 0.0
            for k in range(F1):
                a = max(Hb[k, k], 1e-300)
                inv = 1.0 / a                      # as the kernel: reciprocal, then multiply
                lin = gb[k] + Hd[k] - a * d[k]
                z0 = wb[k] - lin * inv
                thr = lam * inv if pn[k] else 0.0
                z = z0
                if thr > 0:
                    z = z0 - thr if z0 > thr else (z0 + thr if z0 < -thr else 0.0)
                nd = z - wb[k]
                step = nd - d[k]
                if step != 0.0:
                    Hd += Hb[:, k] * step
                    d[k] = nd
                    mx = max(mx, abs(step))
            left = mx <= tol
            if not left and sweep % 4 == 3:   # ops/csrc/l1qp.h: exact finish on the sign pattern, if optimal
                dn = _newton_finish(Hb, gb, wb, pn, lam, d, eps_diag)
                if dn is not None:
                    d = dn
                    left = True
            if left:
                if capped is not None:
                    capped[-1] = False
                break
        out[b] = d
    return torch.as_tensor(out, dtype=g.dtype, device=g.device)


FUSED = os.environ.get("HFENS_LOGREG_FUSED", "1") != "0"
MEMBERS = int(os.environ.get("HFENS_LOGREG_MEMBERS", "0"))   # 0 = auto
MIN_ROWS_PER_MEMBER = 512
LAST_PATH = {"path": None}
_WARNED_EMULATION = [False]
# workgroups a cooperative LR launch may occupy (None = all CUs).  The stacking trainer lowers it
# while a cooperative SMO holds most CUs on another stream: LR members spin on each other, so all of
# them must fit on the CUs the SMO leaves free (stack_trainer._launch_bases).
BLOCK_BUDGET = [None]


def lr_members(B: int, n: int, ncu: int) -> int:
    if MEMBERS > 0:
        return max(1, min(16, MEMBERS, ncu // B))
    budget = ncu if BLOCK_BUDGET[0] is None else min(ncu, BLOCK_BUDGET[0])
    return max(1, min(16, budget // B, -(-n // MIN_ROWS_PER_MEMBER)))


def _launch_fused(Xa, s, ypm, penal, C: float, l1: bool, max_outer: int, flags=None) -> dict:
    """All B solves in one launch, enqueued with no host synchronisation; :func:`_finish_fused`
    returns (W [B, F1], n_iter [B] int32).  ``flags``: the input guards as device bools (finite X,
    binary y) — or a callable producing them, called right after the launch — read with the
    cooperative launch's error word in one transfer (a failed guard raises after the launch)."""
    E = ops.ext()
    B, n = s.shape
    F1 = Xa.shape[1]
    dev = Xa.device
    Xc, sc, yc = Xa.contiguous(), s.contiguous(), ypm.contiguous()
    W = torch.empty(B, F1, dtype=torch.float64, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    Z = torch.empty(B, n, dtype=torch.float64, device=dev)
    Xd = torch.empty_like(Z)
    h = dict(args=(B, n, F1, Xc, sc, yc, penal, C, l1, max_outer, Z, Xd, W, iters), flags=flags, err=None)
    from .smo import _num_cus
    M = lr_members(B, n, _num_cus(dev))
    if M > 1:
        nv = max(F1 * (F1 + 1) // 2 + F1 + 1, 8)   # (logreg.hip logreg_nvmax: ≥ the 8 trial losses)
        xchg = torch.empty(B * 2 * M * nv * 2, dtype=torch.int64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        from ..utils.timing import hmark, dmark
        hmark("lr_launch")
        dmark("lr_launch")
        E.logreg_coop(B, M, n, F1, Xc.data_ptr(), sc.data_ptr(), yc.data_ptr(), penal.data_ptr(), float(C), int(l1),
                      int(max_outer), Z.data_ptr(), Xd.data_ptr(), W.data_ptr(), iters.data_ptr(), xchg.data_ptr(),
                      err.data_ptr(), ops.stream_ptr(dev))
        dmark("lr_kernel")
        LAST_PATH["members"] = M
        h.update(err=err, xchg=xchg)
    else:
        _launch_single(h)
    if callable(flags):
        # (the guards computed behind the solve: nothing but the read-back consumes them)
        flags = h["flags"] = flags()
    # the error word and guards' read-back queued right behind the solve (pinned + event):
    # _finish_fused then waits for this solve only
    parts = ([h["err"]] if h["err"] is not None else []) + ([flags.to(torch.int32)] if flags is not None else [])
    if parts:
        dv = torch.cat(parts)
        from ..utils.hostread import stage
        host, ev = stage(dv)
        h["staged"] = (host, ev, dv)
    return h


def _launch_single(h):
    B, n, F1, Xc, sc, yc, penal, C, l1, max_outer, Z, Xd, W, iters = h["args"]
    LAST_PATH["members"] = 1
    from ..utils.timing import dmark
    dmark("lr_launch")
    ops.ext().logreg_fused(B, n, F1, Xc.data_ptr(), sc.data_ptr(), yc.data_ptr(), penal.data_ptr(), float(C),
                           int(l1), int(max_outer), Z.data_ptr(), Xd.data_ptr(), W.data_ptr(), iters.data_ptr(),
                           ops.stream_ptr(Xc.device))
    dmark("lr_kernel")


def _finish_fused(h):
    from ..utils import guards
    from ..utils.timing import hmark
    flags, err = h["flags"], h["err"]
    parts = ([err] if err is not None else []) + ([flags.to(torch.int32)] if flags is not None else [])
    st = h.get("staged")
    if st is not None and st[2].numel() == sum(int(p.numel()) for p in parts):
        from ..utils.hostread import landed
        host = landed(st[0], st[1]).tolist()
    else:
        host = torch.cat(parts).cpu().tolist() if parts else []
    hmark("lr_host_read")
    if flags is not None:
        guards.raise_flags(host[len(host) - 2:], _GUARD_SPECS)
    if err is not None and host[0] != 0:
        import warnings
        warnings.warn("cooperative logistic regression timed out waiting for a member; re-solving with one "
                      "workgroup per model")
        LAST_PATH["coop_fallback"] = True
        h["refit"] = True        # (models set at launch hold the failed solve's intercept copies)
        _launch_single(h)
    W, iters = h["args"][12], h["args"][13]
    return W, iters


_GUARD_SPECS = (("finite", "LogisticRegression.fit X"), ("binary", "LogisticRegression.fit y"))


def set_fitted_from(h: dict, only=None):
    """``set_fitted`` of a fused launch's models from its device coefficients, without the host read
    of :func:`finish_logreg_batch` (the caller has read the launch's error word and guards itself,
    e.g. through :class:`hfens.utils.guards.Deferred`).  ``only``: model indices to finish."""
    models, F, scale, fit_intercept, dev = h["models"], h["F"], h["scale"], h["fit_intercept"], h["dev"]
    W, iters = h["fused"]["args"][12], h["fused"]["args"][13]
    for b, m in enumerate(models):
        if only is not None and b not in only:
            continue
        intercept = W[b, F] * scale if fit_intercept else torch.zeros((), dtype=torch.float64, device=dev)
        m.set_fitted(W[b, :F], intercept.reshape(1), iters[b:b + 1], F, device=dev)
    return models


def _allreduce(ts, group):
    if group is None:
        return ts
    from ..parallel import dist as pdist
    return pdist.all_reduce_sum_f64(ts, group)


def _check_random_state(rs):
    """scikit-learn's check_random_state: None → numpy's global RandomState (the one
    ``train_ensemble_public.py:31`` seeds), an int → a fresh RandomState, an instance → itself."""
    if rs is None:
        return np.random.mtrand._rand
    if isinstance(rs, (int, np.integer)):
        return np.random.RandomState(int(rs))
    return rs


def _fit_liblinear_exact(models, X: torch.Tensor, yv: torch.Tensor, masks: torch.Tensor, max_iter: int,
                         seed_order=None):
    """liblinear's own default-tolerance iterate (ops/csrc/liblinear_host.hip), one host solve per
    model.  The seeds are drawn exactly as scikit-learn's ``_fit_liblinear`` draws them —
    ``check_random_state(random_state).randint(INT_MAX)`` — in model order, so a stacking fit
    that lists the refit first and then the CV folds consumes numpy's global stream in the
    reference's order (StackingClassifier refits every estimator, then cross_val_predict fold by
    fold: the six 'lg' fits are the only draws after ``seed(2020)``).
    ``seed_order``: the model indices in draw order (default: list order)."""
    from concurrent.futures import ThreadPoolExecutor
    m0 = models[0]
    E = ops.ext()
    Xh = np.ascontiguousarray(X.detach().to("cpu", torch.float64).numpy())
    yh = np.ascontiguousarray(yv.detach().to("cpu", torch.float64).numpy())
    mh = masks.detach().cpu().numpy().astype(bool)
    seeds = [0] * len(models)
    for b in (seed_order if seed_order is not None else range(len(models))):
        seeds[b] = int(_check_random_state(models[b].random_state).randint(np.iinfo("i").max))
    F = Xh.shape[1]
    bias = float(m0.intercept_scaling) if m0.fit_intercept else -1.0

    def solve(b):
        rows = np.flatnonzero(mh[b])
        Xb = np.ascontiguousarray(Xh[rows])
        yb = np.ascontiguousarray(yh[rows])
        n1 = float((yb > 0.5).sum())
        n0 = float(yb.shape[0]) - n1
        cw = (yb.shape[0] / (2.0 * np.array([n0, n1]))) if m0.class_weight == "balanced" else np.ones(2)
        sw = np.ones(yb.shape[0])
        w = np.zeros(F + (1 if bias > 0 else 0))
        it = E.liblinear_l1r_lr(Xb.ctypes.data, yb.ctypes.data, sw.ctypes.data, int(yb.shape[0]), F, bias,
                                float(m0.C) * cw[0], float(m0.C) * cw[1], float(m0.tol), int(max_iter), seeds[b],
                                w.ctypes.data)
        return w, it

    with ThreadPoolExecutor(min(8, len(models))) as ex:
        outs = list(ex.map(solve, range(len(models))))
    dev = X.device
    for m, (w, it) in zip(models, outs):
        icpt = w[F] * bias if bias > 0 else 0.0
        m.set_fitted(torch.as_tensor(w[:F]), torch.tensor([icpt], dtype=torch.float64),
                     torch.tensor([it], dtype=torch.int32), F, device=dev)
    LAST_PATH["path"] = "liblinear-host"
    return models


def fit_logreg_batch(models, X: torch.Tensor, y: torch.Tensor, masks: Optional[torch.Tensor] = None,
                     group=None, max_outer: int = 100, seed_order=None):
    return finish_logreg_batch(launch_logreg_batch(models, X, y, masks, group, max_outer, seed_order))


def finish_logreg_batch(h: dict):
    """Completes :func:`launch_logreg_batch`: the fused path's one host read (error word and input
    guards), then ``set_fitted``; other paths finished inside the launch."""
    if "fused" not in h:
        return h["models"]
    _finish_fused(h["fused"])
    if not h.get("preset") or h["fused"].get("refit"):
        _set_models(h)
    return h["models"]


def _set_models(h: dict) -> None:
    """``set_fitted`` of a fused launch's models from its device solution (stream-ordered behind
    the solve: valid to call before the solve has run)."""
    models, F, scale, fit_intercept, dev = h["models"], h["F"], h["scale"], h["fit_intercept"], h["dev"]
    W, iters = h["fused"]["args"][12], h["fused"]["args"][13]
    for b, m in enumerate(models):
        intercept = W[b, F] * scale if fit_intercept else torch.zeros((), dtype=torch.float64, device=dev)
        m.set_fitted(W[b, :F], intercept.reshape(1), iters[b:b + 1], F, device=dev)


_PENAL: dict = {}


def _penal_mask(F1: int, l1: bool, fit_intercept: bool, device) -> torch.Tensor:
    """The penalty mask (1 = penalised; the lbfgs-path intercept is not), one per shape and device:
    the kernels only read it, so a fit's critical path carries no fills for it."""
    key = (F1, l1, fit_intercept, str(device))
    t = _PENAL.get(key)
    if t is None:
        # (a blocking host → device copy, once: complete before any stream can read it)
        t = torch.tensor([1] * (F1 - 1) + [0 if (not l1 and fit_intercept) else 1], dtype=torch.uint8).to(device)
        _PENAL[key] = t
    return t


def logreg_label_prep(models, y: torch.Tensor, n: int, device) -> dict:
    """The label-only inputs of a single-process fused :func:`launch_logreg_batch` (the labels'
    guard, ±1 labels, sample weights, penalty mask, intercept column), enqueued on the CURRENT
    stream — so a caller can compute them while the features are still being produced on another
    stream (the stacking trainer's meta model, behind the out-of-fold columns)."""
    from ..utils import guards
    m0 = models[0]
    B = len(models)
    yv = y.to(device=device, dtype=torch.float64)
    masks = torch.ones(B, n, dtype=torch.bool, device=device)
    mk = masks.to(torch.float64)
    if m0.class_weight == "balanced":
        cnt1 = (mk * yv[None]).sum(1)
        cnt = torch.stack([mk.sum(1) - cnt1, cnt1], 1)
        cw = cnt.sum(1, keepdim=True) / (2.0 * cnt)
        sw = mk * torch.where(yv[None] > 0.5, cw[:, 1:2], cw[:, 0:1])
    else:
        sw = mk
    F1_extra = int(bool(m0.fit_intercept))
    ones = (torch.full((n, 1), float(m0.intercept_scaling), dtype=torch.float64, device=device)
            if m0.fit_intercept else None)
    return dict(n=n, yflag=guards.binary_flag(yv), masks=masks, yv=yv, ypm=2.0 * yv - 1.0, s=sw, ones=ones,
                extra=F1_extra)


def launch_logreg_batch(models, X: torch.Tensor, y: torch.Tensor, masks: Optional[torch.Tensor] = None,
                        group=None, max_outer: int = 100, seed_order=None, prep: Optional[dict] = None,
                        preset: bool = False) -> dict:
    """Fit ``models`` (one per row mask); on the fused device path the solve is only enqueued —
    no host synchronisation until :func:`finish_logreg_batch` (the stacking trainer launches the
    meta model this way before it reads the SVC's results back).  ``prep``: the label-only inputs
    from :func:`logreg_label_prep` (no masks; single process).  ``preset`` (with ``prep``): the
    models' ``set_fitted`` runs here, behind the enqueued solve, so :func:`finish_logreg_batch`
    is left with the error word / guards read only (the stacking fit's last host step)."""
    m0 = models[0]
    if prep is not None and masks is None and group is None and X.is_cuda and FUSED and X.dim() == 2 \
            and int(X.shape[0]) == prep["n"] and X.shape[1] + prep["extra"] <= 64 and m0.penalty in ("l1", "l2") \
            and not (m0.penalty == "l1" and m0.solver == "liblinear"
                     and all(getattr(mm, "emulate_liblinear", False) for mm in models)):
        # only the feature-dependent work remains: the finite guard and the intercept column
        from ..utils import guards
        _check_same(models, ("penalty", "C", "fit_intercept", "intercept_scaling", "class_weight", "solver"))
        X = X.to(torch.float64)
        flags = lambda: torch.stack([guards.finite_flag(X), prep["yflag"]])   # noqa: E731 (after the launch)
        Xa = torch.cat([X, prep["ones"]], 1) if prep["ones"] is not None else X
        F1 = Xa.shape[1]
        l1 = m0.penalty == "l1"
        penal = _penal_mask(F1, l1, bool(m0.fit_intercept), X.device)
        scale = float(m0.intercept_scaling) if (m0.fit_intercept and l1) else 1.0
        LAST_PATH["path"] = "fused"
        h = dict(models=models, F=int(X.shape[1]), scale=scale, fit_intercept=bool(m0.fit_intercept), dev=X.device,
                 fused=_launch_fused(Xa, prep["s"], prep["ypm"], penal, float(m0.C), l1, max_outer, flags))
        if preset:
            _set_models(h)
            h["preset"] = True
        return h
    _check_same(models, ("penalty", "C", "fit_intercept", "intercept_scaling", "class_weight", "solver"))
    if m0.penalty not in ("l1", "l2"):
        raise NotImplementedError("penalty must be 'l1' or 'l2'")
    from ..utils import guards
    want = (m0.penalty == "l1" and m0.solver == "liblinear"
            and all(getattr(m, "emulate_liblinear", False) for m in models))
    emulate = want and group is None
    if want and group is not None and not _WARNED_EMULATION[0]:
        # rows sharded over ranks (the data-parallel policy): liblinear's sequential host iterate
        # would need every row on every rank, so the device solve runs — the exact optimum of the
        # same objective, not the reference's default-tolerance iterate and seed draw (T:31/T:46)
        import warnings
        warnings.warn("liblinear emulation is single-process only: with rows sharded over ranks 'lg' is "
                      "solved to its exact optimum instead of reproducing liblinear's seeded iterate",
                      RuntimeWarning, stacklevel=2)
        _WARNED_EMULATION[0] = True
    fused = (X.is_cuda and group is None and FUSED and not emulate and X.dim() == 2
             and X.shape[1] + int(bool(m0.fit_intercept)) <= 64 and X.shape[0] > 0)
    flags = None
    from ..utils.timing import hmark
    hmark("lr_in")
    if fused:
        # the guards ride on the fused launch's one host read instead of two synchronous checks
        flags = torch.stack([guards.finite_flag(X), guards.binary_flag(y.to(X.device))])
        hmark("lr_flags")
    else:
        guards.check_finite(X, "LogisticRegression.fit X")
        guards.check_binary(y, "LogisticRegression.fit y")
    dev = X.device
    X = X.to(torch.float64)
    n, F = X.shape
    B = len(models)
    if masks is None:
        masks = torch.ones(B, n, dtype=torch.bool, device=dev)
    yv = y.to(device=dev, dtype=torch.float64)
    if emulate:
        return dict(models=_fit_liblinear_exact(models, X, yv, masks, int(m0.max_iter), seed_order))
    ypm = 2.0 * yv - 1.0
    if m0.fit_intercept:
        Xa = torch.cat([X, torch.full((n, 1), float(m0.intercept_scaling), dtype=torch.float64, device=dev)], 1)
    else:
        Xa = X
    F1 = Xa.shape[1]
    hmark("lr_xa")
    # per-model sample weights: class weights computed on that model's training rows
    mk = masks.to(torch.float64)
    if m0.class_weight == "balanced":
        cnt1 = (mk * yv[None]).sum(1)
        cnt = torch.stack([mk.sum(1) - cnt1, cnt1], 1)
        cnt, = _allreduce([cnt], group)
        cw = cnt.sum(1, keepdim=True) / (2.0 * cnt)             # [B, 2]
        s = mk * torch.where(yv[None] > 0.5, cw[:, 1:2], cw[:, 0:1])
    else:
        s = mk
    C = float(m0.C)
    l1 = m0.penalty == "l1"
    penal = torch.ones(F1, dtype=torch.uint8, device=dev)
    if not l1 and m0.fit_intercept:
        penal[-1:].zero_()  # lbfgs path: intercept not penalised (a fill: no host→device copy)
    scale = float(m0.intercept_scaling) if (m0.fit_intercept and l1) else 1.0
    if fused:
        LAST_PATH["path"] = "fused"
        hmark("lr_prep")
        return dict(models=models, F=F, scale=scale, fit_intercept=bool(m0.fit_intercept), dev=dev,
                    fused=_launch_fused(Xa, s, ypm, penal, C, l1, max_outer, flags))
    LAST_PATH["path"] = "loop"
    W, n_iter = _solve_loop(Xa, s, ypm, penal, C, l1, max_outer, group)
    for b, m in enumerate(models):
        coef = W[b, :F]
        intercept = W[b, F] * scale if m0.fit_intercept else torch.zeros((), dtype=torch.float64, device=dev)
        m.set_fitted(coef, intercept.reshape(1), [n_iter], F, device=dev)
    return dict(models=models)


def _solve_loop(Xa, s, ypm, penal, C: float, l1: bool, max_outer: int, group=None):
    """The host-driven solve of B models (the arguments of :func:`_launch_fused`): returns
    (W [B, F1], outer iterations).  The batch stops when every model has converged."""
    B, F1, dev = s.shape[0], Xa.shape[1], Xa.device
    pen_f = penal.to(torch.float64)
    W = torch.zeros(B, F1, dtype=torch.float64, device=dev)
    alphas = 0.5 ** torch.arange(8, dtype=torch.float64, device=dev)

    def objective(Z, Wc):
        # Z: [..., n, B] margins; returns [..., B]
        data = C * (s.t() * torch.nn.functional.softplus(-ypm[:, None] * Z)).sum(-2)
        if l1:
            reg = (Wc.abs() * pen_f).sum(-1)
        else:
            reg = 0.5 * (Wc * Wc * pen_f).sum(-1)
        return data, reg

    n_iter = 0
    Z = Xa @ W.t()                                                # [n, B]
    g0norm = None
    for it in range(max_outer):
        n_iter = it + 1
        M = ypm[:, None] * Z
        sig = torch.sigmoid(M)
        coef_g = s.t() * (sig - 1.0) * ypm[:, None]               # [n, B]
        D = s.t() * sig * (1.0 - sig)                             # [n, B]
        H, _, grad = ops.weighted_moments(Xa, D.t(), coef_g.t())   # X̃ᵀDX̃, X̃ᵀr in one kernel
        H = C * H
        grad = C * grad                                           # [B, F1]
        data0 = C * (s.t() * torch.nn.functional.softplus(-M)).sum(0)
        grad, H, data0 = _allreduce([grad, H, data0], group)
        if l1:
            # min-norm subgradient for the stopping rule (an unpenalised coordinate: its gradient)
            sub = torch.where(W != 0, grad + torch.sign(W),
                              torch.sign(grad) * (grad.abs() - 1.0).clamp(min=0.0))
            sub = torch.where(penal.bool()[None], sub, grad)
            gn = sub.abs().sum(1)
            if g0norm is None:
                g0norm = gn.clamp(min=1e-300)
            if bool((gn <= 1e-9 * g0norm).all()):
                break
            Hr = H + 1e-12 * torch.eye(F1, dtype=torch.float64, device=dev)
            if Xa.is_cuda:
                E = ops.ext()
                d = torch.empty_like(W)
                E.l1_qp_cd(B, F1, Hr.contiguous().data_ptr(), grad.contiguous().data_ptr(),
                           W.contiguous().data_ptr(), penal.data_ptr(), 1.0, 200, 1e-12,
                           d.data_ptr(), ops.stream_ptr(dev))
            else:
                d = _host_l1_qp(Hr, grad, W, penal, 1.0)
            delta = (grad * d).sum(1) + ((W + d).abs() * pen_f).sum(1) - (W.abs() * pen_f).sum(1)
        else:
            gfull = grad + W * pen_f
            if g0norm is None:
                g0norm = gfull.abs().sum(1).clamp(min=1e-300)
            if bool((gfull.abs().sum(1) <= 1e-10 * g0norm).all()):
                break
            Hf = H + torch.diag_embed(pen_f.expand(B, -1))
            d = -torch.linalg.solve(Hf, gfull.unsqueeze(-1)).squeeze(-1)
            delta = (gfull * d).sum(1)
        Xd = Xa @ d.t()                                           # [n, B]
        Zc = Z[None] + alphas[:, None, None] * Xd[None]           # [8, n, B]
        Wc = W[None] + alphas[:, None, None] * d[None]            # [8, B, F1]
        dataK = C * (s.t()[None] * torch.nn.functional.softplus(-ypm[None, :, None] * Zc)).sum(1)
        dataK, = _allreduce([dataK], group)
        regK = (Wc.abs() * pen_f).sum(-1) if l1 else 0.5 * (Wc * Wc * pen_f).sum(-1)
        reg0 = (W.abs() * pen_f).sum(-1) if l1 else 0.5 * (W * W * pen_f).sum(-1)
        F0 = data0 + reg0
        FK = dataK + regK                                         # [8, B]
        ok = FK <= F0[None] + 1e-2 * alphas[:, None] * delta[None]
        # largest admissible step (first True); none → smallest step if it decreases, else 0
        first = torch.where(ok.any(0), ok.to(torch.int8).argmax(0), torch.full((B,), 7, device=dev))
        a = alphas[first]
        a = torch.where(ok.any(0) | (FK[7] < F0), a, torch.zeros_like(a))
        if bool((a == 0).all()):
            break
        W = W + a[:, None] * d
        Z = Z + a[None, :] * Xd
        if bool(((a[:, None] * d).abs().max(1).values <= 1e-14 * (1 + W.abs().max(1).values)).all()):
            break
    return W, n_iter
