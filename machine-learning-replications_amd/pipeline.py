"""End-to-end model development (reference ``train_ensemble_public.py:33-90``).

``develop(X_dev, y_dev, X_sel, y_sel, names)``:
KNN-impute (fit on dev, applied to both) → LassoCV/SelectFromModel top-17 →
stacking fit on dev → held-out ``predict_proba`` → report / AUROC / AP (+ plots).
Every step runs on the tensors' device; with ``group`` the dev rows are sharded
across ranks (see :mod:`hfens.parallel`).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from .config import EnsembleConfig, build_estimators, build_selector
from .models.imputer import KNNImputer
from .utils import metrics
from .utils.timing import StageTimer


# Multi-process policy for the stacking fit:
#   "dp"   — rows stay sharded; LassoCV moments, GBDT int64 histograms and LR Newton moments are
#            all-reduced every step, the SVC fits are spread over ranks.
#   "task" — after the (sharded) KNN imputation the imputed development rows are all-gathered
#            once; every rank then runs the cheap, latency-bound fits (LassoCV, GBDT, L1-LR, meta)
#            on the full rows itself and only the 36 SMO problems — the critical path — are
#            spread over the ranks (one SUM all-reduce of the solutions).  Identical results to a
#            single process, three collectives per fit instead of hundreds.
#   "auto" — task below HFENS_TASK_MAX_ROWS development rows (small data: the DP collectives'
#            latency exceeds the compute they split), dp above.
DP_POLICY = os.environ.get("HFENS_DP_POLICY", "auto")
TASK_MAX_ROWS = int(os.environ.get("HFENS_TASK_MAX_ROWS", str(1 << 18)))
AUX_STREAM = os.environ.get("HFENS_AUX_STREAM", "1") != "0"   # held-out imputation on a side stream
PLAN_AHEAD = os.environ.get("HFENS_PLAN_AHEAD", "1") != "0"   # stacking bookkeeping under the LassoCV path


def choose_policy(n_total: int) -> str:
    if DP_POLICY in ("dp", "task"):
        return DP_POLICY
    return "task" if n_total <= TASK_MAX_ROWS else "dp"


def _plan_start(clf, y: torch.Tensor):
    """Start the stacking fit's label-only plan (stack_trainer.plan_stacking) from the device labels.
    Returns (``join()`` → the plan, native).  native: the label work already runs natively on a helper
    thread (GIL released) while the caller launches the imputation and the LassoCV prelude, and the
    join only collects it — otherwise ``join`` computes the plan on the calling thread."""
    from .models.stack_trainer import plan_stacking, plan_stacking_start
    # (pinned, non-blocking copy + event: the labels' copy is done at once on an idle device)
    y_pin = torch.empty(y.shape[0], dtype=torch.float64, pin_memory=True)
    y_pin.copy_(y, non_blocking=True)
    y_ev = torch.cuda.Event()
    y_ev.record()
    y_ev.synchronize()
    y_np = y_pin.numpy().copy()
    join = plan_stacking_start(clf, y_np)
    if join is not None:
        return join, True
    return (lambda: plan_stacking(clf, y_np)), False


def _prelaunch(clf, sel, X_dev, y_dev, plan, svc_group):
    """The stacking fit (SVC batch, then the GBC / L1-LR batches and the meta model) enqueued from the
    selector's DEVICE column list — speculative (lasso.SPECULATE: the smallest-alpha refit's
    selection, enqueued before the LassoCV's grid read, lasso.EARLY_SPEC) — while the device still
    imputes / runs the LassoCV path.  Returns stack_trainer.prelaunch_stack's state, or None."""
    from .models.stack_trainer import prelaunch_bases, prelaunch_stack
    from .utils.timing import hmark
    pre = None
    cols = getattr(sel, "cols_dev_", None)
    if cols is not None and plan is not None:
        pre = prelaunch_stack(clf, X_dev, cols, y_dev, plan, svc_group=svc_group)
        if pre is not None:
            pre["speculative"] = bool(getattr(sel, "cols_speculative_", False))
            pre["cols_host"] = getattr(sel, "cols_host_", None)
    prelaunch_bases(pre)
    hmark("bases_prelaunched")
    return pre


@dataclass
class DevelopResult:
    model: object
    selected: np.ndarray
    selected_names: List[str]
    proba_sel: torch.Tensor
    report: str
    scores: Dict[str, float]
    timer: StageTimer
    n_train: int = 0
    bases_sel: Optional[torch.Tensor] = None      # keep_bases: [n_sel, 3] f64 base-learner P(class 1)
    base_names: Optional[List[str]] = None
    X_sel: Optional[torch.Tensor] = None          # keep_heldout: [n_sel, F] f64 imputed, selected held-out columns


def develop(X_dev, y_dev, X_sel, y_sel, names, device="cpu", cfg: Optional[EnsembleConfig] = None,
            timer: Optional[StageTimer] = None, group=None, evaluate: bool = True,
            keep_bases: bool = False, keep_heldout: bool = False) -> DevelopResult:
    cfg = cfg or EnsembleConfig()
    timer = timer or StageTimer(enabled=True, device=device if str(device).startswith("cuda") else None)
    dev = torch.device(device)
    X_dev = torch.as_tensor(np.asarray(X_dev) if not isinstance(X_dev, torch.Tensor) else X_dev,
                            dtype=torch.float64).to(dev)
    y_dev = torch.as_tensor(np.asarray(y_dev) if not isinstance(y_dev, torch.Tensor) else y_dev,
                            dtype=torch.float64).to(dev)
    X_sel = torch.as_tensor(np.asarray(X_sel) if not isinstance(X_sel, torch.Tensor) else X_sel,
                            dtype=torch.float64).to(dev)
    y_sel = torch.as_tensor(np.asarray(y_sel) if not isinstance(y_sel, torch.Tensor) else y_sel,
                            dtype=torch.float64).to(dev)
    if dev.type == "cuda":
        from . import runtime
        runtime.init_fit_streams(dev)
    task = False
    if group is not None:
        from .parallel import dist as pdist
        task = choose_policy(pdist.all_reduce_int(X_dev.shape[0], group)) == "task"
    clf = build_estimators(cfg)
    # (task policy: every rank holds every row after the imputation, so the single-process critical
    # path applies — the plan, the speculative LassoCV refit and the stacking prelaunch; only the SMO
    # problems are spread over the ranks, by the one all-reduce inside the prelaunched SVC batch)
    svc_group = group if task else None
    # the stacking fit's label-only bookkeeping (folds, SVC problem expansions, Platt column maps)
    # is computed on the host while the device imputes and runs the LassoCV path (_plan_start)
    plan, plan_join, plan_native = None, None, False
    y_full = None
    if group is None and dev.type == "cuda" and PLAN_AHEAD:
        plan_join, plan_native = _plan_start(clf, y_dev)
    elif task:
        # the labels are gathered first (they do not wait for the imputation), so every rank plans
        # from the same full labels while the device imputes, as in one process
        y_full = pdist.all_gather_rows(y_dev[:, None], group)[:, 0]
        if dev.type == "cuda" and PLAN_AHEAD:
            plan_join, plan_native = _plan_start(clf, y_full)
    from .utils.timing import hmark, dmark, dmarks_flush
    hmark("develop")
    dmark("develop")
    with timer.stage("impute"):
        if group is None:
            imputer = KNNImputer(n_neighbors=cfg.knn_neighbors).fit(X_dev)
        else:
            imputer = KNNImputer(n_neighbors=cfg.knn_neighbors).fit(pdist.all_gather_rows(X_dev, group))
        # this rank's rows (the O(n²) donor search is sharded) and the held-out rows, planned from
        # ONE host read; the held-out rows are only needed for the evaluation, so on the GPU
        # their donor search runs on a side stream, overlapped with LassoCV and the stacking fit
        # (joined before the evaluation below)
        aux = None
        if dev.type == "cuda" and AUX_STREAM:
            aux = runtime.stream(dev, "aux")
        hmark("imputer_fit")
        run_sel = None
        if aux is not None and (group is None or task):
            # the held-out rows' planning and launch (host numpy, ≈ 1 ms at 10k rows) are deferred
            # into the LassoCV path's device time below, off the host's critical path
            (X_dev, _), run_sel = imputer.transform_many([X_dev, X_sel], streams=[None, aux], defer=True)
        else:
            X_dev, X_sel = imputer.transform_many([X_dev, X_sel], streams=[None, aux])
        hmark("impute_enqueued")
        if task:
            X_dev = pdist.all_gather_rows(X_dev, group)
            y_dev = y_full
    fit_group = None if task else group
    sel = build_selector(cfg)
    if plan_join is not None and not plan_native:
        # the plan now, on this thread, while the device imputes (LassoCV's prelude reads wait for
        # the imputation anyway): it is ready before the LassoCV path is launched.  (The native plan
        # runs on its helper thread meanwhile and is joined under the path, in early_overlap)
        plan = plan_join()
        hmark("plan_ready")
    with timer.stage("select"):
        pre = None

        def early_overlap():
            # under the LassoCV's early speculation: the whole stacking fit enqueued on the
            # selector's (speculative) device column list, the SVC batch first
            nonlocal plan, pre
            if plan is None:
                plan = plan_join()
            pre = _prelaunch(clf, sel, X_dev, y_dev, plan, svc_group)

        def overlap():
            # under the CV paths, after the stacking fit: the held-out rows are needed last
            run_sel()
            hmark("heldout_impute_enqueued")
        sfm = sel.fit(X_dev, y_dev, group=fit_group, overlap=overlap if run_sel is not None else None,
                      early_overlap=early_overlap if plan_join is not None else None)
        if run_sel is not None:
            X_sel = run_sel()[1]      # (already run inside the LassoCV path; a no-op then)
        hmark("lasso_fit")
        dmark("lasso_fit")
        mask = sfm.get_support()
        mt = torch.as_tensor(mask, device=dev)
        X_dev_optm = X_dev[:, mt]
        fn_new = [n for n, m in zip(names, mask) if m]
        hmark("selected")
    if pre is not None:
        plan = dict(plan, prelaunch=pre, cols=np.nonzero(mask)[0])
    clf.fit(X_dev_optm, y_dev, timer=timer, group=fit_group, svc_group=svc_group, plan=plan)
    dmark("stack_fit")
    hmark("stack_fit")
    if aux is not None:
        # join the side stream while the imputer and X_sel are alive (their blocks are not reused
        # by the main stream before this point)
        torch.cuda.current_stream(dev).wait_stream(aux)
    X_sel_optm = X_sel[:, mt]
    proba = None
    report = ""
    scores: Dict[str, float] = {}
    if evaluate:
        with timer.stage("predict_select"):
            proba = clf.predict_proba(X_sel_optm)[:, 1]
        yy = (proba > 0.5).to(torch.float64)
        if group is not None:
            from .parallel import dist as pdist
            proba_all = pdist.all_gather_rows(proba[:, None], group)[:, 0]
            ysel_all = pdist.all_gather_rows(y_sel[:, None], group)[:, 0]
            yy_all = (proba_all > 0.5).to(torch.float64)
        else:
            proba_all, ysel_all, yy_all = proba, y_sel, yy
        report = metrics.classification_report(ysel_all, yy_all)
        # (the held-out rows are already gathered for the report, so the AUROC comes from them;
        # metrics.roc_auc_sharded is the R8 path for callers that keep scores sharded)
        scores = metrics.evaluate(ysel_all, proba_all)
    bases, base_names = None, None
    if keep_bases and evaluate:
        bases = clf.transform(X_sel_optm)
        base_names = [name for name, _ in clf.estimators]
    hmark("develop_end")
    dmarks_flush()
    n_train = X_dev.shape[0]
    if fit_group is not None:
        from .parallel import dist as pdist
        n_train = pdist.all_reduce_int(n_train, group)
    return DevelopResult(clf, mask, fn_new, proba, report, scores, timer, n_train, bases, base_names,
                         X_sel_optm if keep_heldout else None)
