"""Evaluation/reporting (reference ``train_ensemble_public.py:62-90``).

* :func:`classification_report` — sklearn's text layout at the reference's strict
  ``> 0.5`` threshold (``train_ensemble_public.py:63-64``).
* :func:`roc_curve` / :func:`roc_auc` / :func:`precision_recall_curve` /
  :func:`average_precision` — tie-aware, device-resident (sort + cumulative sums);
  ``roc_curve`` drops collinear points like sklearn's ``drop_intermediate=True``.
* :func:`wald_band` — the reference's ``±1.96·sqrt(p(1−p)/n)`` band with ``n`` =
  total held-out rows (``train_ensemble_public.py:74-77,82-85``).
* :func:`bootstrap_ci` — percentile intervals of AUROC, AP and the thresholded rates from the
  nonparametric bootstrap of the held-out rows (``ops.bootstrap_metrics``), plus a ROC band.
* :func:`calibration_ci` / :func:`save_calibration_plots` — Brier, O:E, calibration intercept and
  slope, ECE, the reliability curve and the decision curve with bootstrap intervals
  (``ops.bootstrap_calibration``, the same resamples), and their two figures.
* :func:`compare_ci` / :func:`delong_test` / :func:`save_compare_plot` — paired differences of one
  model against others on the same resamples (``ops.bootstrap_compare``): ΔAUROC, ΔAP, NRI, IDI,
  … with intervals and p-values, DeLong's test, and the models' ROC curves on one axis.
* :func:`save_plots` — headless PNGs of both figures (the reference calls
  ``plt.show()``; its PR axis labels are swapped, ``:86-87`` — kept here with a
  corrected label since the plot is re-drawn, not pixel-copied).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch


def _t(x) -> torch.Tensor:
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))


def _binary_clf_curve(y_true, score):
    y = _t(y_true).to(torch.float64).reshape(-1)
    s = _t(score).to(torch.float64).reshape(-1).to(y.device)
    order = torch.argsort(s, descending=True, stable=True)
    s, y = s[order], y[order]
    distinct = torch.nonzero(s[1:] != s[:-1]).squeeze(1)
    thr_idx = torch.cat([distinct, torch.tensor([y.numel() - 1], device=y.device)])
    tps = torch.cumsum(y, 0)[thr_idx]
    fps = 1 + thr_idx.to(torch.float64) - tps
    return fps, tps, s[thr_idx]


def roc_curve(y_true, score, drop_intermediate: bool = True):
    fps, tps, thr = _binary_clf_curve(y_true, score)
    if drop_intermediate and fps.numel() > 2:
        d2f = fps[2:] - 2 * fps[1:-1] + fps[:-2]
        d2t = tps[2:] - 2 * tps[1:-1] + tps[:-2]
        keep = torch.cat([torch.tensor([True], device=fps.device),
                          (d2f != 0) | (d2t != 0), torch.tensor([True], device=fps.device)])
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    z = torch.zeros(1, dtype=torch.float64, device=fps.device)
    fps = torch.cat([z, fps])
    tps = torch.cat([z, tps])
    thr = torch.cat([torch.full((1,), float("inf"), dtype=torch.float64, device=fps.device), thr])
    fpr = fps / fps[-1] if fps[-1] > 0 else torch.full_like(fps, float("nan"))
    tpr = tps / tps[-1] if tps[-1] > 0 else torch.full_like(tps, float("nan"))
    return fpr, tpr, thr


def auc(x, y) -> float:
    x, y = _t(x).to(torch.float64), _t(y).to(torch.float64)
    return float(torch.trapezoid(y, x))


def roc_auc(y_true, score) -> float:
    fpr, tpr, _ = roc_curve(y_true, score, drop_intermediate=False)
    return auc(fpr, tpr)


def roc_auc_sharded(y_local, score_local, group, bins: int = 1 << 16) -> float:
    """Exact AUROC of rows sharded over a process group without gathering them (SURVEY.md §5.8
    R8): scores are bucketed on a global [min, max] grid and every rank's per-bucket positive /
    negative counts are summed in ONE int64 all-reduce; pairs in different buckets are then
    ordered by their buckets.  Only the rows of buckets holding both classes are all-gathered; the
    pairs inside them are ordered by one sort + binary searches (ties count ½, as sklearn): O(m log m)
    in the gathered rows m, also when every score is tied into one bucket."""
    from ..parallel import dist as pdist
    import torch.distributed as dist
    y = _t(y_local).to(torch.float64).reshape(-1)
    s = _t(score_local).to(torch.float64).reshape(-1).to(y.device)
    dev = s.device
    big = torch.tensor([float("inf")], dtype=torch.float64, device=dev)
    mm = torch.cat([s.min().reshape(1) if s.numel() else big, (-s.max()).reshape(1) if s.numel() else big])
    dist.all_reduce(mm, op=dist.ReduceOp.MIN, group=group)
    lo, hi = float(mm[0]), -float(mm[1])
    width = (hi - lo) / bins if hi > lo else 1.0
    b = torch.clamp(((s - lo) / width).floor().to(torch.int64), 0, bins - 1)
    pos = y > 0.5
    cnt = torch.zeros(2, bins, dtype=torch.int64, device=dev)
    cnt[1].index_add_(0, b[pos], torch.ones_like(b[pos]))
    cnt[0].index_add_(0, b[~pos], torch.ones_like(b[~pos]))
    dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
    neg_c, pos_c = cnt[0].to(torch.float64), cnt[1].to(torch.float64)
    n_pos, n_neg = float(pos_c.sum()), float(neg_c.sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    neg_below = torch.cumsum(neg_c, 0) - neg_c
    cross = float((pos_c * neg_below).sum())
    mixed = (pos_c > 0) & (neg_c > 0)
    mine = mixed[b]
    rows = pdist.all_gather_rows(torch.stack([s[mine], y[mine]], 1), group)
    within = 0.0
    if rows.shape[0]:
        # pairs inside a mixed bucket, by one sort: a positive beats the negatives of its bucket
        # with a lower score (ties ½); negatives of lower buckets are already in ``cross``.
        # Equal scores share a bucket, so the counts below never straddle one.
        sc, pos_r = rows[:, 0], rows[:, 1] > 0.5
        bb = torch.clamp(((sc - lo) / width).floor().to(torch.int64), 0, bins - 1)
        neg_s, _ = torch.sort(sc[~pos_r])
        neg_b, _ = torch.sort(bb[~pos_r])
        sp, bp = sc[pos_r], bb[pos_r]
        less = torch.searchsorted(neg_s, sp, right=False)
        leq = torch.searchsorted(neg_s, sp, right=True)
        lower_buckets = torch.searchsorted(neg_b, bp, right=False)
        within = float((less - lower_buckets).sum()) + 0.5 * float((leq - less).sum())
    return (cross + within) / (n_pos * n_neg)


def precision_recall_curve(y_true, score):
    fps, tps, thr = _binary_clf_curve(y_true, score)
    ps = tps + fps
    precision = torch.where(ps > 0, tps / ps.clamp(min=1), torch.ones_like(tps))
    recall = tps / tps[-1] if tps[-1] > 0 else torch.ones_like(tps)
    # reverse so recall is decreasing, then append (precision=1, recall=0)
    precision = torch.cat([precision.flip(0), torch.ones(1, dtype=torch.float64, device=tps.device)])
    recall = torch.cat([recall.flip(0), torch.zeros(1, dtype=torch.float64, device=tps.device)])
    return precision, recall, thr.flip(0)


def average_precision(y_true, score) -> float:
    precision, recall, _ = precision_recall_curve(y_true, score)
    return float(-torch.sum(torch.diff(recall) * precision[:-1]))


def wald_band(p, n: int):
    p = _t(p).to(torch.float64)
    ci = 1.96 * torch.sqrt(p * (1 - p) / n)
    return p - ci, p + ci


def confusion(y_true, y_pred) -> Tuple[int, int, int, int]:
    yt = _t(y_true).to(torch.float64).reshape(-1) > 0.5
    yp = _t(y_pred).to(torch.float64).reshape(-1).to(yt.device) > 0.5
    tp = int((yt & yp).sum())
    tn = int((~yt & ~yp).sum())
    fp = int((~yt & yp).sum())
    fn = int((yt & ~yp).sum())
    return tn, fp, fn, tp


def classification_report(y_true, y_pred, digits: int = 2) -> str:
    """sklearn ``classification_report`` text for a binary problem."""
    tn, fp, fn, tp = confusion(y_true, y_pred)
    rows = []
    for lab, (t, f_p, f_n) in ((0.0, (tn, fn, fp)), (1.0, (tp, fp, fn))):
        prec = t / (t + f_p) if t + f_p > 0 else 0.0
        rec = t / (t + f_n) if t + f_n > 0 else 0.0
        f1 = 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
        rows.append((str(lab), prec, rec, f1, t + f_n))
    total = sum(r[4] for r in rows)
    acc = (tp + tn) / total if total else 0.0
    macro = [np.mean([r[k] for r in rows]) for k in (1, 2, 3)]
    weighted = [sum(r[k] * r[4] for r in rows) / total for k in (1, 2, 3)]
    headers = ["precision", "recall", "f1-score", "support"]
    width = max(len("weighted avg"), max(len(r[0]) for r in rows), digits)
    head_fmt = "{:>{width}s} " + " {:>9}" * len(headers)
    out = head_fmt.format("", *headers, width=width) + "\n\n"
    row_fmt = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
    for r in rows:
        out += row_fmt.format(r[0], r[1], r[2], r[3], r[4], width=width, digits=digits)
    out += "\n"
    out += ("{:>{width}s} " + " {:>9}" * 2 + " {:>9.{digits}f} {:>9}\n").format(
        "accuracy", "", "", acc, total, width=width, digits=digits)
    out += row_fmt.format("macro avg", *macro, total, width=width, digits=digits)
    out += row_fmt.format("weighted avg", *weighted, total, width=width, digits=digits)
    return out


def evaluate(y_true, proba1) -> Dict[str, float]:
    yy = (_t(proba1) > 0.5).to(torch.float64)
    tn, fp, fn, tp = confusion(y_true, yy)
    return {"auroc": roc_auc(y_true, proba1), "average_precision": average_precision(y_true, proba1),
            "accuracy": (tp + tn) / max(1, tp + tn + fp + fn), "tp": tp, "fp": fp, "tn": tn, "fn": fn}


def _percentile_bounds(v: np.ndarray, qs):
    """``lo, hi, se`` of the replicate values ``v`` (NaN: replicate left out): the quantiles ``qs`` by
    linear interpolation and the standard deviation (ddof 1); NaN without enough replicates."""
    nan = float("nan")
    ok = v[~np.isnan(v)]
    lo, hi = np.quantile(ok, qs) if ok.size else (nan, nan)
    return float(lo), float(hi), float(np.std(ok, ddof=1)) if ok.size > 1 else nan


def _ci_inputs(name: str, y_true, proba1, alpha: float, device):
    """Labels and scores as flat tensors on ``device`` (default: where the scores live), scores floating."""
    y = _t(y_true).reshape(-1)
    p = _t(proba1).reshape(-1)
    dev = torch.device(device) if device is not None else p.device
    y, p = y.to(dev), p.to(dev)
    if not p.is_floating_point():
        p = p.to(torch.float64)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"{name}: alpha = {alpha} outside (0, 1)")
    return y, p


def bootstrap_ci(y_true, proba1, n_boot: int = 2000, seed: int = 2020, alpha: float = 0.05,
                 stratified: bool = False, threshold: float = 0.5, device=None) -> Dict[str, object]:
    """Nonparametric bootstrap of the held-out rows: ``n_boot`` resamples with replacement
    (``ops.bootstrap_metrics``: the fused kernel on a GPU, its torch mirror on the host;
    ``device`` defaults to where ``proba1`` lives), everything recomputed on each.

    For ``auroc``, ``average_precision`` and, at ``proba1 > threshold``, the class-1
    ``precision`` and ``recall``, the ``specificity`` and the ``accuracy``, returns
    ``{"point", "lo", "hi", "se"}``: the point estimate from this module's functions on the
    original sample, the percentile interval bounds at ``alpha/2`` and ``1 − alpha/2`` (linear
    interpolation) and the standard deviation of the replicates.  A degenerate replicate (no
    positive or no negative row drawn; plain mode only) is counted in ``n_degenerate`` and left out
    of every quantile, as is a replicate whose own ratio is 0/0.  ``fpr_grid`` and ``tpr_lo`` /
    ``tpr_median`` / ``tpr_hi`` are the pointwise band of the replicates' ROC curves.  All values
    are Python floats and lists."""
    from .. import ops
    y, p = _ci_inputs("bootstrap_ci", y_true, proba1, alpha, device)
    auroc, ap, _, pn, conf, tpr = ops.bootstrap_metrics(y, p, n_boot, seed=seed, stratified=stratified,
                                                        threshold=threshold)
    auroc, ap, tpr = auroc.cpu().numpy(), ap.cpu().numpy(), tpr.cpu().numpy()
    pn, conf = pn.cpu().numpy(), conf.cpu().numpy().astype(np.float64)
    deg = (pn[:, 0] == 0) | (pn[:, 1] == 0)
    tp, fp, fn, tn = conf.T
    with np.errstate(invalid="ignore", divide="ignore"):
        reps = {"auroc": auroc, "average_precision": ap, "precision": tp / (tp + fp), "recall": tp / (tp + fn),
                "specificity": tn / (tn + fp), "accuracy": (tp + tn) / (tp + fp + fn + tn)}
    # point estimates on host copies: one sort, and the same digits whatever the device
    yh, ph = y.cpu(), p.cpu()
    tn0, fp0, fn0, tp0 = confusion(yh, (ph > threshold).to(torch.float64))

    def ratio(a, b):
        return a / b if b > 0 else float("nan")
    point = {"auroc": roc_auc(yh, ph), "average_precision": average_precision(yh, ph),
             "precision": ratio(tp0, tp0 + fp0), "recall": ratio(tp0, tp0 + fn0),
             "specificity": ratio(tn0, tn0 + fp0), "accuracy": ratio(tp0 + tn0, tp0 + tn0 + fp0 + fn0)}
    qs = [alpha / 2, 1 - alpha / 2]
    out: Dict[str, object] = {"n_boot": int(n_boot), "seed": int(seed), "alpha": float(alpha),
                              "stratified": bool(stratified), "threshold": float(threshold),
                              "n_degenerate": int(deg.sum())}
    for k, v in reps.items():
        lo, hi, se = _percentile_bounds(np.where(deg, np.nan, v), qs)
        out[k] = {"point": float(point[k]), "lo": lo, "hi": hi, "se": se}
    G = tpr.shape[1]
    keep = tpr[~deg]
    band = np.quantile(keep, [qs[0], 0.5, qs[1]], axis=0) if keep.shape[0] else np.full((3, G), np.nan)
    out["fpr_grid"] = [g / (G - 1) for g in range(G)]
    out["tpr_lo"], out["tpr_median"], out["tpr_hi"] = (band[i].tolist() for i in range(3))
    return out


def calibration_ci(y_true, proba1, n_boot: int = 2000, seed: int = 2020, alpha: float = 0.05,
                   stratified: bool = False, bins: int = 10, thresholds: int = 99, device=None) -> Dict[str, object]:
    """Calibration and clinical usefulness of predicted risks with bootstrap intervals
    (``ops.bootstrap_calibration``: the fused kernel on a GPU, its torch mirror on the host, on the
    resamples :func:`bootstrap_ci` uses for the same ``seed`` and ``stratified``).

    ``brier``, ``oe_ratio`` (observed positives / Σp), ``intercept`` and ``slope`` (logistic fit of y on
    logit p: 0 and 1 when calibrated) and ``ece`` (Σ_k (n_k/n)·|observed rate − mean p| over the
    non-empty uniform bins) are ``{"point", "lo", "hi", "se"}`` with the percentile rules of
    :func:`bootstrap_ci`; the point estimates are ``reference.calibration_point`` on the original
    sample.  ``reliability`` holds per bin ``pred_mean``, ``obs``, ``obs_lo``, ``obs_hi`` and ``count``
    (replicates where the bin is empty are left out of its quantiles); ``decision_curve`` holds
    ``thresholds`` t, ``net_benefit`` = TP/n − (FP/n)·t/(1−t) treating p ≥ t, with ``net_benefit_lo`` /
    ``_hi``, and ``net_benefit_all`` (treat everyone).  Replicates without a fit are counted in
    ``n_degenerate`` (one class drawn), ``n_separable`` (no MLE) and ``n_unconverged`` and left out of
    the slope and intercept quantiles only.  ``n_boot = 0`` gives the points with NaN bounds."""
    from .. import ops
    from ..ops import reference as ref
    y, p = _ci_inputs("calibration_ci", y_true, proba1, alpha, device)
    n_boot = int(n_boot)
    if n_boot < 0:
        raise ValueError(f"calibration_ci: n_boot = {n_boot} is negative")
    # n_boot = 0: the empty range of one replicate, so the inputs are validated all the same
    r = ops.bootstrap_calibration(y, p, max(n_boot, 1), seed=seed, stratified=stratified, bins=bins,
                                  thresholds=thresholds, b1=None if n_boot else 0)
    r = {k: v.cpu().numpy() for k, v in zip(ref.CalibrationBootstrap._fields, r)}
    pt = ref.calibration_point(y.cpu(), p.cpu(), bins, thresholds)
    n = int(y.numel())
    t = np.asarray(pt["thresholds"], dtype=np.float64)
    odds = t / (1.0 - t)

    def derive(d):
        pn, bn = np.asarray(d["pn"], dtype=np.float64), np.asarray(d["bin_n"], dtype=np.float64)
        bp, bs = np.asarray(d["bin_pos"], dtype=np.float64), np.asarray(d["bin_sum_p"], dtype=np.float64)
        dc, coef = np.asarray(d["dc"], dtype=np.float64), np.asarray(d["coef"], dtype=np.float64)
        sp = np.asarray(d["sum_p"], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            obs, pred = bp / bn, bs / bn
            ece = np.where(bn > 0, (bn / n) * np.abs(obs - pred), 0.0).sum(-1)
            oe = np.where(sp > 0, pn[..., 0] / sp, np.nan)
        return {"brier": np.asarray(d["brier"], dtype=np.float64), "oe_ratio": oe, "intercept": coef[..., 0],
                "slope": coef[..., 1], "ece": ece, "obs": obs, "pred": pred,
                "nb": dc[..., 0] / n - (dc[..., 1] / n) * odds}
    point, reps = derive(pt), derive(r)
    qs = [alpha / 2, 1 - alpha / 2]
    out: Dict[str, object] = {"n_boot": n_boot, "seed": int(seed), "alpha": float(alpha),
                              "stratified": bool(stratified), "bins": int(bins),
                              "n_degenerate": int((r["status"] == 1).sum()),
                              "n_separable": int((r["status"] == 2).sum()),
                              "n_unconverged": int((r["status"] == 3).sum())}
    for k in ("brier", "oe_ratio", "intercept", "slope", "ece"):
        lo, hi, se = _percentile_bounds(reps[k], qs)
        out[k] = {"point": float(point[k]), "lo": lo, "hi": hi, "se": se}
    ob = [_percentile_bounds(reps["obs"][:, k], qs) for k in range(int(bins))]
    out["reliability"] = {"pred_mean": [float(v) for v in point["pred"]], "obs": [float(v) for v in point["obs"]],
                          "obs_lo": [b[0] for b in ob], "obs_hi": [b[1] for b in ob],
                          "count": [int(v) for v in pt["bin_n"]]}
    nbq = [_percentile_bounds(reps["nb"][:, g], qs) for g in range(t.size)]
    P0, N0 = pt["pn"]
    out["decision_curve"] = {"thresholds": t.tolist(), "net_benefit": point["nb"].tolist(),
                             "net_benefit_lo": [b[0] for b in nbq], "net_benefit_hi": [b[1] for b in nbq],
                             "net_benefit_all": (P0 / n - (N0 / n) * odds).tolist()}
    return out


def _midranks(x: np.ndarray) -> np.ndarray:
    """1-based ranks of ``x``, tied values sharing the mean of their ranks (f64)."""
    order = np.argsort(x, kind="stable")
    xs = x[order]
    first = np.concatenate([[True], xs[1:] != xs[:-1]])
    start = np.nonzero(first)[0]
    end = np.concatenate([start[1:], [x.size]])
    mid = 0.5 * (start + end - 1) + 1.0
    out = np.empty(x.size, dtype=np.float64)
    out[order] = mid[np.cumsum(first) - 1]
    return out


def delong_test(y_true, pa, pb) -> Dict[str, float]:
    """DeLong's test of the difference of two correlated AUROCs (scores ``pa`` and ``pb`` of the same
    rows), by mid-ranks in f64 (Sun and Xu 2014), O(n log n) on the host: with T the mid-ranks of a
    column over all rows, TX over the positives alone and TY over the negatives alone, the structural
    components are V10 = (T[pos] − TX)/N and V01 = 1 − (T[neg] − TY)/P, and the variance of the
    difference is that of ``reference.delong_oracle``.  Returns ``auc_a``, ``auc_b``, ``delta`` =
    ``auc_a − auc_b``, its ``se``, ``z`` = delta/se and the two-sided normal ``p``; ``se = 0`` (equal
    columns) gives ``z = 0`` and ``p = 1``.  All NaN when a class is missing or has one row only."""
    y = np.asarray(_t(y_true).cpu().numpy()).reshape(-1)
    pos = y > 0
    P, N = int(pos.sum()), int((~pos).sum())
    nan = float("nan")
    if P < 2 or N < 2:
        return {k: nan for k in ("auc_a", "auc_b", "delta", "se", "z", "p")}
    V10, V01, aucs = [], [], []
    for s in (pa, pb):
        s = np.asarray(_t(s).cpu().numpy(), dtype=np.float64).reshape(-1)
        tz, tx, ty = _midranks(s), _midranks(s[pos]), _midranks(s[~pos])
        V10.append((tz[pos] - tx) / N)
        V01.append(1.0 - (tz[~pos] - ty) / P)
        aucs.append(float(V10[-1].mean()))
    d10, d01 = V10[0] - V10[1], V01[0] - V01[1]
    var = float(np.var(d10, ddof=1)) / P + float(np.var(d01, ddof=1)) / N
    se = math.sqrt(max(var, 0.0))
    delta = aucs[0] - aucs[1]
    z = delta / se if se > 0 else 0.0
    return {"auc_a": aucs[0], "auc_b": aucs[1], "delta": delta, "se": se, "z": z,
            "p": float(math.erfc(abs(z) / math.sqrt(2.0))) if se > 0 else 1.0}


COMPARE_STATS = ("delta_auroc", "delta_ap", "delta_sensitivity", "delta_specificity", "delta_net_benefit", "nri",
                 "nri_event", "nri_nonevent", "idi", "delta_brier")


def compare_ci(y_true, scores: Dict[str, object], reference: str, n_boot: int = 2000, seed: int = 2020,
               alpha: float = 0.05, stratified: bool = False, threshold: float = 0.5, device=None) -> Dict[str, object]:
    """Is model ``reference`` better than each other column of ``scores`` (name → scores of the same
    held-out rows)?  Every model is scored on the same ``n_boot`` resamples
    (``ops.bootstrap_compare``: the fused kernel on a GPU, its torch mirror on the host; the resamples
    of :func:`bootstrap_ci` for the same ``seed`` and ``stratified``), so each replicate gives a paired
    difference, reference minus comparator.

    ``comparisons[name]`` holds, each as ``{"point", "lo", "hi", "se", "p"}``: ``delta_auroc`` (replicate
    value (a2_ref − a2_m)/(2·P_b·N_b): one division of an exact integer difference), ``delta_ap``,
    ``delta_sensitivity``, ``delta_specificity`` and ``delta_net_benefit`` (TP/n − FP/n·t/(1−t)) at
    ``score > threshold``, ``nri`` = (eu − ed)/P_b + (nd − nu)/N_b with its halves ``nri_event`` and
    ``nri_nonevent`` (eu: events above the threshold under the reference only, ed: under the comparator
    only; nu, nd: the same over non-events, so a positive NRI favours the reference), ``idi`` =
    (mean p_ref over events − mean p_ref over non-events) − (the same for the comparator) and
    ``delta_brier``; ``idi`` and ``delta_brier`` are None when either column leaves [0, 1].  ``point`` is
    computed on host copies of the original sample; ``lo``/``hi``/``se`` follow :func:`bootstrap_ci`;
    ``p = min(1, 2·min(#{Δ_b ≤ 0} + 1, #{Δ_b ≥ 0} + 1)/(B_ok + 1))`` over the B_ok replicates kept.
    Degenerate replicates are counted in ``n_degenerate`` and left out of every quantile.
    ``comparisons[name]["delong"]`` is :func:`delong_test` of the two columns.  ``n_boot = 0`` gives the
    points and DeLong only (NaN bounds and p).  All values are Python floats and lists."""
    from .. import ops
    from ..ops import reference as ref
    if reference not in scores:
        raise ValueError(f"compare_ci: reference {reference!r} is not among the models {list(scores)}")
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"compare_ci: alpha = {alpha} outside (0, 1)")
    n_boot = int(n_boot)
    if n_boot < 0:
        raise ValueError(f"compare_ci: n_boot = {n_boot} is negative")
    names = [reference] + [k for k in scores if k != reference]
    cols = [_t(scores[k]).reshape(-1) for k in names]
    dev = torch.device(device) if device is not None else cols[0].device
    y = _t(y_true).reshape(-1).to(dev)
    S = torch.stack([c.to(dev).to(torch.float64) if not c.is_floating_point() else c.to(dev) for c in cols])
    # n_boot = 0: the empty range of one replicate, so the inputs are validated all the same
    r = ops.bootstrap_compare(y, S, max(n_boot, 1), seed=seed, stratified=stratified, threshold=threshold,
                              b1=None if n_boot else 0)
    r = {k: v.cpu().numpy() for k, v in zip(ref.CompareBootstrap._fields, r)}
    yh = y.cpu().numpy() > 0
    Sh = S.cpu().to(torch.float64).numpy()
    n = int(yh.size)
    t = float(threshold)
    odds = t / (1.0 - t) if 0.0 < t < 1.0 else float("nan")
    in_unit = [bool(((s >= 0) & (s <= 1)).all()) for s in Sh]

    def derive(d, m):
        """The paired differences, column 0 minus column m, from arrays shaped like the op's outputs."""
        pn = d["pn"].astype(np.float64)
        Pb, Nb = pn[:, 0], pn[:, 1]
        cf0, cfm = d["conf"][:, 0].astype(np.float64), d["conf"][:, m].astype(np.float64)
        eu, ed, nu, nd = d["reclass"][:, m].astype(np.float64).T
        s0, sm = d["sums"][:, 0], d["sums"][:, m]
        with np.errstate(invalid="ignore", divide="ignore"):
            ev, ne = (eu - ed) / Pb, (nd - nu) / Nb
            out = {"delta_auroc": (d["a2"][:, 0] - d["a2"][:, m]).astype(np.float64) / (2.0 * Pb * Nb),
                   "delta_ap": d["ap"][:, 0] - d["ap"][:, m],
                   "delta_sensitivity": (cf0[:, 0] - cfm[:, 0]) / Pb,
                   "delta_specificity": (cf0[:, 3] - cfm[:, 3]) / Nb,
                   "delta_net_benefit": (cf0[:, 0] / n - cf0[:, 1] / n * odds) - (cfm[:, 0] / n - cfm[:, 1] / n * odds),
                   "nri": ev + ne, "nri_event": ev, "nri_nonevent": ne,
                   "idi": (s0[:, 0] / Pb - s0[:, 1] / Nb) - (sm[:, 0] / Pb - sm[:, 1] / Nb),
                   "delta_brier": (s0[:, 2] - sm[:, 2]) / n}
        return out

    # the original sample as one "replicate" with every count 1
    P0, N0 = int(yh.sum()), int((~yh).sum())
    hi = Sh > t
    yt = torch.as_tensor(yh.astype(np.float64))
    pt = {"pn": np.array([[P0, N0]]), "a2": np.zeros((1, len(names)), dtype=np.int64),
          "ap": np.array([[average_precision(yt, torch.as_tensor(s)) for s in Sh]]),
          "conf": np.array([[[int((h & yh).sum()), int((h & ~yh).sum()), int((~h & yh).sum()),
                              int((~h & ~yh).sum())] for h in hi]]),
          "reclass": np.array([[[int((hi[0] & ~h & yh).sum()), int((~hi[0] & h & yh).sum()),
                                 int((hi[0] & ~h & ~yh).sum()), int((~hi[0] & h & ~yh).sum())] for h in hi]]),
          "sums": np.array([[[float(s[yh].sum()), float(s[~yh].sum()), float(((s - yh) ** 2).sum())] for s in Sh]])}
    auc0 = [roc_auc(yt, torch.as_tensor(s)) for s in Sh]
    deg = (r["pn"][:, 0] == 0) | (r["pn"][:, 1] == 0)
    qs = [alpha / 2, 1 - alpha / 2]
    nan = float("nan")
    out: Dict[str, object] = {"n_boot": n_boot, "seed": int(seed), "alpha": float(alpha),
                              "stratified": bool(stratified), "threshold": t, "reference": reference,
                              "models": names, "n_degenerate": int(deg.sum()),
                              "auroc": {k: float(a) for k, a in zip(names, auc0)}, "comparisons": {}}
    for m in range(1, len(names)):
        point, reps = derive(pt, m), derive(r, m)
        point["delta_auroc"] = np.array([auc0[0] - auc0[m]])
        cmp: Dict[str, object] = {}
        for k in COMPARE_STATS:
            if k in ("idi", "delta_brier") and not (in_unit[0] and in_unit[m]):
                cmp[k] = None
                continue
            v = np.where(deg, np.nan, reps[k])
            lo, hi_, se = _percentile_bounds(v, qs)
            ok = v[~np.isnan(v)]
            p = min(1.0, 2.0 * min(int((ok <= 0).sum()) + 1, int((ok >= 0).sum()) + 1) / (ok.size + 1)) \
                if ok.size else nan
            cmp[k] = {"point": float(point[k][0]), "lo": lo, "hi": hi_, "se": se, "p": float(p)}
        cmp["delong"] = delong_test(yh, Sh[0], Sh[m])
        out["comparisons"][names[m]] = cmp
    return out


def save_compare_plot(y_true, scores: Dict[str, object], prefix: str) -> str:
    """The ROC curves of all models in ``scores`` (name → scores of the same rows) on one axis,
    ``<prefix>_compare``.  PNG through matplotlib when it is installed, otherwise SVG."""
    y = _t(y_true).cpu()
    colours = ("#1f77b4", "#d62728", "#2ca02c", "#ff7f0e", "#9467bd", "#8c564b", "#e377c2", "#7f7f7f")
    curves = []
    for i, (name, s) in enumerate(scores.items()):
        fpr, tpr, _ = roc_curve(y, _t(s).cpu())
        curves.append((fpr.tolist(), tpr.tolist(), colours[i % len(colours)], "", f"{name} (AUC = {auc(fpr, tpr):.3f})"))
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        return _svg_plot(prefix + "_compare.svg", curves + [([0.0, 1.0], [0.0, 1.0], "black", "5,4", "")], None, None,
                         "False Positive Rate", "True Positive Rate", (0.0, 1.0))
    fig = plt.figure()
    for x, v, colour, _, label in curves:
        plt.plot(x, v, color=colour, label=label)
    plt.plot([0, 1], [0, 1], "k--")
    plt.xlim([0.0, 1.0]); plt.ylim([0.0, 1.0])
    plt.xlabel("False Positive Rate"); plt.ylabel("True Positive Rate"); plt.grid(True); plt.legend()
    path = prefix + "_compare.png"
    fig.savefig(path, dpi=120)
    plt.close(fig)
    return path


def save_importance_plot(imp: Dict[str, object], prefix: str) -> str:
    """Horizontal bars of the mean AUROC importance of every variable with its interval as whiskers,
    most important on top, ``<prefix>_importance``; ``imp`` is the CLI's ``"importance"`` record.  PNG
    through matplotlib when it is installed, otherwise SVG."""
    rows = list(imp["variables"])
    names = [r["name"] for r in rows]
    mean = [r["auroc"]["mean"] for r in rows]
    lo = [r["auroc"]["lo"] for r in rows]
    hi = [r["auroc"]["hi"] for r in rows]
    xlabel = f"fall of AUROC under permutation ({imp['n_repeats']} shuffles)"
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        x0, x1 = min(0.0, min(lo)), max(max(hi), 1e-12)
        W, rowh, left, m = 640, 18, 220, 30
        H = 2 * m + rowh * len(rows)

        def px(v):
            return left + (float(v) - x0) / (x1 - x0) * (W - left - m)
        parts = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{W}" height="{H}" font-family="sans-serif" '
                 f'font-size="11">', f'<rect width="{W}" height="{H}" fill="white"/>',
                 f'<line x1="{px(0):.1f}" y1="{m}" x2="{px(0):.1f}" y2="{H - m}" stroke="black"/>']
        for i, name in enumerate(names):
            yc = m + rowh * i + rowh / 2
            a, b = sorted((px(0.0), px(mean[i])))
            parts.append(f'<text x="{left - 6}" y="{yc + 4:.1f}" text-anchor="end">{name}</text>')
            parts.append(f'<rect x="{a:.1f}" y="{yc - 5:.1f}" width="{b - a:.1f}" height="10" fill="#1f77b4"/>')
            parts.append(f'<line x1="{px(lo[i]):.1f}" y1="{yc:.1f}" x2="{px(hi[i]):.1f}" y2="{yc:.1f}" stroke="black"/>')
        parts.append(f'<text x="{(left + W - m) / 2:.1f}" y="{H - 8}" text-anchor="middle">{xlabel}</text></svg>')
        path = prefix + "_importance.svg"
        with open(path, "w") as f:
            f.write("\n".join(parts))
        return path
    fig = plt.figure(figsize=(7, max(3.0, 0.3 * len(rows) + 1.0)))
    pos = list(range(len(rows)))[::-1]
    err = [[max(0.0, m_ - l) for m_, l in zip(mean, lo)], [max(0.0, h - m_) for m_, h in zip(mean, hi)]]
    plt.barh(pos, mean, xerr=err, color="#1f77b4", ecolor="black", capsize=2)
    plt.yticks(pos, names)
    plt.axvline(0.0, color="black", linewidth=0.8)
    plt.xlabel(xlabel); plt.grid(True, axis="x"); plt.tight_layout()
    path = prefix + "_importance.png"
    fig.savefig(path, dpi=120)
    plt.close(fig)
    return path


def _svg_plot(path: str, curves, band, points, xlabel: str, ylabel: str, ylim) -> str:
    """The approach of :func:`_svg_curve` for several curves on a y-range that need not be [0, 1]:
    ``curves`` = ``(x, y, colour, dash, label)``, ``band`` = ``(x, lo, hi)`` or None, ``points`` =
    ``(x, y)`` markers or None.  NaN vertices are skipped and values are clipped to ``ylim``."""
    W, H, m = 480, 400, 50
    y0, y1 = ylim

    def px(v):
        return m + float(v) * (W - 2 * m)

    def py(v):
        return H - m - (min(y1, max(y0, float(v))) - y0) / (y1 - y0) * (H - 2 * m)

    def pts(xs, ys):
        return " ".join(f"{px(a):.2f},{py(b):.2f}" for a, b in zip(xs, ys) if not (math.isnan(a) or math.isnan(b)))
    parts = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{W}" height="{H}" font-family="sans-serif" font-size="12">',
             f'<rect x="{m}" y="{m}" width="{W - 2 * m}" height="{H - 2 * m}" fill="none" stroke="black"/>']
    if band is not None:
        keep = [(a, b, c) for a, b, c in zip(*band) if not (math.isnan(a) or math.isnan(b) or math.isnan(c))]
        if keep:
            poly = pts([k[0] for k in keep], [k[2] for k in keep]) + " " + \
                pts([k[0] for k in reversed(keep)], [k[1] for k in reversed(keep)])
            parts.append(f'<polygon points="{poly}" fill="grey" fill-opacity="0.2"/>')
    for i, (x, y, colour, dash, label) in enumerate(curves):
        d = f' stroke-dasharray="{dash}"' if dash else ""
        parts.append(f'<polyline points="{pts(x, y)}" fill="none" stroke="{colour}" stroke-width="2"{d}/>')
        parts.append(f'<text x="{m + 10}" y="{m + 18 + 14 * i}" fill="{colour}">{label}</text>')
    if points is not None:
        for a, b in zip(*points):
            if not (math.isnan(a) or math.isnan(b)):
                parts.append(f'<circle cx="{px(a):.2f}" cy="{py(b):.2f}" r="3" fill="#1f77b4"/>')
    for k in range(5):
        parts.append(f'<text x="{px(k / 4) - 8:.1f}" y="{H - m + 16}">{k / 4:g}</text>')
        v = y0 + (y1 - y0) * k / 4
        parts.append(f'<text x="{m - 40}" y="{py(v) + 4:.1f}">{v:.3g}</text>')
    parts += [f'<text x="{W / 2 - 50}" y="{H - 12}">{xlabel}</text>',
              f'<text x="12" y="{H / 2}" transform="rotate(-90 12 {H / 2})">{ylabel}</text>', "</svg>"]
    with open(path, "w") as f:
        f.write("\n".join(parts) + "\n")
    return path


def save_calibration_plots(result, prefix: str) -> Tuple[str, str]:
    """The reliability diagram (``<prefix>_calibration``: the diagonal, the bins' observed rate
    against their mean prediction, the bootstrap band of the observed rate) and the decision curve
    (``<prefix>_decision``: the model, treat-all, treat-none and the model's band) of a
    :func:`calibration_ci` result.  PNG through matplotlib when it is installed, otherwise SVG."""
    rel, dcv = result["reliability"], result["decision_curve"]
    keep = [k for k, c in enumerate(rel["count"]) if c > 0]
    px_, obs = [rel["pred_mean"][k] for k in keep], [rel["obs"][k] for k in keep]
    lo, hi = [rel["obs_lo"][k] for k in keep], [rel["obs_hi"][k] for k in keep]
    has_band = not any(math.isnan(v) for v in lo + hi)
    t, nb, nb_all = dcv["thresholds"], dcv["net_benefit"], dcv["net_benefit_all"]
    nlo, nhi = dcv["net_benefit_lo"], dcv["net_benefit_hi"]
    has_nband = not any(math.isnan(v) for v in nlo + nhi)
    top = max([v for v in nb + nb_all + (nhi if has_nband else []) if not math.isnan(v)] + [0.01])
    ylim = (-0.2 * top, 1.05 * top)     # treat-all dives far below zero: it is clipped there
    label = f"ensemble (slope = {result['slope']['point']:.2f}, Brier = {result['brier']['point']:.3f})"
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        cal = _svg_plot(prefix + "_calibration.svg",
                        [([0.0, 1.0], [0.0, 1.0], "black", "5,4", "ideal"), (px_, obs, "#1f77b4", "", label)],
                        (px_, lo, hi) if has_band else None, (px_, obs), "Mean predicted risk", "Observed rate",
                        (0.0, 1.0))
        dec = _svg_plot(prefix + "_decision.svg",
                        [(t, nb, "#1f77b4", "", "ensemble"), (t, nb_all, "#d62728", "5,4", "treat all"),
                         ([0.0, 1.0], [0.0, 0.0], "black", "2,3", "treat none")],
                        (t, nlo, nhi) if has_nband else None, None, "Threshold probability", "Net benefit", ylim)
        return cal, dec
    fig = plt.figure()
    plt.plot([0, 1], [0, 1], "k--", label="ideal")
    plt.plot(px_, obs, "o-", label=label)
    if has_band:
        plt.fill_between(px_, lo, hi, color="grey", alpha=.2, label="bootstrap band")
    plt.xlim([0.0, 1.0]); plt.ylim([0.0, 1.0])
    plt.xlabel("Mean predicted risk"); plt.ylabel("Observed rate"); plt.grid(True); plt.legend()
    cal = prefix + "_calibration.png"
    fig.savefig(cal, dpi=120)
    plt.close(fig)
    fig = plt.figure()
    plt.plot(t, nb, label="ensemble")
    plt.plot(t, nb_all, "r--", label="treat all")
    plt.plot([0, 1], [0, 0], "k:", label="treat none")
    if has_nband:
        plt.fill_between(t, nlo, nhi, color="grey", alpha=.2, label="bootstrap band")
    plt.xlim([0.0, 1.0]); plt.ylim(list(ylim))
    plt.xlabel("Threshold probability"); plt.ylabel("Net benefit"); plt.grid(True); plt.legend()
    dec = prefix + "_decision.png"
    fig.savefig(dec, dpi=120)
    plt.close(fig)
    return cal, dec


def _svg_curve(path: str, x, y, lo, hi, xlabel: str, ylabel: str, label: str, diagonal: bool, band_x=None) -> str:
    """Minimal dependency-free SVG line plot with a shaded ±band (headless nodes without
    matplotlib): same content as the reference figures (T:66-90).  ``band_x``: abscissae of
    ``lo``/``hi`` when they are not the curve's."""
    W, H, m = 480, 400, 50
    def px(v):
        return m + float(v) * (W - 2 * m)
    def py(v):
        return H - m - float(v) * (H - 2 * m)
    xs = [float(v) for v in x]
    pts = " ".join(f"{px(a):.2f},{py(b):.2f}" for a, b in zip(xs, y))
    if band_x is not None:
        xs = [float(v) for v in band_x]
    band = " ".join(f"{px(a):.2f},{py(min(1.0, max(0.0, float(b)))):.2f}" for a, b in zip(xs, hi))
    band += " " + " ".join(f"{px(a):.2f},{py(min(1.0, max(0.0, float(b)))):.2f}"
                           for a, b in zip(reversed(xs), reversed([float(v) for v in lo])))
    parts = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{W}" height="{H}" font-family="sans-serif" font-size="12">',
             f'<rect x="{m}" y="{m}" width="{W - 2 * m}" height="{H - 2 * m}" fill="none" stroke="black"/>',
             f'<polygon points="{band}" fill="grey" fill-opacity="0.2"/>',
             f'<polyline points="{pts}" fill="none" stroke="#1f77b4" stroke-width="2"/>']
    if diagonal:
        parts.append(f'<line x1="{px(0)}" y1="{py(0)}" x2="{px(1)}" y2="{py(1)}" stroke="black" stroke-dasharray="5,4"/>')
    for t in (0.0, 0.25, 0.5, 0.75, 1.0):
        parts.append(f'<text x="{px(t) - 8:.1f}" y="{H - m + 16}">{t:g}</text>')
        parts.append(f'<text x="{m - 34}" y="{py(t) + 4:.1f}">{t:g}</text>')
    parts += [f'<text x="{W / 2 - 50}" y="{H - 12}">{xlabel}</text>',
              f'<text x="12" y="{H / 2}" transform="rotate(-90 12 {H / 2})">{ylabel}</text>',
              f'<text x="{m + 10}" y="{m + 18}">{label}</text>', "</svg>"]
    with open(path, "w") as f:
        f.write("\n".join(parts) + "\n")
    return path


def save_plots(y_true, proba1, prefix: str, band=None) -> Optional[Tuple[str, str]]:
    """ROC and PR figures with the Wald ±band (reference T:66-90; saved instead of shown).
    PNG through matplotlib when it is installed, otherwise self-contained SVG.  ``band`` =
    ``(fpr_grid, tpr_lo, tpr_hi)`` from :func:`bootstrap_ci` is shaded on the ROC figure in place
    of the Wald band; the PR figure keeps the Wald band (there is no bootstrap PR band)."""
    if band is not None:
        band = tuple(np.asarray(b, dtype=np.float64) for b in band)
        if any(np.isnan(b).any() for b in band):
            band = None     # every replicate degenerate: nothing to shade
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        y = _t(y_true).cpu()
        p = _t(proba1).cpu()
        n = y.numel()
        fpr, tpr, _ = roc_curve(y, p)
        lo, hi = wald_band(tpr, n) if band is None else band[1:]
        roc = _svg_curve(prefix + "_roc.svg", fpr, tpr, lo, hi, "False Positive Rate", "True Positive Rate",
                         f"ensemble (AUC = {auc(fpr, tpr):.2f})", True, band_x=None if band is None else band[0])
        prec, rec, _ = precision_recall_curve(y, p)
        lo, hi = wald_band(prec, n)
        pr = _svg_curve(prefix + "_pr.svg", rec, prec, lo, hi, "Recall", "Precision",
                        f"ensemble (AP = {average_precision(y, p):.2f})", False)
        return roc, pr
    y = _t(y_true).cpu()
    p = _t(proba1).cpu()
    n = y.numel()
    fpr, tpr, _ = roc_curve(y, p)
    lo, hi = wald_band(tpr, n)
    fig = plt.figure()
    plt.plot(fpr.numpy(), tpr.numpy(), label=f"ensemble (AUC = {auc(fpr, tpr):.2f})")
    plt.plot([0, 1], [0, 1], "k--")
    if band is None:
        plt.fill_between(fpr.numpy(), lo.numpy(), hi.numpy(), color="grey", alpha=.2, label=r"$\pm$ 1 std. dev.")
    else:
        plt.fill_between(band[0], band[1], band[2], color="grey", alpha=.2, label="bootstrap band")
    plt.xlim([0.0, 1.0]); plt.ylim([0.0, 1.0])
    plt.xlabel("False Positive Rate"); plt.ylabel("True Positive Rate"); plt.grid(True); plt.legend()
    roc_path = prefix + "_roc.png"
    fig.savefig(roc_path, dpi=120)
    plt.close(fig)
    prec, rec, _ = precision_recall_curve(y, p)
    lo, hi = wald_band(prec, n)
    fig = plt.figure()
    plt.plot(rec.numpy(), prec.numpy(), label=f"ensemble (AP = {average_precision(y, p):.2f})")
    plt.fill_between(rec.numpy(), lo.numpy(), hi.numpy(), color="grey", alpha=.2, label=r"$\pm$ 1 std. dev.")
    plt.xlim([0.0, 1.0]); plt.ylim([0.0, 1.0])
    plt.xlabel("Recall"); plt.ylabel("Precision"); plt.grid(True); plt.legend()
    pr_path = prefix + "_pr.png"
    fig.savefig(pr_path, dpi=120)
    plt.close(fig)
    return roc_path, pr_path
