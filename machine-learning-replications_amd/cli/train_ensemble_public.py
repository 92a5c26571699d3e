"""Model development entry point (reference ``train_ensemble_public.py``).

No-argument behaviour follows the reference: load ``develop_data.mat`` and
``model_select_data.mat`` from the directory of the script that was run
(``T:33-39``: ``os.path.dirname(__file__)``), print the selected feature names and
count (``T:56-59``), fit the stack, print the held-out ``classification_report`` at
``> 0.5`` (``T:62-64``) and ALWAYS draw the ROC/PR curves with Wald bands
(``T:66-90``; written as ``hf_roc.png`` / ``hf_pr.png`` in the working directory
instead of ``plt.show()`` on a headless node, ``--no-plots`` to skip).  Those
``.mat`` files are private, so when they are absent a Table-S1-shaped synthetic
cohort is generated (``--rows``, ``--features``).  Extras: ``--device cuda``, ``--save-model``
(writes the sklearn-0.23.2 ``.pkl`` layout that ``predict_hf.py`` reads),
``--timings``, ``--bootstrap N`` (percentile confidence intervals of the held-out AUROC, AP
and thresholded rates from N bootstrap resamples, and a bootstrap band on the ROC figure;
``--bootstrap-seed``, ``--stratified``), ``--calibration`` (Brier, O:E, calibration intercept and
slope, ECE and net benefit of the held-out risks, a reliability and a decision-curve figure;
intervals from the same resamples with ``--bootstrap N``), ``--compare`` (is the stack better than each of
its base learners: paired ΔAUROC, ΔAP, NRI and IDI on the same resamples, DeLong's test and one ROC
figure of all four models; points and DeLong only with ``--bootstrap 0``), ``--importance [R]`` (permutation
importance of the selected variables on the held-out rows: the fall of AUROC and AP and the rise of the
Brier score over R shuffles, ``--importance-seed``, and a bar figure); under ``torchrun`` the development rows are sharded
over ranks.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def main(argv=None, script_dir=None) -> int:
    ap = argparse.ArgumentParser(description="train the HF-progression stacking ensemble")
    ap.add_argument("--data-dir", default=None,
                    help="directory with develop_data.mat / model_select_data.mat (default: the script's)")
    ap.add_argument("--rows", type=int, default=713, help="synthetic rows per set (when no .mat files)")
    ap.add_argument("--features", type=int, default=64, help="synthetic candidate features")
    ap.add_argument("--seed", type=int, default=2020)
    ap.add_argument("--device", default=None, help="cpu | cuda (default: cuda if available)")
    ap.add_argument("--save-model", default=None, help="write a 0.23.2-layout hf_predict_model.pkl")
    ap.add_argument("--plots", default="hf", help="PNG prefix for the ROC/PR plots (default 'hf')")
    ap.add_argument("--no-plots", action="store_true", help="skip the ROC/PR figures")
    ap.add_argument("--timings", action="store_true")
    ap.add_argument("--json", default=None, help="append a JSON result line to this file")
    ap.add_argument("--lr-optimum", action="store_true",
                    help="solve 'lg' to its exact optimum on the device instead of reproducing liblinear's "
                         "default-tolerance iterate and seed draw (the reference's T:31/T:46 behaviour)")
    ap.add_argument("--bootstrap", type=int, default=0, metavar="N",
                    help="bootstrap the held-out rows N times: confidence intervals and a ROC band (default 0 = off)")
    ap.add_argument("--bootstrap-seed", type=int, default=2020)
    ap.add_argument("--stratified", action="store_true",
                    help="resample positives and negatives separately (class totals fixed)")
    ap.add_argument("--calibration", action="store_true",
                    help="report Brier, O:E, calibration intercept/slope, ECE and net benefit of the held-out "
                         "risks, with two figures; with --bootstrap N, their confidence intervals")
    ap.add_argument("--compare", action="store_true",
                    help="compare the stack with each base learner on the held-out rows: paired differences "
                         "(AUROC, AP, NRI, IDI, ...) with DeLong's test and one ROC figure; with --bootstrap N, "
                         "their confidence intervals and p-values from the same resamples")
    ap.add_argument("--calibration-bins", type=int, default=10)
    ap.add_argument("--calibration-thresholds", type=int, default=99)
    ap.add_argument("--importance", type=int, nargs="?", const=30, default=0, metavar="R",
                    help="permutation importance of the selected variables on the held-out rows: R shuffles "
                         "(30 when given without a value), the same ones for every variable; the fall of AUROC "
                         "and AP and the rise of the Brier score (default 0 = off)")
    ap.add_argument("--importance-seed", type=int, default=2020)
    a = ap.parse_args(argv)
    if a.bootstrap < 0:
        ap.error("--bootstrap must be >= 0")
    if a.importance < 0:
        ap.error("--importance must be >= 0")
    if a.no_plots:
        a.plots = None

    import torch
    from ..io.mat import load_data, names_list
    from ..io.synth import make_dev_select
    from ..pipeline import develop
    from ..utils import metrics
    from ..parallel import dist as pdist

    group, rank, world = pdist.init_from_env()
    device = a.device or ("cuda" if torch.cuda.is_available() else "cpu")
    if device == "cuda":
        device = str(pdist.rank_device())
        torch.cuda.set_device(torch.device(device))
    # T:33-34: the .mat files sit next to the script that was run (not the working directory)
    data_dir = a.data_dir or script_dir or os.path.dirname(os.path.abspath(sys.argv[0] or "."))
    dev_path = os.path.join(data_dir, "develop_data.mat")
    sel_path = os.path.join(data_dir, "model_select_data.mat")
    if os.path.exists(dev_path) and os.path.exists(sel_path):
        X_dev, y_dev, names = load_data(dev_path)
        X_sel, y_sel, _ = load_data(sel_path)
        names = names_list(names)
        source = "mat"
    else:
        X_dev, y_dev, X_sel, y_sel, names = make_dev_select(a.rows, a.features, seed=a.seed)
        source = "synthetic"
        if rank == 0:
            print(f"[hfens] {dev_path} not found: using a synthetic Table-S1 cohort "
                  f"({a.rows} rows x {a.features} features per set)")
    if group is not None:
        X_dev, y_dev = pdist.shard_rows(X_dev, rank, world), pdist.shard_rows(y_dev, rank, world)
        X_sel, y_sel = pdist.shard_rows(X_sel, rank, world), pdist.shard_rows(y_sel, rank, world)
    from ..config import EnsembleConfig
    cfg = EnsembleConfig(liblinear_exact=not a.lr_optimum)
    # T:31: numpy's GLOBAL generator seeded with init_rs — liblinear's seeds ('lg', random_state=None)
    # are drawn from it, six times, in the stacking fit's order
    np.random.seed(cfg.seed)
    res = develop(X_dev, y_dev, X_sel, y_sel, names, device=device, group=group, cfg=cfg,
                  **({"keep_bases": True} if a.compare else {}),
                  **({"keep_heldout": True} if a.importance else {}))
    if a.importance:
        # what the stack itself sees: the imputed, selected held-out columns (gathered on EVERY rank)
        X_imp = res.X_sel
        y_imp = torch.as_tensor(y_sel, device=X_imp.device)
        if group is not None:
            X_imp = pdist.all_gather_rows(X_imp, group)
            y_imp = pdist.all_gather_rows(y_imp.to(X_imp.dtype)[:, None], group)[:, 0]
    if a.plots or a.bootstrap or a.calibration or a.compare:
        # collectives on EVERY rank (before the rank-0 block); only rank 0 draws
        p_all = res.proba_sel
        y_all = torch.as_tensor(y_sel, device=p_all.device)
        if group is not None:
            p_all = pdist.all_gather_rows(p_all[:, None], group)[:, 0]
            y_all = pdist.all_gather_rows(y_all.to(p_all.dtype)[:, None], group)[:, 0]
        if a.compare:
            bases_all = res.bases_sel
            if group is not None:
                bases_all = pdist.all_gather_rows(bases_all, group)
    if rank == 0:
        print("Important Features")
        print(np.array(res.selected_names, dtype=object))
        print("number of features = ", len(res.selected_names))
        print(res.report)
        print(f"AUROC = {res.scores['auroc']:.4f}   AP = {res.scores['average_precision']:.4f}")
        ci = None
        if a.bootstrap:
            ci = metrics.bootstrap_ci(y_all, p_all, n_boot=a.bootstrap, seed=a.bootstrap_seed,
                                      stratified=a.stratified)
            lvl = f"{100 * (1 - ci['alpha']):g}% CI"

            def fmt(k):
                return f"{ci[k]['point']:.4f} ({lvl} {ci[k]['lo']:.4f}\u2013{ci[k]['hi']:.4f})"
            print(f"AUROC = {fmt('auroc')}   AP = {fmt('average_precision')}")
            print("   ".join(f"{k} = {fmt(k)}" for k in ("precision", "recall", "specificity", "accuracy")))
        cal = None
        if a.calibration:
            cal = metrics.calibration_ci(y_all, p_all, n_boot=a.bootstrap, seed=a.bootstrap_seed,
                                         stratified=a.stratified, bins=a.calibration_bins,
                                         thresholds=a.calibration_thresholds)
            lvl = f"{100 * (1 - cal['alpha']):g}% CI"

            def cell(v, digits=4):
                s = f"{v['point']:.{digits}f}"
                return s + (f" ({lvl} {v['lo']:.{digits}f}–{v['hi']:.{digits}f})" if a.bootstrap else "")
            print("   ".join(f"{name} = {cell(cal[k])}" for name, k in (
                ("Brier", "brier"), ("O:E", "oe_ratio"), ("intercept", "intercept"), ("slope", "slope"),
                ("ECE", "ece"))))
            dcv = cal["decision_curve"]
            at = []
            for want in (0.1, 0.2, 0.5):
                g = min(range(len(dcv["thresholds"])), key=lambda i: abs(dcv["thresholds"][i] - want))
                nb = {"point": dcv["net_benefit"][g], "lo": dcv["net_benefit_lo"][g], "hi": dcv["net_benefit_hi"][g]}
                at.append(f"t = {dcv['thresholds'][g]:.2f}: {cell(nb)} vs treat-all {dcv['net_benefit_all'][g]:.4f}")
            print("net benefit   " + "   ".join(at))
        comp = None
        if a.compare:
            models = {"stack": p_all.to(bases_all.dtype)}
            models.update({name: bases_all[:, k] for k, name in enumerate(res.base_names)})
            comp = metrics.compare_ci(y_all, models, "stack", n_boot=a.bootstrap, seed=a.bootstrap_seed,
                                      stratified=a.stratified)
            lvl = f"{100 * (1 - comp['alpha']):g}% CI"

            def diff(v, delong=None):
                if v is None:
                    return "n/a"
                notes = [f"{lvl} {v['lo']:+.4f}–{v['hi']:+.4f}", f"p = {v['p']:.4f}"] if a.bootstrap else []
                if delong is not None:
                    notes.append(f"DeLong p = {delong['p']:.4f}")
                return f"{v['point']:+.4f}" + (f" ({', '.join(notes)})" if notes else "")
            for name in res.base_names:
                c = comp["comparisons"][name]
                print(f"stack vs {name}: ΔAUROC {diff(c['delta_auroc'], c['delong'])}   ΔAP {diff(c['delta_ap'])}"
                      f"   NRI {diff(c['nri'])}   IDI {diff(c['idi'])}")
        imp = None
        if a.importance:
            from .. import ops
            from ..explain import PermutationImportance
            pk = res.model._packed_stack(X_imp.device)
            if pk is None:
                ap.error("--importance needs the HF-shaped stack (scaler+SVC, GBC, LR -> LR)")
            pi = PermutationImportance(list(res.selected_names), *ops.permutation_importance(
                X_imp, y_imp, pk, a.importance, seed=a.importance_seed))
            lo, hi = (v.cpu().tolist() for v in pi.interval("auroc", 0.95))
            sd = pi.std("auroc").cpu().tolist()
            m_ap, m_br = pi.mean("ap").cpu().tolist(), pi.mean("brier").cpu().tolist()
            print(f"permutation importance ({a.importance} shuffles of {X_imp.shape[0]} held-out rows; baseline "
                  f"AUROC {pi.baseline['auroc']:.4f}   AP {pi.baseline['ap']:.4f}   Brier {pi.baseline['brier']:.4f})")
            width = max(len(nm) for nm in pi.names)
            rows = []
            for k, name, m in pi.top(len(pi.names)):
                print(f"  {name:<{width}s}  ΔAUROC {m:+.4f} ± {sd[k]:.4f} (95% {lo[k]:+.4f}–{hi[k]:+.4f})"
                      f"   ΔAP {m_ap[k]:+.4f}   ΔBrier {m_br[k]:+.4f}")
                rows.append({"name": name, "auroc": {"mean": m, "sd": sd[k], "lo": lo[k], "hi": hi[k]},
                             "ap": m_ap[k], "brier": m_br[k]})
            imp = {"n_repeats": a.importance, "seed": a.importance_seed, "baseline": pi.baseline, "variables": rows}
        if a.timings:
            print(res.timer.table())
        if a.plots and imp is not None:
            print("importance plot:", metrics.save_importance_plot(imp, a.plots))
        if a.plots:
            band = (ci["fpr_grid"], ci["tpr_lo"], ci["tpr_hi"]) if ci else None
            print("plots:", metrics.save_plots(y_all, p_all, a.plots, band=band))
            if cal is not None:
                print("calibration plots:", metrics.save_calibration_plots(cal, a.plots))
            if comp is not None:
                print("comparison plot:", metrics.save_compare_plot(y_all, models, a.plots))
        if a.save_model:
            from ..io.checkpoint import save_checkpoint
            model = res.model
            model.to("cpu")
            save_checkpoint(model, a.save_model)
            print(f"saved {a.save_model}")
        if a.json:
            with open(a.json, "a") as f:
                line = {"source": source, "n_train": res.n_train, "scores": res.scores,
                        "timings": dict(res.timer.times), "world_size": world}
                if ci is not None:
                    line["bootstrap"] = ci
                if cal is not None:
                    line["calibration"] = cal
                if comp is not None:
                    line["compare"] = comp
                if imp is not None:
                    line["importance"] = imp
                f.write(json.dumps(line) + "\n")
    pdist.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
