"""Single-patient (or batched) HF-progression probability from ``hf_predict_model.pkl``.

Same no-argument contract as the reference ``predict_hf.py:1-40``: the 17 clinical
inputs (ordered as the model's columns, ``predict_hf.py:5-27``) default to the
shipped example patient and the probability is printed between ``#`` rules.
Additions: ``--set NAME=VALUE`` overrides, ``--csv`` batched scoring, ``--device``
(``cuda`` runs the gfx950 kernels), ``--model`` path, ``--explain [--background CSV]``
(exact Shapley contribution of every variable, printed after the unchanged probability block),
``--explain-pairs [N]`` (the patient's N strongest variable pairs by exact Shapley interaction value),
``--what-if [NAMES]`` / ``--what-if-csv PATH`` (the patient's risk as one variable moves over its
grid, everything else as entered) and ``--interactions [N]`` (Friedman's H² of variable pairs).
"""
from __future__ import annotations

import argparse
import sys
from collections import OrderedDict

import numpy as np
import torch

# Column order of the shipped model (reference predict_hf.py:5-27).
PATIENT_PARAMS = OrderedDict([
    ("Obstructive HCM", 1),          # 0 or 1
    ("Gender", 1),                   # Male:0 or Female: 1
    ("Syncope", 0),                  # 0 or 1
    ("Dyspnea", 0),                  # 0 or 1
    ("Fatigue", 1),                  # 0 or 1
    ("Presyncope", 0),               # 0 or 1
    ("NYHA_Class", 1),               # 1 or 2
    ("Atrial_Fibrillation", 1),      # 0 or 1
    ("Hypertension", 0),             # 0 or 1
    ("Beta_blocker", 0),             # 0 or 1
    ("Ca_Channel_Blockers", 0),      # 0 or 1
    ("ACEI_ARB", 0),                 # 0 or 1
    ("Coumadin", 0),                 # 0 or 1
    ("Max_Wall_Thick", 13),          # mm, echocardiography
    ("Septal_Anterior_Motion", 0),   # 0 or 1
    ("Mitral_Regurgitation", 0),     # 0..4
    ("Ejection_Fraction", 55),       # %, echocardiography
])


def format_probability(p1: float) -> str:
    bar = "###########################################"
    return f"{bar}\nProbability of progressive HF is: {100 * p1:.2f} %\n{bar}"


def predict_patient(params=None, model_path=None, device="cpu") -> float:
    from ..io.checkpoint import load_checkpoint
    params = PATIENT_PARAMS if params is None else params
    x = torch.tensor([[float(v) for v in params.values()]], dtype=torch.float64)
    clf = load_checkpoint(model_path, device=device)
    p = clf.predict_proba(x.to(device))
    return float(p[0, 1])


def _explainer(a):
    from ..explain import StackExplainer
    from ..io.checkpoint import load_checkpoint
    bg = np.loadtxt(a.background, delimiter=",", ndmin=2) if a.background else None
    return StackExplainer(load_checkpoint(a.model, device=a.device), bg, device=a.device,
                          feature_names=list(PATIENT_PARAMS))


def format_explanation(names, values, phi, base: float, pred: float) -> str:
    """Base value, one line per variable (name, value, phi in percentage points) sorted by
    |phi|, and the sum check ``Σ phi = prediction − base``."""
    lines = [f"Base value (mean risk of the background cohort): {100 * base:.2f} %",
             "Contribution of each variable (percentage points):"]
    for k in sorted(range(len(names)), key=lambda k: -abs(phi[k])):
        lines.append(f"  {names[k]:<24s} {values[k]:>8g} {100 * phi[k]:+10.4f}")
    lines.append(f"Sum of contributions: {100 * sum(phi):+.4f} = {100 * pred:.4f} - {100 * base:.4f}")
    return "\n".join(lines)


def format_importance(names, mean_abs) -> str:
    lines = ["Mean |contribution| of each variable over the cohort (percentage points):"]
    for k in sorted(range(len(names)), key=lambda k: -mean_abs[k]):
        lines.append(f"  {names[k]:<24s} {100 * mean_abs[k]:10.4f}")
    return "\n".join(lines)


def format_pairs(e, top: int, p: int = 0) -> str:
    """The ``top`` strongest pairs of row ``p`` (names, pair effect ``2·Phi_ij`` in percentage points), then
    the sum check: main effects (the diagonal) plus all pair effects = prediction − base."""
    lines = ["Strongest variable pairs for this patient (pair effect 2*Phi_ij, percentage points):"]
    for i, j, eff in e.top(top, p):
        lines.append(f"  {e.feature_names[i]:<24s} {e.feature_names[j]:<24s} {100 * eff:+10.4f}")
    m = e.Phi[p].cpu()
    main = float(torch.diag(m).sum())
    pair = float(torch.triu(m, 1).sum()) * 2.0
    pred, base = float(e.prediction[p]), e.base_value
    lines.append(f"Main effects {100 * main:+.4f} + pair effects {100 * pair:+.4f} = {100 * (main + pair):+.4f}"
                 f" = {100 * pred:.4f} - {100 * base:.4f}")
    return "\n".join(lines)


def format_pair_importance(e, top: int) -> str:
    m = e.mean_abs_pairs().cpu()
    F = m.shape[0]
    pairs = sorted(((i, j, float(m[i, j])) for i in range(F) for j in range(i + 1, F)), key=lambda t: -t[2])
    lines = ["Mean |pair effect| of variable pairs over the cohort (percentage points, strongest first):"]
    for i, j, eff in pairs[:top]:
        lines.append(f"  {e.feature_names[i]:<24s} {e.feature_names[j]:<24s} {100 * eff:10.4f}")
    return "\n".join(lines)


def format_what_if(w, p: int = 0) -> str:
    """One line per variable (current value, risk now, lowest and highest risk along the grid and
    where), sorted by ``highest − lowest``, descending."""
    now = 100 * float(w.prediction[p])
    rows = []
    for i, k in enumerate(w.features):
        risk, grid = w.risk[i][p].cpu(), w.grids[i].cpu()
        lo, hi = int(risk.argmin()), int(risk.argmax())
        rows.append((float(risk[hi]) - float(risk[lo]), i,
                     f"  {w.feature_names[i]:<24s} {float(w.x[p, k]):>8g}  now {now:.2f} %"
                     f"  lowest {100 * float(risk[lo]):.2f} % at {float(grid[lo]):g}"
                     f"  highest {100 * float(risk[hi]):.2f} % at {float(grid[hi]):g}"))
    lines = ["What if one variable changes, everything else as entered (risk along the variable's grid):"]
    return "\n".join(lines + [r[2] for r in sorted(rows, key=lambda r: (-r[0], r[1]))])


def write_what_if_csv(path, w, p: int = 0) -> None:
    with open(path, "w") as f:
        f.write("variable,value,risk,cohort_mean_risk\n")
        for i in sorted(range(len(w.features)), key=lambda i: w.features[i]):   # model order
            grid, risk, coh = w.grids[i].cpu().tolist(), w.risk[i][p].cpu().tolist(), w.cohort[i].cpu().tolist()
            for v, r, c in zip(grid, risk, coh):
                f.write(f"{w.feature_names[i]},{v:.9g},{r:.9g},{c:.9g}\n")


def format_interactions(it, top: int) -> str:
    lines = [f"Friedman's H2 of variable pairs over {it.n_rows} patients (strongest first):"]
    for j, k, h in it.top(top):
        lines.append(f"  {it.feature_names[j]:<24s} {it.feature_names[k]:<24s} {h:.4f}")
    return "\n".join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default=None, help="checkpoint path (default: assets/hf_predict_model.pkl)")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--csv", default=None, help="score every row of a CSV with the 17 columns")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--explain", action="store_true",
                    help="exact Shapley contribution of every variable (with --csv: mean |contribution|)")
    ap.add_argument("--explain-pairs", nargs="?", const=10, default=None, type=int, metavar="N",
                    help="after the --explain block (which it implies), the N (default 10) strongest variable "
                         "pairs by exact Shapley interaction value (with --csv: mean |pair effect|)")
    ap.add_argument("--background", default=None, metavar="CSV",
                    help="background cohort for --explain and --explain-pairs (default: 128 synthetic HF patients; "
                         "on --device cpu each background row costs seconds per patient)")
    ap.add_argument("--what-if", nargs="?", const="", default=None, metavar="NAME,NAME",
                    help="risk of the patient as each named variable (default: all) moves over its grid")
    ap.add_argument("--what-if-csv", default=None, metavar="PATH",
                    help="write the what-if curves: variable,value,risk,cohort_mean_risk")
    ap.add_argument("--interactions", nargs="?", const=10, default=None, type=int, metavar="N",
                    help="the N (default 10) strongest pairs by Friedman's H2, over the --csv cohort "
                         "when given, else over the background (first 512 rows)")
    a = ap.parse_args(argv)
    wi_names = None
    if a.what_if:
        wi_names = [nm for nm in a.what_if.split(",") if nm]
        for nm in wi_names:
            if nm not in PATIENT_PARAMS:
                print(f"unknown clinical variable {nm!r}; expected one of {list(PATIENT_PARAMS)}", file=sys.stderr)
                return 2
    if a.csv:
        from ..io.checkpoint import load_checkpoint
        X = np.loadtxt(a.csv, delimiter=",", ndmin=2)
        clf = load_checkpoint(a.model, device=a.device)
        p = clf.predict_proba(torch.as_tensor(X, dtype=torch.float64, device=a.device))[:, 1]
        for v in p.cpu().tolist():
            print(f"{v:.6f}")
        if a.explain_pairs is not None:
            e = _explainer(a).shap_interaction_values(X)
            print(format_importance(e.feature_names, e.phi.abs().mean(0).cpu().tolist()))
            print(format_pair_importance(e, a.explain_pairs))
        elif a.explain:
            ex = _explainer(a)
            print(format_importance(ex.feature_names, ex.mean_abs(X).cpu().tolist()))
        if a.interactions is not None:
            print(format_interactions(_explainer(a).interaction_strength(X), a.interactions))
        return 0
    params = OrderedDict(PATIENT_PARAMS)
    for kv in a.set:
        k, v = kv.split("=", 1)
        if k not in params:
            print(f"unknown clinical variable {k!r}; expected one of {list(params)}", file=sys.stderr)
            return 2
        params[k] = float(v)
    print(format_probability(predict_patient(params, a.model, a.device)))
    if a.explain or a.explain_pairs is not None:
        vals = [float(v) for v in params.values()]
        ex = _explainer(a)
        e = ex.shap_values([vals]) if a.explain_pairs is None else ex.shap_interaction_values([vals])
        print(format_explanation(e.feature_names, vals, e.phi[0].cpu().tolist(), e.base_value,
                                 float(e.prediction[0])))
        if a.explain_pairs is not None:
            print(format_pairs(e, a.explain_pairs))
    if a.what_if is not None or a.what_if_csv:
        w = _explainer(a).what_if([[float(v) for v in params.values()]], wi_names)
        if a.what_if is not None:
            print(format_what_if(w))
        if a.what_if_csv:
            write_what_if_csv(a.what_if_csv, w)
    if a.interactions is not None:
        print(format_interactions(_explainer(a).interaction_strength(), a.interactions))
    return 0


if __name__ == "__main__":
    sys.exit(main())
