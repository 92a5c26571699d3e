"""Time of the fused permutation importance against the composed baseline and a scikit-learn loop.

All paths compute the importances of the same cohort (``--rows`` × the checkpoint's columns ×
``--repeats`` shuffles, the same permutations) on the shipped checkpoint, in one process:

* fused    — ``ops.permutation_importance`` (``stack_permute`` + ``rank_rows``);
* composed — on the same GPU: torch gather into a materialised hybrid matrix (chunked to
  ``--slab-rows`` rows), ``ops.stack_infer``, ``torch.sort`` and the torch rank mirror;
* cpu      — one CPU core: shuffle a column, ``ref.stack_infer``, ``roc_auc_score``; timed over
  ``--cpu-repeats`` repeats of every column and reported in repeats/s.

Kernel A (scores of all hybrid rows) and kernel B (ranking of all score rows) are also timed alone
against their composed halves.  Each GPU path is warmed, then timed ``--reps`` times with device
events, alternating; the median and min–max are reported.  Prints one JSON line and, with ``--md
PATH``, writes the table.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hfens import ops  # noqa: E402
from hfens.io.checkpoint import load_checkpoint  # noqa: E402
from hfens.io.synth import make_hf_cohort  # noqa: E402
from hfens.ops import reference as ref  # noqa: E402


def composed_scores(x32, pk, src, cols, slab_rows):
    """S [K, R, n] through rows in HBM: repeat → gathered column → stack_infer."""
    n, F = x32.shape
    R = src.shape[0]
    S = torch.empty(len(cols), R, n, dtype=torch.float32, device=x32.device)
    per = max(1, slab_rows // n)
    idx = src.long()
    for kf, k in enumerate(cols):
        for c0 in range(0, R, per):
            c1 = min(R, c0 + per)
            rows = x32[None, :, :].repeat(c1 - c0, 1, 1)
            if k >= 0:
                rows[:, :, k] = x32[:, k][idx[c0:c1]]
            S[kf, c0:c1] = ops.stack_infer(rows.reshape(-1, F), pk).reshape(c1 - c0, n)
    return S


def composed_importance(x32, y, pk, src, slab_rows):
    F = x32.shape[1]
    n = x32.shape[0]
    base = ref.rank_metrics(y, composed_scores(x32, pk, src[:1], [-1], slab_rows).reshape(-1, n))
    m = ref.rank_metrics(y, composed_scores(x32, pk, src, list(range(F)), slab_rows).reshape(-1, n))
    return (base.auroc[0] - m.auroc).reshape(F, -1)


def cpu_loop(X, y, pk, repeats):
    """Repeats per second of the scikit-learn style loop on one core."""
    from sklearn.metrics import roc_auc_score
    torch.set_num_threads(1)
    Xn, yn = X.double().cpu().numpy(), y.cpu().numpy()
    rng = __import__("numpy").random.default_rng(0)
    base = roc_auc_score(yn, ref.stack_infer(torch.as_tensor(Xn), pk).numpy())
    t0 = time.perf_counter()
    for _ in range(repeats):
        for k in range(Xn.shape[1]):
            h = Xn.copy()
            h[:, k] = h[rng.permutation(Xn.shape[0]), k]
            base - roc_auc_score(yn, ref.stack_infer(torch.as_tensor(h), pk).numpy())
    return repeats / (time.perf_counter() - t0)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--cpu-repeats", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slab-rows", type=int, default=1 << 23)
    ap.add_argument("--seed", type=int, default=2020)
    ap.add_argument("--md", default=None, help="write the table here")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    ops.ext()
    clf = load_checkpoint(None, device=dev)
    pk = clf._packed_stack(dev)
    F, n, R = pk.F, a.rows, a.repeats
    X, y, _ = make_hf_cohort(n, F, seed=1, nan_frac=0.0)
    x = torch.as_tensor(X).float().to(dev)
    y = torch.as_tensor(y).to(dev)
    src = ops.permutation_sources(n, 0, R, seed=a.seed, device=dev)
    cols = list(range(F))
    S = ops.stack_permute_scores(x, pk, src, cols).reshape(-1, n)

    def sorted_rank():
        return ref.rank_metrics(y, S)

    paths = {
        "fused": lambda: ops.permutation_importance(x, y, pk, R, seed=a.seed)[1]["auroc"],
        "composed": lambda: composed_importance(x, y, pk, src, a.slab_rows),
        "A_fused": lambda: ops.stack_permute_scores(x, pk, src, cols),
        "A_composed": lambda: composed_scores(x, pk, src, cols, a.slab_rows),
        "B_fused": lambda: ops.rank_metrics(y, S).auroc,
        "B_composed": lambda: sorted_rank().auroc,
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    for fn in paths.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in paths}
    outs = {}
    for _ in range(a.reps):
        for k, fn in paths.items():
            t, outs[k] = timed(fn)
            times[k].append(t)
    res = {"rows": n, "F": F, "repeats": R, "hybrid_rows": n * F * R, "score_rows": F * R}
    for k, v in times.items():
        res[k + "_s"] = statistics.median(v)
        res[k + "_s_min_max"] = [min(v), max(v)]
    res["max_abs_dauroc_importance_between_paths"] = float((outs["fused"] - outs["composed"]).abs().max())
    res["max_abs_dS_between_paths"] = float((outs["A_fused"] - outs["A_composed"]).abs().max())
    res["B_auroc_bit_equal"] = bool(torch.equal(outs["B_fused"], outs["B_composed"]))
    res["fused_repeats_per_s"] = R / res["fused_s"]
    res["composed_repeats_per_s"] = R / res["composed_s"]
    res["cpu_repeats_per_s"] = cpu_loop(x, y, clf.to("cpu")._packed_stack(torch.device("cpu")), a.cpu_repeats)
    print(json.dumps(res), flush=True)
    if a.md:
        def ms(k):
            lo, hi = res[k + "_s_min_max"]
            return f"{1e3 * res[k + '_s']:.2f} ms ({1e3 * lo:.2f} – {1e3 * hi:.2f})"
        with open(a.md, "w") as f:
            f.write(f"{n:,} rows × {F} columns × {R} repeats = {n * F * R:,} hybrid rows, {F * R:,} rankings; "
                    f"median of {a.reps} (min – max)\n\n")
            f.write("| what | fused | composed on the GPU | composed / fused |\n|---|---|---|---|\n")
            for name, k in (("whole op", ""), ("A: scores of the hybrid rows", "A_"), ("B: ranking of the score rows", "B_")):
                f.write(f"| {name} | {ms(k + 'fused')} | {ms(k + 'composed')} | "
                        f"{res[k + 'composed_s'] / res[k + 'fused_s']:.2f}× |\n")
            f.write(f"\nrepeats/s: fused {res['fused_repeats_per_s']:.1f}, composed {res['composed_repeats_per_s']:.1f}, "
                    f"one CPU core {res['cpu_repeats_per_s']:.3f}\n\n")
            f.write(f"agreement: max |ΔAUROC importance| fused vs composed {res['max_abs_dauroc_importance_between_paths']:.3g}; "
                    f"max |ΔS| {res['max_abs_dS_between_paths']:.3g}; rank_rows AUROC bit-equal to the torch mirror: "
                    f"{res['B_auroc_bit_equal']}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
