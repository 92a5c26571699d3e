"""Bootstrap replicates/s of the fused op against the composed torch mirror and a sklearn loop.

All paths bootstrap the same labels and scores with the same resampling law, in one process:

* fused    — ``ops.bootstrap_metrics`` on ``cuda`` tensors (``csrc/bootstrap.hip``: one workgroup
  per replicate, counts and scans on chip);
* composed — ``reference.bootstrap_metrics`` on the same ``cuda`` tensors: the draws, a
  ``bincount`` and cumulative sums over ``[replicates, n]`` tensors built from torch ops;
* sklearn  — on the CPU, at ``--sklearn-n`` rows only: materialise each resample and call
  ``roc_auc_score``, ``average_precision_score`` and ``roc_curve`` + ``np.interp`` on it
  (``--sklearn-reps`` replicates, wall clock).

The two GPU paths are warmed, then timed ``--reps`` times with device events, alternating; the
median is reported.  Prints one JSON line per shape and, with ``--out``, writes the markdown
table of ``profiles/bootstrap.md``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hfens import ops  # noqa: E402
from hfens.ops import reference as ref  # noqa: E402


def cohort(n, seed=0):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.2).astype(np.int64)
    s = np.clip(0.25 + 0.3 * y + 0.2 * rng.standard_normal(n), 0.0, 1.0)
    return y, s


def sklearn_rate(y, s, reps, seed):
    from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve
    q = np.arange(101) / 100.0
    n = len(y)
    j = torch.arange(n, dtype=torch.int64)
    sd = torch.tensor(ref._seed_i64(seed))
    t0 = time.perf_counter()
    for b in range(reps):
        u = ref._splitmix64_t(sd ^ ref._splitmix64_t((torch.tensor(b, dtype=torch.int64) << 40) ^ j))
        idx = ((((u >> 32) & 0xFFFFFFFF) * n) >> 32).numpy()
        yy, ss = y[idx], s[idx]
        roc_auc_score(yy, ss)
        average_precision_score(yy, ss)
        fpr, tpr, _ = roc_curve(yy, ss, drop_intermediate=False)
        np.interp(q, fpr, tpr)
    return reps / (time.perf_counter() - t0)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="10000x2000,1000000x2000", help="comma-separated n x B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2020)
    ap.add_argument("--sklearn-n", type=int, default=10000)
    ap.add_argument("--sklearn-reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="write the markdown report here")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    ops.ext()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    rows = []
    for shp in a.shapes.split(","):
        n, B = (int(t) for t in shp.lower().split("x"))
        y, s = cohort(n)
        yd, sd = torch.as_tensor(y).to(dev), torch.as_tensor(s).to(dev)
        paths = {"fused": lambda: ops.bootstrap_metrics(yd, sd, B, seed=a.seed),
                 "composed": lambda: ref.bootstrap_metrics(yd, sd, B, seed=a.seed)}
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
        med = {k: statistics.median(v) for k, v in times.items()}
        same = all(torch.equal(outs["fused"][k], outs["composed"][k]) for k in (2, 3, 4))
        row = {"n": n, "B": B, "path": "lds" if n <= ops.api.BOOTSTRAP_LDS_ROWS else "global",
               "fused_s": med["fused"], "composed_s": med["composed"],
               "fused_reps_per_s": B / med["fused"], "composed_reps_per_s": B / med["composed"],
               "ratio": med["composed"] / med["fused"],
               "fused_s_min_max": [min(times["fused"]), max(times["fused"])],
               "composed_s_min_max": [min(times["composed"]), max(times["composed"])],
               "integer_outputs_equal": same}
        if n == a.sklearn_n and a.sklearn_reps > 0:
            row["sklearn_cpu_reps_per_s"] = sklearn_rate(y, s, a.sklearn_reps, a.seed)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("| n | B | arrays | fused s (min–max) | composed s (min–max) | fused rep/s | composed rep/s | "
                    "composed/fused | sklearn CPU rep/s |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                sk = f"{r['sklearn_cpu_reps_per_s']:.1f}" if "sklearn_cpu_reps_per_s" in r else "—"
                f.write(f"| {r['n']} | {r['B']} | {r['path']} | {r['fused_s']:.4g} ({r['fused_s_min_max'][0]:.4g}–"
                        f"{r['fused_s_min_max'][1]:.4g}) | {r['composed_s']:.4g} ({r['composed_s_min_max'][0]:.4g}–"
                        f"{r['composed_s_min_max'][1]:.4g}) | {r['fused_reps_per_s']:.4g} | "
                        f"{r['composed_reps_per_s']:.4g} | {r['ratio']:.3g} | {sk} |\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
