"""Time of the fused paired comparison op against M separate bootstrap launches and its torch mirror.

All paths bootstrap the same labels and M score columns with the same resampling law, in one process:

* fused    — ``ops.bootstrap_compare`` on ``cuda`` tensors (``csrc/compare.hip``: one workgroup per
  replicate draws once, then gathers the counts through every column's order);
* separate — M calls of ``ops.bootstrap_metrics`` (``csrc/bootstrap.hip``), one per column: the floor
  for the unpaired half of the work (AUROC, AP, confusion counts; it cannot give NRI or IDI, and it
  also computes the ROC grid, which the fused op does not);
* composed — ``reference.bootstrap_compare`` on the same ``cuda`` tensors: torch ops over
  ``[replicates, n]`` tensors.

Each timing covers the whole op (the per-call sort and plan included).  The paths are warmed, then
timed ``--reps`` times with device events, alternating; the median is reported.  Prints one JSON line
per shape and, with ``--out``, writes the markdown table of ``profiles/compare.md``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hfens import ops  # noqa: E402
from hfens.ops import reference as ref  # noqa: E402


def cohort(n, M, seed=0):
    """Labels and M risks that share most of their noise, as a stack and its base learners do."""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.2).astype(np.int64)
    shared = rng.standard_normal(n)
    S = np.stack([1 / (1 + np.exp(-((1.3 - 0.1 * m) * y + shared + (0.3 + 0.1 * m) * rng.standard_normal(n) - 1.0)))
                  for m in range(M)])
    return y, S


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="10000x2000x4", help="comma-separated n x B x M")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2020)
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
        n, B, M = (int(t) for t in shp.lower().split("x"))
        y, S = cohort(n, M)
        yd, Sd = torch.as_tensor(y).to(dev), torch.as_tensor(S).to(dev)
        paths = {"fused": lambda: ops.bootstrap_compare(yd, Sd, B, seed=a.seed),
                 "separate": lambda: [ops.bootstrap_metrics(yd, Sd[m], B, seed=a.seed) for m in range(M)],
                 "composed": lambda: ref.bootstrap_compare(yd, Sd, B, seed=a.seed)}
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
        f, s, c = outs["fused"], outs["separate"], outs["composed"]
        same = all(torch.equal(getattr(f, k), getattr(c, k)) for k in ("a2", "pn", "conf", "reclass"))
        same_sep = all(torch.equal(f.a2[:, m], s[m][2]) and torch.equal(f.ap[:, m], s[m][1]) for m in range(M))
        row = {"n": n, "B": B, "M": M, "path": "lds" if n <= ops.api.COMPARE_LDS_ROWS else "global",
               **{f"{k}_s": med[k] for k in paths},
               **{f"{k}_s_min_max": [min(times[k]), max(times[k])] for k in paths},
               "separate_over_fused": med["separate"] / med["fused"],
               "composed_over_fused": med["composed"] / med["fused"],
               "integer_outputs_equal_composed": same, "a2_ap_equal_separate": same_sep,
               "max_sums_diff": float((f.sums - c.sums).abs().max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("| n | B | M | arrays | fused s (min–max) | M separate launches s (min–max) | composed s (min–max) | "
                     "separate/fused | composed/fused |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                def cell(k):
                    return f"{r[k + '_s']:.4g} ({r[k + '_s_min_max'][0]:.4g}–{r[k + '_s_min_max'][1]:.4g})"
                fh.write(f"| {r['n']} | {r['B']} | {r['M']} | {r['path']} | {cell('fused')} | {cell('separate')} | "
                         f"{cell('composed')} | {r['separate_over_fused']:.3g} | {r['composed_over_fused']:.3g} |\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
