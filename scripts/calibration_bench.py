"""Bootstrap replicates/s of the fused calibration op against its torch mirror and a CPU loop.

All paths bootstrap the same labels and risks with the same resampling law, in one process:

* fused    — ``ops.bootstrap_calibration`` on ``cuda`` tensors (``csrc/calibration.hip``: one
  workgroup per replicate; counts, scans and the Newton fit on chip);
* composed — ``reference.bootstrap_calibration`` on the same ``cuda`` tensors: the draws, a
  ``bincount``, cumulative sums and a batched Newton over ``[replicates, n]`` tensors of torch ops;
* cpu loop — one core, ``--cpu-reps`` replicates, wall clock: each resample is materialised and
  fitted by sklearn ``LogisticRegression(penalty=None)`` on the logit plus ``brier_score_loss``;
  without sklearn, by ``reference.calibration_oracle``.

The two GPU paths are warmed, then timed ``--reps`` times with device events, alternating; the
median is reported.  Prints one JSON line per shape and, with ``--out``, writes the markdown
table of ``profiles/calibration.md``.
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


def cpu_rate(y, s, reps, seed):
    """(replicates/s, name of the fitter) of the one-core loop."""
    torch.set_num_threads(1)
    try:
        from sklearn.linear_model import LogisticRegression
        from sklearn.metrics import brier_score_loss
    except Exception:
        t0 = time.perf_counter()
        ref.calibration_oracle(y, s, reps, seed=seed)
        return reps / (time.perf_counter() - t0), "oracle"
    pc = np.clip(s, 1e-12, 1 - 1e-12)
    lg = (np.log(pc) - np.log1p(-pc))[:, None]
    n = len(y)
    j = torch.arange(n, dtype=torch.int64)
    sd = torch.tensor(ref._seed_i64(seed))
    t0 = time.perf_counter()
    for b in range(reps):
        u = ref._splitmix64_t(sd ^ ref._splitmix64_t((torch.tensor(b, dtype=torch.int64) << 40) ^ j))
        idx = ((((u >> 32) & 0xFFFFFFFF) * n) >> 32).numpy()
        yy = y[idx]
        brier_score_loss(yy, s[idx])
        if 0 < yy.sum() < n:
            LogisticRegression(penalty=None, tol=1e-10, max_iter=1000).fit(lg[idx], yy)
    return reps / (time.perf_counter() - t0), "sklearn"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="10000x2000", help="comma-separated n x B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2020)
    ap.add_argument("--cpu-n", type=int, default=10000)
    ap.add_argument("--cpu-reps", type=int, default=50)
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
        paths = {"fused": lambda: ops.bootstrap_calibration(yd, sd, B, seed=a.seed),
                 "composed": lambda: ref.bootstrap_calibration(yd, sd, B, seed=a.seed)}
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
        f, c = outs["fused"], outs["composed"]
        same = all(torch.equal(getattr(f, k), getattr(c, k)) for k in ("pn", "bin_n", "bin_pos", "dc", "status"))
        ok = f.status == 0
        dcoef = float((f.coef[ok] - c.coef[ok]).abs().max()) if bool(ok.any()) else 0.0
        row = {"n": n, "B": B, "path": "lds" if n <= ops.api.CALIBRATION_LDS_ROWS else "global",
               "fused_s": med["fused"], "composed_s": med["composed"],
               "fused_reps_per_s": B / med["fused"], "composed_reps_per_s": B / med["composed"],
               "ratio": med["composed"] / med["fused"],
               "fused_s_min_max": [min(times["fused"]), max(times["fused"])],
               "composed_s_min_max": [min(times["composed"]), max(times["composed"])],
               "integer_outputs_equal": same, "max_coef_diff": dcoef,
               "newton_steps_mean_max": [float(f.iters[ok].double().mean()) if bool(ok.any()) else 0.0,
                                         int(f.iters.max())]}
        if n == a.cpu_n and a.cpu_reps > 0:
            row["cpu_reps_per_s"], row["cpu_fitter"] = cpu_rate(y, s, a.cpu_reps, a.seed)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("| n | B | arrays | fused s (min–max) | composed s (min–max) | fused rep/s | composed rep/s | "
                    "composed/fused | one-core CPU rep/s |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                cpu = f"{r['cpu_reps_per_s']:.1f} ({r['cpu_fitter']})" if "cpu_reps_per_s" in r else "—"
                f.write(f"| {r['n']} | {r['B']} | {r['path']} | {r['fused_s']:.4g} ({r['fused_s_min_max'][0]:.4g}–"
                        f"{r['fused_s_min_max'][1]:.4g}) | {r['composed_s']:.4g} ({r['composed_s_min_max'][0]:.4g}–"
                        f"{r['composed_s_min_max'][1]:.4g}) | {r['fused_reps_per_s']:.4g} | "
                        f"{r['composed_reps_per_s']:.4g} | {r['ratio']:.3g} | {cpu} |\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
