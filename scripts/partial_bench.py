"""Time of the fused partial-dependence op against the composed baseline.

Both paths compute the same pd over the same cohort and cells on the shipped checkpoint, in one
process:

* fused    — ``ops.stack_partial`` (hybrid rows built on chip, per-lane f64 sums in row order);
* composed — materialise the hybrid rows with torch (the cohort repeated per cell, one or two
  columns overwritten), score them with ``ops.stack_infer`` and take the f64 mean per cell (cells
  are processed in slabs so the hybrid matrix stays below ``--slab-rows`` rows).

Shapes: ``pd`` — the partial-dependence sweep, 10,000 cohort rows × 17·32 one-variable cells;
``h2`` — the de-duplicated cell set of Friedman's H² over all pairs of a 512-row cohort, evaluated
over that cohort.  Each path is warmed, then timed ``--reps`` times with device events, alternating
the two; the median and min–max are reported.  A hybrid row is one (cell, cohort row) evaluation.
Prints one JSON line per shape and, with ``--md PATH``, writes the table.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hfens import ops  # noqa: E402
from hfens.explain import interaction_cells  # noqa: E402
from hfens.io.checkpoint import load_checkpoint  # noqa: E402
from hfens.io.synth import make_hf_cohort  # noqa: E402


def composed(x32, pk, feat, value, slab_rows):
    """pd through rows in HBM: repeat → column writes → stack_infer → f64 mean per cell."""
    n, F = x32.shape
    C = feat.shape[0]
    per = max(1, slab_rows // n)
    pd = torch.empty(C, dtype=torch.float64, device=x32.device)
    for c0 in range(0, C, per):
        c1 = min(C, c0 + per)
        rows = x32[None, :, :].repeat(c1 - c0, 1, 1)                      # [cells, n, F]
        for s in range(2):
            k = feat[c0:c1, s]
            idx = k.clamp(min=0)[:, None, None].expand(-1, n, 1)
            cur = rows.gather(2, idx)
            rows.scatter_(2, idx, torch.where((k >= 0)[:, None, None], value[c0:c1, s][:, None, None].expand(-1, n, 1),
                                              cur))
        pr = ops.stack_infer(rows.reshape(-1, F), pk)
        pd[c0:c1] = pr.reshape(c1 - c0, n).double().sum(1) / n
    return pd


def shape_pd(F, dev, rows, points):
    x = torch.as_tensor(make_hf_cohort(rows, F, seed=1, nan_frac=0.0)[0]).float().to(dev)
    feat = torch.stack([torch.arange(F).repeat_interleave(points), torch.full((F * points,), -1)], 1).to(dev)
    lo, hi = x.min(0).values, x.max(0).values
    t = torch.linspace(0, 1, points, device=dev)
    v = (lo[:, None] + (hi - lo)[:, None] * t[None, :]).reshape(-1)
    return x, feat.contiguous(), torch.stack([v, torch.zeros_like(v)], 1).contiguous()


def shape_h2(F, dev, rows):
    x = torch.as_tensor(make_hf_cohort(rows, F, seed=1, nan_frac=0.0)[0]).float().to(dev)
    pairs = [(j, k) for j in range(F) for k in range(j + 1, F)]
    feat, value, _ = interaction_cells(x.double(), pairs, list(range(F)))
    return x, feat, value


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="pd,h2")
    ap.add_argument("--pd-rows", type=int, default=10000)
    ap.add_argument("--pd-points", type=int, default=32)
    ap.add_argument("--h2-rows", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slab-rows", type=int, default=1 << 23)
    ap.add_argument("--md", default=None, help="write the table here")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    ops.ext()
    clf = load_checkpoint(None, device=dev)
    pk = clf._packed_stack(dev)
    F = pk.F

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    results = []
    for name in a.shapes.split(","):
        x, feat, value = shape_pd(F, dev, a.pd_rows, a.pd_points) if name == "pd" else shape_h2(F, dev, a.h2_rows)
        n, C = x.shape[0], feat.shape[0]
        paths = {"fused": lambda: ops.stack_partial(x, pk, feat, value),
                 "composed": lambda: composed(x, pk, feat, value, a.slab_rows)}
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
        res = {"shape": name, "n": n, "cells": C, "F": F, "hybrid_rows": n * C,
               "fused_s": med["fused"], "composed_s": med["composed"],
               "fused_rows_per_s": n * C / med["fused"], "composed_rows_per_s": n * C / med["composed"],
               "ratio": med["composed"] / med["fused"],
               "fused_s_min_max": [min(times["fused"]), max(times["fused"])],
               "composed_s_min_max": [min(times["composed"]), max(times["composed"])],
               "max_abs_dpd_between_paths": float((outs["fused"] - outs["composed"]).abs().max())}
        results.append(res)
        print(json.dumps(res), flush=True)
    if a.md:
        def ms(r, k):
            lo, hi = r[k + "_s_min_max"]
            return f"{1e3 * r[k + '_s']:.2f} ms ({1e3 * lo:.2f} – {1e3 * hi:.2f})"
        with open(a.md, "w") as f:
            f.write("| shape | cohort rows | cells | hybrid rows | fused | composed | composed / fused | max abs dpd |\n")
            f.write("|---|---|---|---|---|---|---|---|\n")
            for r in results:
                f.write(f"| {r['shape']} | {r['n']:,} | {r['cells']:,} | {r['hybrid_rows']:,} | {ms(r, 'fused')} | "
                        f"{ms(r, 'composed')} | {r['ratio']:.2f}× | {r['max_abs_dpd_between_paths']:.2g} |\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
