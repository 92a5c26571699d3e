"""Hybrid rows/s of the fused exact-Shapley op against the composed baseline.

Both paths explain the same patients against the same background on the shipped checkpoint,
in one process:

* fused    — ``ops.stack_shapley`` (stack_coalition + shapley_reduce: hybrid rows built on chip);
* composed — materialise the hybrid rows with ``torch.where``, score them with
  ``ops.stack_infer``, average over the background and apply the Shapley weights with torch in
  f64 (coalitions are processed in slabs so the hybrid matrix stays below ``--slab-rows`` rows).

Each path is warmed, then timed ``--reps`` times with device events, alternating the two; the
median is reported.  A hybrid row is one (patient, coalition, background) evaluation:
n · 2^F · B of them per call.  Prints one JSON line per shape.

Then the pair reduction (Shapley interaction values) on the table ``v`` that ``stack_coalition`` left
for the same shape, by the same protocol, as a second JSON line (``"op": "pairs"``):

* fused    — the ``shapley_interactions`` kernels into preallocated buffers;
* composed — ``v @ C`` in torch with the f64 coefficient matrix ``C [2^F, F²]`` on the same GPU
  (``composed_s`` is null and ``composed_note`` says why if ``C`` cannot be allocated);

with the whole ``ops.stack_shapley_interactions`` call and ``stack_coalition`` alone beside them.
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
from hfens.io.checkpoint import load_checkpoint  # noqa: E402
from hfens.io.synth import make_hf_cohort  # noqa: E402
from hfens.ops import reference as ref  # noqa: E402


def slab_masks(F, B, slab_rows, device):
    """(coalition index, present-feature mask) of each slab of at most ``slab_rows`` hybrid rows."""
    per = max(1, slab_rows // B)
    k = torch.arange(F, device=device)
    out = []
    for s0 in range(0, 1 << F, per):
        S = torch.arange(s0, min(1 << F, s0 + per), device=device)
        out.append((S, ((S[:, None] >> k[None, :]) & 1).bool()[:, None, :]))
    return out


def composed(x, bg, pk, coef, masks):
    """phi, base, pred through rows in HBM: torch.where → stack_infer → f64 torch reduction
    (``masks`` from :func:`slab_masks`, built once outside the timed region)."""
    n, F = x.shape
    B = bg.shape[0]
    x32, bg32 = x.float(), bg.float()
    v = torch.empty(n, 1 << F, dtype=torch.float64, device=x.device)
    for p in range(n):
        for S, mask in masks:
            rows = torch.where(mask, x32[p][None, None, :], bg32[None, :, :])   # [S, B, F]
            pr = ops.stack_infer(rows.reshape(-1, F), pk)
            v[p, S] = pr.reshape(-1, B).double().sum(1) / B
    return v @ coef, v[0, 0], v[:, -1]


def pair_matrix(F, chunk=4096):
    """``C [2^F, F²]`` f64 with ``(v @ C).reshape(n, F, F)`` = Phi: the mirror's coefficients, the pair
    columns written to both halves and the diagonal's in place."""
    i, j = torch.triu_indices(F, F, 1)
    k = torch.arange(F)
    C = torch.zeros(1 << F, F * F, dtype=torch.float64)
    for s0 in range(0, 1 << F, chunk):
        c, d = ref._interaction_coefficients(F, s0, min(1 << F, s0 + chunk))
        C[s0:s0 + chunk, i * F + j] = c
        C[s0:s0 + chunk, j * F + i] = c
        C[s0:s0 + chunk, k * F + k] = d
    return C


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="1x256,64x16", help="comma-separated n x B")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slab-rows", type=int, default=1 << 25)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    ops.ext()
    clf = load_checkpoint(None, device=dev)
    pk = clf._packed_stack(dev)
    F = pk.F
    S = torch.arange(1 << F)
    inS = ((S[:, None] >> torch.arange(F)[None, :]) & 1).bool()
    size = inS.sum(1)
    w = ref.shapley_weights(F)
    zero = torch.zeros((), dtype=torch.float64)
    coef = torch.where(inS, torch.where(size > 0, w[(size - 1).clamp(min=0)], zero)[:, None],
                       -torch.where(size < F, w[size.clamp(max=F - 1)], zero)[:, None]).to(dev)

    u = ref.shapley_interaction_weights(F).to(dev)
    w_dev = w.to(dev)
    pair_note = None
    try:
        C = pair_matrix(F).to(dev)
    except torch.OutOfMemoryError as e:
        C, pair_note = None, f"C [{1 << F}, {F * F}] f64 could not be allocated: {e}"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    for shp in a.shapes.split(","):
        n, B = (int(t) for t in shp.lower().split("x"))
        x = torch.as_tensor(make_hf_cohort(n, F, seed=1, nan_frac=0.0)[0]).to(dev)
        bg = torch.as_tensor(make_hf_cohort(B, F, seed=0, nan_frac=0.0)[0]).to(dev)
        masks = slab_masks(F, B, a.slab_rows, dev)
        paths = {"fused": lambda: ops.stack_shapley(x, bg, pk),
                 "composed": lambda: composed(x, bg, pk, coef, masks)}
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
        rows = n * (1 << F) * B
        med = {k: statistics.median(v) for k, v in times.items()}
        dphi = float((outs["fused"][0] - outs["composed"][0]).abs().max())
        print(json.dumps({
            "n": n, "B": B, "F": F, "hybrid_rows": rows,
            "fused_s": med["fused"], "composed_s": med["composed"],
            "fused_rows_per_s": rows / med["fused"], "composed_rows_per_s": rows / med["composed"],
            "ratio": med["composed"] / med["fused"],
            "fused_s_min_max": [min(times["fused"]), max(times["fused"])],
            "composed_s_min_max": [min(times["composed"]), max(times["composed"])],
            "max_abs_dphi_between_paths": dphi}), flush=True)
        pairs_line(n, B, x, bg, pk, u, w_dev, C, pair_note, timed, a)
    return 0


def pairs_line(n, B, x, bg, pk, u, w, C, note, timed, a):
    """Time the pair reduction both ways on the v of this shape and print its JSON line."""
    from hfens.ops import api
    dev, F = x.device, pk.F
    ext, sp = ops.ext(), ops.stream_ptr(dev)
    phi, _, _, v = ops.stack_shapley(x, bg, pk, return_values=True)
    Phi = torch.empty(n, F, F, dtype=torch.float64, device=dev)
    part = torch.empty(n * api._pair_part_len(F), dtype=torch.float64, device=dev)
    x32, bg32 = x.float().contiguous(), bg.float().contiguous()
    v2 = torch.empty_like(v)
    model = api._stack_model_args(pk)

    def fused():
        ext.shapley_interactions(v.data_ptr(), n, F, u.data_ptr(), phi.data_ptr(), part.data_ptr(), part.numel(),
                                 Phi.data_ptr(), sp)
        return Phi

    paths = {"fused": fused,
             "call": lambda: ops.stack_shapley_interactions(x, bg, pk)[0],
             "coalition": lambda: ext.stack_coalition(x32.data_ptr(), n, bg32.data_ptr(), B, *model, v2.data_ptr(), 0, sp),
             "phi_reduce": lambda: ext.shapley_reduce(v.data_ptr(), n, F, w.data_ptr(), phi.data_ptr(), sp)}
    if C is not None:
        paths["composed"] = lambda: (v @ C).reshape(n, F, F)
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
    med = {k: statistics.median(t) for k, t in times.items()}
    line = {"op": "pairs", "n": n, "B": B, "F": F, "v_bytes": 8 * v.numel()}
    for k in paths:
        line[f"{k}_s"] = med[k]
        line[f"{k}_s_min_max"] = [min(times[k]), max(times[k])]
    if C is None:
        line.update(composed_s=None, composed_note=note)
    else:
        line["ratio"] = med["composed"] / med["fused"]
        line["max_abs_dPhi_between_paths"] = float((outs["fused"] - outs["composed"]).abs().max())
        line["C_bytes"] = 8 * C.numel()
    line["fused_share_of_call"] = med["fused"] / med["call"]
    line["call_equals_fused"] = bool(torch.equal(outs["call"], outs["fused"]))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    sys.exit(main())
