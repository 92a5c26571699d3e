"""Op entry points: validate, then route ``cuda`` tensors to the HIP extension and
host tensors to :mod:`hfens.ops.reference`."""
from __future__ import annotations

import torch

from . import reference as ref
from .packing import pack_forest, pack_stack, pack_svs

__all__ = ["rbf_decision", "svc_proba1", "tree_raw", "expit", "pack_svs", "pack_forest", "pack_stack",
           "stack_infer", "stack_shapley", "stack_shapley_interactions", "shapley_interactions_from_values",
           "stack_partial", "weighted_moments", "bootstrap_metrics",
           "bootstrap_calibration", "bootstrap_compare", "permutation_sources", "stack_permute_scores",
           "rank_metrics", "permutation_importance"]


def _c(t: torch.Tensor, dtype) -> torch.Tensor:
    return t.to(dtype).contiguous()


def rbf_decision(z, sv, coef, gamma: float, intercept: float, packed=None):
    """libsvm RBF decision values; ``packed`` = cached :class:`PackedSV` for ``sv``/``coef``."""
    if z.is_cuda:
        from . import ext, stream_ptr
        pk = packed if packed is not None else pack_svs(sv, coef, z.device)
        z32 = _c(z, torch.float32)
        n, F = z32.shape
        if F != pk.F:
            raise ValueError(f"rbf_decision: X has {F} features, model has {pk.F}")
        out = torch.empty(n, dtype=torch.float32, device=z.device)
        ext().rbf_decision(z32.data_ptr(), n, F, pk.svt.data_ptr(), pk.sn.data_ptr(), pk.coef.data_ptr(),
                           pk.mp, float(gamma), float(intercept), out.data_ptr(), stream_ptr(z.device))
        return out
    return ref.rbf_decision(z, sv, coef, gamma, intercept)


def svc_proba1(dec, A: float, B: float):
    if dec.is_cuda:
        from . import ext, stream_ptr
        d32 = _c(dec, torch.float32)
        out = torch.empty_like(d32)
        ext().svc_proba1(d32.data_ptr(), out.data_ptr(), d32.numel(), float(A), float(B),
                         stream_ptr(dec.device))
        return out
    return ref.svc_proba1(dec, A, B)


def tree_raw(x, feature, threshold, left, right, value, init: float, lr: float, packed=None):
    if x.is_cuda:
        from . import ext, stream_ptr
        pk = packed if packed is not None else pack_forest(feature, threshold, left, right, value, x.device)
        x32 = _c(x, torch.float32)
        n, F = x32.shape
        if pk.max_feature >= F:
            raise ValueError("tree_raw: a split feature index exceeds the input width")
        out = torch.empty(n, dtype=torch.float32, device=x.device)
        ext().forest_raw(x32.data_ptr(), n, F, pk.nodes.data_ptr(), pk.values.data_ptr(), pk.n_trees,
                         pk.max_nodes, float(init), float(lr), out.data_ptr(), stream_ptr(x.device))
        return out
    return ref.tree_raw(x, feature, threshold, left, right, value, init, lr)


def _stack_model_args(pk):
    """The model arguments every fused stack op of the extension takes after its inputs, from a
    :class:`PackedStack`: F, the padded SV count, the tree table shape, −γ·log2(e) and the other
    scalars, then the device pointers (stump table: zeros when the stack keeps its generic trees)."""
    f, s, st = pk.forest, pk.sv, pk.stumps
    stumps = (st.off.data_ptr(), st.pairs.data_ptr(), st.base) if st is not None else (0, 0, 0.0)
    return (pk.F, s.mp, f.n_trees, f.max_nodes, -pk.gamma * 1.4426950408889634, pk.svc_b, pk.probA, pk.probB,
            pk.gb_init, pk.gb_lr, pk.lr_b, pk.meta_w[0], pk.meta_w[1], pk.meta_w[2], pk.meta_b,
            pk.mean.data_ptr(), pk.inv_scale.data_ptr(), s.svt.data_ptr(), s.sn.data_ptr(), s.coef.data_ptr(),
            f.nodes.data_ptr(), f.values.data_ptr(), pk.lr_w.data_ptr(), *stumps)


def stack_infer(x, pk, out=None, grid: int = 0, stream=None):
    """Fused P(class 1) of the whole HF stack (one kernel, one pass over ``x``).
    ``x``: [n, F] f32 or f64; ``pk``: :class:`PackedStack` on ``x``'s device.  Returns f32 on
    the GPU (written into ``out`` if given), f64 on the host."""
    if x.is_cuda:
        from . import ext, stream_ptr
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float32)
        x = x.contiguous()
        n, F = x.shape
        if F != pk.F:
            raise ValueError(f"stack_infer: X has {F} features, model has {pk.F}")
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=x.device)
        elif out.dtype != torch.float32 or out.numel() < n or not out.is_contiguous():
            raise ValueError("stack_infer: out must be a contiguous f32 buffer of >= n elements")
        ext().stack_infer(x.data_ptr(), int(x.dtype == torch.float64), n, *_stack_model_args(pk),
                          out.data_ptr(), int(grid),
                          stream if stream is not None else stream_ptr(x.device))
        return out[:n]
    return ref.stack_infer(x, pk)


SHAPLEY_MAX_F = 20                 # v is 8 MB per patient at F = 20
SHAPLEY_WS_BYTES = 256 << 20       # byte budget of the coalition-value workspace (patients are chunked)
SHAPLEY_PAIR_GROUP = 16            # pairs (f64 accumulators) per thread of shapley_interactions (csrc/shapley.hip)
SHAPLEY_PAIR_SLAB = 4096           # coalitions per workgroup there; each of its 256 threads takes 16 of them
SHAPLEY_PAIR_THREADS = 256


def stack_shapley(x, background, pk, *, return_values: bool = False, grid: int = 0, stream=None):
    """Exact interventional Shapley values of the fused stack's P(class 1).

    ``x``: [n, F] patients, ``background``: [B, F] cohort, both f32 or f64 on ``pk``'s device
    (rounded to f32 as ``stack_infer`` does).  With ``h(S, b)[k] = x[k]`` if bit k of S is set,
    else ``background[b][k]``, and ``v(S) = mean_b P(h(S, b))`` over all 2^F coalitions:
    ``phi[k] = Σ_S c_k(S)·v(S)``, ``c_k(S) = w(|S|−1)`` if k ∈ S else ``−w(|S|)``,
    ``w(s) = s!(F−s−1)!/F!``.  Returns ``phi [n, F]``, ``base = v(∅)`` (0-dim) and
    ``pred [n] = v(all)``, all f64, plus ``v [n, 2^F]`` when ``return_values``; ``phi`` sums to
    ``pred − base`` per row.  ``stream``, if given, is a raw HIP stream handle: the kernels and
    the torch ops that slice the results out all run on it."""
    return _stack_shapley("stack_shapley", x, background, pk, return_values, grid, stream, False)


def _stack_shapley(op: str, x, background, pk, return_values: bool, grid: int, stream, pairs: bool):
    """``stack_shapley`` (``pairs`` false) and ``stack_shapley_interactions``: validate, then route."""
    if x.dim() != 2 or background.dim() != 2:
        raise ValueError(f"{op}: x must be [n, F] and background [B, F]")
    n, F = x.shape
    B = background.shape[0]
    if F != pk.F or background.shape[1] != pk.F:
        raise ValueError(f"{op}: x has {F} and background {background.shape[1]} features, "
                         f"model has {pk.F}")
    if F > SHAPLEY_MAX_F:
        raise ValueError(f"{op}: exact enumeration is limited to {SHAPLEY_MAX_F} features, got {F}")
    if B < 1:
        raise ValueError(f"{op}: background needs at least one row")
    if x.device != background.device:
        raise ValueError(f"{op}: x and background must be on the same device")
    if not x.is_cuda:
        mirror = ref.stack_shapley_interactions if pairs else ref.stack_shapley
        return mirror(x, background, pk, return_values=return_values)
    if stream is not None:
        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=x.device)):
            return _stack_shapley_device(x, background, pk, return_values, grid, pairs)
    return _stack_shapley_device(x, background, pk, return_values, grid, pairs)


def _stack_shapley_device(x, background, pk, return_values: bool, grid: int, pairs: bool = False):
    """Validated ``cuda`` inputs; everything is enqueued on torch's current stream."""
    from . import ext, stream_ptr
    dev = x.device
    n, F = x.shape
    B = background.shape[0]
    x32 = _c(x, torch.float32)
    bg32 = _c(background, torch.float32)
    nS = 1 << F
    w = ref.shapley_weights(F).to(dev)
    phi = torch.empty(n, F, dtype=torch.float64, device=dev)
    pred = torch.empty(n, dtype=torch.float64, device=dev)
    base = torch.zeros((), dtype=torch.float64, device=dev)
    per = max(1, SHAPLEY_WS_BYTES // (8 * nS))
    v_all = torch.empty(n, nS, dtype=torch.float64, device=dev) if return_values else None
    ws = None if return_values else torch.empty(min(n, per), nS, dtype=torch.float64, device=dev)
    if pairs:
        u = ref.shapley_interaction_weights(F).to(dev)
        Phi = torch.empty(n, F, F, dtype=torch.float64, device=dev)
        part = torch.empty(min(n, per) * _pair_part_len(F), dtype=torch.float64, device=dev)
    model = _stack_model_args(pk)
    sp = stream_ptr(dev)
    for p0 in range(0, n, per):
        p1 = min(n, p0 + per)
        v = v_all[p0:p1] if return_values else ws[:p1 - p0]
        ext().stack_coalition(x32[p0:p1].data_ptr(), p1 - p0, bg32.data_ptr(), B, *model, v.data_ptr(),
                              int(grid), sp)
        ext().shapley_reduce(v.data_ptr(), p1 - p0, F, w.data_ptr(), phi[p0:p1].data_ptr(), sp)
        if pairs:
            ext().shapley_interactions(v.data_ptr(), p1 - p0, F, u.data_ptr(), phi[p0:p1].data_ptr(), part.data_ptr(),
                                       (p1 - p0) * _pair_part_len(F), Phi[p0:p1].data_ptr(), sp)
        pred[p0:p1] = v[:, nS - 1]
        if p0 == 0:
            base = v[0, 0].clone()
    out = (Phi, phi, base, pred) if pairs else (phi, base, pred)
    return out + (v_all,) if return_values else out


def _pair_part_len(F: int) -> int:
    """f64 slab partials ``shapley_interactions`` keeps per patient: slabs × pair groups × group size."""
    groups = -(-(F * (F - 1) // 2) // SHAPLEY_PAIR_GROUP)
    return -(-(1 << F) // SHAPLEY_PAIR_SLAB) * groups * SHAPLEY_PAIR_GROUP


def stack_shapley_interactions(x, background, pk, *, return_values: bool = False, grid: int = 0, stream=None):
    """Exact Shapley interaction values of the fused stack's P(class 1), on the coalition values
    :func:`stack_shapley` is computed from.

    Arguments as :func:`stack_shapley`.  With ``u(s) = s!(F−s−2)!/(2(F−1)!)``, for i ≠ j
    ``Phi[i][j] = Σ_{S ⊆ N∖{i,j}} u(|S|)·(v(S∪{i,j}) − v(S∪{i}) − v(S∪{j}) + v(S))`` — half of the
    pair's effect in each of ``[i][j]`` and ``[j][i]``, the SHAP convention — and
    ``Phi[i][i] = phi[i] − Σ_{j≠i} Phi[i][j]``, so row i sums to ``phi[i]`` and the matrix to
    ``pred − base``.  Returns ``Phi [n, F, F]`` f64, then ``phi``, ``base``, ``pred`` (and ``v`` with
    ``return_values``), which are bit-equal to :func:`stack_shapley`'s on the same inputs."""
    return _stack_shapley("stack_shapley_interactions", x, background, pk, return_values, grid, stream, True)


def shapley_interactions_from_values(v, F: int):
    """Shapley values and interaction values of any game: ``v [n, 2^F]`` f64 (bit k of the column index
    set: player k present), 1 ≤ F ≤ 20.  Returns ``(Phi [n, F, F], phi [n, F])`` f64 as defined in
    :func:`stack_shapley_interactions` — ``shapley_reduce`` and ``shapley_interactions`` on ``cuda``,
    the mirror on the host."""
    F = int(F)
    if not 1 <= F <= SHAPLEY_MAX_F:
        raise ValueError(f"shapley_interactions_from_values: 1 <= F <= {SHAPLEY_MAX_F}, got {F}")
    if v.dim() != 2 or v.shape[1] != 1 << F:
        raise ValueError(f"shapley_interactions_from_values: v {tuple(v.shape)} must be [n, {1 << F}]")
    if v.dtype != torch.float64:
        raise ValueError("shapley_interactions_from_values: v must be f64")
    if not v.is_cuda:
        return ref.shapley_interactions_from_values(v, F)
    from . import ext, stream_ptr
    dev = v.device
    v = v.contiguous()
    n = v.shape[0]
    w = ref.shapley_weights(F).to(dev)
    u = ref.shapley_interaction_weights(F).to(dev)
    phi = torch.empty(n, F, dtype=torch.float64, device=dev)
    Phi = torch.empty(n, F, F, dtype=torch.float64, device=dev)
    part = torch.empty(n * _pair_part_len(F), dtype=torch.float64, device=dev)
    sp = stream_ptr(dev)
    ext().shapley_reduce(v.data_ptr(), n, F, w.data_ptr(), phi.data_ptr(), sp)
    ext().shapley_interactions(v.data_ptr(), n, F, u.data_ptr(), phi.data_ptr(), part.data_ptr(), part.numel(),
                               Phi.data_ptr(), sp)
    return Phi, phi


PARTIAL_ICE_BYTES = 1 << 30        # largest ice [n, C] f32 that stack_partial returns


def stack_partial(x, pk, feat, value, *, return_ice: bool = False, grid: int = 0, stream=None):
    """Partial dependence of the fused stack's P(class 1) over the cohort ``x``.

    ``x``: [n, F] f32 or f64 on ``pk``'s device; ``feat``: [C, 2] integer, ``value``: [C, 2] float, on
    the same device.  Cell c substitutes ``value[c, s]`` for column ``feat[c, s]`` of every cohort row,
    for each slot s with ``feat[c, s] != -1`` (−1: no substitution; ``(-1, ·, -1, ·)`` is the plain
    row).  ``x`` and ``value`` are rounded to f32 as ``stack_infer`` does.  Returns ``pd [C]`` f64 =
    ``(Σ_r ice[r, c]) / n`` summed over r = 0, 1, …, n−1 in that order, and with ``return_ice`` also
    ``ice [n, C]`` = P of every hybrid row (f32 on the GPU: the value that is widened and summed;
    f64 on the host).  ``stream``, if given, is a raw HIP stream handle: the kernel and the torch
    ops around it all run on it."""
    if x.dim() != 2 or feat.dim() != 2 or value.dim() != 2 or feat.shape[1] != 2 or value.shape != feat.shape:
        raise ValueError("stack_partial: x must be [n, F], feat and value [C, 2]")
    n, F = x.shape
    C = feat.shape[0]
    if F != pk.F:
        raise ValueError(f"stack_partial: x has {F} features, model has {pk.F}")
    if n < 1:
        raise ValueError("stack_partial: the cohort needs at least one row")
    if C < 1:
        raise ValueError("stack_partial: at least one cell is needed")
    if feat.is_floating_point() or feat.dtype == torch.bool or not value.is_floating_point():
        raise ValueError("stack_partial: feat must be integer and value floating point")
    if not (x.device == feat.device == value.device == pk.mean.device):
        raise ValueError("stack_partial: x, feat, value and the packed model must be on the same device")
    if bool(((feat < -1) | (feat >= F)).any()):
        raise ValueError(f"stack_partial: feature indices must lie in [-1, {F})")
    if bool(((feat[:, 0] == feat[:, 1]) & (feat[:, 0] >= 0)).any()):
        raise ValueError("stack_partial: a cell substitutes the same column twice")
    if not bool(torch.isfinite(value.to(torch.float32))[feat >= 0].all()):
        raise ValueError("stack_partial: a substituted value is not finite")
    if return_ice and 4 * n * C > PARTIAL_ICE_BYTES:
        raise ValueError(f"stack_partial: ice [{n}, {C}] f32 exceeds {PARTIAL_ICE_BYTES} bytes")
    if not x.is_cuda:
        return ref.stack_partial(x, pk, feat, value, return_ice=return_ice)
    if stream is not None:
        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=x.device)):
            return _stack_partial_device(x, pk, feat, value, return_ice, grid)
    return _stack_partial_device(x, pk, feat, value, return_ice, grid)


def _stack_partial_device(x, pk, feat, value, return_ice: bool, grid: int):
    """Validated ``cuda`` inputs; everything is enqueued on torch's current stream."""
    from . import ext, stream_ptr
    dev = x.device
    n, F = x.shape
    C = feat.shape[0]
    x32 = _c(x, torch.float32)
    k32 = _c(feat, torch.int32)
    v32 = _c(value, torch.float32)
    pd = torch.empty(C, dtype=torch.float64, device=dev)
    ice = torch.empty(n, C, dtype=torch.float32, device=dev) if return_ice else None
    ext().stack_partial(x32.data_ptr(), n, k32.data_ptr(), v32.data_ptr(), C, *_stack_model_args(pk),
                        pd.data_ptr(), ice.data_ptr() if ice is not None else 0, int(grid), stream_ptr(dev))
    return (pd, ice) if return_ice else pd


BOOTSTRAP_MAX_B = 1 << 24         # the replicate index shares the draw counter: b < 2^24
BOOTSTRAP_MAX_N = 1 << 25          # keeps the doubled AUROC numerator below 2^53
BOOTSTRAP_LDS_ROWS = 20000         # rows whose two u32 arrays fit the CU's 160 KiB LDS (csrc/bootstrap.hip)
BOOTSTRAP_WS_BYTES = 1 << 30       # byte budget of the global workspace above that (8n bytes per resident workgroup)
_BOOTSTRAP_FORCE_GLOBAL = False    # tests: take the global-workspace path below the LDS limit too


def _bootstrap_args(op: str, y, score, name: str, n_boot, b0, b1, stratified):
    """The checks the three bootstrap ops share, on labels ``y [n]`` and ``score [n]`` (``name`` "score")
    or ``[M, n]`` ("scores"); returns the normalised ``n_boot, b0, b1``."""
    if name == "scores":
        if y.dim() != 1 or score.dim() != 2 or y.numel() != score.shape[1]:
            raise ValueError(f"{op}: y {tuple(y.shape)} must be [n] and scores {tuple(score.shape)} "
                             "[M, n] of one length n")
    elif y.dim() != 1 or score.dim() != 1 or y.numel() != score.numel():
        raise ValueError(f"{op}: y {tuple(y.shape)} and score {tuple(score.shape)} must be "
                         "1-D of one length")
    n = y.numel()
    if n == 0:
        raise ValueError(f"{op}: y and {name} are empty (n = 0)")
    if n > BOOTSTRAP_MAX_N:
        raise ValueError(f"{op}: y has {n} rows, the limit is n <= {BOOTSTRAP_MAX_N}")
    if y.device != score.device:
        raise ValueError(f"{op}: y and {name} must be on the same device")
    if not score.is_floating_point() or not bool(torch.isfinite(score).all()):
        raise ValueError(f"{op}: {name} must be finite floating point")
    if not bool(((y == 0) | (y == 1)).all()):
        raise ValueError(f"{op}: y must hold labels 0 and 1 only")
    n_boot = int(n_boot)
    if not 1 <= n_boot <= BOOTSTRAP_MAX_B:
        raise ValueError(f"{op}: n_boot = {n_boot} outside 1..{BOOTSTRAP_MAX_B}")
    b1 = n_boot if b1 is None else int(b1)
    b0 = int(b0)
    if not 0 <= b0 <= b1 <= n_boot:
        raise ValueError(f"{op}: b0:b1 = {b0}:{b1} is not a range within 0..n_boot = {n_boot}")
    if stratified:
        P = int((y == 1).sum())
        if P == 0 or P == n:
            raise ValueError(f"{op}: stratified resampling needs both classes in y")
    return n_boot, b0, b1


def _bootstrap_workspace(dev, n: int, B: int, words: int):
    """The global workspace of ``words`` u32 per row, one slice per workgroup that can be resident
    within the byte budget; returns it and the number of slices."""
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    slices = max(1, min(B, 2 * ncu, BOOTSTRAP_WS_BYTES // (4 * words * n)))
    return torch.empty(slices, words * n, dtype=torch.int32, device=dev), slices


def _on_stream(stream, device, fn, *args, **kw):
    """``fn(*args, **kw)`` with the raw HIP stream handle ``stream``, if given, as torch's current stream."""
    if stream is None:
        return fn(*args, **kw)
    with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=device)):
        return fn(*args, **kw)


def bootstrap_metrics(y, score, n_boot: int, *, seed: int = 0, stratified: bool = False,
                      threshold: float = 0.5, grid_points: int = 101, b0: int = 0, b1=None,
                      grid: int = 0, stream=None):
    """Bootstrap replicates ``b0:b1`` (default all ``n_boot``) of the held-out metrics of binary
    labels ``y [n]`` and scores ``score [n]`` (f32 or f64) on one device.

    Replicate b resamples n rows with replacement by the counter-based law of
    ``csrc/resample.h`` (plain, or ``stratified``: P positives and N negatives drawn within
    their class), so it does not depend on the range, grid or device it is computed in.  Returns
    ``auroc [B]`` = ``a2 / (2·P_b·N_b)`` and ``ap [B]`` (f64), the exact doubled AUROC numerator
    ``a2 [B]``, the class totals ``pn [B, 2]``, the confusion counts ``conf [B, 4]`` = TP, FP, FN,
    TN at ``score > threshold`` (all int64) and ``tpr [B, grid_points]`` (f64): the replicate's ROC
    read at FPR = g/(grid_points − 1), the upper point of a vertical run.  A degenerate replicate
    (``P_b = 0`` or ``N_b = 0``; plain mode only) has NaN ``auroc``, ``ap`` and ``tpr``.
    ``stream``, if given, is a raw HIP stream handle: everything is enqueued on it."""
    n_boot, b0, b1 = _bootstrap_args("bootstrap_metrics", y, score, "score", n_boot, b0, b1, stratified)
    G = int(grid_points)
    if not 2 <= G <= 65536:
        raise ValueError(f"bootstrap_metrics: grid_points = {G} outside 2..65536")
    if threshold != threshold:
        raise ValueError("bootstrap_metrics: threshold is NaN")
    kw = dict(seed=seed, stratified=bool(stratified), threshold=float(threshold), grid_points=G, b0=b0, b1=b1)
    if not score.is_cuda:
        return ref.bootstrap_metrics(y, score, n_boot, **kw)
    return _on_stream(stream, score.device, _bootstrap_device, y, score, grid=grid, **kw)


def _bootstrap_device(y, score, *, seed, stratified, threshold, grid_points, b0, b1, grid):
    """Validated ``cuda`` inputs; everything is enqueued on torch's current stream."""
    from . import ext, stream_ptr
    dev = score.device
    pl = ref.BootstrapPlan(y, score, stratified, threshold)
    n, G, B = pl.n, grid_points, b1 - b0
    f64, i64 = torch.float64, torch.int64
    auroc = torch.empty(B, dtype=f64, device=dev)
    ap = torch.empty(B, dtype=f64, device=dev)
    a2 = torch.empty(B, dtype=i64, device=dev)
    pn = torch.empty(B, 2, dtype=i64, device=dev)
    conf = torch.empty(B, 4, dtype=i64, device=dev)
    tpr = torch.empty(B, G, dtype=f64, device=dev)
    if B == 0:
        return auroc, ap, a2, pn, conf, tpr
    use_lds = n <= BOOTSTRAP_LDS_ROWS and not _BOOTSTRAP_FORCE_GLOBAL
    ws, slices = (None, 0) if use_lds else _bootstrap_workspace(dev, n, B, 2)
    ext().bootstrap_metrics(pl.y.data_ptr(), pl.gfirst.data_ptr(), pl.glast.data_ptr(), pl.map.data_ptr(), n,
                            pl.p0, pl.k0, G, ref._seed_i64(seed), b0, B, int(use_lds),
                            ws.data_ptr() if ws is not None else 0, slices, auroc.data_ptr(), ap.data_ptr(),
                            a2.data_ptr(), pn.data_ptr(), conf.data_ptr(), tpr.data_ptr(), int(grid),
                            stream_ptr(dev))
    return auroc, ap, a2, pn, conf, tpr


CALIBRATION_LDS_ROWS = 20000       # rows whose two u32 arrays fit beside the kernel's 2,176 B of scratch (csrc/calibration.hip)
CALIBRATION_MAX_BINS = 64
CALIBRATION_MAX_THRESHOLDS = 4096
_CALIBRATION_FORCE_GLOBAL = False  # tests: take the global-workspace path below the LDS limit too


def bootstrap_calibration(y, score, n_boot: int, *, seed: int = 0, stratified: bool = False, bins: int = 10,
                          thresholds: int = 99, b0: int = 0, b1=None, grid: int = 0, stream=None):
    """Bootstrap replicates ``b0:b1`` (default all ``n_boot``) of the calibration and decision-curve
    statistics of binary labels ``y [n]`` and predicted risks ``score [n]`` in [0, 1] (f32 or f64).

    The resamples are those of :func:`bootstrap_metrics` for the same ``seed``, mode and replicate.
    Returns a :class:`reference.CalibrationBootstrap` (a tuple with named fields): ``pn [B, 2]``,
    ``brier [B]`` = Σc(p−y)²/n, ``sum_p [B]`` = Σc·p, the reliability bins ``bin_n``, ``bin_pos``
    (int64) and ``bin_sum_p`` (f64) ``[B, bins]`` (bin of p = #{k ∈ 1..bins−1 : p ≥ k/bins}),
    ``dc [B, thresholds, 2]`` = TP and FP among the rows with p ≥ g/(thresholds+1), ``status [B]``
    (0 fitted, 1 one class only, 2 classes separable: no MLE, 3 iteration cap), ``coef [B, 2]`` = the
    intercept and slope of the count-weighted logistic fit of y on logit(p) (p clamped to
    [1e-12, 1 − 1e-12]; NaN unless status 0) and its Newton step count ``iters [B]``.
    ``stream``, if given, is a raw HIP stream handle: everything is enqueued on it."""
    n_boot, b0, b1 = _bootstrap_args("bootstrap_calibration", y, score, "score", n_boot, b0, b1, stratified)
    if not bool(((score >= 0) & (score <= 1)).all()):
        raise ValueError("bootstrap_calibration: score must lie in [0, 1]")
    K, T = int(bins), int(thresholds)
    if not 1 <= K <= CALIBRATION_MAX_BINS:
        raise ValueError(f"bootstrap_calibration: bins = {K} outside 1..{CALIBRATION_MAX_BINS}")
    if not 1 <= T <= CALIBRATION_MAX_THRESHOLDS:
        raise ValueError(f"bootstrap_calibration: thresholds = {T} outside 1..{CALIBRATION_MAX_THRESHOLDS}")
    kw = dict(seed=seed, stratified=bool(stratified), bins=K, thresholds=T, b0=b0, b1=b1)
    if not score.is_cuda:
        return ref.bootstrap_calibration(y, score, n_boot, **kw)
    return _on_stream(stream, score.device, _calibration_device, y, score, grid=grid, **kw)


def _calibration_device(y, score, *, seed, stratified, bins, thresholds, b0, b1, grid):
    """Validated ``cuda`` inputs; everything is enqueued on torch's current stream."""
    from . import ext, stream_ptr
    dev = score.device
    pl = ref.CalibrationPlan(y, score, stratified, bins, thresholds)
    n, K, T, B = pl.n, bins, thresholds, b1 - b0
    f64, i64 = torch.float64, torch.int64

    def e(*shape, dtype):
        return torch.empty(*shape, dtype=dtype, device=dev)
    out = ref.CalibrationBootstrap(e(B, 2, dtype=i64), e(B, dtype=f64), e(B, dtype=f64), e(B, K, dtype=i64),
                                   e(B, K, dtype=i64), e(B, K, dtype=f64), e(B, T, 2, dtype=i64), e(B, dtype=i64),
                                   e(B, 2, dtype=f64), e(B, dtype=i64))
    if B == 0:
        return out
    use_lds = n <= CALIBRATION_LDS_ROWS and not _CALIBRATION_FORCE_GLOBAL
    ws, slices = (None, 0) if use_lds else _bootstrap_workspace(dev, n, B, 2)
    ext().bootstrap_calibration(pl.y.data_ptr(), pl.map.data_ptr(), pl.p.data_ptr(), pl.l.data_ptr(),
                                pl.bin_end.data_ptr(), pl.thr_prefix.data_ptr(), n, pl.p0, K, T,
                                ref._seed_i64(seed), b0, B, int(use_lds), ws.data_ptr() if ws is not None else 0,
                                slices, *(t.data_ptr() for t in out), int(grid), stream_ptr(dev))
    return out


COMPARE_LDS_ROWS = 13000           # rows whose three u32 arrays fit beside the kernel's 1,664 B of scratch (csrc/compare.hip)
COMPARE_MAX_MODELS = 8
_COMPARE_FORCE_GLOBAL = False      # tests: take the global-workspace path below the LDS limit too


def bootstrap_compare(y, scores, n_boot: int, *, seed: int = 0, stratified: bool = False, threshold: float = 0.5,
                      b0: int = 0, b1=None, grid: int = 0, stream=None):
    """Bootstrap replicates ``b0:b1`` (default all ``n_boot``) of the held-out metrics of ``M`` score
    columns ``scores [M, n]`` (f32 or f64) for binary labels ``y [n]``, all scored on the SAME
    resamples: those of :func:`bootstrap_metrics` for the same ``seed``, mode and replicate.  Column 0
    is the reference model, columns 1..M−1 its comparators.

    Returns a :class:`reference.CompareBootstrap` (a tuple with named fields): ``auroc [B, M]`` =
    ``a2 / (2·P_b·N_b)`` and ``ap [B, M]`` (f64; NaN for a degenerate replicate), the exact doubled
    AUROC numerators ``a2 [B, M]``, the class totals ``pn [B, 2]``, ``conf [B, M, 4]`` = TP, FP, FN, TN at
    ``score > threshold``, ``reclass [B, M, 4]`` = (eu, ed, nu, nd): drawn events above the threshold
    under column 0 but not under column m (the reference moves the event up), the reverse, and the same
    two patterns over the drawn non-events (column 0: zeros), and ``sums [B, M, 3]`` (f64) = Σc·p over
    the drawn positives, over the drawn negatives, and Σc·(p − y)².
    ``stream``, if given, is a raw HIP stream handle: everything is enqueued on it."""
    n_boot, b0, b1 = _bootstrap_args("bootstrap_compare", y, scores, "scores", n_boot, b0, b1, stratified)
    M = scores.shape[0]
    if not 1 <= M <= COMPARE_MAX_MODELS:
        raise ValueError(f"bootstrap_compare: scores has M = {M} columns outside 1..{COMPARE_MAX_MODELS}")
    if threshold != threshold:
        raise ValueError("bootstrap_compare: threshold is NaN")
    kw = dict(seed=seed, stratified=bool(stratified), threshold=float(threshold), b0=b0, b1=b1)
    if not scores.is_cuda:
        return ref.bootstrap_compare(y, scores, n_boot, **kw)
    return _on_stream(stream, scores.device, _compare_device, y, scores, grid=grid, **kw)


def _compare_device(y, scores, *, seed, stratified, threshold, b0, b1, grid):
    """Validated ``cuda`` inputs; everything is enqueued on torch's current stream."""
    from . import ext, stream_ptr
    dev = scores.device
    pl = ref.ComparePlan(y, scores, stratified, threshold)
    n, M, B = pl.n, pl.M, b1 - b0
    f64, i64 = torch.float64, torch.int64

    def e(*shape, dtype):
        return torch.empty(*shape, dtype=dtype, device=dev)
    out = ref.CompareBootstrap(e(B, M, dtype=f64), e(B, M, dtype=f64), e(B, M, dtype=i64), e(B, 2, dtype=i64),
                               e(B, M, 4, dtype=i64), e(B, M, 4, dtype=i64), e(B, M, 3, dtype=f64))
    if B == 0:
        return out
    use_lds = n <= COMPARE_LDS_ROWS and not _COMPARE_FORCE_GLOBAL
    ws, slices = (None, 0) if use_lds else _bootstrap_workspace(dev, n, B, 3)
    ext().bootstrap_compare(pl.y.data_ptr(), pl.rowmap.data_ptr() if pl.rowmap is not None else 0,
                            pl.order.data_ptr(), pl.ys.data_ptr(), pl.gfirst.data_ptr(), pl.glast.data_ptr(),
                            pl.k0.data_ptr(), pl.hi.data_ptr(), pl.p.data_ptr(), n, pl.p0, M, ref._seed_i64(seed),
                            b0, B, int(use_lds), ws.data_ptr() if ws is not None else 0, slices,
                            *(t.data_ptr() for t in out), int(grid), stream_ptr(dev))
    return out


PERMUTE_MAX_N = BOOTSTRAP_MAX_N    # row index i < 2^25 shares the counter with the repeat
PERMUTE_MAX_R = BOOTSTRAP_MAX_B    # repeat index r < 2^24
PERMUTE_MAX_F = 64                 # stack_infer's limit
PERMUTE_WS_BYTES = 256 << 20       # byte budget of the score workspace S (score rows (k, r) are chunked)
PERMUTE_LDS_ROWS = 12500           # rows whose 13 B (u32 key, two u32 cumulative counts, u8 label) fit the CU's 160 KiB LDS beside 544 B of scratch (csrc/permute.hip)
_PERMUTE_FORCE_GLOBAL = False      # tests: take the presorted global path below the LDS limit too


def permutation_sources(n: int, r0: int, r1: int, seed: int = 0, device="cpu"):
    """``src [r1 − r0, n]`` (int32): row r is the permutation of repeat ``r0 + r`` under the law of
    ``reference.permutation_sources`` — the stable ascending argsort of counter-based keys, int64 torch
    ops on either device, so the tensor is the same on ``cpu`` and ``cuda`` and repeat r does not depend
    on the range it is computed in."""
    n, r0, r1 = int(n), int(r0), int(r1)
    if not 1 <= n <= PERMUTE_MAX_N:
        raise ValueError(f"permutation_sources: n = {n} outside 1..{PERMUTE_MAX_N}")
    if not 0 <= r0 <= r1 <= PERMUTE_MAX_R:
        raise ValueError(f"permutation_sources: r0:r1 = {r0}:{r1} is not a range within 0..{PERMUTE_MAX_R}")
    return ref.permutation_sources(n, r0, r1, seed, device)


def _permute_x_args(op: str, x, pk):
    if x.dim() != 2:
        raise ValueError(f"{op}: x {tuple(x.shape)} must be [n, F]")
    n, F = x.shape
    if F != pk.F:
        raise ValueError(f"{op}: x has {F} features, model has {pk.F}")
    if F > PERMUTE_MAX_F:
        raise ValueError(f"{op}: the fused stack is limited to {PERMUTE_MAX_F} features, got {F}")
    if n == 0:
        raise ValueError(f"{op}: x is empty (n = 0)")
    if n > PERMUTE_MAX_N:
        raise ValueError(f"{op}: x has {n} rows, the limit is n <= {PERMUTE_MAX_N}")
    if x.device != pk.mean.device:
        raise ValueError(f"{op}: x and the packed model must be on the same device")
    if not x.is_floating_point() or not bool(torch.isfinite(x.to(torch.float32)).all()):
        raise ValueError(f"{op}: x must be finite floating point")


def stack_permute_scores(x, pk, src, features, *, grid: int = 0, stream=None):
    """Scores of the permuted cohort: ``S [K, R, n]`` with ``S[kf, r, i]`` = P(class 1) of ``x[i]`` with
    column ``k = features[kf]`` replaced by ``x[src[r, i], k]`` (``k = −1``: the row as it is).

    ``x``: [n, F] f32 or f64 on ``pk``'s device (rounded to f32 as ``stack_infer`` does); ``src``: [R, n]
    integer with values in [0, n) on the same device; ``features``: a sequence or 1-D integer tensor of
    columns in [−1, F).  Returns f32 on ``cuda`` (one fused kernel; the hybrid rows never reach HBM and
    ``S`` is bit-identical for every ``grid``), the f64 mirror on the host.  ``K·R·n`` must stay below 2^31:
    :func:`permutation_importance` chunks.  ``stream``, if given, is a raw HIP stream handle."""
    op = "stack_permute_scores"
    _permute_x_args(op, x, pk)
    n, F = x.shape
    if src.dim() != 2 or src.shape[1] != n or src.shape[0] < 1:
        raise ValueError(f"{op}: src {tuple(src.shape)} must be [R, {n}] with R >= 1")
    if src.is_floating_point() or src.dtype == torch.bool:
        raise ValueError(f"{op}: src must be integer")
    if src.device != x.device:
        raise ValueError(f"{op}: x and src must be on the same device")
    if bool(((src < 0) | (src >= n)).any()):
        raise ValueError(f"{op}: src must hold row indices in [0, {n})")
    feat = torch.as_tensor(features, dtype=torch.int64).reshape(-1).cpu()
    K, R = feat.numel(), src.shape[0]
    if K < 1 or bool(((feat < -1) | (feat >= F)).any()):
        raise ValueError(f"{op}: features must be a non-empty list of columns in [-1, {F})")
    if K * R * n >= 1 << 31:
        raise ValueError(f"{op}: K*R*n = {K * R * n} must stay below 2^31")
    if not x.is_cuda:
        return ref.stack_permute_scores(x, pk, src, feat)
    return _on_stream(stream, x.device, _permute_scores_device, x, pk, src, feat, grid)


def _permute_scores_device(x, pk, src, feat, grid: int, xt=None):
    """Validated ``cuda`` inputs; everything is enqueued on torch's current stream."""
    from . import ext, stream_ptr
    dev = x.device
    n, F = x.shape
    x32 = _c(x, torch.float32)
    if xt is None:
        xt = x32.t().contiguous()       # column-major copy: the gathered value is one 4-byte read
    s32 = _c(src, torch.int32)
    k32 = feat.to(device=dev, dtype=torch.int32).contiguous()
    K, R = k32.numel(), s32.shape[0]
    S = torch.empty(K, R, n, dtype=torch.float32, device=dev)
    ext().stack_permute(x32.data_ptr(), xt.data_ptr(), n, s32.data_ptr(), R, k32.data_ptr(), K,
                        *_stack_model_args(pk), S.data_ptr(), int(grid), stream_ptr(dev))
    return S


def _labels_args(op: str, y, n: int, device):
    if y.dim() != 1 or y.numel() != n:
        raise ValueError(f"{op}: y {tuple(y.shape)} must be [n] with n = {n}")
    if y.device != device:
        raise ValueError(f"{op}: y must be on the device of the rows it labels")
    if not bool(((y == 0) | (y == 1)).all()):
        raise ValueError(f"{op}: y must hold labels 0 and 1 only")
    P = int((y == 1).sum())
    if P == 0 or P == n:
        raise ValueError(f"{op}: both classes must be present in y")


def rank_metrics(y, scores, *, grid: int = 0, stream=None):
    """Rank every row of ``scores [M, n]`` (f32 or f64) against the binary labels ``y [n]`` on one
    device: M models or M score vectors in one launch.  Returns a :class:`reference.RankMetrics` (a tuple
    with named fields): ``a2 [M]`` (int64), the exact doubled AUROC numerator over tie groups, ``auroc`` =
    ``a2 / (2·P·N)``, ``ap`` (average precision, ties grouped) and ``brier`` = ``Σ(score − y)² / n`` (f64).
    On ``cuda`` the scores are rounded to f32 and each row is sorted inside the kernel up to
    ``PERMUTE_LDS_ROWS`` rows; above that ``torch.sort`` orders them and the same kernel runs on its
    presorted path.  ``a2`` and ``auroc`` do not depend on the path.  ``stream``: a raw HIP stream handle."""
    op = "rank_metrics"
    if scores.dim() != 2 or y.dim() != 1 or scores.shape[1] != y.numel():
        raise ValueError(f"{op}: y {tuple(y.shape)} must be [n] and scores {tuple(scores.shape)} [M, n] of one length n")
    n = y.numel()
    if n == 0:
        raise ValueError(f"{op}: y and scores are empty (n = 0)")
    if n > PERMUTE_MAX_N:
        raise ValueError(f"{op}: y has {n} rows, the limit is n <= {PERMUTE_MAX_N}")
    if not scores.is_floating_point() or not bool(torch.isfinite(scores).all()):
        raise ValueError(f"{op}: scores must be finite floating point")
    _labels_args(op, y, n, scores.device)
    if not scores.is_cuda:
        return ref.rank_metrics(y, scores)
    return _on_stream(stream, scores.device, _rank_device, y, scores, grid)


def _rank_device(y, scores, grid: int):
    """Validated ``cuda`` inputs; everything is enqueued on torch's current stream."""
    from . import ext, stream_ptr
    dev = scores.device
    S = _c(scores, torch.float32)
    M, n = S.shape
    y8 = (y > 0).to(torch.uint8).contiguous()
    f64 = torch.float64
    out = ref.RankMetrics(torch.empty(M, dtype=torch.int64, device=dev), torch.empty(M, dtype=f64, device=dev),
                          torch.empty(M, dtype=f64, device=dev), torch.empty(M, dtype=f64, device=dev))
    sp = stream_ptr(dev)
    if n <= PERMUTE_LDS_ROWS and not _PERMUTE_FORCE_GLOBAL:
        ext().rank_rows(S.data_ptr(), y8.data_ptr(), 0, 0, n, M, 1, 0, 0, *(t.data_ptr() for t in out),
                        int(grid), sp)
        return out
    # presorted path.  The arrays this function keeps stay within BOOTSTRAP_WS_BYTES: at most half of it
    # for the scan arrays (8n B per resident workgroup; 8n <= 2^28 B), the rest for the presorted rows of a
    # chunk (13n B per score row: 4 B sorted score + 8 B sort index + 1 B label; 13n < 2^29 B).
    # torch.sort's own temporaries come on top of that
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    slices = max(1, min(M, 2 * ncu, (BOOTSTRAP_WS_BYTES // 2) // (8 * n)))
    ws = torch.empty(slices, 2 * n, dtype=torch.int32, device=dev)
    per = max(1, (BOOTSTRAP_WS_BYTES - 8 * n * slices) // (13 * n))
    for c0 in range(0, M, per):
        c1 = min(M, c0 + per)
        ss, order = torch.sort(S[c0:c1], dim=1, descending=True)
        ys = y8[order].contiguous()
        ext().rank_rows(S[c0:c1].data_ptr(), y8.data_ptr(), ss.data_ptr(), ys.data_ptr(), n, c1 - c0, 0,
                        ws.data_ptr(), slices, *(t[c0:c1].data_ptr() for t in out), int(grid), sp)
    return out


def permutation_importance(x, y, pk, n_repeats: int, *, seed: int = 0, features=None, r0: int = 0, r1=None,
                           grid: int = 0, stream=None):
    """Permutation importance of the fused stack on the held-out rows ``x [n, F]`` with labels ``y [n]``.

    Repeat r permutes the rows by ``permutation_sources`` (one permutation per repeat, shared by every
    column: a paired design); column k of repeat r is scored on ``x`` with column k taken from the
    permuted rows, and every score row is ranked against ``y`` (:func:`stack_permute_scores`,
    :func:`rank_metrics`: two fused kernels on ``cuda``, the f64 mirrors on the host).  The baseline is
    the unpermuted cohort through the same two ops.  Returns ``(baseline, importances)``: ``baseline`` =
    ``{"auroc", "ap", "brier"}`` (floats) and ``importances[metric]`` = ``[F', R]`` f64 for the columns
    ``features`` (default all) and repeats ``r0:r1`` (default all ``n_repeats``): ``baseline − permuted``
    for ``auroc`` and ``ap``, ``permuted − baseline`` for ``brier`` — positive means the variable helps.
    Score rows are chunked so that ``S`` stays under ``PERMUTE_WS_BYTES``; no result depends on the
    chunking, the range or ``grid``.  ``stream``, if given, is a raw HIP stream handle."""
    op = "permutation_importance"
    _permute_x_args(op, x, pk)
    n, F = x.shape
    _labels_args(op, y, n, x.device)
    n_repeats = int(n_repeats)
    if not 1 <= n_repeats <= PERMUTE_MAX_R:
        raise ValueError(f"{op}: n_repeats = {n_repeats} outside 1..{PERMUTE_MAX_R}")
    r1 = n_repeats if r1 is None else int(r1)
    r0 = int(r0)
    if not 0 <= r0 <= r1 <= n_repeats:
        raise ValueError(f"{op}: r0:r1 = {r0}:{r1} is not a range within 0..n_repeats = {n_repeats}")
    cols = list(range(F)) if features is None else [int(k) for k in features]
    if not cols or any(not 0 <= k < F for k in cols):
        raise ValueError(f"{op}: features must be a non-empty list of columns in [0, {F})")
    return _on_stream(stream if x.is_cuda else None, x.device, _permutation_importance, x, y, pk, cols, seed,
                      r0, r1, grid)


def _permutation_importance(x, y, pk, cols, seed, r0, r1, grid):
    dev = x.device
    n = x.shape[0]
    K, R = len(cols), r1 - r0
    if x.is_cuda:
        x = _c(x, torch.float32)
        xt = x.t().contiguous()

        def score(src, feat):
            return _permute_scores_device(x, pk, src, torch.as_tensor(feat), grid, xt=xt)

        def rank(S):
            return _rank_device(y, S.reshape(-1, n), grid)
    else:
        def score(src, feat):
            return ref.stack_permute_scores(x, pk, src, torch.as_tensor(feat))

        def rank(S):
            return ref.rank_metrics(y, S.reshape(-1, n))
    ident = torch.arange(n, dtype=torch.int32, device=dev)[None, :]
    b = rank(score(ident, [-1]))
    base = {"auroc": b.auroc[0], "ap": b.ap[0], "brier": b.brier[0]}
    perm = {m: torch.empty(K, R, dtype=torch.float64, device=dev) for m in base}
    rows = max(1, PERMUTE_WS_BYTES // (4 * n))        # score rows (k, r) per chunk of S
    rc = min(R, rows)                                 # repeats per chunk, then columns per chunk
    kc = max(1, rows // rc) if rc == R else 1
    for c0 in range(0, R, rc):
        c1 = min(R, c0 + rc)
        src = ref.permutation_sources(n, r0 + c0, r0 + c1, seed, dev)
        for k0 in range(0, K, kc):
            k1 = min(K, k0 + kc)
            m = rank(score(src, cols[k0:k1]))
            for name in perm:
                perm[name][k0:k1, c0:c1] = getattr(m, name).reshape(k1 - k0, c1 - c0)
    imp = {"auroc": base["auroc"] - perm["auroc"], "ap": base["ap"] - perm["ap"],
           "brier": perm["brier"] - base["brier"]}
    return {k: float(v) for k, v in base.items()}, imp


def expit(x):
    return torch.sigmoid(x)


def weighted_moments(X, W, V=None):
    """``G[p] = Σ_n W[p,n] x_n x_nᵀ``, ``a[p] = Σ_n W[p,n] x_n``, ``v[p] = Σ_n V[p,n] x_n`` (f64)."""
    X = X.to(torch.float64).contiguous()
    W = W.to(torch.float64).contiguous()
    n, F = X.shape
    P = W.shape[0]
    if X.is_cuda:
        from . import ext, stream_ptr
        C = (n + 127) // 128
        npairs = F * (F + 1) // 2
        Gp = torch.empty(P, C, npairs, dtype=torch.float64, device=X.device)
        ap = torch.empty(P, C, F, dtype=torch.float64, device=X.device)
        vp = torch.empty(P, C, F, dtype=torch.float64, device=X.device)
        Vc = V.to(torch.float64).contiguous() if V is not None else None
        ext().weighted_moments(X.data_ptr(), n, F, W.data_ptr(), Vc.data_ptr() if Vc is not None else 0,
                               P, Gp.data_ptr(), ap.data_ptr(), vp.data_ptr(), stream_ptr(X.device))
        Gu = Gp.sum(1)
        iu = torch.triu_indices(F, F, device=X.device)
        G = torch.zeros(P, F, F, dtype=torch.float64, device=X.device)
        G[:, iu[0], iu[1]] = Gu
        G[:, iu[1], iu[0]] = Gu
        return G, ap.sum(1), (vp.sum(1) if V is not None else None)
    G = torch.einsum("pn,ni,nj->pij", W, X, X)
    a = W @ X
    v = V.to(torch.float64) @ X if V is not None else None
    return G, a, v
