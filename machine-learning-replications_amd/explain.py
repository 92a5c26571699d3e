"""Exact Shapley attributions for a fitted HF stack.

The stack is not additive (three sigmoids feed a fourth; the SVC is an RBF expansion), so the
question "which variable moved this patient's risk, and by how much" is answered by the
interventional Shapley value of each feature against a background cohort.  The stack always
sees at most 20 columns (17 for the shipped model), so all 2^F coalitions are enumerated
exactly — no sampling, no KernelSHAP regression — by :func:`hfens.ops.stack_shapley`: one fused
HIP kernel on ``cuda``, the f64 mirror on the host.  :func:`hfens.ops.stack_shapley_interactions`
reduces the same coalition table to the Shapley interaction values of every pair as well.

Bit convention: feature k is "present" (takes the patient's value) in coalition S when bit k of
S is set; absent features take a background row's value.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from . import ops


@dataclass
class Explanation:
    phi: torch.Tensor           # [n, F] f64: phi[i].sum() == prediction[i] − base_value
    base_value: float           # mean risk of the background cohort
    prediction: torch.Tensor    # [n] f64 P(class 1) of each explained row
    feature_names: List[str]


class StackExplainer:
    def __init__(self, model, background=None, device="cuda", feature_names: Optional[List[str]] = None):
        self.device = torch.device(device)
        if self.device.type == "cuda":
            ops.ext()
        self.model = model.to(self.device)
        self.pk = model._packed_stack(self.device)
        if self.pk is None:
            raise ValueError("model is not an HF-shaped stack (scaler+SVC, GBC, LR -> LR)")
        F = self.pk.F
        if background is None:
            from .io.synth import MODEL_FEATURES, make_hf_cohort
            if F != len(MODEL_FEATURES):
                raise ValueError(f"the default background is the {len(MODEL_FEATURES)}-feature HF cohort; "
                                 f"a {F}-feature stack needs an explicit background")
            background = make_hf_cohort(128, F, seed=0, nan_frac=0.0)[0]
            feature_names = feature_names or list(MODEL_FEATURES)
        bg = torch.as_tensor(background, dtype=torch.float64)
        if bg.dim() != 2 or bg.shape[0] < 1 or bg.shape[1] != F:
            raise ValueError(f"background must be a non-empty [B, {F}] array")
        self.background = bg.to(self.device).contiguous()
        self.feature_names = list(feature_names) if feature_names else [f"x{k}" for k in range(F)]
        if len(self.feature_names) != F:
            raise ValueError(f"expected {F} feature names")

    def shap_values(self, X) -> Explanation:
        X = torch.as_tensor(X, dtype=torch.float64)
        if X.dim() == 1:
            X = X[None, :]
        phi, base, pred = ops.stack_shapley(X.to(self.device), self.background, self.pk)
        return Explanation(phi, float(base), pred, list(self.feature_names))

    def mean_abs(self, X) -> torch.Tensor:
        """Global importance over a cohort: mean |phi| per feature ([F] f64)."""
        return self.shap_values(X).phi.abs().mean(0)

    def shap_interaction_values(self, X) -> "InteractionExplanation":
        """Exact Shapley interaction values of each row of ``X`` (:func:`hfens.ops.stack_shapley_interactions`);
        ``phi``, ``base_value`` and ``prediction`` are :meth:`shap_values`'s, bit for bit."""
        X = torch.as_tensor(X, dtype=torch.float64)
        if X.dim() == 1:
            X = X[None, :]
        Phi, phi, base, pred = ops.stack_shapley_interactions(X.to(self.device), self.background, self.pk)
        return InteractionExplanation(Phi, phi, float(base), pred, list(self.feature_names))

    # ------------------------------------------------------------------ partial dependence
    def _columns(self, features) -> List[int]:
        F = self.pk.F
        if features is None:
            return list(range(F))
        cols = [self.feature_names.index(f) if isinstance(f, str) else int(f) for f in features]
        if any(not 0 <= k < F for k in cols):
            raise ValueError(f"feature indices must lie in [0, {F})")
        return cols

    def grid(self, k: int, points: int = 32) -> torch.Tensor:
        """Grid of column ``k``: the sorted distinct background values if there are at most
        ``points`` of them, else ``points`` equally spaced values from the column's minimum to its
        maximum, inclusive.  f64 values rounded to f32 (what the kernel sees)."""
        col = _f32(self.background[:, k])
        u = torch.unique(col)                                     # sorted
        if u.numel() <= points:
            return u
        g = _f32(torch.linspace(float(u[0]), float(u[-1]), points, dtype=torch.float64, device=col.device))
        g[0], g[-1] = u[0], u[-1]
        return g

    def _single_cells(self, cols, grids):
        """One cell ``(k, v, -1, 0)`` per grid point, column after column."""
        feat = torch.cat([torch.tensor([[k, -1]], device=self.device).expand(g.numel(), 2)
                          for k, g in zip(cols, grids)])
        value = torch.cat([torch.stack([g, torch.zeros_like(g)], 1) for g in grids])
        return feat.contiguous(), value

    def partial_dependence(self, features=None, points: int = 32) -> "PartialDependence":
        """Partial-dependence curve of each chosen column over the background cohort:
        ``pd[g]`` = mean risk with the column set to ``grid[g]`` in every row (one op call)."""
        cols = self._columns(features)
        grids = [self.grid(k, points) for k in cols]
        feat, value = self._single_cells(cols, grids)
        pd = ops.stack_partial(self.background, self.pk, feat, value)
        curves = list(torch.split(pd, [g.numel() for g in grids]))
        return PartialDependence(cols, [self.feature_names[k] for k in cols], grids, curves)

    def what_if(self, x, features=None, points: int = 32) -> "WhatIf":
        """ICE curves of the patients ``x`` ([m, F] or [F]): each patient's risk as one column moves
        over its grid with everything else as entered.  The patients' own values are merged into
        each grid (sorted, de-duplicated), so every curve passes through the patient's prediction.
        Also returns the background cohort's PD on the same grids."""
        X = torch.as_tensor(x, dtype=torch.float64)
        if X.dim() == 1:
            X = X[None, :]
        X = _f32(X.to(self.device))
        cols = self._columns(features)
        grids = [torch.unique(torch.cat([self.grid(k, points), X[:, k]])) for k in cols]
        feat, value = self._single_cells(cols, grids)
        plain = torch.tensor([[-1, -1]], device=self.device)      # last cell: the row as entered
        _, ice = ops.stack_partial(X, self.pk, torch.cat([feat, plain]),
                                   torch.cat([value, torch.zeros(1, 2, dtype=value.dtype, device=self.device)]),
                                   return_ice=True)
        ice = ice.to(torch.float64)
        cohort = ops.stack_partial(self.background, self.pk, feat, value)
        sizes = [g.numel() for g in grids]
        return WhatIf(cols, [self.feature_names[k] for k in cols], grids,
                      list(torch.split(ice[:, :-1], sizes, 1)), list(torch.split(cohort, sizes)),
                      ice[:, -1].clone(), X)

    def interaction_strength(self, X=None, pairs=None, max_rows: int = 512) -> "Interactions":
        """Friedman's H² of variable pairs over the cohort ``X`` (default: the background; all
        pairs).  Only the first ``max_rows`` rows are used — a deterministic truncation.  With
        ``a_i = PD_jk(x_ij, x_ik)``, ``b_i = PD_j(x_ij)``, ``c_i = PD_k(x_ik)`` over those rows, each
        centred by its mean over i: ``H²_jk = Σ(a_i − b_i − c_i)² / Σ a_i²`` (0 when the denominator
        is 0), in f64.  Cells are de-duplicated exactly on ``(k1, f32 v1, k2, f32 v2)`` before the
        op and scattered back afterwards."""
        F = self.pk.F
        X = self.background if X is None else torch.as_tensor(X, dtype=torch.float64).to(self.device)
        if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] != F:
            raise ValueError(f"X must be a non-empty [n, {F}] array")
        X = _f32(X[:max_rows]).contiguous()
        n = X.shape[0]
        if pairs is None:
            pairs = [(j, k) for j in range(F) for k in range(j + 1, F)]
        pairs = [tuple(self._columns(p)) for p in pairs]
        if any(len(p) != 2 or p[0] == p[1] for p in pairs):
            raise ValueError("pairs must name two different variables each")
        singles = sorted({k for p in pairs for k in p})
        dev = self.device
        pj = torch.tensor([p[0] for p in pairs], device=dev)
        pk_ = torch.tensor([p[1] for p in pairs], device=dev)
        feat, value, inv = interaction_cells(X, pairs, singles)
        pd = ops.stack_partial(X, self.pk, feat, value)[inv]
        pd2 = pd[:len(pairs) * n].reshape(len(pairs), n)
        pd1 = pd[len(pairs) * n:].reshape(len(singles), n)
        pd1 = pd1 - pd1.mean(1, keepdim=True)
        a = pd2 - pd2.mean(1, keepdim=True)
        slot = {k: i for i, k in enumerate(singles)}
        b = pd1[[slot[p[0]] for p in pairs]]
        c = pd1[[slot[p[1]] for p in pairs]]
        num, den = ((a - b - c) ** 2).sum(1), (a ** 2).sum(1)
        h = torch.where(den > 0, num / den.clamp(min=torch.finfo(torch.float64).tiny), torch.zeros_like(num))
        h2 = torch.zeros(F, F, dtype=torch.float64, device=dev)
        h2[pj, pk_] = h
        h2[pk_, pj] = h
        return Interactions(h2, n, list(self.feature_names))


    # ------------------------------------------------------------------ permutation importance
    def permutation_importance(self, X, y, n_repeats: int = 30, seed: int = 2020) -> "PermutationImportance":
        """Permutation importance of every column on the held-out rows ``X [n, F]`` with labels ``y [n]``
        (:func:`hfens.ops.permutation_importance`): how far AUROC and AP fall, and the Brier score rises,
        when the column is shuffled — ``n_repeats`` shuffles, the same ones for every column."""
        X = torch.as_tensor(X, dtype=torch.float64).to(self.device)
        y = torch.as_tensor(y).to(self.device)
        base, imp = ops.permutation_importance(X, y, self.pk, n_repeats, seed=seed)
        return PermutationImportance(list(self.feature_names), base, imp)


def interaction_cells(X: torch.Tensor, pairs, singles):
    """The cells Friedman's H² needs over cohort ``X`` ([n, F], f32-representable): for every pair
    (j, k) and row i the two-variable cell ``(j, x_ij, k, x_ik)``, then for every single k and row i
    ``(k, x_ik, -1, 0)`` — de-duplicated exactly on ``(k1, f32 v1, k2, f32 v2)``.  Returns the distinct
    cells ``feat [U, 2]``, ``value [U, 2]`` (f32) and ``inverse`` with ``pd_of_cell = pd[inverse]`` in
    [pair][row], [single][row] order."""
    n, dev = X.shape[0], X.device
    ks = torch.tensor(singles, device=dev)
    pj = torch.tensor([p[0] for p in pairs], device=dev)
    pk_ = torch.tensor([p[1] for p in pairs], device=dev)
    feat = torch.cat([torch.stack([pj, pk_], 1).repeat_interleave(n, 0),
                      torch.stack([ks, torch.full_like(ks, -1)], 1).repeat_interleave(n, 0)])
    value = torch.cat([torch.stack([X[:, pj].t().reshape(-1), X[:, pk_].t().reshape(-1)], 1),
                       torch.stack([X[:, ks].t().reshape(-1),
                                    torch.zeros(len(singles) * n, dtype=X.dtype, device=dev)], 1)])
    bits = value.to(torch.float32).view(torch.int32).to(torch.int64)
    key = torch.stack([feat[:, 0], bits[:, 0], feat[:, 1], bits[:, 1]], 1)
    ukey, inv = torch.unique(key, dim=0, return_inverse=True)
    uvalue = torch.stack([ukey[:, 1], ukey[:, 3]], 1).to(torch.int32).view(torch.float32)
    return ukey[:, [0, 2]].contiguous(), uvalue.contiguous(), inv


def _f32(t: torch.Tensor) -> torch.Tensor:
    """f64 values rounded to f32."""
    return t.to(torch.float32).to(torch.float64)


@dataclass
class InteractionExplanation:
    Phi: torch.Tensor           # [n, F, F] f64, symmetric: Phi[p, i, j] = half of the pair (i, j)'s effect (SHAP's
    #                             split); Phi[p, i, i] = the main effect; row i sums to phi[p, i]
    phi: torch.Tensor           # [n, F] f64 Shapley values
    base_value: float
    prediction: torch.Tensor    # [n] f64
    feature_names: List[str]

    def top(self, n: int, p: int = 0):
        """The ``n`` strongest pairs of row ``p`` as ``(i, j, 2·Phi[p, i, j])`` with i < j — the full pair
        effect — by descending magnitude."""
        F = self.Phi.shape[1]
        m = self.Phi[p].cpu()
        pairs = [(i, j, 2.0 * float(m[i, j])) for i in range(F) for j in range(i + 1, F)]
        return sorted(pairs, key=lambda t: -abs(t[2]))[:n]

    def mean_abs_pairs(self) -> torch.Tensor:
        """Mean over the rows of |2·Phi[p, i, j]| ([F, F] f64, zero diagonal)."""
        m = (2.0 * self.Phi).abs().mean(0)
        return m - torch.diag(torch.diag(m))


@dataclass
class PartialDependence:
    features: List[int]          # column of each curve
    feature_names: List[str]
    grids: List[torch.Tensor]    # per curve [G] f64 (f32-representable)
    pd: List[torch.Tensor]       # per curve [G] f64: mean risk of the background with the column set to grid[g]


@dataclass
class WhatIf:
    features: List[int]
    feature_names: List[str]
    grids: List[torch.Tensor]    # per variable [G] f64: the background grid merged with the patients' own values
    risk: List[torch.Tensor]     # per variable [m, G] f64: each patient's risk along the grid (ICE)
    cohort: List[torch.Tensor]   # per variable [G] f64: PD of the background cohort on the same grid
    prediction: torch.Tensor     # [m] f64 P(class 1) of each patient as entered
    x: torch.Tensor              # [m, F] f64 the patients, rounded to f32


@dataclass
class PermutationImportance:
    names: List[str]
    baseline: Dict[str, float]            # auroc, ap, brier of the rows as they are
    importances: Dict[str, torch.Tensor]  # metric → [F, R] f64; positive: the variable helps (auroc, ap: the
    #                                       fall under permutation; brier: the rise)

    def mean(self, metric: str = "auroc") -> torch.Tensor:
        return self.importances[metric].mean(1)

    def std(self, metric: str = "auroc") -> torch.Tensor:
        """Sample standard deviation over the repeats (ddof = 1; NaN with one repeat)."""
        v = self.importances[metric]
        if v.shape[1] < 2:
            return torch.full((v.shape[0],), float("nan"), dtype=v.dtype, device=v.device)
        return v.std(1, unbiased=True)

    def interval(self, metric: str = "auroc", level: float = 0.95):
        """Percentile interval over the repeats: ``(lo [F], hi [F])``."""
        a = (1.0 - level) / 2.0
        q = torch.tensor([a, 1.0 - a], dtype=torch.float64, device=self.importances[metric].device)
        lo, hi = torch.quantile(self.importances[metric], q, dim=1)
        return lo, hi

    def top(self, n: int, metric: str = "auroc"):
        """The ``n`` most important variables as ``(k, name, mean importance)``, descending (ties: by column)."""
        m = self.mean(metric).cpu().tolist()
        order = sorted(range(len(m)), key=lambda k: (-m[k], k))
        return [(k, self.names[k], m[k]) for k in order[:n]]


@dataclass
class Interactions:
    h2: torch.Tensor             # [F, F] f64 Friedman's H², symmetric, zero diagonal (and zero for pairs not asked for)
    n_rows: int                  # cohort rows used (the first max_rows)
    feature_names: List[str]

    def top(self, n: int):
        """The ``n`` strongest pairs as ``(j, k, H²)`` with j < k, descending."""
        F = self.h2.shape[0]
        h = self.h2.cpu()
        pairs = [(j, k, float(h[j, k])) for j in range(F) for k in range(j + 1, F)]
        return sorted(pairs, key=lambda t: -t[2])[:n]
