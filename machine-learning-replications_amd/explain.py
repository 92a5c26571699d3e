"""Exact Shapley attributions for a fitted HF stack.

The stack is not additive (three sigmoids feed a fourth; the SVC is an RBF expansion), so the
question "which variable moved this patient's risk, and by how much" is answered by the
interventional Shapley value of each feature against a background cohort.  The stack always
sees at most 20 columns (17 for the shipped model), so all 2^F coalitions are enumerated
exactly — no sampling, no KernelSHAP regression — by :func:`hfens.ops.stack_shapley`: one fused
HIP kernel on ``cuda``, the f64 mirror on the host.

Bit convention: feature k is "present" (takes the patient's value) in coalition S when bit k of
S is set; absent features take a background row's value.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

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
