"""Plain-PyTorch reference implementations of every device op.

These define the semantics the gfx950 HIP kernels must reproduce and run the
host (CPU) path.  They follow the algorithms the reference delegates to
(libsvm / sklearn trees / liblinear), re-derived from the published math; see
the per-function notes and SURVEY.md §2.2 (E2-E12).

GBDT training oracles (Python ints, Fractions, longdouble; nothing shared with
models/hist_gbdt.py): ``gbdt_q``, ``gbdt_hist_oracle``, ``gbdt_split_oracle`` (with
``GbdtSplit.certify`` and ``gbdt_split_children``), ``gbdt_bag_oracle``,
``gbdt_route_oracle``, ``gbdt_route_r2_oracle``, ``gbdt_apply_prep_oracle``.

Nyström interior-point SVC oracles (numpy longdouble and plain f64; nothing shared with
models/svc_lowrank.py): ``wgram_oracle``, ``phi_mv_oracle``, ``phit_oracle``, ``rbf_oracle_f64``,
``chol_certificate``, ``chol_solve_certificate``, ``ipm_rows_oracle``, ``svc_dual_certificate``.
"""
from __future__ import annotations

import math

import torch

LOG2E = 1.4426950408889634


# ----------------------------------------------------------------------------- SVC inference
def rbf_decision(z: torch.Tensor, sv: torch.Tensor, coef: torch.Tensor, gamma: float,
                 intercept: float, chunk: int = 65536) -> torch.Tensor:
    """``dec_i = Σ_j coef_j · exp(-γ‖z_i − sv_j‖²) + intercept`` (libsvm ``svm_predict_values``,
    RBF kernel ``k(x,y)=exp(-γ‖x−y‖²)``)."""
    out = torch.empty(z.shape[0], dtype=z.dtype, device=z.device)
    for s in range(0, z.shape[0], chunk):
        zz = z[s:s + chunk]
        d2 = ((zz[:, None, :] - sv[None, :, :]) ** 2).sum(-1)
        out[s:s + chunk] = torch.exp(-gamma * d2) @ coef + intercept
    return out


def sigmoid_predict(dec: torch.Tensor, A: float, B: float) -> torch.Tensor:
    """Platt ``1/(1+exp(A·f+B))`` evaluated in libsvm's overflow-safe form."""
    fApB = dec * A + B
    pos = torch.exp(-fApB.clamp(min=0)) / (1.0 + torch.exp(-fApB.clamp(min=0)))
    neg = 1.0 / (1.0 + torch.exp(fApB.clamp(max=0)))
    return torch.where(fApB >= 0, pos, neg)


def couple2(r01: torch.Tensor, max_iter: int = 100) -> torch.Tensor:
    """Two-class pairwise coupling (Wu, Lin & Weng 2004, method 2 — the iterative
    solver libsvm's ``multiclass_probability`` runs even for k = 2), vectorised over
    rows.  Input r01 = P(class 0 | {0,1}); returns p1 = P(class 1).  Stopping rule
    ``max_t |(Qp)_t − pᵀQp| < 0.005/k``."""
    r10 = 1.0 - r01
    q00 = r10 * r10
    q11 = r01 * r01
    q01 = -r10 * r01
    p0 = torch.full_like(r01, 0.5)
    p1 = torch.full_like(r01, 0.5)
    eps = 0.005 / 2
    active = torch.ones_like(r01, dtype=torch.bool)
    for _ in range(max_iter):
        qp0 = q00 * p0 + q01 * p1
        qp1 = q01 * p0 + q11 * p1
        pqp = p0 * qp0 + p1 * qp1
        err = torch.maximum((qp0 - pqp).abs(), (qp1 - pqp).abs())
        active = active & ~(err < eps)
        if not bool(active.any()):
            break
        # t = 0 update
        d = (-qp0 + pqp) / q00
        np0 = p0 + d
        npqp = (pqp + d * (d * q00 + 2 * qp0)) / (1 + d) / (1 + d)
        nqp0 = (qp0 + d * q00) / (1 + d)
        nqp1 = (qp1 + d * q01) / (1 + d)
        np0 = np0 / (1 + d)
        np1 = p1 / (1 + d)
        # t = 1 update
        d = (-nqp1 + npqp) / q11
        np1 = np1 + d
        np0 = np0 / (1 + d)
        np1 = np1 / (1 + d)
        p0 = torch.where(active, np0, p0)
        p1 = torch.where(active, np1, p1)
    return p1


def svc_proba1(dec: torch.Tensor, A: float, B: float) -> torch.Tensor:
    """libsvm ``svm_predict_probability`` for two classes → P(class 1)."""
    r01 = sigmoid_predict(dec, A, B).clamp(1e-7, 1 - 1e-7)
    return couple2(r01)


# ----------------------------------------------------------------------------- tree inference
def tree_raw(x: torch.Tensor, feature: torch.Tensor, threshold: torch.Tensor, left: torch.Tensor,
             right: torch.Tensor, value: torch.Tensor, init: float, lr: float) -> torch.Tensor:
    """Sum of tree outputs ``init + lr·Σ_t value_t[leaf_t(x)]``.  Decision rule
    ``float32(x[f]) <= threshold`` → left (sklearn compares the float32-cast input
    against the float64 threshold).  Arrays are [T, K] node tables, leaves have
    feature < 0."""
    x32 = x.to(torch.float32).to(torch.float64)
    n = x.shape[0]
    T = feature.shape[0]
    # all trees walk together ([T, n] node ids, one step per level: a handful of tensor ops
    # instead of ~10 per tree), then the per-tree contributions are added in tree order
    # (cumsum over [init, lr·v_0, …] reproduces sklearn's sequential raw += lr·v_t rounding)
    node = torch.zeros(T, n, dtype=torch.long, device=x.device)
    cols = torch.arange(n, device=x.device)[None, :].expand(T, n)
    feature = feature.long()
    for _ in range(feature.shape[1]):
        f = feature.gather(1, node)
        leaf = f < 0
        if bool(leaf.all()):
            break
        fv = x32[cols, f.clamp(min=0)]
        go_left = fv <= threshold.gather(1, node)
        nxt = torch.where(go_left, left.long().gather(1, node), right.long().gather(1, node))
        node = torch.where(leaf, node, nxt)
    v = value.to(torch.float64).reshape(T, feature.shape[1]).gather(1, node)          # [T, n]
    terms = torch.cat([torch.full((1, n), float(init), dtype=torch.float64, device=x.device), lr * v])
    return torch.cumsum(terms, 0)[-1]


def expit(x: torch.Tensor) -> torch.Tensor:
    return torch.sigmoid(x)


# ----------------------------------------------------------------------------- fused stack
def stack_infer(x: torch.Tensor, pk) -> torch.Tensor:
    """fp64 reference of the fused ``stack_infer`` kernel on a :class:`PackedStack` (host
    tensors): scaler → RBF SVC (Platt + coupling) / trees / L1-LR → meta LR, P(class 1)."""
    x = x.to(torch.float64)
    F = pk.F
    z = (x - pk.mean.to(torch.float64)) * pk.inv_scale.to(torch.float64)
    sv = pk.sv.svt[:F].t().to(torch.float64)
    dec = rbf_decision(z, sv, pk.sv.coef.to(torch.float64), pk.gamma, pk.svc_b)
    return _stack_tail(x, dec, pk)


def _stack_tail(x: torch.Tensor, dec: torch.Tensor, pk) -> torch.Tensor:
    """Everything of :func:`stack_infer` after the SVC decision values ``dec`` of rows ``x``."""
    F = pk.F
    p_svc = svc_proba1(dec, pk.probA, pk.probB)
    if pk.stumps is not None:
        st = pk.stumps
        x32 = x.to(torch.float32).to(torch.float64)
        raw = torch.full((x.shape[0],), st.base, dtype=torch.float64)
        off = st.off.tolist()
        for f in range(F):
            for j in range(off[f], off[f + 1]):
                t, d = float(st.pairs[j, 0]), float(st.pairs[j, 1])
                raw += (x32[:, f] > t).to(torch.float64) * d
    else:
        nd = pk.forest.nodes.reshape(pk.forest.n_trees, pk.forest.max_nodes, 4)
        thr = nd[..., 3].contiguous().view(torch.float32).to(torch.float64)
        raw = tree_raw(x, nd[..., 0], thr, nd[..., 1], nd[..., 2],
                       pk.forest.values.reshape(pk.forest.n_trees, pk.forest.max_nodes), pk.gb_init, pk.gb_lr)
    p_gbc = torch.sigmoid(raw)
    p_lg = torch.sigmoid(x @ pk.lr_w.to(torch.float64) + pk.lr_b)
    w0, w1, w2 = pk.meta_w
    return torch.sigmoid(pk.meta_b + w0 * p_svc + w1 * p_gbc + w2 * p_lg)


# ----------------------------------------------------------------------------- exact Shapley
def shapley_weights(F: int) -> torch.Tensor:
    """``w(s) = s!(F−s−1)!/F!`` for s = 0 … F−1 (f64): the weight of a coalition of size s that
    a feature joins."""
    return torch.tensor([math.factorial(s) * math.factorial(F - s - 1) / math.factorial(F)
                         for s in range(F)], dtype=torch.float64)


def coalition_values(x: torch.Tensor, background: torch.Tensor, pk, chunk: int = 16384) -> torch.Tensor:
    """``v[p, S] = mean_b P(h(S, b))`` with ``h(S, b)[k] = x[p, k]`` if bit k of S is set, else
    ``background[b, k]`` — every one of the 2^F coalitions, in chunks of ``chunk`` hybrid rows
    (the RBF kernel matrix of a chunk is all that is ever held).  The rows get
    :func:`stack_infer`'s arithmetic; only ‖sv − z‖² is formed differently: a hybrid row's
    distance is a sum of per-feature terms that take one of two values, so the chunk's distances
    are ``mask @ dxᵀ + (1 − mask) @ dbᵀ`` (two f64 GEMMs) instead of a [chunk, m, F] broadcast."""
    x = x.to(torch.float64)
    background = background.to(torch.float64)
    n, F = x.shape
    B = background.shape[0]
    nS = 1 << F
    k = torch.arange(F)
    mean, inv = pk.mean.to(torch.float64), pk.inv_scale.to(torch.float64)
    sv = pk.sv.svt[:F].t().to(torch.float64)
    coef = pk.sv.coef.to(torch.float64)
    dx = [((sv - (x[p] - mean) * inv) ** 2).t().contiguous() for p in range(n)]            # [F, m]
    db = [((sv - (background[b] - mean) * inv) ** 2).t().contiguous() for b in range(B)]
    v = torch.zeros(n, nS, dtype=torch.float64)
    for s0 in range(0, nS, chunk):
        S = torch.arange(s0, min(nS, s0 + chunk))
        mask = ((S[:, None] >> k[None, :]) & 1).bool()
        mf = mask.to(torch.float64)
        for p in range(n):
            for b in range(B):
                d2 = mf @ dx[p] + (1.0 - mf) @ db[b]
                dec = torch.exp(-pk.gamma * d2) @ coef + pk.svc_b
                v[p, S] += _stack_tail(torch.where(mask, x[p], background[b]), dec, pk)
    return v / B


def shapley_from_values(v: torch.Tensor, F: int) -> torch.Tensor:
    """``φ[p, k] = Σ_S c_k(S)·v[p, S]``, ``c_k(S) = w(|S|−1)`` if k ∈ S else ``−w(|S|)``."""
    w = shapley_weights(F)
    S = torch.arange(1 << F)
    inS = ((S[:, None] >> torch.arange(F)[None, :]) & 1).bool()         # [2^F, F]
    size = inS.sum(1)
    w_in = torch.where(size > 0, w[(size - 1).clamp(min=0)], torch.zeros((), dtype=torch.float64))
    w_out = torch.where(size < F, w[size.clamp(max=F - 1)], torch.zeros((), dtype=torch.float64))
    c = torch.where(inS, w_in[:, None], -w_out[:, None])                # [2^F, F]
    return v.to(torch.float64) @ c


def stack_shapley(x: torch.Tensor, background: torch.Tensor, pk, return_values: bool = False):
    """fp64 mirror of ``ops.stack_shapley``: exact interventional Shapley values of the fused
    stack's P(class 1) for each row of ``x`` against ``background``.  Returns ``phi [n, F]``,
    ``base`` (mean background risk, ``v(∅)``), ``pred [n]`` (``v(all)``) and optionally ``v``."""
    v = coalition_values(x, background, pk)
    phi = shapley_from_values(v, pk.F)
    out = (phi, v[0, 0].clone(), v[:, -1].clone())
    return out + (v,) if return_values else out


# ----------------------------------------------------------------------------- Shapley interactions
def shapley_interaction_weights(F: int) -> torch.Tensor:
    """``u(s) = s!(F−s−2)!/(2(F−1)!)`` for s = 0 … F−2 (f64; empty for F = 1): the weight of a
    coalition of size s that a pair joins, halved so that ``Φ[i][j]`` and ``Φ[j][i]`` each carry half of
    the pair's effect (the SHAP convention)."""
    return torch.tensor([math.factorial(s) * math.factorial(F - s - 2) / (2 * math.factorial(F - 1))
                         for s in range(F - 1)], dtype=torch.float64)


def _interaction_coefficients(F: int, s0: int, s1: int):
    """Coefficients of coalitions s0 ≤ T < s1 (f64).  ``c[T − s0, q]`` for the pairs i < j numbered row by
    row, q = 0 … F(F−1)/2 − 1: ``u(|T|−2)`` if i and j are both in T, ``−u(|T|−1)`` if exactly one is,
    ``u(|T|)`` if neither.  ``d[T − s0, i] = c_i(T) − Σ_{j≠i} c_ij(T)``, the diagonal's coefficient, with
    :func:`shapley_from_values`'s ``c_i`` and the sum in closed form (|T|−1 or |T| partners of i inside T)."""
    T = torch.arange(s0, s1)
    inT = ((T[:, None] >> torch.arange(F)[None, :]) & 1)                 # [C, F]
    size = inT.sum(1)
    ue = torch.zeros(F + 3, dtype=torch.float64)                         # ue[x] = u(x − 2)
    ue[2:F + 1] = shapley_interaction_weights(F)
    table = torch.stack([ue[size + 2], -ue[size + 1], ue[size]], 1)      # by the members of {i, j} in T
    i, j = torch.triu_indices(F, F, 1)
    c = table.gather(1, inT[:, i] + inT[:, j])                           # [C, pairs]
    w = torch.zeros(F + 1, dtype=torch.float64)
    w[:F] = shapley_weights(F)
    sz = size.to(torch.float64)[:, None]
    none, one, both = table[:, 0:1], table[:, 1:2], table[:, 2:3]
    d = torch.where(inT.bool(), w[(size - 1).clamp(min=0)][:, None] - ((sz - 1) * both + (F - sz) * one),
                    -w[size][:, None] - (sz * one + (F - 1 - sz) * none))
    return c, d


def _pairs_to_matrix(c: torch.Tensor, F: int) -> torch.Tensor:
    """``[n, pairs]`` → symmetric ``[n, F, F]`` with a zero diagonal."""
    i, j = torch.triu_indices(F, F, 1)
    m = torch.zeros(c.shape[0], F, F, dtype=c.dtype)
    m[:, i, j] = c
    m[:, j, i] = c
    return m


def shapley_interaction_abs_sums(F: int, v: torch.Tensor = None, chunk: int = 4096) -> torch.Tensor:
    """``Σ_T |c_ij(T)|·|v[p, T]|`` as ``[n, F, F]``, or ``Σ_T |c_ij(T)|`` as ``[F, F]`` without ``v``
    (2 off the diagonal) — what a rounding-error bound of Φ scales with."""
    nS = 1 << F
    a = torch.ones(1, nS, dtype=torch.float64) if v is None else v.to(torch.float64).abs()
    off = torch.zeros(a.shape[0], F * (F - 1) // 2, dtype=torch.float64)
    diag = torch.zeros(a.shape[0], F, dtype=torch.float64)
    for s0 in range(0, nS, chunk):
        s1 = min(nS, s0 + chunk)
        c, d = _interaction_coefficients(F, s0, s1)
        off += a[:, s0:s1] @ c.abs()
        diag += a[:, s0:s1] @ d.abs()
    out = _pairs_to_matrix(off, F) + torch.diag_embed(diag)
    return out[0] if v is None else out


def shapley_interactions_from_values(v: torch.Tensor, F: int, chunk: int = 4096):
    """f64 mirror of the ``shapley_interactions`` kernel on any game ``v [n, 2^F]``: off the diagonal
    ``Φ[p, i, j] = Φ[p, j, i] = Σ_T c_ij(T)·v[p, T]`` (coefficient form, ``chunk`` coalitions at a time),
    on it ``Φ[p, i, i] = φ[p, i] − Σ_{j≠i} Φ[p, i, j]`` with ``φ`` = :func:`shapley_from_values` and the
    sum over j ascending from 0.  Returns ``(Phi, phi)``."""
    v = v.to(torch.float64)
    n, nS = v.shape[0], 1 << F
    phi = shapley_from_values(v, F)
    acc = torch.zeros(n, F * (F - 1) // 2, dtype=torch.float64)
    for s0 in range(0, nS, chunk):
        s1 = min(nS, s0 + chunk)
        acc += v[:, s0:s1] @ _interaction_coefficients(F, s0, s1)[0]
    Phi = _pairs_to_matrix(acc, F)
    off = torch.zeros(n, F, dtype=torch.float64)
    for j in range(F):                                                   # j ascending; Φ[i][i] is 0 here
        off += Phi[:, :, j]
    return Phi + torch.diag_embed(phi - off), phi


def stack_shapley_interactions(x: torch.Tensor, background: torch.Tensor, pk, return_values: bool = False):
    """fp64 mirror of ``ops.stack_shapley_interactions``: ``Phi [n, F, F]`` and, exactly as
    :func:`stack_shapley` returns them, ``phi``, ``base``, ``pred`` and optionally ``v``."""
    v = coalition_values(x, background, pk)
    Phi, phi = shapley_interactions_from_values(v, pk.F)
    out = (Phi, phi, v[0, 0].clone(), v[:, -1].clone())
    return out + (v,) if return_values else out


def shapley_interaction_oracle(v, F: int):
    """Shapley interaction values straight from the subset-sum definition, numpy ``longdouble``
    with weights from exact ``Fraction``s; nothing shared with the coefficient form (F ≤ 10).

    ``Φ[i][j] = Σ_{S ⊆ N∖{i,j}} u(|S|)·(v(S∪{i,j}) − v(S∪{i}) − v(S∪{j}) + v(S))`` for i ≠ j,
    ``φ[i] = Σ_{S ⊆ N∖{i}} w(|S|)·(v(S∪{i}) − v(S))``, ``Φ[i][i] = φ[i] − Σ_{j≠i} Φ[i][j]``.
    ``v``: [n, 2^F].  Returns ``(Phi [n, F, F], phi [n, F])`` as longdouble arrays."""
    import numpy as np
    from fractions import Fraction
    if not 1 <= F <= 10:
        raise ValueError("shapley_interaction_oracle: 1 <= F <= 10")
    L = np.longdouble
    v = np.asarray(v, dtype=np.float64).astype(L)
    n = v.shape[0]
    if v.shape != (n, 1 << F):
        raise ValueError(f"shapley_interaction_oracle: v must be [n, {1 << F}]")
    fact = math.factorial

    def ld(fr: Fraction):
        return L(fr.numerator) / L(fr.denominator)

    w = [ld(Fraction(fact(s) * fact(F - s - 1), fact(F))) for s in range(F)]
    u = [ld(Fraction(fact(s) * fact(F - s - 2), 2 * fact(F - 1))) for s in range(F - 1)]
    subsets = np.arange(1 << F)
    sizes = np.array([bin(int(S)).count("1") for S in subsets])
    phi = np.zeros((n, F), dtype=L)
    Phi = np.zeros((n, F, F), dtype=L)
    for i in range(F):
        bi = 1 << i
        S = subsets[(subsets & bi) == 0]
        wt = np.array([w[s] for s in sizes[S]], dtype=L)
        phi[:, i] = ((v[:, S | bi] - v[:, S]) * wt).sum(1)
        for j in range(i + 1, F):
            bj = 1 << j
            S2 = S[(S & bj) == 0]
            ut = np.array([u[s] for s in sizes[S2]], dtype=L)
            d = v[:, S2 | bi | bj] - v[:, S2 | bi] - v[:, S2 | bj] + v[:, S2]
            Phi[:, i, j] = Phi[:, j, i] = (d * ut).sum(1)
    for i in range(F):
        Phi[:, i, i] = phi[:, i] - Phi[:, i, :].sum(1)        # Φ[i][i] is still 0 in the sum
    return Phi, phi


# ----------------------------------------------------------------------------- partial dependence
def stack_partial(x: torch.Tensor, pk, feat: torch.Tensor, value: torch.Tensor, return_ice: bool = False,
                  chunk: int = 16384):
    """fp64 mirror of ``ops.stack_partial``.  Cell c = ``(feat[c, 0], value[c, 0], feat[c, 1],
    value[c, 1])``; its hybrid row of cohort row r is ``x[r]`` with column ``feat[c, s]`` set to
    ``value[c, s]`` for each slot s whose index is not −1.  ``ice[r, c]`` = :func:`stack_infer` of that
    row, ``pd[c]`` = the mean of ``ice[:, c]`` summed in row order.  ``x`` and ``value`` are first
    rounded to f32, as the kernel sees them; the hybrid rows are materialised ``chunk`` at a time."""
    x = x.to(torch.float32).to(torch.float64)
    value = value.to(torch.float32).to(torch.float64)
    feat = feat.to(torch.int64)
    n, C = x.shape[0], feat.shape[0]
    ice = torch.empty(n, C, dtype=torch.float64)
    per = max(1, chunk // n)
    rows = torch.arange(per)
    for c0 in range(0, C, per):
        c1 = min(C, c0 + per)
        h = x[None, :, :].repeat(c1 - c0, 1, 1)                         # [cells, n, F]
        for s in range(2):
            k, v = feat[c0:c1, s], value[c0:c1, s]
            on = (k >= 0).nonzero().flatten()
            h[rows[:c1 - c0][on], :, k[on]] = v[on][:, None]
        ice[:, c0:c1] = stack_infer(h.reshape(-1, x.shape[1]), pk).reshape(c1 - c0, n).t()
    pd = torch.cumsum(ice, 0)[-1] / n                                   # Σ over r = 0, 1, …, n−1 in that order
    return (pd, ice) if return_ice else pd


# ----------------------------------------------------------------------------- KNN imputation
def knn_impute1(fit, X, undecided_rel: float = 2.0 ** -45):
    """Brute-force 1-NN imputation (sklearn ``KNNImputer(n_neighbors=1)`` semantics, numpy
    ``longdouble`` arithmetic; nothing shared with the kernels or ``KNNImputer._impute_host``).

    For a missing cell (r, c) of a column with any fit value the candidates are the fit rows that
    have c and share at least one present feature with r; the distance is
    ``F/|common| · Σ_common (x−y)²`` from direct differences; the donor is the lowest index among
    the exact minima; with no candidate the cell gets the column mean of the fit rows.  Columns
    with no fit value are dropped.

    Returns ``(out, mean_mask, n_ties, n_undecided)``: the imputed f64 matrix, the mask (shape of
    ``out``) of the column-mean cells, the number of cells with more than one exact minimum, and
    the number of cells where a candidate with a DIFFERENT value in column c lies strictly above
    the minimum by at most ``undecided_rel`` of it — no f64 evaluation can be asked to referee
    such a cell, so test inputs must have none."""
    import numpy as np
    L = np.longdouble
    fit = np.asarray(fit, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    nd, F = fit.shape
    mf, mx = np.isnan(fit), np.isnan(X)
    valid = ~mf.all(0)
    fitL = np.where(mf, 0.0, fit).astype(L)
    XL = np.where(mx, 0.0, X).astype(L)
    col_mean = (fitL.sum(0) / np.maximum((~mf).sum(0), 1).astype(L)).astype(np.float64)
    out = X.copy()
    mean_mask = np.zeros(X.shape, dtype=bool)
    n_ties = n_undecided = 0
    recv = np.nonzero((mx & valid[None, :]).any(1))[0]
    pf = (~mf).astype(L)
    step = max(1, (1 << 21) // max(1, nd * F))
    for s in range(0, recv.size, step):
        rr = recv[s:s + step]
        pr = (~mx[rr]).astype(L)
        both = pr[:, None, :] * pf[None, :, :]
        diff = XL[rr][:, None, :] - fitL[None, :, :]
        d2 = (both * diff * diff).sum(-1)
        common = both.sum(-1)
        dist = np.where(common > 0, L(F) * d2 / np.maximum(common, 1), L(np.inf))
        for c in np.nonzero(valid)[0]:
            j = np.nonzero(mx[rr, c])[0]
            if j.size == 0:
                continue
            donors = np.nonzero(~mf[:, c])[0]
            dd = dist[np.ix_(j, donors)]
            dmin = dd.min(1)
            first = donors[np.argmin(dd, axis=1)]          # first minimum = lowest index
            none = ~np.isfinite(dmin)
            vals = fit[first, c]
            out[rr[j], c] = np.where(none, col_mean[c], vals)
            mean_mask[rr[j], c] = none
            ok = ~none
            n_ties += int(((dd == dmin[:, None]).sum(1)[ok] > 1).sum())
            near = (dd > dmin[:, None]) & (dd <= dmin[:, None] * (L(1) + L(undecided_rel)))
            near &= fit[donors, c][None, :] != vals[:, None]
            n_undecided += int(near.any(1)[ok].sum())
    return out[:, valid], mean_mask[:, valid], n_ties, n_undecided


# ----------------------------------------------------------------------------- inference oracle
# numpy longdouble, written from the published rules (libsvm svm_predict_values / sigmoid_predict /
# multiclass_probability, sklearn's tree rule), on the UNPACKED model: nothing here imports torch
# or ops.packing, so a wrong rounding direction, stump merge, base, pad or ‖sv‖² in the packing is
# on one side of the comparison only.
_U = 2.0 ** -24                 # f32 unit roundoff
_TINY = 2.0 ** -125             # an f32 result flushed at the subnormal edge
# Hardware transcendentals (v_exp_f32 behind __builtin_amdgcn_exp2f, and __expf = exp2(x·log2 e)),
# measured once on an MI355X against long double on 2²² arguments (exp2: [−150, 1], a quarter of
# them in [−2, 0.01]; __expf: [−100, 100], a quarter in [−8, 8]):
#   exp2:   largest relative error of a normal result  EXP2_MEASURED · 2⁻²⁴; results below 2⁻¹²⁶
#           are flushed to 0 (largest absolute error there 1.175e-38 = 2⁻¹²⁶, the _TINY term)
#   __expf: largest relative error / (1 + |x|)          EXPF_MEASURED · 2⁻²⁴  (the f32 product
#           x·log2 e is rounded before the exp2, which costs |x|·2⁻²⁴ relative); the whole f32
#           sigmoid 1/(1 + __expf(−x)) was within 1.55 · 2⁻²⁴ absolute everywhere
# The budgets use twice the measured values.
EXP2_MEASURED = 1.40            # measured 1.3936
EXPF_MEASURED = 1.27            # measured 1.2677
EPS_EXP2 = 2 * EXP2_MEASURED * _U
EPS_EXPF = 2 * EXPF_MEASURED * _U


def _np():
    import numpy as np
    return np


def _f32(a):
    """The f32 rounding the kernels apply to rows and parameters, as longdouble."""
    np = _np()
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float32).astype(np.longdouble)


class StackSpec:
    """The unpacked HF stack, f64 numpy: ``mean, scale [F]``, ``sv [m, F]``, ``coef [m]``, ``gamma``,
    ``intercept``, ``A, B``, tree tables ``feature, threshold, left, right, value [T, K]`` (leaves
    have feature < 0), ``init, lr``, ``lr_w [F]``, ``lr_b``, ``meta_w (svc, gbc, lg)``, ``meta_b``."""

    def __init__(self, **kw):
        np = _np()
        for k in ("mean", "scale", "sv", "coef", "threshold", "value", "lr_w"):
            setattr(self, k, np.asarray(kw.pop(k), dtype=np.float64))
        for k in ("feature", "left", "right"):
            setattr(self, k, np.asarray(kw.pop(k), dtype=np.int64))
        for k in ("gamma", "intercept", "A", "B", "init", "lr", "lr_b", "meta_b"):
            setattr(self, k, float(kw.pop(k)))
        self.meta_w = tuple(float(w) for w in kw.pop("meta_w"))
        assert not kw, f"unknown fields {sorted(kw)}"
        self.F = int(self.mean.shape[0])


def _rbf_core(z, dz, sv32, c32, gamma, b, x3):
    """``dec = Σ c·exp(−γ·Σ(sv−z)²) + b`` by direct differences, and the forward bound of the
    kernels' f32 evaluation of it through ``‖sv‖² + ‖z‖² − 2 sv·z`` (see :func:`stack_oracle`).
    ``z``: exact longdouble rows, ``dz``: bound of the kernel's error on each ``z``."""
    np = _np()
    L = np.longdouble
    n, F = z.shape
    m = sv32.shape[0]
    g2 = L(gamma) * L(LOG2E)
    ln2 = np.log(L(2))
    sn = (sv32 * sv32).sum(1)
    asv, ac = np.abs(sv32), np.abs(c32)
    dec = np.zeros(n, dtype=L)
    bud = np.zeros(n, dtype=L)
    step = max(1, (1 << 20) // max(1, m * F))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s in range(0, n, step):
            zz, dzz = z[s:s + step], dz[s:s + step]
            diff = sv32[None, :, :] - zz[:, None, :]
            d2 = (diff * diff).sum(-1)
            cross = (asv[None, :, :] * np.abs(zz)[:, None, :]).sum(-1)
            mag = sn[None, :] + (zz * zz).sum(-1)[:, None] + 2 * cross
            dd2 = (F + 3) * _U * mag + 2 * (np.abs(diff) * dzz[:, None, :]).sum(-1)
            if x3:
                dd2 = dd2 + 2 * 3 * _U * cross
            k = np.exp(-L(gamma) * d2)
            # exponent (base 2) error: the distance error and the f32 roundings of −γ·log2 e
            de = g2 * dd2 + 2 * _U * g2 * d2
            dk = np.where(k > 0, k * (ln2 * de + EPS_EXP2), 0) + _TINY
            ck = ac[None, :] * k
            d = (c32[None, :] * k).sum(-1) + L(b)
            dec[s:s + step] = d
            bud[s:s + step] = (ac[None, :] * dk).sum(-1) + m * _U * ck.sum(-1) + 2 * _U * (np.abs(d) + abs(b))
    return dec, 2 * bud


def rbf_oracle(z, sv, coef, gamma, intercept):
    """``rbf_decision``'s oracle: rows, SVs and coefficients rounded to f32 here, the distance
    direct.  Returns ``(dec, Δdec)`` per row (longdouble)."""
    np = _np()
    z32 = _f32(z)
    return _rbf_core(z32, np.zeros_like(z32), _f32(sv), _f32(coef), gamma, float(np.float32(intercept)), False)


def couple_oracle(dec, A, B, clip=True):
    """libsvm ``sigmoid_predict`` + ``multiclass_probability`` (k = 2, eps = 0.005/k, at most 100
    iterations) step by step in longdouble.  Returns ``(p1, it)``: P(class 1) and the number of
    update sweeps done before the stopping test held."""
    np = _np()
    L = np.longdouble
    dec = np.asarray(dec, dtype=L)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        f = dec * L(A) + L(B)
        e = np.exp(-np.abs(f))
        r01 = np.where(f >= 0, e / (1 + e), 1 / (1 + e))
        if clip:
            lo = L(np.float64(1e-7))
            r01 = np.minimum(np.maximum(r01, lo), L(np.float64(1) - np.float64(1e-7)))
        r = [[None, r01], [1 - r01, None]]                 # r[i][j] = P(i | {i, j})
        Q = [[r[1][0] * r[1][0], -r[1][0] * r[0][1]], [-r[0][1] * r[1][0], r[0][1] * r[0][1]]]
        p = [np.full(dec.shape, L(0.5)), np.full(dec.shape, L(0.5))]
        it = np.zeros(dec.shape, dtype=np.int64)
        active = np.ones(dec.shape, dtype=bool)
        for _ in range(100):
            Qp = [Q[t][0] * p[0] + Q[t][1] * p[1] for t in range(2)]
            pQp = p[0] * Qp[0] + p[1] * Qp[1]
            err = np.maximum(np.abs(Qp[0] - pQp), np.abs(Qp[1] - pQp))
            active &= ~(err < L(0.005) / 2)
            if not active.any():
                break
            q = [x.copy() for x in p]
            for t in range(2):
                diff = (-Qp[t] + pQp) / Q[t][t]
                q[t] = q[t] + diff
                pQp = (pQp + diff * (diff * Q[t][t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
                for j in range(2):
                    Qp[j] = (Qp[j] + diff * Q[t][j]) / (1 + diff)
                    q[j] = q[j] / (1 + diff)
            p = [np.where(active, q[j], p[j]) for j in range(2)]
            it += active
    return p[1], it


def proba_oracle(dec, A, B, ddec=None):
    """P(class 1) of a decision value the kernel holds with error ≤ ``ddec``.  The coupling's
    stopping rule makes p a step function of the iteration count, so p(dec) jumps (by up to
    5·10⁻³) where the count changes: a row whose count differs over ``dec − δ, dec, dec + δ`` is
    ``undecided`` — no tolerance short of the jump can referee it; otherwise Δp is the largest of
    the three differences plus the f32 cast of the result.  δ is at least 2⁻⁴⁰·(1 + |dec|), the
    kernels' own f64 evaluation of A·dec + B and of the sigmoid.  Returns ``(p, it, Δp, undecided)``."""
    np = _np()
    L = np.longdouble
    dec = np.asarray(dec, dtype=L)
    d = np.maximum(np.zeros_like(dec) if ddec is None else np.asarray(ddec, dtype=L),
                   L(2.0 ** -40) * (1 + np.abs(dec)))
    p, it = couple_oracle(dec, A, B)
    pl, il = couple_oracle(dec - d, A, B)
    ph, ih = couple_oracle(dec + d, A, B)
    und = (il != it) | (ih != it)
    dp = np.maximum(np.abs(pl - p), np.abs(ph - p)) + 2 * _U * p
    return p, it, dp, und


def _leaf_sums(X, feature, threshold, left, right, value):
    """Per row: Σ_t value_t[leaf_t] (longdouble, unrounded values) under sklearn's rule
    ``float64(float32(x)) <= threshold64`` → left, and Σ_t max_k |value_t[k]|."""
    np = _np()
    L = np.longdouble
    with np.errstate(over="ignore"):
        x = np.asarray(X).astype(np.float32).astype(np.float64)
    n = x.shape[0]
    T = feature.shape[0]
    acc = np.zeros(n, dtype=L)
    rows = np.arange(n)
    for t in range(T):
        node = np.zeros(n, dtype=np.int64)
        for _ in range(feature.shape[1]):
            f = feature[t, node]
            leaf = f < 0
            if leaf.all():
                break
            go = x[rows, np.maximum(f, 0)] <= threshold[t, node]
            node = np.where(leaf, node, np.where(go, left[t, node], right[t, node]))
        acc += value[t, node].astype(L)
    vmax = np.abs(value).max(1).sum() if T else 0.0
    return acc, float(vmax)


def forest_oracle(X, feature, threshold, left, right, value, init, lr):
    """``init + lr·Σ_t value_t[leaf_t(x)]`` with the leaf chosen on the unrounded f64 thresholds,
    and its budget: the kernels hold f32 leaf values (or f32 stump deltas lr·(v_r − v_l) and an
    f32 base), add them one by one (T roundings on a partial sum ≤ S) and finish with
    init + lr·raw: 2·(T + 4)·2⁻²⁴·S with S = |init| + 2·lr·Σ_t max_k|value_t[k]|."""
    np = _np()
    acc, vmax = _leaf_sums(X, *(np.asarray(a) for a in (feature, threshold, left, right, value)))
    raw = np.longdouble(init) + np.longdouble(lr) * acc
    S = abs(init) + 2 * abs(lr) * vmax
    return raw, np.full(raw.shape, 2 * (feature.shape[0] + 4) * _U * S, dtype=np.longdouble)


def _sigmoid_budget(v, dv):
    """σ(v) and the bound of ``1/(1 + __expf(−v))`` evaluated in f32 at an argument off by ≤ dv:
    slope·(dv + (1 + |v|)·EPS_EXPF) + 2 roundings, the slope σ' taken at the point of [v−dv, v+dv]
    nearest 0."""
    np = _np()
    L = np.longdouble
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = 1 / (1 + np.exp(-v))
        a = np.maximum(np.abs(v) - dv, 0)
        sl = np.exp(-a) / (1 + np.exp(-a)) ** 2
        return s, 2 * (sl * (dv + (1 + np.abs(v)) * L(EPS_EXPF)) + 2 * _U * s) + _TINY


def stack_oracle(M, X, x3=True):
    """The fused stack on the unpacked model ``M`` (:class:`StackSpec`), per row of ``X``, in
    longdouble — with every stage's forward error budget for the f32 kernels.

    Semantics (defined here, not read off the kernels): rows, scaler mean, 1/scale, SVs, dual
    coefficients, LR weights and the scalar parameters are rounded to f32 (what the kernels hold);
    ``z = (x − mean)·(1/scale)`` exactly from those; the distance is the direct ``Σ(sv − z)²``; trees
    follow ``float64(float32(x)) <= threshold64`` on the unrounded thresholds (stumps too) with
    unrounded leaf values; sigmoid and coupling are libsvm's (:func:`couple_oracle`).

    Budgets, first order, u = 2⁻²⁴, every stage × 2 for the second-order terms:
      z        two roundings (subtract, scale): |δz_f| ≤ 2u|z_f|
      d²       2Σ|sv_f − z_f||δz_f| + (F + 3)u·(‖sv‖² + ‖z‖² + 2Σ|sv_f||z_f|) for the F-term fma/MFMA
               chains of ‖sv‖², ‖z‖², sv·z and the 3 operations joining them; the X3 path's dropped
               piece products add 3u·Σ|sv_f||z_f| to sv·z (twice that to d²)
      k        k·(ln 2·(γ log2 e·δd² + 2u·|exponent|) + EPS_EXP2) + 2⁻¹²⁵ (−γ·log2 e is held in f32)
      dec      Σ|c_j|δk_j + m·u·Σ|c_j|k_j (m accumulations of c·k) + 2u(|dec| + |b|)
      p_svc    :func:`proba_oracle` at dec ± δdec (``undecided`` where the iteration count changes)
      raw_gbc  :func:`forest_oracle`
      p_lg     F·u·(|b| + Σ|x_f w_f|) for the LR dot, then the sigmoid
      σ        :func:`_sigmoid_budget`
      P        Σ|w_i|Δp_i + 4u(|b_m| + Σ|w_i|p_i) through the meta sigmoid (slope ≤ ¼)
    ``x3=False`` leaves the dropped-product term out: the budget of the f32-MFMA path.

    Where the budgets do not apply (rows outside the domain; the kernels and the f64 host paths
    differ there and no tolerance referees it — known, kept, and documented here):
      * a row whose scaled feature ``(x − mean)·(1/scale)`` or LR product ``x_f·w_f`` overflows f32
        (|·| > 3.4e38): ``stack_infer`` holds z in f32, so z = ±inf, the expanded distance is inf − inf
        and the row's output is NaN, while ``reference.stack_infer`` (f64) stays finite, and so
        does this oracle (z in longdouble).  The ±3e38 threshold-edge inputs of the tests therefore
        scale by 2⁻⁷⁰ and carry zero LR weights: they are about the trees.  Such a row never disturbs another row
        (tests/test_infer_reference_gpu.py, row isolation).
      * a NaN feature: every comparison is false, so the stump table adds no delta (the row goes
        LEFT) while the tree walk of the same stumps fails ``x <= thr`` and goes RIGHT; P is NaN either
        way through z.  The predict paths impute before inference; rows must be finite.
    Returns a dict of longdouble arrays: dec, it, p_svc, raw_gbc, p_gbc, p_lg, P, their budgets
    d_dec, d_p_svc, d_raw_gbc, d_p_gbc, d_p_lg, d_P, and the boolean ``undecided``."""
    np = _np()
    L = np.longdouble
    x32 = _f32(X)
    F = M.F
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        z = (x32 - _f32(M.mean)) * _f32(1.0 / M.scale)
        dec, d_dec = _rbf_core(z, 2 * _U * np.abs(z), _f32(M.sv), _f32(M.coef), M.gamma,
                               float(np.float32(M.intercept)), x3)
        p_svc, it, d_p_svc, und = proba_oracle(dec, M.A, M.B, d_dec)
        raw, d_raw = forest_oracle(X, M.feature, M.threshold, M.left, M.right, M.value, M.init, M.lr)
        p_gbc, d_p_gbc = _sigmoid_budget(raw, d_raw)
        w32 = _f32(M.lr_w)
        b_lr = L(np.float32(M.lr_b))
        lin = (x32 * w32[None, :]).sum(1) + b_lr
        d_lin = 2 * F * _U * (abs(b_lr) + (np.abs(x32) * np.abs(w32)[None, :]).sum(1))
        p_lg, d_p_lg = _sigmoid_budget(lin, d_lin)
        w = [L(np.float32(v)) for v in M.meta_w]
        mb = L(np.float32(M.meta_b))
        mm = mb + w[0] * p_svc + w[1] * p_gbc + w[2] * p_lg
        d_mm = abs(w[0]) * d_p_svc + abs(w[1]) * d_p_gbc + abs(w[2]) * d_p_lg + \
            2 * 4 * _U * (abs(mb) + abs(w[0]) * p_svc + abs(w[1]) * p_gbc + abs(w[2]) * p_lg)
        P = 1 / (1 + np.exp(-mm))
        d_P = 0.25 * (d_mm + 2 * (1 + np.abs(mm)) * L(EPS_EXPF)) + 4 * _U * P
    return dict(dec=dec, it=it, p_svc=p_svc, raw_gbc=raw, p_gbc=p_gbc, p_lg=p_lg, P=P, d_dec=d_dec,
                d_p_svc=d_p_svc, d_raw_gbc=d_raw, d_p_gbc=d_p_gbc, d_p_lg=d_p_lg, d_P=d_P, undecided=und)


# ---- bootstrap of the held-out metrics ------------------------------------------------------------
# Resampling law (shared by the three mirrors through _resample_counts, the kernels through
# csrc/resample.h and the oracles through bootstrap_resample):
# draw j of replicate b over a stratum of m rows is row r of it,
#     u = splitmix64(seed ^ splitmix64((b << 40) ^ j)),   r = ((u >> 32)·m) >> 32   ∈ [0, m)
# (bias ≤ m/2^32).  Plain: j ∈ [0, n), m = n.  Stratified: j < P draws the r-th positive (m = P),
# j ≥ P the r-th negative (m = N), both numbered in original row order.

COMPARE_THREADS = 1024   # kBootThreads and kWave of csrc/resample.h: the f64 folds of the mirrors follow them
COMPARE_WAVE = 64

def _splitmix64_t(x: torch.Tensor) -> torch.Tensor:
    """splitmix64 on int64 tensors (two's-complement wraparound = mod 2^64)."""
    def srl(v, k):
        return (v >> k) & ((1 << (64 - k)) - 1)

    def c(v):
        return torch.tensor(v - (1 << 64), dtype=torch.int64, device=x.device)
    x = x + c(0x9E3779B97F4A7C15)
    x = (x ^ srl(x, 30)) * c(0xBF58476D1CE4E5B9)
    x = (x ^ srl(x, 27)) * c(0x94D049BB133111EB)
    return x ^ srl(x, 31)


def _seed_i64(seed: int) -> int:
    s = int(seed) & ((1 << 64) - 1)
    return s - (1 << 64) if s >= (1 << 63) else s


class _NamedOutputs(tuple):
    """The outputs of an op in order (``_fields``), also by name."""
    _fields = ()

    def __new__(cls, *vals):
        assert len(vals) == len(cls._fields)
        return super().__new__(cls, vals)

    def __getattr__(self, name):
        try:
            return self[self._fields.index(name)]
        except ValueError:
            raise AttributeError(name) from None


def _tie_groups(ss: torch.Tensor):
    """For the sorted values ``ss [n]``: every position's first and last position of its run of equal
    values (int64 ``[n]`` each)."""
    n, dev = ss.numel(), ss.device
    start = torch.ones(n, dtype=torch.bool, device=dev)
    start[1:] = ss[1:] != ss[:-1]
    firsts = torch.nonzero(start).squeeze(1)
    gid = torch.cumsum(start.to(torch.int64), 0) - 1
    lasts = torch.cat([firsts[1:] - 1, torch.tensor([n - 1], device=dev)])
    return firsts[gid], lasts[gid]


def _resample_counts(rowmap, p0: int, n: int, seed: int, b0: int, b1: int, per: int, dev):
    """The law above, ``per`` replicates at a time: yields ``(bs, cnt)`` with ``bs`` the replicate numbers
    (int64 ``[Bc]``) and ``cnt [Bc, n]`` (int64) how often each was drawn of the indices ``rowmap[p0·[j ≥ p0]
    + r]`` (int64 ``[n]``; None: the drawn row itself).  Draws j < p0 take the stratum [0, p0)."""
    i64 = torch.int64
    j = torch.arange(n, dtype=i64, device=dev)
    head = j < p0
    m = torch.where(head, p0, n - p0)
    off = torch.where(head, 0, p0)
    sd = torch.tensor(_seed_i64(seed), dtype=i64, device=dev)
    for c0 in range(b0, b1, per):
        bs = torch.arange(c0, min(b1, c0 + per), dtype=i64, device=dev)
        Bc = bs.numel()
        u = _splitmix64_t(sd ^ _splitmix64_t((bs[:, None] << 40) ^ j[None, :]))
        r = (((u >> 32) & 0xFFFFFFFF) * m[None, :]) >> 32
        at = off[None, :] + r
        if rowmap is not None:
            at = rowmap[at]
        at = at + torch.arange(Bc, device=dev)[:, None] * n
        yield bs, torch.bincount(at.reshape(-1), minlength=Bc * n).reshape(Bc, n)


def _group_ends(gfirst: torch.Tensor, glast: torch.Tensor):
    """The last position of every tie group ``[E]`` and the group's first position (int64)."""
    ends = torch.nonzero(glast == torch.arange(glast.numel(), device=glast.device)).squeeze(1)
    return ends, gfirst[ends]


def _rank_stats(cm: torch.Tensor, ys: torch.Tensor, ends: torch.Tensor, f: torch.Tensor, k0: int):
    """The kernels' rank statistics of the count matrix ``cm [Bc, n]`` in a descending score order with
    labels ``ys`` and tie groups ``ends``, ``f`` = :func:`_group_ends` (all int64): returns ``Pb``, ``Nb``,
    ``deg`` (a class missing), the cumulative counts ``TP``, ``FP`` at the group ends ``[Bc, E]``, ``a2``,
    ``auroc`` and ``ap`` (NaN where ``deg``) and ``conf [Bc, 4]`` = TP FP FN TN of the first ``k0`` rows."""
    f64 = torch.float64
    prev = (f - 1).clamp(min=0)
    cp = torch.cumsum(cm * ys, 1)
    cn = torch.cumsum(cm * (1 - ys), 1)
    Pb, Nb = cp[:, -1], cn[:, -1]
    deg = (Pb == 0) | (Nb == 0)
    TP, FP = cp[:, ends], cn[:, ends]
    TP0 = torch.where(f > 0, cp[:, prev], 0)
    FP0 = torch.where(f > 0, cn[:, prev], 0)
    a2 = ((FP - FP0) * (TP + TP0)).sum(1)
    auroc = a2.to(f64) / (2 * Pb * Nb).to(f64)
    tot = TP + FP
    term = torch.where(tot > 0, ((TP - TP0) * TP).to(f64) / tot.clamp(min=1).to(f64), 0.0)
    ap = term.sum(1) / Pb.to(f64)
    if k0 > 0:
        tpc, fpc = cp[:, k0 - 1], cn[:, k0 - 1]
    else:
        tpc, fpc = torch.zeros_like(Pb), torch.zeros_like(Pb)
    conf = torch.stack([tpc, fpc, Pb - tpc, Nb - fpc], 1)
    nan = float("nan")
    return Pb, Nb, deg, TP, FP, a2, torch.where(deg, nan, auroc), torch.where(deg, nan, ap), conf


class BootstrapPlan:
    """What is prepared once per call: the descending stable score order and, in it, the labels
    ``y`` (uint8), every row's tie-group ``gfirst``/``glast`` (int32), ``map`` (int32: drawn row →
    position in the order; stratified: the positives' positions, then the negatives'), ``p0``
    (draws j < p0 take the first stratum; plain: n) and ``k0`` = number of rows scoring > threshold."""

    def __init__(self, y: torch.Tensor, score: torch.Tensor, stratified: bool, threshold: float):
        dev = score.device
        n = score.numel()
        s = score.to(torch.float64)
        order = torch.argsort(s, descending=True, stable=True)
        pos = y.to(dev) > 0
        gfirst, glast = _tie_groups(s[order])
        rank = torch.empty(n, dtype=torch.int64, device=dev)
        rank[order] = torch.arange(n, device=dev)
        self.n = n
        self.y = pos[order].to(torch.uint8).contiguous()
        self.gfirst = gfirst.to(torch.int32).contiguous()
        self.glast = glast.to(torch.int32).contiguous()
        self.P = int(pos.sum())
        if stratified:
            self.map = torch.cat([rank[pos], rank[~pos]]).to(torch.int32).contiguous()
            self.p0 = self.P
        else:
            self.map = rank.to(torch.int32).contiguous()
            self.p0 = n
        self.k0 = int((s > threshold).sum())


def bootstrap_metrics(y: torch.Tensor, score: torch.Tensor, n_boot: int, *, seed: int = 0,
                      stratified: bool = False, threshold: float = 0.5, grid_points: int = 101,
                      b0: int = 0, b1=None, chunk_elems: int = 1 << 22):
    """Vectorised torch mirror of the bootstrap kernel (and the host path of
    ``ops.bootstrap_metrics``, which validates): counts by ``bincount`` over the draws of the law
    above, then the kernel's formulas in int64 and f64.  Returns ``auroc [B]``, ``ap [B]`` (f64),
    ``a2 [B]``, ``pn [B, 2]``, ``conf [B, 4]`` (int64; TP FP FN TN) and ``tpr [B, G]`` (f64) for
    replicates ``b0:b1``.  A replicate with ``P_b = 0`` or ``N_b = 0`` has NaN ``auroc``, ``ap``
    and ``tpr``.  Replicates are processed ``chunk_elems // n`` at a time."""
    pl = BootstrapPlan(y, score, stratified, threshold)
    dev = score.device
    n, G = pl.n, int(grid_points)
    b1 = n_boot if b1 is None else b1
    i64, f64 = torch.int64, torch.float64
    ys = pl.y.to(i64)
    ends, f = _group_ends(pl.gfirst.to(i64), pl.glast.to(i64))
    g = torch.arange(G, dtype=i64, device=dev)
    G1 = G - 1
    nan = float("nan")
    outs = [[] for _ in range(6)]
    for bs, cnt in _resample_counts(pl.map.to(i64), pl.p0, n, seed, b0, b1, max(1, chunk_elems // n), dev):
        Pb, Nb, deg, TP, FP, a2, auroc, ap, conf = _rank_stats(cnt, ys, ends, f, pl.k0)
        # ROC vertices: (0, 0), then the tie-group ends
        E = TP.shape[1]
        z = torch.zeros(bs.numel(), 1, dtype=i64, device=dev)
        V, T = torch.cat([z, FP], 1), torch.cat([z, TP], 1)
        bound = g[None, :] * Nb[:, None]
        ks = torch.searchsorted((V * G1).contiguous(), bound.contiguous(), right=True) - 1
        nx = (ks + 1).clamp(max=E)
        vk, tk = torch.gather(V, 1, ks), torch.gather(T, 1, ks)
        v1, t1 = torch.gather(V, 1, nx), torch.gather(T, 1, nx)
        exact = (vk * G1 == bound) | (ks == E)
        num = bound - vk * G1
        den = torch.where(exact, 1, G1 * (v1 - vk))
        frac = num.to(f64) / den.to(f64)
        pbf = Pb.to(f64)[:, None]
        tpr = torch.where(exact, tk.to(f64) / pbf, (tk.to(f64) + (t1 - tk).to(f64) * frac) / pbf)
        tpr = torch.where(deg[:, None], nan, tpr)
        for o, v in zip(outs, (auroc, ap, a2, torch.stack([Pb, Nb], 1), conf, tpr)):
            o.append(v)
    if not outs[0]:
        e = torch.empty
        return (e(0, dtype=f64, device=dev), e(0, dtype=f64, device=dev), e(0, dtype=i64, device=dev),
                e(0, 2, dtype=i64, device=dev), e(0, 4, dtype=i64, device=dev), e(0, G, dtype=f64, device=dev))
    return tuple(torch.cat(o) for o in outs)


def _splitmix64_py(x: int) -> int:
    M = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def bootstrap_resample(y, b: int, seed: int = 0, stratified: bool = False):
    """The original row indices replicate ``b`` draws, in draw order, by Python integers."""
    y = [int(v) for v in y]
    n = len(y)
    sd = int(seed) & ((1 << 64) - 1)

    def draw(j, m):
        u = _splitmix64_py(sd ^ _splitmix64_py(((b << 40) & ((1 << 64) - 1)) ^ j))
        return ((u >> 32) * m) >> 32
    if not stratified:
        return [draw(j, n) for j in range(n)]
    pos = [i for i in range(n) if y[i] == 1]
    neg = [i for i in range(n) if y[i] != 1]
    return [pos[draw(j, len(pos))] for j in range(len(pos))] + [neg[draw(j, len(neg))] for j in range(len(pos), n)]


def bootstrap_oracle(y, score, n_boot: int, *, seed: int = 0, stratified: bool = False,
                     threshold: float = 0.5, grid_points: int = 101, b0: int = 0, b1=None):
    """Independent oracle for the tests, O(n²) per replicate: the resampled rows are materialised
    from a Python-integer splitmix64; AUROC counts (positive, negative) pairs, 2 for a win and 1
    for a tie, and divides the exact integers as ``numpy.longdouble``; AP and the grid TPR follow
    the textbook definitions on the materialised sample (AP = Σ ΔR·precision over the distinct
    scores; TPR = the ROC polyline with a (0, 0) vertex, read at FPR = g/(G−1), the upper point of a
    vertical run), in longdouble with the vertex comparisons in exact integers; the confusion
    counts are counted.  Returns numpy arrays named as the op's outputs (``auroc``, ``ap``, ``tpr``
    longdouble, the rest int64) in a dict, plus ``n_degenerate``."""
    np = _np()
    ld = np.longdouble
    y = [int(v) for v in np.asarray(y).reshape(-1)]
    s = [float(v) for v in np.asarray(score, dtype=np.float64).reshape(-1)]
    G = int(grid_points)
    b1 = n_boot if b1 is None else b1
    out = {k: [] for k in ("auroc", "ap", "a2", "pn", "conf", "tpr")}
    for b in range(b0, b1):
        idx = bootstrap_resample(y, b, seed, stratified)
        yy = [y[i] for i in idx]
        sc = [s[i] for i in idx]
        ps = [v for v, l in zip(sc, yy) if l == 1]
        ns = [v for v, l in zip(sc, yy) if l != 1]
        P, N = len(ps), len(ns)
        a2 = sum(2 if p > q else (1 if p == q else 0) for p in ps for q in ns)
        tp = sum(1 for v, l in zip(sc, yy) if v > threshold and l == 1)
        fp = sum(1 for v, l in zip(sc, yy) if v > threshold and l != 1)
        out["a2"].append(a2)
        out["pn"].append([P, N])
        out["conf"].append([tp, fp, P - tp, N - fp])
        if P == 0 or N == 0:
            out["auroc"].append(ld("nan"))
            out["ap"].append(ld("nan"))
            out["tpr"].append([ld("nan")] * G)
            continue
        out["auroc"].append(ld(a2) / ld(2 * P * N))
        verts = [(0, 0)]                       # (FP, TP) at every distinct score, descending
        ap = ld(0)
        for v in sorted(set(sc), reverse=True):
            t = sum(1 for q in ps if q >= v)
            f_ = sum(1 for q in ns if q >= v)
            ap += (ld(t) / ld(P) - ld(verts[-1][1]) / ld(P)) * (ld(t) / ld(t + f_))
            verts.append((f_, t))
        out["ap"].append(ap)
        row = []
        for gi in range(G):
            k = max(i for i, (f_, _) in enumerate(verts) if f_ * (G - 1) <= gi * N)
            fk, tk = verts[k]
            if k == len(verts) - 1 or fk * (G - 1) == gi * N:
                row.append(ld(tk) / ld(P))
                continue
            f1, t1 = verts[k + 1]
            q = ld(gi) / ld(G - 1)
            x0, x1 = ld(fk) / ld(N), ld(f1) / ld(N)
            y0, y1 = ld(tk) / ld(P), ld(t1) / ld(P)
            row.append(y0 + (y1 - y0) * (q - x0) / (x1 - x0))
        out["tpr"].append(row)
    res = {"auroc": np.array(out["auroc"], dtype=ld), "ap": np.array(out["ap"], dtype=ld),
           "a2": np.array(out["a2"], dtype=np.int64), "pn": np.array(out["pn"], dtype=np.int64).reshape(-1, 2),
           "conf": np.array(out["conf"], dtype=np.int64).reshape(-1, 4),
           "tpr": np.array(out["tpr"], dtype=ld).reshape(-1, G)}
    res["n_degenerate"] = int(np.isnan(res["auroc"]).sum())
    return res


# ---- bootstrap of the calibration and decision-curve statistics --------------------------------------
# Same resampling law as above (_resample_counts here, csrc/resample.h in the kernels).  Definitions
# shared by the kernel, this mirror and the oracle:
#   bin of p     = #{k ∈ 1..K−1 : p ≥ k/K}, k/K the f64 quotient, compared in f64 (0.3 is in [0.3, 0.4));
#   treated at t = p ≥ t, thresholds t_g = g/(T+1), g = 1..T, the f64 quotient;
#   logit        l = log(p̃) − log1p(−p̃), p̃ = min(max(p, 1e-12), 1 − 1e-12);
#   status       1 degenerate (P_b = 0 or N_b = 0), 2 no MLE (the drawn classes do not overlap in l:
#                not both min_pos < max_neg and min_neg < max_pos), 3 iteration cap, else 0;
#   the fit      Newton on the weighted log-likelihood of logit P(y=1) = a + b·l from a = log(P_b/N_b),
#                b = 0; it stops, applying the full step, when the undamped step has |δa|, |δb| ≤ 1e-10;
#                otherwise the step is halved while the deviance rises by more than 1e-12·|deviance|
#                (at most 40 times); at most 50 steps.  Deviance term: log1p(exp(−|e|)) + max(e, 0) − y·e.

CAL_CLAMP = 1e-12
CAL_STEP_TOL = 1e-10
CAL_RISE = 1e-12
CAL_MAX_ITER = 50
CAL_MAX_HALVE = 40


class CalibrationBootstrap(_NamedOutputs):
    """The outputs of ``bootstrap_calibration`` in order, also by name."""
    _fields = ("pn", "brier", "sum_p", "bin_n", "bin_pos", "bin_sum_p", "dc", "status", "coef", "iters")


class CalibrationPlan(BootstrapPlan):
    """``BootstrapPlan`` plus, in the same descending stable order: the scores ``p`` and their
    clamped logits ``l`` (f64), ``bin_end`` (int32 [K]: rows scoring ≥ k/K, ``bin_end[0] = n``, so bin
    k is rows ``bin_end[k+1]:bin_end[k]``) and ``thr_prefix`` (int32 [T]: rows scoring ≥ g/(T+1))."""

    def __init__(self, y: torch.Tensor, score: torch.Tensor, stratified: bool, bins: int, thresholds: int):
        super().__init__(y, score, stratified, 0.5)
        dev = score.device
        f64 = torch.float64
        n, K, T = self.n, int(bins), int(thresholds)
        asc = torch.sort(score.to(f64)).values
        self.p = asc.flip(0).contiguous()
        pt = self.p.clamp(CAL_CLAMP, 1.0 - CAL_CLAMP)
        self.l = (torch.log(pt) - torch.log1p(-pt)).contiguous()
        self.K, self.T = K, T
        # the quotients are formed on the host: a device may divide by multiplying with a reciprocal
        edges = torch.tensor([k / K for k in range(K)], dtype=f64).to(dev)
        self.thresholds = torch.tensor([g / (T + 1) for g in range(1, T + 1)], dtype=f64).to(dev)
        # rows ≥ t = n − #{rows < t}
        self.bin_end = (n - torch.searchsorted(asc, edges, right=False)).to(torch.int32).contiguous()
        self.bin_end[0] = n
        self.thr_prefix = (n - torch.searchsorted(asc, self.thresholds, right=False)).to(torch.int32).contiguous()


def _cal_eval(C, yf, l, a, b):
    """Deviance, gradient and Hessian sums of the count-weighted log-likelihood at ``(a, b)`` [m]."""
    e = a[:, None] + b[:, None] * l[None, :]
    z = torch.exp(-e.abs())
    q = 1.0 / (1.0 + z)
    zq = z * q
    dev = (C * (torch.log1p(z) + e.clamp(min=0) - yf[None, :] * e)).sum(1)
    wr = C * (yf[None, :] - torch.where(e >= 0, q, zq))
    wv = C * (zq * q)
    return torch.stack([dev, wr.sum(1), wr @ l, wv.sum(1), wv @ l, wv @ (l * l)])


def _cal_newton(C, yf, l, Pb, Nb):
    """The fit of the header on every row of the count matrix ``C [m, n]`` (f64) at once.  Returns
    ``coef [m, 2]`` (NaN where the cap was hit), ``iters [m]`` and ``capped [m]`` (bool)."""
    m = C.shape[0]
    dev = C.device
    a = torch.log(Pb / Nb)
    b = torch.zeros_like(a)
    iters = torch.zeros(m, dtype=torch.int64, device=dev)
    done = torch.zeros(m, dtype=torch.bool, device=dev)
    S = _cal_eval(C, yf, l, a, b) if m else torch.zeros(6, 0, dtype=torch.float64, device=dev)
    act = torch.arange(m, device=dev)
    for it in range(1, CAL_MAX_ITER + 1):
        if act.numel() == 0:
            break
        d0, g0, g1, h00, h01, h11 = S[:, act]
        det = h00 * h11 - h01 * h01
        da = (h11 * g0 - h01 * g1) / det
        db = (h00 * g1 - h01 * g0) / det
        iters[act] = it
        conv = (da.abs() <= CAL_STEP_TOL) & (db.abs() <= CAL_STEP_TOL)
        ca = act[conv]
        a[ca] = a[ca] + da[conv]
        b[ca] = b[ca] + db[conv]
        done[ca] = True
        act, da, db, d0 = act[~conv], da[~conv], db[~conv], d0[~conv]
        if act.numel() == 0:
            break
        t = torch.ones_like(da)
        a1, b1 = a[act].clone(), b[act].clone()
        Sn = torch.empty(6, act.numel(), dtype=torch.float64, device=dev)
        pend = torch.arange(act.numel(), device=dev)
        Ca = C[act] if act.numel() < m else C
        for h in range(CAL_MAX_HALVE + 1):
            a1[pend] = a[act[pend]] + t[pend] * da[pend]
            b1[pend] = b[act[pend]] + t[pend] * db[pend]
            Sn[:, pend] = _cal_eval(Ca[pend] if pend.numel() < Ca.shape[0] else Ca, yf, l, a1[pend], b1[pend])
            if h == CAL_MAX_HALVE:
                break
            rise = Sn[0, pend] - d0[pend] > CAL_RISE * d0[pend].abs()
            pend = pend[rise]
            if pend.numel() == 0:
                break
            t[pend] = t[pend] * 0.5
        a[act], b[act] = a1, b1
        S[:, act] = Sn
    coef = torch.stack([a, b], 1)
    coef[~done] = float("nan")
    return coef, iters, ~done


def _cal_stats(pl: CalibrationPlan, cnt: torch.Tensor):
    """The ten outputs for the rows of the count matrix ``cnt [m, n]`` (int64) over the plan's order."""
    i64, f64 = torch.int64, torch.float64
    dev = cnt.device
    m, n, K = cnt.shape[0], pl.n, pl.K
    ys = pl.y.to(i64)
    yf = ys.to(f64)
    cp = torch.cumsum(cnt * ys, 1)
    cn = torch.cumsum(cnt * (1 - ys), 1)
    Pb, Nb = cp[:, -1], cn[:, -1]
    C = cnt.to(f64)
    brier = (C * ((pl.p - yf) ** 2)[None, :]).sum(1) / n
    sum_p = (C * pl.p[None, :]).sum(1)
    z = torch.zeros(m, 1, dtype=i64, device=dev)
    cpz, cnz = torch.cat([z, cp], 1), torch.cat([z, cn], 1)
    be = pl.bin_end.to(i64)
    bs = torch.cat([be[1:], torch.zeros(1, dtype=i64, device=dev)])
    bin_pos = cpz[:, be] - cpz[:, bs]
    bin_n = bin_pos + cnz[:, be] - cnz[:, bs]
    bin_sum_p = torch.stack([(C[:, s:e] * pl.p[None, s:e]).sum(1) for s, e in zip(bs.tolist(), be.tolist())], 1)
    th = pl.thr_prefix.to(i64)
    dc = torch.stack([cpz[:, th], cnz[:, th]], 2)
    # a class's largest l sits at its first drawn row of the descending order, its smallest at the last
    rows = torch.arange(n, device=dev)
    dpos, dneg = (cnt > 0) & (ys > 0)[None, :], (cnt > 0) & (ys == 0)[None, :]
    fpos = torch.where(dpos, rows, n).min(1).values.clamp(max=n - 1)
    lpos = torch.where(dpos, rows, -1).max(1).values.clamp(min=0)
    fneg = torch.where(dneg, rows, n).min(1).values.clamp(max=n - 1)
    lneg = torch.where(dneg, rows, -1).max(1).values.clamp(min=0)
    deg = (Pb == 0) | (Nb == 0)
    exists = (pl.l[lpos] < pl.l[fneg]) & (pl.l[lneg] < pl.l[fpos])
    status = torch.where(deg, 1, torch.where(exists, 0, 2))
    coef = torch.full((m, 2), float("nan"), dtype=f64, device=dev)
    iters = torch.zeros(m, dtype=i64, device=dev)
    fit = torch.nonzero(status == 0).squeeze(1)
    if fit.numel():
        c, it, capped = _cal_newton(C[fit] if fit.numel() < m else C, yf, pl.l, Pb[fit].to(f64), Nb[fit].to(f64))
        coef[fit], iters[fit] = c, it
        status[fit[capped]] = 3
    return (torch.stack([Pb, Nb], 1), brier, sum_p, bin_n, bin_pos, bin_sum_p, dc, status, coef, iters)


def bootstrap_calibration(y: torch.Tensor, score: torch.Tensor, n_boot: int, *, seed: int = 0,
                          stratified: bool = False, bins: int = 10, thresholds: int = 99, b0: int = 0, b1=None,
                          chunk_elems: int = 1 << 20):
    """Vectorised torch mirror of the calibration kernel (and the host path of
    ``ops.bootstrap_calibration``, which validates): the counts of ``bootstrap_metrics`` above, then
    the kernel's formulas in int64 and f64 and its Newton rules on ``chunk_elems // n`` replicates at
    a time.  Returns a :class:`CalibrationBootstrap` for replicates ``b0:b1``: ``pn [B, 2]``,
    ``brier [B]``, ``sum_p [B]``, ``bin_n``/``bin_pos``/``bin_sum_p [B, K]``, ``dc [B, T, 2]`` (TP, FP),
    ``status [B]``, ``coef [B, 2]`` (intercept, slope; NaN unless status 0) and ``iters [B]``."""
    pl = CalibrationPlan(y, score, stratified, bins, thresholds)
    dev = score.device
    n, K, T = pl.n, pl.K, pl.T
    b1 = n_boot if b1 is None else b1
    i64, f64 = torch.int64, torch.float64
    outs = [[] for _ in range(10)]
    for _, cnt in _resample_counts(pl.map.to(i64), pl.p0, n, seed, b0, b1, max(1, chunk_elems // n), dev):
        for o, v in zip(outs, _cal_stats(pl, cnt)):
            o.append(v)
    if not outs[0]:
        def e(*shape, dtype):
            return torch.empty(*shape, dtype=dtype, device=dev)
        return CalibrationBootstrap(e(0, 2, dtype=i64), e(0, dtype=f64), e(0, dtype=f64), e(0, K, dtype=i64),
                                    e(0, K, dtype=i64), e(0, K, dtype=f64), e(0, T, 2, dtype=i64), e(0, dtype=i64),
                                    e(0, 2, dtype=f64), e(0, dtype=i64))
    return CalibrationBootstrap(*(torch.cat(o) for o in outs))


def calibration_point(y, p, bins: int = 10, thresholds: int = 99):
    """The statistics of ``bootstrap_calibration`` on the original sample (every count 1), on the host:
    a dict of Python numbers and lists named as the op's outputs, plus ``thresholds`` (the t_g)."""
    y = torch.as_tensor(_np().asarray(y) if not isinstance(y, torch.Tensor) else y).reshape(-1).cpu()
    p = torch.as_tensor(_np().asarray(p) if not isinstance(p, torch.Tensor) else p).reshape(-1).cpu().to(torch.float64)
    pl = CalibrationPlan(y, p, False, bins, thresholds)
    vals = _cal_stats(pl, torch.ones(1, pl.n, dtype=torch.int64))
    out = {k: v[0].tolist() for k, v in zip(CalibrationBootstrap._fields, vals)}
    out["thresholds"] = pl.thresholds.tolist()
    return out


def calibration_oracle(y, score, n_boot: int, *, seed: int = 0, stratified: bool = False, bins: int = 10,
                       thresholds: int = 99, b0: int = 0, b1=None):
    """Independent oracle for the tests, one replicate at a time on the rows materialised by
    ``bootstrap_resample``: bins and treated rows are counted by comparing every drawn score with
    k/K and g/(T+1); Brier and the sums are ``numpy.longdouble``; separability is decided on the
    drawn (clamped) scores themselves; the fit is a longdouble Newton on the materialised rows, run
    until the undamped step is below 1e-16·max(1, |a|, |b|).  Returns numpy arrays named as the
    op's outputs (``brier``, ``sum_p``, ``bin_sum_p``, ``coef`` longdouble, the rest int64) in a dict."""
    np = _np()
    ld = np.longdouble
    y = [int(v) for v in np.asarray(y).reshape(-1)]
    s = [float(v) for v in np.asarray(score, dtype=np.float64).reshape(-1)]
    n, K, T = len(y), int(bins), int(thresholds)
    b1 = n_boot if b1 is None else b1
    out = {k: [] for k in CalibrationBootstrap._fields}
    for b in range(b0, b1):
        idx = bootstrap_resample(y, b, seed, stratified)
        yy = [y[i] for i in idx]
        pp = [s[i] for i in idx]
        P = sum(yy)
        N = n - P
        out["pn"].append([P, N])
        out["brier"].append(sum(((ld(p) - ld(l)) ** 2 for p, l in zip(pp, yy)), ld(0)) / ld(n))
        out["sum_p"].append(sum((ld(p) for p in pp), ld(0)))
        bn, bp, bsum = [0] * K, [0] * K, [ld(0)] * K
        for p, l in zip(pp, yy):
            k = sum(1 for e in range(1, K) if p >= e / K)
            bn[k] += 1
            bp[k] += l
            bsum[k] += ld(p)
        out["bin_n"].append(bn)
        out["bin_pos"].append(bp)
        out["bin_sum_p"].append(bsum)
        out["dc"].append([[sum(1 for p, l in zip(pp, yy) if p >= g / (T + 1) and l == 1),
                           sum(1 for p, l in zip(pp, yy) if p >= g / (T + 1) and l != 1)] for g in range(1, T + 1)])
        pc = [min(max(p, CAL_CLAMP), 1.0 - CAL_CLAMP) for p in pp]
        ps = [v for v, l in zip(pc, yy) if l == 1]
        ns = [v for v, l in zip(pc, yy) if l != 1]
        nan2 = [ld("nan"), ld("nan")]
        if P == 0 or N == 0:
            st, cf, it = 1, nan2, 0
        elif not (min(ps) < max(ns) and min(ns) < max(ps)):
            st, cf, it = 2, nan2, 0
        else:
            x = np.array(pc, dtype=ld)
            x = np.log(x) - np.log1p(-x)
            t = np.array(yy, dtype=ld)

            def deviance(a_, b_):
                e = a_ + b_ * x
                return np.sum(np.log1p(np.exp(-np.abs(e))) + np.maximum(e, 0) - t * e)
            a_, b_ = np.log(ld(P) / ld(N)), ld(0)
            st, cf, it = 3, nan2, 0
            d_old = deviance(a_, b_)
            for it in range(1, 201):
                mu = 1 / (1 + np.exp(-(a_ + b_ * x)))
                w = mu * (1 - mu)
                g0, g1 = np.sum(t - mu), np.sum((t - mu) * x)
                h00, h01, h11 = np.sum(w), np.sum(w * x), np.sum(w * x * x)
                det = h00 * h11 - h01 * h01
                da, db = (h11 * g0 - h01 * g1) / det, (h00 * g1 - h01 * g0) / det
                if max(abs(da), abs(db)) <= ld(1e-16) * max(1, abs(a_), abs(b_)):
                    st, cf = 0, [a_ + da, b_ + db]
                    break
                step = ld(1)
                for _ in range(60):
                    d_new = deviance(a_ + step * da, b_ + step * db)
                    if not d_new - d_old > ld(1e-17) * abs(d_old):
                        break
                    step = step / 2
                a_, b_, d_old = a_ + step * da, b_ + step * db, d_new
        out["status"].append(st)
        out["coef"].append(cf)
        out["iters"].append(it)
    B = b1 - b0
    return {"pn": np.array(out["pn"], dtype=np.int64).reshape(B, 2), "brier": np.array(out["brier"], dtype=ld),
            "sum_p": np.array(out["sum_p"], dtype=ld), "bin_n": np.array(out["bin_n"], dtype=np.int64).reshape(B, K),
            "bin_pos": np.array(out["bin_pos"], dtype=np.int64).reshape(B, K),
            "bin_sum_p": np.array(out["bin_sum_p"], dtype=ld).reshape(B, K),
            "dc": np.array(out["dc"], dtype=np.int64).reshape(B, T, 2),
            "status": np.array(out["status"], dtype=np.int64), "coef": np.array(out["coef"], dtype=ld).reshape(B, 2),
            "iters": np.array(out["iters"], dtype=np.int64)}


# ---- paired bootstrap comparison of score columns -----------------------------------------------------
# Same resampling law again (_resample_counts here, csrc/resample.h in the kernels), the rows drawn ONCE
# per replicate and every column scored on them.  Column 0 is the reference model.  Definitions shared
# by the kernel, this mirror and the oracle, with hi_m = score_m > threshold:
#   reclass[m] = (eu, ed, nu, nd): drawn events with hi_0 = 1, hi_m = 0 (the reference moves the event
#                up) / with hi_0 = 0, hi_m = 1, and the same two patterns over the drawn non-events;
#   sums[m]    = Σc·p over the drawn positives, Σc·p over the drawn negatives, Σc·(p − y)², folded in
#                original row order: thread t of 1024 over rows [t·chunk, (t+1)·chunk), chunk =
#                ceil(n/1024), then the 64 lanes of a wave by an xor tree, then the 16 waves in order.


class CompareBootstrap(_NamedOutputs):
    """The outputs of ``bootstrap_compare`` in order, also by name."""
    _fields = ("auroc", "ap", "a2", "pn", "conf", "reclass", "sums")


class ComparePlan:
    """What is prepared once per call for labels ``y [n]`` and score columns ``scores [M, n]``: by
    original row ``y`` (uint8), ``p`` (f64 [M, n]) and ``hi`` (uint8 [M, n]: score > threshold); per
    column its descending stable score order ``order`` (int32 [M, n]: position → row) and, in that
    order, the labels ``ys`` (uint8) and every position's tie group ``gfirst``/``glast`` (int32);
    ``k0`` (int32 [M]: rows scoring > threshold); ``rowmap`` (int32 [n]: the positives' rows, then the
    negatives'; None in plain mode) and ``p0`` (draws j < p0 take the first stratum; plain: n)."""

    def __init__(self, y: torch.Tensor, scores: torch.Tensor, stratified: bool, threshold: float):
        dev = scores.device
        M, n = scores.shape
        s = scores.to(torch.float64).contiguous()
        pos = y.to(dev) > 0
        rows = torch.arange(n, device=dev)
        order, ys, gf, gl = [], [], [], []
        for m in range(M):
            o = torch.argsort(s[m], descending=True, stable=True)
            gfirst, glast = _tie_groups(s[m][o])
            order.append(o)
            ys.append(pos[o])
            gf.append(gfirst)
            gl.append(glast)
        self.n, self.M = n, M
        self.y = pos.to(torch.uint8).contiguous()
        self.p = s
        self.hi = (s > threshold).to(torch.uint8).contiguous()
        self.order = torch.stack(order).to(torch.int32).contiguous()
        self.ys = torch.stack(ys).to(torch.uint8).contiguous()
        self.gfirst = torch.stack(gf).to(torch.int32).contiguous()
        self.glast = torch.stack(gl).to(torch.int32).contiguous()
        self.k0 = (s > threshold).sum(1).to(torch.int32).contiguous()
        self.P = int(pos.sum())
        if stratified:
            self.rowmap = torch.cat([rows[pos], rows[~pos]]).to(torch.int32).contiguous()
            self.p0 = self.P
        else:
            self.rowmap = None
            self.p0 = n


def _compare_fold(t: torch.Tensor) -> torch.Tensor:
    """Σ over the last axis of ``t [B, n]`` (f64) in the kernel's order: chunk, wave xor tree, waves."""
    B, n = t.shape
    T, W = COMPARE_THREADS, COMPARE_WAVE
    chunk = (n + T - 1) // T
    pad = torch.zeros(B, T * chunk, dtype=t.dtype, device=t.device)
    pad[:, :n] = t
    pad = pad.reshape(B, T, chunk)
    acc = torch.zeros(B, T, dtype=t.dtype, device=t.device)
    for k in range(chunk):
        acc = acc + pad[:, :, k]
    acc = acc.reshape(B, T // W, W)
    lanes = torch.arange(W, device=t.device)
    o = W // 2
    while o > 0:
        acc = acc + acc[:, :, lanes ^ o]
        o //= 2
    out = torch.zeros(B, dtype=t.dtype, device=t.device)
    for w in range(T // W):
        out = out + acc[:, w, 0]
    return out


def bootstrap_compare(y: torch.Tensor, scores: torch.Tensor, n_boot: int, *, seed: int = 0,
                      stratified: bool = False, threshold: float = 0.5, b0: int = 0, b1=None,
                      chunk_elems: int = 1 << 22):
    """Vectorised torch mirror of the comparison kernel (and the host path of
    ``ops.bootstrap_compare``, which validates): the counts by ``bincount`` over the draws of the law
    above, indexed by original row, then per column the formulas of :func:`bootstrap_metrics` on the
    counts gathered through that column's order, and the paired statistics of the header.  Returns a
    :class:`CompareBootstrap` for replicates ``b0:b1``: ``auroc``, ``ap`` (f64) and ``a2`` (int64)
    ``[B, M]``, ``pn [B, 2]``, ``conf [B, M, 4]`` (TP FP FN TN), ``reclass [B, M, 4]`` (eu ed nu nd; column
    0 zero) and ``sums [B, M, 3]`` (f64).  Replicates are processed ``chunk_elems // n`` at a time."""
    pl = ComparePlan(y, scores, stratified, threshold)
    dev = scores.device
    n, M = pl.n, pl.M
    b1 = n_boot if b1 is None else b1
    i64, f64 = torch.int64, torch.float64
    rowmap = pl.rowmap.to(i64) if pl.rowmap is not None else None
    yb = pl.y > 0
    yf = pl.y.to(f64)
    hi = pl.hi > 0
    k0 = pl.k0.tolist()
    groups = [_group_ends(pl.gfirst[m].to(i64), pl.glast[m].to(i64)) for m in range(M)]
    outs = [[] for _ in range(7)]
    for _, cnt in _resample_counts(rowmap, pl.p0, n, seed, b0, b1, max(1, chunk_elems // n), dev):
        C = cnt.to(f64)
        cols = [[] for _ in range(6)]
        pn = None
        for m in range(M):
            Pb, Nb, _, _, _, a2, auroc, ap, conf = _rank_stats(cnt[:, pl.order[m].to(i64)], pl.ys[m].to(i64),
                                                               *groups[m], k0[m])
            if m == 0:
                pn = torch.stack([Pb, Nb], 1)
            up, down = hi[0] & ~hi[m], ~hi[0] & hi[m]
            rc = torch.stack([(cnt * (m_ & c_).to(i64)).sum(1) for m_, c_ in
                              ((up, yb), (down, yb), (up, ~yb), (down, ~yb))], 1)
            cpm = C * pl.p[m][None, :]
            d = pl.p[m] - yf
            sm = torch.stack([_compare_fold(torch.where(yb[None, :], cpm, 0.0)),
                              _compare_fold(torch.where(yb[None, :], 0.0, cpm)),
                              _compare_fold(C * (d * d)[None, :])], 1)
            for o_, v in zip(cols, (auroc, ap, a2, conf, rc, sm)):
                o_.append(v)
        au, ap_, a2_, cf, rc_, sm_ = (torch.stack(c, 1) for c in cols)
        for o_, v in zip(outs, (au, ap_, a2_, pn, cf, rc_, sm_)):
            o_.append(v)
    if not outs[0]:
        def e(*shape, dtype):
            return torch.empty(*shape, dtype=dtype, device=dev)
        return CompareBootstrap(e(0, M, dtype=f64), e(0, M, dtype=f64), e(0, M, dtype=i64), e(0, 2, dtype=i64),
                                e(0, M, 4, dtype=i64), e(0, M, 4, dtype=i64), e(0, M, 3, dtype=f64))
    return CompareBootstrap(*(torch.cat(o) for o in outs))


# ---- permutation importance -----------------------------------------------------------------------
# The permutation law (the only place it is written on the host side; ops.permutation_sources runs
# this function on either device): for seed s and repeat r, row i ∈ [0, n) gets
#     key = splitmix64(s ^ splitmix64((r << 25) ^ i)) >> 1         (logical shift: 0 ≤ key < 2^63)
# and src_r = the stable ascending argsort of the keys — a permutation even when two keys collide.
# One permutation per repeat, shared by every column (a paired design).  Hybrid row (k, r, i) is x[i]
# with column k replaced by x[src_r[i]][k].  n ≤ 2^25, r < 2^24.

def permutation_sources(n: int, r0: int, r1: int, seed: int = 0, device="cpu", chunk_elems: int = 1 << 22):
    """``src [r1 − r0, n]`` (int32) of the law above for repeats ``r0:r1``, ``chunk_elems // n`` repeats
    at a time; repeat r does not depend on the range or the chunk it is computed in."""
    i64 = torch.int64
    dev = torch.device(device)
    i = torch.arange(n, dtype=i64, device=dev)
    sd = torch.tensor(_seed_i64(seed), dtype=i64, device=dev)
    out = torch.empty(r1 - r0, n, dtype=torch.int32, device=dev)
    per = max(1, chunk_elems // max(n, 1))
    for c0 in range(r0, r1, per):
        rs = torch.arange(c0, min(r1, c0 + per), dtype=i64, device=dev)
        key = _splitmix64_t(sd ^ _splitmix64_t((rs[:, None] << 25) ^ i[None, :]))
        key = (key >> 1) & ((1 << 63) - 1)
        out[c0 - r0:c0 - r0 + rs.numel()] = torch.argsort(key, dim=1, stable=True).to(torch.int32)
    return out


def stack_permute_scores(x: torch.Tensor, pk, src: torch.Tensor, features: torch.Tensor, chunk: int = 4096):
    """fp64 mirror of ``ops.stack_permute_scores``: ``S [K, R, n]`` = :func:`stack_infer` of the
    materialised hybrid rows (``features[kf] = −1``: the rows as they are).  ``x`` is first rounded to
    f32, as the kernel sees it; ``chunk // n`` repeats are materialised at a time (a few thousand rows per
    call: :func:`rbf_decision` builds a [rows, SVs, F] f64 tensor, 59 kB per row of the shipped model)."""
    x = x.to(torch.float32).to(torch.float64)
    src = src.to(torch.int64)
    n, F = x.shape
    R = src.shape[0]
    S = torch.empty(len(features), R, n, dtype=torch.float64)
    per = max(1, chunk // n)
    for kf, k in enumerate(int(v) for v in features):
        for c0 in range(0, R, per):
            c1 = min(R, c0 + per)
            h = x[None, :, :].repeat(c1 - c0, 1, 1)                     # [repeats, n, F]
            if k >= 0:
                h[:, :, k] = x[:, k][src[c0:c1]]
            S[kf, c0:c1] = stack_infer(h.reshape(-1, F), pk).reshape(c1 - c0, n)
    return S


class RankMetrics(_NamedOutputs):
    """The outputs of ``rank_metrics`` in order, also by name."""
    _fields = ("a2", "auroc", "ap", "brier")


def rank_metrics(y: torch.Tensor, scores: torch.Tensor, chunk_elems: int = 1 << 22):
    """Torch mirror of the ``rank_rows`` kernel (and the host path of ``ops.rank_metrics``, which
    validates): every row of ``scores [M, n]`` ranked against the labels ``y [n]``.  ``a2 [M]`` (int64) =
    the exact doubled AUROC numerator over tie groups, ``auroc`` = ``a2 / (2·P·N)``, ``ap`` = the kernel's
    tie-group formula and ``brier`` = ``Σ(score − y)² / n`` folded as the kernel folds it (f64).  Ties
    are equal values of ``scores``' own dtype.  ``chunk_elems // n`` rows at a time."""
    i64, f64 = torch.int64, torch.float64
    dev = scores.device
    M, n = scores.shape
    yi = (y.to(dev) > 0).to(i64)
    P = int(yi.sum())
    N = n - P
    last = torch.ones(1, dtype=torch.bool, device=dev)
    outs = [[] for _ in range(4)]
    per = max(1, chunk_elems // n)
    for c0 in range(0, M, per):
        s = scores[c0:c0 + per]
        m = s.shape[0]
        ss, order = torch.sort(s, dim=1, descending=True, stable=True)
        ys = yi[order]
        cp, cn = torch.cumsum(ys, 1), torch.cumsum(1 - ys, 1)
        end = torch.cat([ss[:, 1:] != ss[:, :-1], last.expand(m, 1)], 1)
        # the cumulative counts at the previous group end (both are nondecreasing along the row)
        z = torch.zeros(m, 1, dtype=i64, device=dev)
        cp0 = torch.cat([z, torch.cummax(torch.where(end, cp, 0), 1).values[:, :-1]], 1)
        cn0 = torch.cat([z, torch.cummax(torch.where(end, cn, 0), 1).values[:, :-1]], 1)
        a2 = torch.where(end, (cn - cn0) * (cp + cp0), 0).sum(1)
        term = torch.where(end & (cp != cp0), ((cp - cp0) * cp).to(f64) / (cp + cn).to(f64), 0.0)
        d = s.to(f64) - yi.to(f64)[None, :]
        nan = float("nan")
        deg = P == 0 or N == 0
        outs[0].append(a2)
        # tensor divisors: torch turns a division by a Python scalar on ``cuda`` into a product with its reciprocal
        den = torch.tensor([2 * P * N, P, n], dtype=f64, device=dev)
        outs[1].append(a2.to(f64) / den[0] if not deg else torch.full((m,), nan, dtype=f64, device=dev))
        outs[2].append(term.sum(1) / den[1] if not deg else torch.full((m,), nan, dtype=f64, device=dev))
        outs[3].append(_compare_fold(d * d) / den[2])
    if not outs[0]:
        return RankMetrics(torch.empty(0, dtype=i64, device=dev), *(torch.empty(0, dtype=f64, device=dev)
                                                                    for _ in range(3)))
    return RankMetrics(*(torch.cat(o) for o in outs))


def compare_oracle(y, scores, n_boot: int, *, seed: int = 0, stratified: bool = False, threshold: float = 0.5,
                   b0: int = 0, b1=None):
    """Independent oracle for the tests: ``a2``, ``ap`` and ``conf`` of every column come from
    :func:`bootstrap_oracle` on that column alone (which materialises the resample itself);
    ``reclass`` is counted row by row on the rows ``bootstrap_resample`` draws by comparing each drawn
    score with the threshold; ``sums`` add the drawn rows' terms in ``numpy.longdouble``.  Returns numpy
    arrays named as the op's outputs (``auroc``, ``ap``, ``sums`` longdouble, the rest int64) in a dict,
    plus ``n_degenerate``."""
    np = _np()
    ld = np.longdouble
    y = [int(v) for v in np.asarray(y).reshape(-1)]
    S = np.asarray(scores, dtype=np.float64)
    M = S.shape[0]
    b1 = n_boot if b1 is None else b1
    B = b1 - b0
    per = [bootstrap_oracle(y, S[m], n_boot, seed=seed, stratified=stratified, threshold=threshold,
                            grid_points=2, b0=b0, b1=b1) for m in range(M)]
    reclass = np.zeros((B, M, 4), dtype=np.int64)
    sums = np.zeros((B, M, 3), dtype=ld)
    for b in range(b0, b1):
        idx = bootstrap_resample(y, b, seed, stratified)
        for m in range(M):
            for i in idx:
                p, p_ref, event = float(S[m][i]), float(S[0][i]), y[i] == 1
                if m > 0 and p_ref > threshold and not p > threshold:
                    reclass[b - b0, m, 0 if event else 2] += 1
                if m > 0 and not p_ref > threshold and p > threshold:
                    reclass[b - b0, m, 1 if event else 3] += 1
                sums[b - b0, m, 0 if event else 1] += ld(p)
                sums[b - b0, m, 2] += (ld(p) - ld(1 if event else 0)) ** 2
    res = {"auroc": np.stack([o["auroc"] for o in per], 1).reshape(B, M),
           "ap": np.stack([o["ap"] for o in per], 1).reshape(B, M),
           "a2": np.stack([o["a2"] for o in per], 1).reshape(B, M), "pn": per[0]["pn"],
           "conf": np.stack([o["conf"] for o in per], 1).reshape(B, M, 4), "reclass": reclass, "sums": sums}
    res["n_degenerate"] = per[0]["n_degenerate"]
    return res


def delong_oracle(y, pa, pb):
    """DeLong, DeLong and Clarke-Pearson's test of two correlated AUROCs by its O(P·N) structural
    components, in ``numpy.longdouble``: ψ(x, z) = 1, ½, 0 for x >, =, < z; V10_i = mean_j ψ(x_i, z_j)
    over the negatives, V01_j = mean_i ψ(x_i, z_j) over the positives; the variance of the AUROC
    difference is (S10_aa + S10_bb − 2·S10_ab)/P + (S01_aa + S01_bb − 2·S01_ab)/N with the sample
    covariances S (denominators P − 1 and N − 1).  Returns ``auc_a``, ``auc_b``, ``delta`` and ``se``."""
    np = _np()
    ld = np.longdouble
    y = np.asarray(y).reshape(-1)
    pos = y == 1
    P, N = int(pos.sum()), int((~pos).sum())
    V10, V01, auc = [], [], []
    for s in (pa, pb):
        s = np.asarray(s, dtype=np.float64).reshape(-1)
        x, z = s[pos].astype(ld), s[~pos].astype(ld)
        psi = (x[:, None] > z[None, :]).astype(ld) + (x[:, None] == z[None, :]).astype(ld) / ld(2)
        V10.append(psi.sum(1) / ld(N))
        V01.append(psi.sum(0) / ld(P))
        auc.append(psi.sum() / ld(P) / ld(N))

    def cov(u, v, k):
        return ((u - u.mean()) * (v - v.mean())).sum() / ld(k - 1)
    var = (cov(V10[0], V10[0], P) + cov(V10[1], V10[1], P) - 2 * cov(V10[0], V10[1], P)) / ld(P) \
        + (cov(V01[0], V01[0], N) + cov(V01[1], V01[1], N) - 2 * cov(V01[0], V01[1], N)) / ld(N)
    return {"auc_a": auc[0], "auc_b": auc[1], "delta": auc[0] - auc[1], "se": np.sqrt(max(var, ld(0)))}


# ----------------------------------------------------------------------------- working-set SVC oracle
# numpy only, written from libsvm's published rules (Fan, Chen, Lin 2005: the C-SVC dual, I_up / I_low,
# m(α) − M(α), calculate_rho) and from the documented behaviour of ops/csrc/svm_ws.hip.  Nothing here
# imports torch or models/smo.py, so a wrong sign, membership test or rounding in the solver is on one
# side of the comparison only.  Conventions of the solver's problem table (``WsProb``): the first
# ``npos`` points have y = +1, the rest y = −1; the box is [0, Cp] / [0, Cn]; the kernel is
# K(a, b) = 2^(ngl2e·‖a − b‖²) with ``ngl2e`` = −γ·log2 e AS STORED, an f32.  That f32 defines γ
# (γ = −ngl2e / log2 e exactly): quantising γ is part of the problem, not an arithmetic error.
WS_LONGDOUBLE_MAX = 4096        # points up to which the oracle runs in longdouble


def _ws_labels(l, npos, Cp, Cn):
    np = _np()
    pos = np.arange(l) < int(npos)
    return pos, np.where(pos, 1.0, -1.0), np.where(pos, float(Cp), float(Cn))


def ws_kernel_matvec(Z32, e2, v, dtype=None, rows=None):
    """``Σ_c 2^(e2·‖z_t − z_c‖²)·v_c`` for every row t (or ``rows``), distances by direct differences,
    over the columns with v_c ≠ 0 only (a zero column contributes an exact zero).  ``e2`` is the
    base-2 exponent scale (−γ·log2 e), taken as given.  ``dtype`` longdouble, or float64 in row
    chunks (see :func:`svc_dual_oracle`)."""
    np = _np()
    T = np.longdouble if dtype is None else dtype
    Z = np.asarray(Z32, dtype=np.float32).astype(T)
    v = np.asarray(v).astype(T)
    cols = np.flatnonzero(v != 0)
    R = Z if rows is None else Z[rows]
    out = np.zeros(R.shape[0], dtype=T)
    if cols.size == 0:
        return out
    B, vb = Z[cols], v[cols]
    step = max(1, (1 << 21) // max(1, B.shape[0] * Z.shape[1]))
    e2 = T(e2)
    with np.errstate(under="ignore"):
        for s in range(0, R.shape[0], step):
            diff = R[s:s + step, None, :] - B[None, :, :]
            d2 = (diff * diff).sum(-1)
            out[s:s + step] = (np.exp2(e2 * d2) * vb[None, :]).sum(-1)
    return out


def svc_kkt(alpha, G, npos, Cp, Cn):
    """libsvm's optimality measure and threshold from α and a gradient G (any float type):

    * I_up = {y = +1, α < C} ∪ {y = −1, α > 0},  I_low = {y = +1, α > 0} ∪ {y = −1, α < C};
      ``m = max_{I_up} −yG``, ``M = min_{I_low} −yG``; libsvm stops when m − M < eps.  Returned as
      ``(gap, gmax_up, gmax_low)`` with gmax_up = m, gmax_low = −M, gap = gmax_up + gmax_low
      (−inf for an empty set).
    * ``calculate_rho``: the mean of yG over the free points (0 < α < C); with none,
      (ub + lb)/2 where ub = min yG over {α = C, y = −1} ∪ {α = 0, y = +1} and lb = max yG over
      {α = C, y = +1} ∪ {α = 0, y = −1}."""
    np = _np()
    alpha = np.asarray(alpha)
    G = np.asarray(G)
    pos, y, C = _ws_labels(alpha.shape[0], npos, Cp, Cn)
    yG = np.where(pos, G, -G)
    up = np.where(pos, alpha < C, alpha > 0)
    low = np.where(pos, alpha > 0, alpha < C)
    ninf = -np.inf
    gu = (-yG[up]).max() if up.any() else ninf
    gl = yG[low].max() if low.any() else ninf
    upper, lower = alpha >= C, alpha <= 0
    free = ~upper & ~lower
    if free.any():
        rho = yG[free].sum() / free.sum()
    else:
        ubm = (upper & ~pos) | (lower & ~upper & pos)
        lbm = (upper & pos) | (lower & ~upper & ~pos)
        ub = yG[ubm].min() if ubm.any() else np.inf
        lb = yG[lbm].max() if lbm.any() else ninf
        rho = (ub + lb) / 2
    return {"gap": gu + gl, "gmax_up": gu, "gmax_low": gl, "rho": rho}


def svc_dual_oracle(Z32, npos, Cp, Cn, ngl2e_f32, alpha):
    """The C-SVC dual at ``alpha`` for the f32 rows ``Z32`` as the solver sees them.

    Dual: min ½ αᵀQα − Σα, Q_tc = y_t y_c K_tc, 0 ≤ α ≤ C, Σ yα = 0.  Its gradient is
    ``G* = Qα − 1 = −1 + y ∘ K (y ∘ α)``, so αᵀQα = α·(G* + 1) and the objective is ½ α·(G* − 1).
    K is evaluated with direct-difference distances and the exponent scale read back from the
    stored f32 (see the section comment).  Returns a dict: ``G`` (per point), ``obj``, ``sya``
    (Σ yα), ``gap``, ``gmax_up``, ``gmax_low``, ``rho`` (:func:`svc_kkt` of α and G*).

    Up to ``WS_LONGDOUBLE_MAX`` points everything is longdouble.  Above, K (y∘α) runs in f64 row
    chunks over the columns with α ≠ 0: a row's f64 sum is off by at most nSV·2⁻⁵³·Σ_c α_c K_tc, while
    every budget it is compared with (:func:`ws_gupdate_budget`) holds a term U·Σ_c |Δα_c| K_tc with
    U = 2⁻²⁴ per update and the coefficients moved at least once in total: the ratio is
    nSV·2⁻²⁹ ≈ 2e-9·nSV, below 1e-4 of the budget for any nSV this oracle can afford."""
    np = _np()
    L = np.longdouble
    alpha = np.asarray(alpha, dtype=np.float64)
    l = alpha.shape[0]
    pos, y, C = _ws_labels(l, npos, Cp, Cn)
    T = L if l <= WS_LONGDOUBLE_MAX else np.float64
    e2 = np.float32(ngl2e_f32)
    G = (-1 + y.astype(T) * ws_kernel_matvec(Z32, e2, y * alpha, T)).astype(L)
    a = alpha.astype(L)
    out = svc_kkt(a, G, npos, Cp, Cn)
    out.update(G=G, obj=(a * (G - 1)).sum() / 2, sya=(y.astype(L) * a).sum())
    return out


def ws_kernel_error(Z32, ngl2e_f32, cols=None, rows=None):
    """``(K, dK)`` [rows (default all), cols], f64: the kernel values and the forward bound of svm_ws.hip's f32
    evaluation ``exp2(min(fma(k2, a·b, sn_a + sn_b), 0))`` with k2 = −2·ngl2e (exact, a power of two
    times an f32), a·b an F-term f32 fma chain from 0 and sn_x = fl(ngl2e·fl_chain(‖x‖²)) — the
    expression whose bound :func:`_rbf_core` derives for inference, without its term for rounding
    γ·log2 e (here the stored f32 IS the scale).  In base-2 exponent units, with g2 = −ngl2e and
    n-term chains costing γ_n = nU/(1 − nU):

    * the two ‖x‖² chains and their products with ngl2e: g2·γ_{F+1}·(‖a‖² + ‖b‖²);
    * the rounding of sn_a + sn_b: g2·U·(‖a‖² + ‖b‖²);
    * the dot chain through k2: 2·g2·γ_F·|a|·|b|;
    * the final fma: U·g2·(‖a‖² + ‖b‖² + 2|a|·|b|) at most;

    together ≤ g2·γ_{F+3}·mag, mag = ‖a‖² + ‖b‖² + 2|a|·|b| (the ``(F+3)·U·mag`` term of
    ``_rbf_core``).  The clamp at 0 only moves the exponent towards the true one (≤ 0).  Then
    exp2's own error: K̂ = K·2^δ·(1 + ε), |ε| ≤ EPS_EXP2, plus _TINY for a flushed result.  This
    function's own f64 Gram-form distances are off by ≤ (F+2)·2⁻⁵²·mag, added to δ."""
    np = _np()
    Z = np.asarray(Z32, dtype=np.float32).astype(np.float64)
    F = Z.shape[1]
    B = Z if cols is None else Z[cols]
    if rows is not None:
        Z = Z[rows]
    g2 = -float(np.float32(ngl2e_f32))
    na, nb = (Z * Z).sum(1), (B * B).sum(1)
    cross = np.abs(Z) @ np.abs(B).T
    mag = na[:, None] + nb[None, :] + 2 * cross
    d2 = np.maximum(na[:, None] + nb[None, :] - 2 * (Z @ B.T), 0.0)
    n = F + 3
    de = g2 * mag * (n * _U / (1 - n * _U) + (F + 2) * 2.0 ** -52)
    with np.errstate(under="ignore"):
        K = np.exp2(-g2 * d2)
    x = np.expm1(math.log(2.0) * de)
    return K, K * (x + EPS_EXP2 + x * EPS_EXP2) + _TINY


def ws_gupdate_budget(Z32, ngl2e_f32, dalpha, ncp, order=None, npos=None, rows=None):
    """Per-row forward error bound of ONE gradient update of svm_ws.hip,
    ``G_t += y_t·Σ_c fl32(y_c Δα_c)·K̂_tc`` accumulated by f32 fmas over the ``ncp`` staged columns
    (changed coefficients padded to a multiple of 32), then added to the f64 G:

    * the kernel values: Σ_c |Δα_c|·dK_tc (:func:`ws_kernel_error`);
    * the coefficient rounded to f32 (``wdc`` is float): U·Σ_c |Δα_c|·K̂_tc;
    * the f32 accumulation.  Without ``order``, the worst case of any summation of ncp terms:
      γ_ncp·Σ_c |Δα_c|·K̂_tc, γ_n = nU/(1 − nU) (at 1,024 columns this term is 6e-5 of the sum
      of magnitudes and dominates everything else by an order of magnitude).  With ``order`` — the
      changed points in the order the solver staged them (working-set slot order) — and ``npos``,
      the kernel's real summation tree: staged position p goes to half h = (p/4) mod 2 of a lane
      pair; each half is ONE sequential chain pa = fma(cf_p, K̂_p, pa), whose k-th step rounds
      once, by ≤ U·|ŝ_k| with ŝ_k the computed partial sum, and the halves are added once.  With
      s_k the exact signed partial sum of y_c Δα_c K_tc, |ŝ_k| ≤ |s_k| + Σ_{i≤k}|Δα_i|(dK_i +
      U·K̂_i) + γ_n·Σ_{i≤k}|Δα_i|K̂_i (n = the chain's length), so the chain costs
      U·Σ_k [that bound] and the final add U·(1 + γ_n)·Σ_c|Δα_c|K̂_tc at most.  Padding columns
      carry cf = 0: fma(0, ·, pa) = pa exactly.  Signed partial sums of a gradient update cancel
      like a random walk, which the worst case cannot see;

    with K̂ ≤ K + dK.  The f64 add to G (2⁻⁵³·|G_t|) is left to the caller, who knows G.  Budgets
    add over rounds.  ``rows``: bound these rows only.  A seeded start (``ws_seed``) is the
    worst-case expression with Δα = the seed and ncp = 256: at most 256 compacted coefficients per
    f32 partial, the partials summed in f64.

    Measured on an MI355X (tests/test_svm_ws_reference_gpu.py, summation-tree form, every round of
    every case): the largest |G_dev − G*| / cumulative budget is 0.12 (0.029 at the end-to-end
    tests' sizes, 0.013 after a seed)."""
    np = _np()
    sd = np.asarray(dalpha, dtype=np.float64)
    d = np.abs(sd)
    l = d.shape[0] if rows is None else len(rows)
    cols = np.flatnonzero(d != 0) if order is None else np.asarray(order, dtype=np.int64)
    if cols.size == 0:
        return np.zeros(l)
    K, dK = ws_kernel_error(Z32, ngl2e_f32, cols, rows)
    w = d[cols]
    Kh = K + dK
    term = dK @ w + _U * (Kh @ w)
    if order is None:
        n = float(ncp)
        return term + n * _U / (1 - n * _U) * (Kh @ w)
    assert npos is not None and np.array_equal(np.sort(cols), np.flatnonzero(d != 0))
    sgn = np.where(cols < int(npos), 1.0, -1.0) * sd[cols]
    half = (np.arange(cols.size) // 4) % 2
    acc = np.zeros(l)
    for h in (0, 1):
        ix = np.flatnonzero(half == h)
        if ix.size == 0:
            continue
        n = float(ix.size)
        gam = n * _U / (1 - n * _U)
        S = np.abs(np.cumsum(K[:, ix] * sgn[ix][None, :], axis=1))
        E = np.cumsum((dK[:, ix] + _U * Kh[:, ix]) * w[ix][None, :], axis=1)
        P = np.cumsum(Kh[:, ix] * w[ix][None, :], axis=1)
        acc += _U * (S + E + gam * P).sum(1)
    n = float((cols.size + 1) // 2)
    return term + acc + _U * (1 + n * _U / (1 - n * _U)) * (Kh @ w)


def ws_okey(v):
    """The solver's order-preserving u32 key of the f32 rounding of ``v`` (common.h f32_okey)."""
    np = _np()
    u = np.asarray(v, dtype=np.float64).astype(np.float32).view(np.uint32)
    return u ^ np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


WS_KEY_BITS = 22   # two 11-bit radix levels: the selector ranks keys by their top 22 bits


def ws_select_oracle(alpha, G, npos, Cp, Cn, Q, prev, key_bits=WS_KEY_BITS):
    """The working-set selection rule of svm_ws.hip, from the α and G the selector saw.

    1. keys: the f32 values of −yG for the members of I_up and of yG for the members of I_low
       (membership from the f64 α, :func:`svc_kkt`), as order-preserving u32 (:func:`ws_okey`);
    2. the min(Q/4, n_up) largest up keys;
    3. the min(Q/4, n_low) largest low keys, WITHOUT the positions already taken for up: the
       threshold is found over every member of I_low, the up picks are then left out and not
       replaced, so the low list may be shorter than Q/4;
    4. keys are ranked by their top ``key_bits`` bits (the selector's two 11-bit radix levels resolve
       no more: within a 2⁻¹³ relative window below the threshold, keys are ties).  With T the
       truncated key of the k-th largest member and ``above`` the members over T, every free
       position over T is taken and then the first k − above free ties at T in position order;
    5. then the previous round's new picks ``prev`` that were not picked again, in their old order.

    Returns ``(up, low, carried)``: the new up and low picks in position order and the carried-over
    sequence (int64).  With an empty I_up or I_low the selector stops: all three are empty."""
    np = _np()
    alpha = np.asarray(alpha, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    l = alpha.shape[0]
    pos, y, C = _ws_labels(l, npos, Cp, Cn)
    yG = np.where(pos, G, -G)
    up = np.where(pos, alpha < C, alpha > 0)
    low = np.where(pos, alpha > 0, alpha < C)
    sh = np.uint32(32 - key_bits)
    ku = np.where(up, ws_okey(-yG), np.uint32(0))
    kl = np.where(low, ws_okey(yG), np.uint32(0))
    e = np.zeros(0, dtype=np.int64)
    n_up, n_low = int((ku != 0).sum()), int((kl != 0).sum())
    if n_up == 0 or n_low == 0:
        return e, e, e

    taken = np.zeros(l, dtype=bool)

    def top(k, count):
        kt = (k >> sh).astype(np.int64)
        member = k != 0
        T = np.sort(kt[member])[::-1][count - 1]
        need = count - int((member & (kt > T)).sum())
        free = member & ~taken
        return np.sort(np.concatenate([np.flatnonzero(free & (kt > T)), np.flatnonzero(free & (kt == T))[:need]]))

    pu = top(ku, min(Q // 4, n_up))
    taken[pu] = True
    pl = top(kl, min(Q // 4, n_low))
    taken[pl] = True
    prev = np.asarray(prev, dtype=np.int64)
    return pu, pl, prev[~taken[prev]] if prev.size else e


# ----------------------------------------------------------------------------- linear-model certificates
# numpy longdouble, written from the objectives themselves (liblinear's L1 / lbfgs's L2 logistic
# objective, newGLMNET's quadratic subproblem, sklearn's Gram-form lasso duality gap), with the f64
# arrays a kernel receives taken as exact.  A convex optimum needs no second solver: the min-norm
# subgradient or the duality gap at the kernel's own answer certifies it however it was reached.
# Nothing here imports torch, models/logreg_solver.py or models/lasso.py.
def _ld(a):
    np = _np()
    return np.asarray(a, dtype=np.float64).astype(np.longdouble)


def _lm_softplus(x):
    """log(1 + e^x) without overflow: max(x, 0) + log1p(e^−|x|)."""
    np = _np()
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _lm_sigmoid(x):
    """1 / (1 + e^−x) without overflow (e^x / (1 + e^x) for x < 0)."""
    np = _np()
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def logreg_objective(Xa, s, ypm, w, C, l1, penal):
    """``C·Σ_r s_r·softplus(−y_r·x̃_r·w) + Σ_{j penalised} |w_j|`` (``l1``) or ``½ w_j²``."""
    np = _np()
    Xa, s, y, w = _ld(Xa), _ld(s), _ld(ypm), _ld(w)
    pen = np.asarray(penal).astype(bool)
    data = np.longdouble(C) * (s * _lm_softplus(-y * (Xa @ w))).sum()
    return data + (np.abs(w[pen]).sum() if l1 else (w[pen] * w[pen]).sum() / 2)


def _logreg_grad(Xa, s, y, w, C):
    # d/dw C·Σ s·softplus(−y z) = −C·Σ s·y·σ(−y z)·x̃
    return _np().longdouble(C) * ((-(s * y * _lm_sigmoid(-y * (Xa @ w)))) @ Xa)


def _min_norm_subgradient(g, w, pen, l1):
    np = _np()
    if not l1:
        return np.where(pen, g + w, g)
    at0 = np.sign(g) * np.maximum(np.abs(g) - 1, 0)
    return np.where(pen, np.where(w != 0, g + np.sign(w), at0), g)


def logreg_kkt(Xa, s, ypm, w, C, l1, penal):
    """The 1-norm of the min-norm subgradient of :func:`logreg_objective` at ``w``, with g the
    gradient of the data term: L1 and penalised, g_j + sign(w_j) where w_j ≠ 0 and
    sign(g_j)·max(|g_j| − 1, 0) where w_j = 0; L2 and penalised, g_j + w_j; unpenalised, g_j.
    Returns ``{"norm", "norm0", "ratio"}``: the norm at w, at w = 0, and norm / norm0 (the solvers'
    relative stopping measure; 0 when w = 0 is itself optimal and the norm at w is 0)."""
    np = _np()
    Xa, s, y, w = _ld(Xa), _ld(s), _ld(ypm), _ld(w)
    pen = np.asarray(penal).astype(bool)
    norm = np.abs(_min_norm_subgradient(_logreg_grad(Xa, s, y, w, C), w, pen, l1)).sum()
    w0 = np.zeros_like(w)
    norm0 = np.abs(_min_norm_subgradient(_logreg_grad(Xa, s, y, w0, C), w0, pen, l1)).sum()
    ratio = norm / norm0 if norm0 > 0 else (np.longdouble(0) if norm == 0 else np.longdouble(np.inf))
    return {"norm": norm, "norm0": norm0, "ratio": ratio}


def _ld_solve(A, b):
    """A x = b in longdouble by Gaussian elimination with partial pivoting (numpy's LAPACK front end
    has no longdouble)."""
    np = _np()
    A = np.array(A, dtype=np.longdouble)
    x = np.array(b, dtype=np.longdouble)
    m = A.shape[0]
    for k in range(m):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            x[[k, p]] = x[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        x[k + 1:] -= f * x[k]
    for k in range(m - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def logreg_newton_step(Xa, s, ypm, C, penal):
    """The first damped-Newton step of the L2 objective from w = 0, exactly.  At w = 0 every σ is ½:
    g = −½·C·Σ s·y·x̃, H = ¼·C·X̃ᵀ diag(s) X̃, and the direction is d = −(H + diag(pen))⁻¹ g.
    Returns a dict: ``d``, ``A`` (= H + diag(pen)), ``g``, ``F0``, ``delta`` (= gᵀd), ``FK`` (the eight
    trial objectives F(2^-k·d)), ``k`` (the first step with F_k ≤ F0 + 0.01·2^-k·delta, the
    solvers' Armijo rule; None when no step passes) and ``margin`` (the smallest
    |F_k − (F0 + 0.01·2^-k·delta)| over the steps tested up to and including k: how far the choice
    is from flipping)."""
    np = _np()
    L = np.longdouble
    Xa, s, y = _ld(Xa), _ld(s), _ld(ypm)
    pen = np.asarray(penal).astype(bool)
    g = -L(C) / 2 * ((s * y) @ Xa)
    A = L(C) / 4 * ((Xa * s[:, None]).T @ Xa) + np.diag(pen.astype(L))
    d = -_ld_solve(A, g)
    zero = np.zeros_like(d)
    F0 = logreg_objective(Xa, s, y, zero, C, False, pen)
    delta = g @ d
    FK = np.array([logreg_objective(Xa, s, y, d * L(2.0) ** -k, C, False, pen) for k in range(8)], dtype=L)
    thr = F0 + L(0.01) * L(2.0) ** -np.arange(8) * delta
    ok = FK <= thr
    k = int(np.argmax(ok)) if ok.any() else None
    margin = np.abs(FK - thr)[: (k + 1) if k is not None else 8].min()
    return {"d": d, "A": A, "g": g, "F0": F0, "delta": delta, "FK": FK, "k": k, "margin": margin}


def l1qp_kkt(H, g, w, penal, lam, d, tol=1e-12):
    """Per-coordinate KKT residual of ``min_d gᵀd + ½dᵀHd + λ·Σ_{pen}|w_j + d_j|`` at ``d``: with
    r = g + Hd and u = w + d, r_j + λ·sign(u_j) where penalised and u_j ≠ 0,
    sign(r_j)·max(|r_j| − λ, 0) where penalised and u_j = 0, r_j where unpenalised.

    Also the bound a cyclic coordinate descent stopped by "largest step of the last sweep ≤ tol"
    must meet: coordinate j is exact when it is updated and every later step of that sweep moves
    r_j by at most tol·|H_jk|, so |res_j| ≤ tol·Σ_k|H_jk| plus the f64 rounding of the terms of
    r_j, 4·eps·(|g_j| + Σ_k|H_jk||d_k| + λ).  Returns ``(res, bound)``, longdouble [F1]."""
    np = _np()
    H, g, w, d = _ld(H), _ld(g), _ld(w), _ld(d)
    pen = np.asarray(penal).astype(bool)
    lam = np.longdouble(lam)
    r, u = g + H @ d, w + d
    at0 = np.sign(r) * np.maximum(np.abs(r) - lam, 0)
    res = np.where(pen, np.where(u != 0, r + lam * np.sign(u), at0), r)
    eps = np.longdouble(np.finfo(np.float64).eps)
    aH = np.abs(H)
    bound = np.longdouble(tol) * aH.sum(1) + 4 * eps * (np.abs(g) + aH @ np.abs(d) + lam)
    return res, bound


def lasso_gap_oracle(G, q, yy, n, alpha, w):
    """sklearn's Gram-form duality gap (``enet_coordinate_descent_gram``, l2_reg = 0) of
    ``½‖y − Xw‖² + α·n·‖w‖₁`` from G = XᵀX, q = Xᵀy, yy = yᵀy: with R² = yy − 2wᵀq + wᵀGw and
    ν = max|q − Gw|, c = min(1, αn/ν), gap = ½R²(1 + c²) + αn‖w‖₁ − c·(yy − wᵀq)  (R² when c = 1).
    Also the cancellation budget of an f64 evaluation of R² from its three terms,
    ``8·eps·(yy + 2Σ|w_j q_j| + Σ|w_j||(Gw)_j|)``.  Returns ``(gap, budget)``."""
    np = _np()
    G, q, w = _ld(G), _ld(q), _ld(w)
    yy, l1 = np.longdouble(yy), np.longdouble(alpha) * np.longdouble(n)
    Gw = G @ w
    wq = w @ q
    R2 = yy - 2 * wq + w @ Gw
    nu = np.abs(q - Gw).max()
    if nu > l1:
        c = l1 / nu
        gp = (R2 + R2 * c * c) / 2
    else:
        c, gp = np.longdouble(1), R2
    gap = gp + l1 * np.abs(w).sum() - c * (yy - wq)
    eps = np.longdouble(np.finfo(np.float64).eps)
    budget = 8 * eps * (np.abs(yy) + 2 * np.abs(w * q).sum() + (np.abs(w) * np.abs(Gw)).sum())
    return gap, budget


def moments_oracle(X, W, V=None):
    """``G[p] = Σ_n W[p,n]·x_n x_nᵀ``, ``a[p] = Σ_n W[p,n]·x_n``, ``v[p] = Σ_n V[p,n]·x_n`` in
    longdouble, and the magnitudes Σ|W x_i x_j|, Σ|W x_f|, Σ|V x_f| that scale the (n + 2)·eps bound of
    an f64 sum of those terms in any order.  Returns ``(G, a, v, Gmag, amag, vmag)`` (v, vmag None
    without V)."""
    np = _np()
    X, W = _ld(X), _ld(W)
    aX, aW = np.abs(X), np.abs(W)
    G = np.stack([(X * W[p][:, None]).T @ X for p in range(W.shape[0])])
    Gmag = np.stack([(aX * aW[p][:, None]).T @ aX for p in range(W.shape[0])])
    a, amag = W @ X, aW @ aX
    if V is None:
        return G, a, None, Gmag, amag, None
    V = _ld(V)
    return G, a, V @ X, Gmag, amag, np.abs(V) @ aX


# ----------------------------------------------------------------------------- GBDT training oracles
# Written from the header of ops/csrc/gbdt.hip (what each kernel is documented to compute), in Python
# ``int``, ``fractions.Fraction`` and numpy longdouble.  Nothing here imports models/hist_gbdt.py, and
# the bagging hash is the Python-int ``_splitmix64_py`` above, not a tensor transcription.
GBDT_U = 2.0 ** -53             # f64 unit roundoff
GBDT_LEAF_EPS = 2.220446049250313e-16
# relative f64 error of the device's per-row deviance and w·r² expressions (exp, log1p, one division
# and a few products).  No ulp table of the device math library ships with the toolchain, so this is
# twice the largest per-row discrepancy measured on an MI355X against the longdouble oracle: one row per
# model, 8192 rows, the deviance at scale 2^48 on rows with |x| ≥ 1 and w·r² at 2^50 on rows with x ≥ ¼.
# No row was off by more than one fixed-point unit, which is 31.93u relative at the smallest such x —
# the resolution of the measurement, so an upper bound.  tests/test_gbdt_reference_gpu.py
# ::test_apply_prep_row_error_within_measured repeats the measurement and asserts it stays within
# GBDT_EPS_MEASURED.  At the scales the fit uses (2^26, 2^40) the ε term adds < 2^-6 unit per row to the
# 1 unit each row is granted, so the sums are in effect tested to ± one unit per row whatever ε is.
GBDT_EPS_MEASURED = 32 * GBDT_U
GBDT_EPS_F64 = 2 * GBDT_EPS_MEASURED


def gbdt_q(v, shift: int) -> int:
    """``rint_half_even(v · 2^shift)`` of a float taken exactly (``round`` of a Fraction is exact and
    rounds halves to even)."""
    from fractions import Fraction
    return round(Fraction(float(v)) * (1 << shift))


def gbdt_hist_oracle(bins, nbins, g, h, w, node, node0: int, NL: int, shift: int):
    """int64 ``[B, NL, F, 256, 3]``: for every row of model b with ``w > 0`` whose node lies in
    ``node0 .. node0+NL-1``, the exact fixed-point (g, h, w) added in Python ints to its bin of every
    feature.  ``bins`` [F, n] uint8, ``g``/``h``/``w`` [B, n] float32, ``node`` [B, n]."""
    np = _np()
    bins, g, h, w, node = (np.asarray(a) for a in (bins, g, h, w, node))
    B, n = g.shape
    F = bins.shape[0]
    H = [0] * (B * NL * F * 768)
    for b in range(B):
        for i in range(n):
            nd = int(node[b, i]) - node0
            if nd < 0 or nd >= NL or not w[b, i] > 0:
                continue
            q = (gbdt_q(g[b, i], shift), gbdt_q(h[b, i], shift), gbdt_q(w[b, i], shift))
            for f in range(F):
                k = (((b * NL + nd) * F + f) * 256 + int(bins[f, i])) * 3
                H[k] += q[0]
                H[k + 1] += q[1]
                H[k + 2] += q[2]
    assert max(abs(v) for v in H) < 1 << 63
    return np.array(H, dtype=np.int64).reshape(B, NL, F, 256, 3)


class GbdtSplit:
    """One node's exact split analysis (``gbdt_split_oracle``).

    ``kind``: 'empty' (Σw ≤ 0: the kernel writes feat = −3 and nothing else), 'leaf' or 'split'.
    ``cands``: {(f, j): (gain, err)} — exact proxy gain as a Fraction and the relative f64 error bound
    of the kernel's value of it.  ``best``: the exact maximiser after the tie rule.  ``decided``: no
    candidate outside best's identical-integer class (or tied with it at a gain of exactly 0, which
    the kernel computes exactly) comes within the two error bounds of it."""

    def certify(self, f: int, j: int):
        """None when the kernel's choice (f, j) is admissible, else the reason."""
        if (f, j) not in self.cands:
            return f"({f}, {j}) is not a candidate"
        gk, ek = self.cands[(f, j)]
        gb, eb = self.cands[self.best]
        if gk < gb * (1 - ek - eb):
            return f"gain({f}, {j}) = {float(gk):.17g} < best {self.best} {float(gb):.17g} beyond the f64 margin"
        if self.decided and (f, j) != self.best:
            return f"decided case: ({f}, {j}) chosen, exact best is {self.best}"
        return None


def gbdt_split_oracle(hist, nbins, lo_val, hi_val, r2: int, shift: int, min_leaf_q: int, min_split_q: int,
                      rank=None) -> GbdtSplit:
    """The split of one node from its integer histogram ``hist[f][bin] = (Σg, Σh, Σw)`` (fixed point,
    scale 2^shift), per the rule in gbdt.hip's header: node totals are feature 0's sums; a cut after
    bin j < nb−1 is a candidate when both sides carry ≥ ``min_leaf_q`` and the node ≥ ``min_split_q``;
    the best cut maximises the friedman_mse proxy ``(rw·lg − lw·rg)² / (lw·rw)``, ties to the lowest
    feature (lowest ``rank[f]`` when given), then the lowest bin; the node is a leaf without a candidate
    or when its impurity ``r2/tw − (tg/tw)²`` ≤ 2^-52.

    Error bound of the kernel's f64 gain ``(diff/dlw)·(diff/drw)`` (a product of two quotients, so the
    same bits when a mirrored cut swaps the sides), first order in u = 2^-53.  Each
    int64→f64 conversion is off by ≤ u, so a product of two converted integers is off by ≤ 3u of
    itself and ``diff = fl(fl(drw·dlg) − fl(dlw·drg))`` by ≤ 3u·(|rw·lg| + |lw·rg|) + u·|diff|, i.e.
    (3κ + 1)u relative with κ = (|rw·lg| + |lw·rg|) / |rw·lg − lw·rg|.  diff enters twice: 2(3κ + 1)u;
    the divisors dlw, drw carry u each; two divisions and one product round once each: 3u.  Sum:
    (6κ + 7)u.  A fused multiply-add removes a rounding and only lowers it.  With an exact diff = 0 and
    all four integers below 2^53 both products are the same real number, so the kernel's gain is
    exactly 0 (error 0); above 2^53 such a candidate is given an infinite bound."""
    from fractions import Fraction
    u = Fraction(1, 1 << 53)
    F = len(nbins)
    o = GbdtSplit()
    o.hist, o.nbins, o.lo_val, o.hi_val = hist, nbins, lo_val, hi_val
    nb0 = int(nbins[0])
    o.tg, o.th, o.tw = (sum(int(hist[0][j][s]) for j in range(nb0)) for s in range(3))
    o.cands, o.key, o.best, o.decided = {}, {}, None, True
    if o.tw <= 0:
        o.kind = "empty"
        return o
    o.imp = Fraction(int(r2), o.tw) - Fraction(o.tg, o.tw) ** 2
    if o.tw >= min_split_q:
        for f in range(F):
            lw = lg = 0
            for j in range(int(nbins[f]) - 1):
                lg += int(hist[f][j][0])
                lw += int(hist[f][j][2])
                rw, rg = o.tw - lw, o.tg - lg
                if lw < min_leaf_q or rw < min_leaf_q:
                    continue
                a, c = rw * lg, lw * rg
                if a != c:
                    err = (6 * Fraction(abs(a) + abs(c), abs(a - c)) + 7) * u
                elif max(abs(lw), abs(rw), abs(lg), abs(rg)) < 1 << 53:
                    err = Fraction(0)
                else:
                    err = Fraction(1 << 60)
                o.cands[(f, j)] = (Fraction((a - c) ** 2, lw * rw), err)
                o.key[(f, j)] = tuple(sorted([(lw, lg), (rw, rg)]))   # a mirrored cut swaps the sides
    if not o.cands or o.imp <= Fraction(GBDT_LEAF_EPS):
        o.kind = "leaf"
        return o
    o.kind = "split"
    rk = (lambda f: f) if rank is None else (lambda f: int(rank[f]))
    gmax = max(g for g, _ in o.cands.values())
    top = [k for k, (g, _) in o.cands.items() if g == gmax]
    o.best = min(top, key=lambda k: (rk(k[0]), k[1]))
    gb, eb = o.cands[o.best]
    for k, (g, e) in o.cands.items():
        if o.key[k] == o.key[o.best] or (g == gb and e == 0 and eb == 0):
            continue      # identical integers, or both gains an exact 0 in f64 too: the tie rule decides
        if not g < gb * (1 - e - eb):
            o.decided = False
    return o


def gbdt_split_children(o: GbdtSplit, f: int, j: int):
    """For the cut (f, j) of ``o``: ``(left, right, thr)`` — the children's (Σw, Σg, Σh) as ints and the
    f64 threshold: the midpoint ``a/2 + c/2`` of bin j's highest value ``a`` and the lowest value ``c`` of
    the next non-empty bin (the search stops at the last bin, empty or not); ``a`` when the midpoint
    equals ``c`` or overflows."""
    hf = o.hist[f]
    lg, lh, lw = (sum(int(hf[b][s]) for b in range(j + 1)) for s in range(3))
    hi = j + 1
    while hi < int(o.nbins[f]) - 1 and int(hf[hi][2]) == 0:
        hi += 1
    a, c = float(o.hi_val[f][j]), float(o.lo_val[f][hi])
    t = a / 2.0 + c / 2.0
    if t == c or math.isinf(t):
        t = a
    return (lw, lg, lh), (o.tw - lw, o.tg - lg, o.th - lh), t


def gbdt_bag_oracle(seed: int, stage: int, gidx: int, subsample: float) -> bool:
    """Row ``gidx`` (global index) is in stage ``stage``'s bag of the model with u64 ``seed`` iff the top
    24 bits of splitmix64(seed ⊕ splitmix64(stage·2^40 ⊕ gidx)) are below round(subsample·2^24)."""
    M = (1 << 64) - 1
    k = _splitmix64_py(((int(stage) << 40) ^ int(gidx)) & M)
    return (_splitmix64_py((int(seed) & M) ^ k) >> 40) < int(round(subsample * 16777216.0))


def gbdt_route_oracle(bins, node, feat, blo, node0: int, NL: int):
    """Rows whose node lies in ``node0 .. node0+NL-1`` and has ``feat ≥ 0`` move to child
    ``2·node + 1`` (``bins[feat] ≤ blo``) or ``2·node + 2``; every other row stays.  Returns the new
    [B, n] int64 nodes and the bool mask of moved rows."""
    np = _np()
    bins, node, feat, blo = (np.asarray(a) for a in (bins, node, feat, blo))
    B, n = node.shape
    new = node.astype(np.int64).copy()
    moved = np.zeros((B, n), dtype=bool)
    for b in range(B):
        for i in range(n):
            nd = int(node[b, i])
            if nd < node0 or nd >= node0 + NL or int(feat[b, nd]) < 0:
                continue
            new[b, i] = 2 * nd + (1 if int(bins[int(feat[b, nd]), i]) <= int(blo[b, nd]) else 2)
            moved[b, i] = True
    return new, moved


def gbdt_route_r2_oracle(g, w, new, moved, NN: int, shift: int):
    """[B, NN] Python-int child sums of ``rint(w·(g/w)²·2^shift)`` over the moved rows with w > 0 (exact
    for w ∈ {0, 1}, where r = g and g² is exact in f64)."""
    from fractions import Fraction
    np = _np()
    g, w = np.asarray(g), np.asarray(w)
    B, n = g.shape
    out = [[0] * NN for _ in range(B)]
    for b in range(B):
        for i in np.nonzero(moved[b] & (w[b] > 0))[0]:
            wi, gi = Fraction(float(w[b, i])), Fraction(float(g[b, i]))
            out[b][int(new[b, i])] += round(gi * gi / wi * (1 << shift))
    return out


def _f32_round_info(v):
    """float32 nearest to the longdouble ``v`` and its distance to the nearest f32 rounding boundary."""
    np = _np()
    f = v.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.longdouble)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.longdouble)
    fl = f.astype(np.longdouble)
    dist = np.minimum(np.abs(v - (fl + up) / 2), np.abs(v - (fl + dn) / 2))
    return f, dist, np.maximum(up - fl, fl - dn)


class GbdtPrep:
    """Outputs of ``gbdt_apply_prep_oracle`` (arrays [B, n] unless noted)."""


def gbdt_apply_prep_oracle(bins, y, w, raw, node, prev, lr: float, shift: int, dshift: int = 26,
                           subsample: float = 1.0, seeds=None, row_off: int = 0, stage: int = 0) -> GbdtPrep:
    """``gbdt_apply_prep`` in longdouble.  ``prev`` = (feat, blo, value) [B, NN] of the previous tree or
    None at stage 0.  With a previous tree: the pending last-level split routes each row, ``raw`` gains
    lr·value[leaf]; rows of the previous stage's bag add ``w·(y − σ(raw_before))²`` to their leaf's
    ``prev_r2`` and the binomial deviance ``−2w(y·raw − log(1 + e^raw))`` of the updated raw to ``dev``.
    Then g = w_t(y − p), h = w_t·p(1 − p) (float32) with this stage's in-bag weight w_t, and
    ``cur_r2`` = Σ w_t(y − p)².

    ``g_und`` / ``h_und`` mark rows whose longdouble value lies within 2^-50 relative of an f32 rounding
    boundary: there either neighbour is right.  One departure from a pure relative band: the f64
    expression ``y − p`` (and ``1 − p``) inherits the ABSOLUTE error of p, δp = 4u·p (exp, add, divide)
    + 2u·|raw|·p(1 − p) (the rounding of raw + lr·value carried through σ), which no f64 kernel can
    undercut.  Only on rows where δp exceeds the relative band — p next to 1 with y = 1, |raw| large —
    does δp replace it (and is added to the one-f32-ulp tolerance); every other row keeps 2^-50 and one
    ulp.  The fixed-point sums come as exact ints of the rounded longdouble terms with the budget
    Σ_rows (1 + ε·|x|·scale), ε = ``GBDT_EPS_F64``; at the scales in use the ε term is below 2^-6 per row,
    so the sums are in effect held to one unit per contributing row."""
    np = _np()
    ld = np.longdouble
    bins, y, w, node = np.asarray(bins), np.asarray(y), np.asarray(w), np.asarray(node)
    rawl = np.asarray(raw, dtype=np.float64).astype(ld)
    B, n = w.shape
    o = GbdtPrep()
    wl = w.astype(ld)
    wt, wp = wl.copy(), wl.copy()
    if subsample < 1.0:
        for b in range(B):
            for i in range(n):
                if not gbdt_bag_oracle(int(seeds[b]), stage, row_off + i, subsample):
                    wt[b, i] = 0
                if prev is None or not gbdt_bag_oracle(int(seeds[b]), stage - 1, row_off + i, subsample):
                    wp[b, i] = 0
    o.wt = wt.astype(np.float32)
    yl = y.astype(ld)[None, :]
    qs, ds = ld(2) ** shift, ld(2) ** dshift
    eps = ld(GBDT_EPS_F64)

    def fixed(x, scale, on):
        q = np.where(on, np.rint(x * scale), 0)
        bud = np.where(on, 1 + eps * np.abs(x) * scale, 0)
        return q.astype(np.int64), bud

    o.leaf = node.astype(np.int64)
    if prev is not None:
        feat, blo, value = (np.asarray(a) for a in prev)
        NN = feat.shape[1]
        o.leaf, _ = gbdt_route_oracle(bins, node, feat, blo, 0, NN)
        r0 = yl - _lm_sigmoid(rawl)
        q, bud = fixed(wp * r0 * r0, qs, wp > 0)
        o.prev_r2 = [[int(q[b][o.leaf[b] == k].sum()) for k in range(NN)] for b in range(B)]
        o.prev_r2_budget = [[float(bud[b][o.leaf[b] == k].sum()) for k in range(NN)] for b in range(B)]
        o.step = ld(lr) * np.take_along_axis(np.asarray(value, dtype=np.float64), o.leaf, 1).astype(ld)
        rawl = rawl + o.step
        q, bud = fixed(wp * -2 * (yl * rawl - _lm_softplus(rawl)), ds, wp > 0)
        o.dev = [int(q[b].sum()) for b in range(B)]
        o.dev_budget = [float(bud[b].sum()) for b in range(B)]
    o.raw = rawl
    p = _lm_sigmoid(rawl)
    r = yl - p
    # 1 − p without cancellation: σ(−raw)
    o.g, o.h = wt * r, wt * p * _lm_sigmoid(-rawl)
    u = ld(GBDT_U)
    dp = 4 * u * p + (2 * u * np.abs(rawl) * p * _lm_sigmoid(-rawl) if prev is not None else 0)
    for name, v in (("g", o.g), ("h", o.h)):
        f, dist, ulp = _f32_round_info(v)
        band = ld(2.0 ** -50) * np.abs(v)
        extra = np.where(dp > band, dp, 0)               # the saturated / cancelling rows only
        setattr(o, name + "32", f)
        setattr(o, name + "_und", (v != 0) & (dist <= np.maximum(band, extra)))   # w = 0: exactly 0
        setattr(o, name + "_tol", ulp + extra)
    q, bud = fixed(wt * r * r, qs, wt > 0)
    o.cur_r2 = [int(q[b].sum()) for b in range(B)]
    o.cur_r2_budget = [float(bud[b].sum()) for b in range(B)]
    return o


# ----------------------------------------------------------------------------- exact-SMO SVC oracles
# numpy and Python only, written from Fan, Chen and Lin (2005), libsvm's published Solver rules
# (select_working_set, the pair update, calculate_rho), Lin, Lin and Weng (2007) for the sigmoid fit
# and sklearn's documented gamma='scale'.  Like the working-set section above, nothing here imports
# torch or models/smo.py: the kernels of ops/csrc/svm.hip, svm_coop.hip and stackdev.hip's svm_gamma
# and the host mirrors in models/smo.py are all on the other side of every comparison.
SMO_U = 2.0 ** -53              # f64 unit roundoff
SMO_TAU = 1e-12                 # libsvm's TAU
SMO_VARIANTS = ("ties_first", "no_tau", "clip_swapped", "rho_ub", "stop_after_select")


def gram_kernel_error(Z32, ngl2e_f32):
    """``(K, dK)`` [l, l], longdouble: the RBF Gram ``K_ab = 2^(ngl2e·‖z_a − z_b‖²)`` of the f32 rows
    ``Z32`` with the scale read back from the stored f32 (it IS the scale, as in
    :func:`ws_kernel_error`), distances by direct differences in longdouble, and the forward bound
    of ``gram_rbf_kernel``'s f32 evaluation

        na = fma-chain ‖a‖², nb likewise;  dot = MFMA(a, b);
        d2 = max(fma(−2, dot, fl(na + nb)), 0);  K̂ = exp2(fl(ngl2e·d2)),  K̂_aa = 1.

    Term by term, with U = 2⁻²⁴, γ_n = nU/(1 − nU), mag = ‖a‖² + ‖b‖² + 2|a|·|b| (|a|·|b| the dot
    product of the absolute values) and g2 = −ngl2e:

    * the two norm chains: fma(z, z, s) over the padded width rounds once per step and the padding
      adds exact zeros, so each is off by ≤ γ_F·‖x‖²;
    * fl(na + nb): one rounding of a sum of two computed norms, ≤ U·(1 + γ_F)·(‖a‖² + ‖b‖²);
    * the dot product through v_mfma_f32_32x32x2_f32: two roundings per term (its product and its
      accumulation), in whatever order the unit takes them: ≤ γ_2F·|a|·|b|, doubled by the −2;
    * the final fma rounds once: ≤ U·|d̂2| ≤ U·(1 + γ_2F)·mag;
    * where nothing can round, nothing is budgeted: when the entries of both rows are integer
      multiples of a power of two q and mag < 2²⁴·q², every product and every partial sum, in any
      order, is a multiple of q² below 2²⁴·q², hence an f32: Δd2 = 0 for that pair (this is what
      lets the tests tell a scale that is off by one ulp from the kernel's);
    * the clamp at 0 only moves d̂2 towards the true d2 ≥ 0;
    * fl(ngl2e·d̂2): ≤ U·g2·(d2 + Δd2) in the exponent;
    * exp2 itself: K̂ = 2^(e + δ)·(1 + ε), |ε| ≤ EPS_EXP2, plus _TINY for a flushed result.

    So Δd2 = (γ_F + U(1 + γ_F))(‖a‖² + ‖b‖²) + 2γ_2F|a|·|b| + U(1 + γ_2F)·mag, the exponent is off by
    δ ≤ g2·Δd2 + U·g2·(d2 + Δd2), and dK = K·((2^δ − 1)(1 + EPS_EXP2) + EPS_EXP2) + _TINY.  With
    row norms near 1e3 and ‖a − b‖ = O(1), Δd2 is O(1) (cancellation), and dK legitimately reaches
    O(K).  The diagonal is forced: K_aa = 1, dK_aa = 0."""
    np = _np()
    L = np.longdouble
    Z = np.asarray(Z32, dtype=np.float32).astype(L)
    l, F = Z.shape
    e2 = L(np.float32(ngl2e_f32))
    g2 = -e2
    U = L(_U)
    gF, g2F = F * U / (1 - F * U), 2 * F * U / (1 - 2 * F * U)
    nrm = (Z * Z).sum(1)
    aZ = np.abs(Z)
    # the lowest set bit of each row's entries: the row's values are integer multiples of quant
    mant, ex = np.frexp(np.asarray(Z32, dtype=np.float32).astype(np.float64))
    mi = np.round(mant * 2.0 ** 24).astype(np.int64)
    low = np.where(mi != 0, ex - 24 + np.log2((mi & -mi).astype(np.float64) + (mi == 0)), 0.0)
    quant = np.exp2(np.where(mi != 0, low, np.inf).min(1, initial=126.0))
    K = np.empty((l, l), dtype=L)
    dK = np.empty((l, l), dtype=L)
    step = max(1, (1 << 20) // max(1, l * F))
    ln2 = np.log(L(2))
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for s in range(0, l, step):
            diff = Z[s:s + step, None, :] - Z[None, :, :]
            d2 = (diff * diff).sum(-1)
            cross = aZ[s:s + step] @ aZ.T
            nn = nrm[s:s + step, None] + nrm[None, :]
            dd2 = (gF + U * (1 + gF)) * nn + 2 * g2F * cross + U * (1 + g2F) * (nn + 2 * cross)
            qq = np.minimum(quant[s:s + step, None], quant[None, :]) ** 2
            dd2 = np.where(nn + 2 * cross < qq * 2.0 ** 24, 0, dd2)
            de = g2 * dd2 + U * g2 * (d2 + dd2)
            k = np.exp2(e2 * d2)
            x = np.expm1(ln2 * de)
            K[s:s + step] = k
            dK[s:s + step] = np.where(k > 0, k * (x * (1 + L(EPS_EXP2)) + L(EPS_EXP2)), 0) + L(_TINY)
    ix = np.arange(l)
    K[ix, ix] = 1
    dK[ix, ix] = 0
    return K, dK


def gram_inside(Khat, K, dK):
    """Entries of a computed Gram that :func:`gram_kernel_error` admits: within dK of K, and at most
    1 (the clamp makes the exponent non-positive, and exp2 of a non-positive f32 never exceeds 1)."""
    np = _np()
    Kh = np.asarray(Khat).astype(np.longdouble)
    return (np.abs(Kh - K) <= dK) & (Kh <= 1)


class SmoResult:
    """What :func:`smo_oracle` returns: ``alpha`` [l] f64, ``rho``, ``iters`` (pair updates made),
    ``pairs`` (the (i, j) of every update, in order), ``gap`` (the last m − M the stop rule saw),
    ``G`` (the incrementally updated gradient, f64) and ``drift`` [l] (forward bound of G − (Qα − 1))."""
    __slots__ = ("alpha", "rho", "iters", "pairs", "gap", "G", "drift")

    def __iter__(self):
        return iter((self.alpha, self.rho, self.iters, self.pairs, self.drift))


def smo_oracle(K, npos, Cp, Cn, eps, max_iter, variant=None):
    """libsvm's Solver::Solve for C-SVC without shrinking, on the stored kernel matrix ``K``
    (rounded to f32 here: libsvm keeps Q as float), the first ``npos`` points y = +1.

    Plain float64, one IEEE operation at a time in libsvm's operation order (numpy's elementwise
    multiply and add are separate roundings: no fused operation anywhere):

    * start: α = 0, G = −1;
    * first selection: i = argmax over I_up of −y_t G_t, ``>=`` so ties go to the LAST index;
    * second selection over t ∈ I_low with b = Gmax + y_t G_t > 0: a = QD_i + QD_t − 2·K_it (QD the
      diagonal; a ≤ 0 → τ = 1e-12), minimise −b²/a, ``<=`` so ties go to the LAST index.  Gmax2 =
      max over I_low of y_t G_t is taken in the same sweep, over every member of I_low;
    * stop rule: m − M = Gmax + Gmax2 < eps, or no candidate t.  It depends on the two maxima only,
      not on the chosen t: it is tested before the second choice is used;
    * the pair update with its four clipping cases (y_i ≠ y_j: δ = (−G_i − G_j)/a with a = QD_i +
      QD_j + 2Q_ij; y_i = y_j: δ = (G_i − G_j)/a with a = QD_i + QD_j − 2Q_ij; a ≤ 0 → τ);
    * G_t += Q_it·Δα_i + Q_jt·Δα_j with Q_it = y_i y_t K_it (a sign flip, exact);
    * ``calculate_rho``: the index-ordered sum of y G over the free points divided by their count,
      else (ub + lb)/2 (:func:`svc_kkt`'s sets).

    ``drift``: G is updated incrementally, Qα − 1 (Q the stored f32 entries, α the returned one)
    is what it stands for.  One update computes pa = fl(Q_it·Δα_i), pb = fl(Q_jt·Δα_j), s = fl(pa +
    pb), G' = fl(G + s) with Δα = fl(α_new − α_old): five roundings, each ≤ 2⁻⁵³ times the computed
    magnitude, so the update moves G_t away from the exact sum by at most
    2⁻⁵³·(2|pa| + 2|pb| + |s| + |G'|)·(1 + 2⁻⁵⁰), and the drift is the sum of that over the replayed
    updates (the exact increments telescope to the returned α).

    ``variant``: one of ``SMO_VARIANTS``, a deliberately WRONG rule, for the tests that show the
    comparison with libsvm notices each of them: first-index ties, no τ floor, a swapped clipping
    case (the y_i ≠ y_j upper clip compares with C_j − C_i), ρ = ub with no free vector, and the
    stop rule evaluated on the selected second index instead of on Gmax2."""
    np = _np()
    assert variant is None or variant in SMO_VARIANTS, variant
    K32 = np.asarray(K, dtype=np.float32)
    l = K32.shape[0]
    pos, y, C = _ws_labels(l, npos, Cp, Cn)
    QD = np.diagonal(K32).astype(np.float64)
    G = -np.ones(l)
    alpha = np.zeros(l)
    drift = np.zeros(l)
    pairs = []
    gap = 0.0
    last = variant != "ties_first"
    floor = variant != "no_tau"
    ninf = -np.inf

    def pick(v, best):
        w = np.flatnonzero(v == best)
        return int(w[-1] if last else w[0])

    it = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while it < max_iter:
            up = np.where(pos, alpha < C, alpha > 0)
            if not up.any():
                break
            yG = np.where(pos, G, -G)
            v = np.where(up, -yG, ninf)
            Gmax = v.max()
            i = pick(v, Gmax)
            Ki = K32[i].astype(np.float64)
            low = np.where(pos, alpha > 0, alpha < C)
            Gmax2 = yG[low].max() if low.any() else ninf
            b = Gmax + yG
            cand = low & (b > 0)
            a = (QD[i] + QD) - 2.0 * Ki
            if floor:
                a = np.where(a <= 0, SMO_TAU, a)
            obj = np.where(cand, -(b * b) / a, np.inf)
            j = pick(obj, obj[cand].min()) if cand.any() else -1
            gap = Gmax + Gmax2
            if variant == "stop_after_select":
                if j < 0 or Gmax + yG[j] < eps:
                    break
            elif gap < eps or j < 0:
                break
            yi, yj = y[i], y[j]
            Ci, Cj = C[i], C[j]
            Qij = yi * yj * float(K32[i, j])
            ai_old, aj_old = alpha[i], alpha[j]
            ai, aj = ai_old, aj_old
            if yi != yj:
                a2 = (QD[i] + QD[j]) + 2.0 * Qij
                if a2 <= 0 and floor:
                    a2 = SMO_TAU
                delta = (-G[i] - G[j]) / a2
                diff = ai - aj
                ai += delta
                aj += delta
                if diff > 0:
                    if aj < 0:
                        aj, ai = 0.0, diff
                else:
                    if ai < 0:
                        ai, aj = 0.0, -diff
                if diff > (Cj - Ci if variant == "clip_swapped" else Ci - Cj):
                    if ai > Ci:
                        ai, aj = Ci, Ci - diff
                else:
                    if aj > Cj:
                        aj, ai = Cj, Cj + diff
            else:
                a2 = (QD[i] + QD[j]) - 2.0 * Qij
                if a2 <= 0 and floor:
                    a2 = SMO_TAU
                delta = (G[i] - G[j]) / a2
                sm = ai + aj
                ai -= delta
                aj += delta
                if sm > Ci:
                    if ai > Ci:
                        ai, aj = Ci, sm - Ci
                else:
                    if aj < 0:
                        aj, ai = 0.0, sm
                if sm > Cj:
                    if aj > Cj:
                        aj, ai = Cj, sm - Cj
                else:
                    if ai < 0:
                        ai, aj = 0.0, sm
            dai, daj = ai - ai_old, aj - aj_old
            pa = ((yi * y) * Ki) * dai
            pb = ((yj * y) * K32[j].astype(np.float64)) * daj
            s = pa + pb
            G = G + s
            drift += SMO_U * (1 + 2.0 ** -50) * (2 * np.abs(pa) + 2 * np.abs(pb) + np.abs(s) + np.abs(G))
            alpha[i], alpha[j] = ai, aj
            pairs.append((i, j))
            it += 1
            if not (np.isfinite(ai) and np.isfinite(aj)):      # only a wrong variant gets here
                break
    out = SmoResult()
    kkt = svc_kkt(alpha, G, npos, Cp, Cn)
    free = (alpha > 0) & (alpha < C)
    yG = np.where(pos, G, -G)
    if free.any():
        rho = float(np.cumsum(yG[free])[-1] / int(free.sum()))      # libsvm's index-ordered sum
    elif variant == "rho_ub":
        ubm = np.where(pos, alpha <= 0, alpha >= C)
        rho = float(yG[ubm].min()) if ubm.any() else np.inf
    else:
        rho = float(kkt["rho"])
    out.alpha, out.rho, out.iters, out.pairs, out.gap, out.G, out.drift = alpha, rho, it, pairs, float(gap), G, drift
    return out


# f64 must also DETERMINE each Newton direction: the determinant h11·h22 − h21² of sums of n (or
# ``depth``) terms is known to (n + 8)·2⁻⁵³·(h11·h22 + h21²) at best, so the direction carries that over
# |det| as a relative error.  Runs where it exceeds 2⁻²⁰ are undecided: with a Hessian that is singular
# up to the 1e-12 ridge (a constant decision value) the ratio is of order 1e-2, and f64 and longdouble
# runs that take the same branches still end percent apart; on regular inputs it is below 1e-11.
PLATT_DIRECTION_MAX = 2.0 ** -20


class PlattResult:
    """What :func:`platt_oracle` returns.  ``A, B``: the fit; ``iters``: Newton iterations made;
    ``capped``: the run ended at the iteration cap or at the minimum step instead of the stop rule;
    ``margin``: the smallest |f_trial − (f + 1e-4·step·∇·d)| over every backtracking test of the run
    (inf when none was made); ``stop_margin``: the smallest | max|∇| − 1e-5 | over the stop tests;
    ``direction``: the largest relative error f64 leaves in a Newton direction (see
    ``PLATT_DIRECTION_MAX``); ``decided``: every such test lies further from its threshold than
    the f64 evaluation error there (:meth:`evaluate`'s bounds) and every direction is determined,
    so an f64 implementation takes the same branches through the same iterates."""

    def __init__(self, dec, labels, T, depth=None):
        np = _np()
        self.T = T
        self.depth = depth
        self.d = np.asarray(dec, dtype=np.float64).astype(T)
        lab = np.asarray(labels)
        n1 = int((lab > 0).sum())
        n0 = int(lab.size - n1)
        self.n1, self.n0 = n1, n0
        self.t = np.where(lab > 0, (T(n1) + 1) / (T(n1) + 2), 1 / (T(n0) + 2)).astype(T)

    def evaluate(self, A, B):
        """``(f, g1, g2, df, dg)`` at (A, B) in the oracle's float type: the objective
        Σ t·z + log(1 + e^−z) (z = A·d + B, the overflow-free form of either sign), its gradient
        (Σ d·(t − p), Σ (t − p)), and the bounds of an f64 evaluation of them in ANY summation order:
        with u = 2⁻⁵³ and n points, a sum of n terms is off by ≤ γ_n·Σ|term| (γ_n = nu/(1 − nu); with
        ``depth`` given, n is the depth of the summation tree instead — no term passes through more
        additions than that: platt_kernel adds ≤ 16 values per thread, 6 wave levels and 16 wave
        totals, platt_coop_kernel 8 workgroup totals more, numpy's pairwise sum fewer); each
        term carries ≤ 8 further roundings (the product and sum of z, exp, log, the divisions: a
        few ulp each, counted as 8u·|term|), and z's own error 2u(|A·d| + |B|) enters f through
        |∂term/∂z| = |t − p| ≤ 1 and the gradient through p(1 − p) ≤ ¼:
        df = u(n + 8)·Σ|term| + 2u·Σ(|A·d| + |B|) + u·N,  dg = u(n + 8)·Σ|d|·|t − p| + ½u·Σ|d|(|A·d| + |B|)
        + 4u·Σ|d|·p (for g1; g2 is the same with |d| = 1, and dg is the larger of the two).  The last
        term of each is absolute, one per point (N points): libsvm and the kernels evaluate
        log(1 + e) and e/(1 + e), not log1p, and rounding 1 + e costs up to u absolutely in the log
        whatever the size of the term (a well-classified negative's term is ≈ t₋·z, far below 1), and
        a few u relative to p — not to t − p — in the gradient."""
        np = _np()
        T = self.T
        A, B = T(A), T(B)
        z = self.d * A + B
        with np.errstate(over="ignore", under="ignore"):
            e = np.exp(-np.abs(z))
            lg = np.log1p(e)
            terms = np.where(z >= 0, self.t * z, (self.t - 1) * z) + lg
            p = np.where(z >= 0, e / (1 + e), 1 / (1 + e))
        d1 = self.t - p
        f, g1, g2 = terms.sum(), (self.d * d1).sum(), d1.sum()
        n = self.d.size if self.depth is None else min(self.d.size, int(self.depth))
        u = T(SMO_U)
        zmag = np.abs(self.d * A) + abs(B)
        absterm = np.abs(np.where(z >= 0, self.t * z, (self.t - 1) * z)) + lg
        npts = self.d.size
        df = u * (n + 8) * absterm.sum() + 2 * u * zmag.sum() + u * npts
        ad = np.abs(self.d)
        dg1 = u * (n + 8) * (ad * np.abs(d1)).sum() + u / 2 * (ad * zmag).sum() + 4 * u * (ad * p).sum()
        dg2 = u * (n + 8) * np.abs(d1).sum() + u / 2 * zmag.sum() + 4 * u * p.sum()
        return f, g1, g2, df, max(dg1, dg2)

    def _hessian(self, A, B):
        np = _np()
        z = self.d * self.T(A) + self.T(B)
        with np.errstate(over="ignore", under="ignore"):
            e = np.exp(-np.abs(z))
        pq = (e / (1 + e)) * (1 / (1 + e))
        return (self.d * self.d * pq).sum(), pq.sum(), (self.d * pq).sum()


def platt_oracle(dec, labels, dtype=None, depth=None):
    """Platt's sigmoid fit by Lin, Lin and Weng's (2007) algorithm, as libsvm's ``sigmoid_train``
    states it: targets t₊ = (N₊ + 1)/(N₊ + 2), t₋ = 1/(N₋ + 2); start A = 0, B = log((N₋ + 1)/(N₊ + 1));
    Newton direction from the Hessian with a 1e-12 ridge on its diagonal; stop when both |∂/∂A| and
    |∂/∂B| are below 1e-5; backtracking from step 1 by halving while step ≥ 1e-10, accepting when
    f_trial < f + 1e-4·step·(∇·d); at most 100 iterations.  Everything in ``dtype`` (longdouble by
    default; float64 runs the same code for the reference-against-reference margin of the tests;
    ``depth``: see :meth:`PlattResult.evaluate`).
    Returns a :class:`PlattResult` (``A``, ``B``, ``evaluate``, ``margin``, ``decided`` …)."""
    np = _np()
    T = np.longdouble if dtype is None else dtype
    r = PlattResult(dec, labels, T, depth)
    A, B = T(0), np.log((T(r.n0) + 1) / (T(r.n1) + 1))
    f, g1, g2, df, dg = r.evaluate(A, B)
    margin, stop_margin, decided = T(np.inf), T(np.inf), True
    capped, it, direction = True, 0, T(0)
    sigma, eps, min_step = T(1e-12), T(1e-5), T(1e-10)
    for it in range(100):
        for g in (g1, g2):
            stop_margin = min(stop_margin, abs(abs(g) - eps))
            decided = decided and abs(abs(g) - eps) > dg
        if abs(g1) < eps and abs(g2) < eps:
            capped = False
            break
        h11, h22, h21 = r._hessian(A, B)
        h11, h22 = h11 + sigma, h22 + sigma
        det = h11 * h22 - h21 * h21
        nd = r.d.size if depth is None else min(r.d.size, int(depth))
        direction = max(direction, (nd + 8) * T(SMO_U) * (h11 * h22 + h21 * h21) / abs(det))
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = T(1)
        while step >= min_step:
            nA, nB = A + step * dA, B + step * dB
            nf, ng1, ng2, ndf, ndg = r.evaluate(nA, nB)
            thr = f + T(0.0001) * step * gd
            m = abs(nf - thr)
            margin = min(margin, m)
            decided = decided and m > ndf + df + 4 * T(SMO_U) * abs(thr)
            if nf < thr:
                A, B, f, g1, g2, df, dg = nA, nB, nf, ng1, ng2, ndf, ndg
                break
            step = step / 2
        if step < min_step:
            break
    else:
        it = 100
    r.A, r.B, r.iters, r.capped = A, B, it, capped
    r.margin, r.stop_margin, r.direction = margin, stop_margin, direction
    r.decided = bool(decided and direction <= PLATT_DIRECTION_MAX)
    return r


def gamma_oracle(Z, offs, F):
    """sklearn's ``gamma='scale'`` = 1/(F·Var(Z)) for every fit f over the rows offs[f] … offs[f+1] of
    ``Z`` [rows, F], in longdouble: the population variance in two passes (the mean, then the mean
    of the squared deviations), γ = 1 where the variance is exactly 0 (sklearn's rule), NaN where
    a value is not finite.  Returns ``(gamma [K] longdouble, ngl2e [K] f32)`` with
    ngl2e = f32(−γ·log2 e)."""
    np = _np()
    L = np.longdouble
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, F).astype(L)
    offs = np.asarray(offs, dtype=np.int64)
    g = np.empty(offs.size - 1, dtype=L)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for f in range(offs.size - 1):
            z = Z[offs[f]:offs[f + 1]].ravel()
            if z.size == 0:
                g[f] = 1
                continue
            mean = z.sum() / z.size
            d = z - mean
            var = (d * d).sum() / z.size
            g[f] = 1 / (F * var) if var != 0 else 1
            if not np.isfinite(z).all():
                g[f] = np.nan
        ngl2e = (-g * np.log2(np.exp(L(1)))).astype(np.float32)
    return g, ngl2e


# ----------------------------------------------------------------------------- Nyström interior-point SVC oracles
# numpy only, written from the headers of ops/csrc/lowrank.hip, linalg.hip and nystrom.hip (what each
# kernel is documented to compute), from Higham, "Accuracy and Stability of Numerical Algorithms"
# (2002; §3.1 sums in any order, Theorem 10.3 Cholesky, Theorem 8.5 substitution) and from the C-SVC
# dual itself.  longdouble where a value is compared, plain f64 in the kernel's own operation order
# where bits are compared.  Nothing here imports torch.linalg or models/svc_lowrank.py.
#
# Notation: u = 2⁻⁵³ (LR_U), γ_k = k·u/(1 − k·u) (lr_gamma); γ32_k the same with 2⁻²⁴.  Every bound is
# per entry and relative to the magnitude of that entry's own terms, so one wrong small entry cannot
# hide behind a large one.
LR_U = 2.0 ** -53
LR_U32 = 2.0 ** -24
LR_WF_FLUSH = 256               # lowrank.hip kWfFlush: rows per f32 accumulation of wsyrk_f32
LR_EXP_ULP = 2                  # assumed error of the device's double exp, in ulp (profiles/lowrank_oracles.md)
LR_JIT0 = 1e-14                 # linalg.hip: the jitter ladder 1e-14, ×100 per retry, up to 1
LR_IPM_TOL = 1e-8               # models/svc_lowrank.py IPM_TOL (gap) and the tight residual / equality rule
LR_RD_LOOSE = 1e-5              # models/svc_lowrank.py RD_LOOSE
LR_SNAP = 1e-9                  # the final snap of α onto a bound it is within 1e-9·c of


def lr_gamma(k, u=LR_U):
    """γ_k = k·u/(1 − k·u), longdouble."""
    L = _np().longdouble
    return L(k) * L(u) / (1 - L(k) * L(u))


def wgram_oracle(Phi, d):
    """``(S, M)`` longdouble [r, r]: S = Φᵀ diag(d) Φ and M = |Φ|ᵀ diag(|d|) |Φ|.

    f64 kernels (wsyrk_f64, wsyrk_f64x): each term is fl(d_i·φ_ij)·φ_ik — one rounding — entering an
    fma accumulation (no product rounding); the n terms of an entry are then summed in SOME order
    (16- or 32-row slabs, 4 rows per MFMA, row groups, the group-order reduction), and a sum of n
    terms in any order puts at most n − 1 roundings on a term (Higham §3.1).  So
    |Ŝ − S| ≤ γ_{n+2}·M (:func:`wgram_bound_f64`; n + 2 ≥ 1 + (n − 1), the slack is Higham's)."""
    np = _np()
    P, dd = _ld(Phi), _ld(d)
    # (row-major transposes: numpy's longdouble product is a plain loop, fastest over contiguous rows)
    Pt = np.ascontiguousarray(P.T)
    S = np.ascontiguousarray((P * dd[:, None]).T) @ Pt.T
    aPt = np.abs(Pt)
    M = (aPt * np.abs(dd)[None, :]) @ aPt.T
    return S, M


def wgram_bound_f64(M, n):
    return lr_gamma(n + 2) * M


def wgram_bound_f32(M, n):
    """wsyrk_f32's bound from its own arithmetic.  Φ is exactly f32.  A term d_i·φ_ij is formed in
    f64 (u) and rounded to f32 (2⁻²⁴); its product with the exact φ_ik and the f32 accumulation over
    at most F = min(n, kWfFlush) rows put at most 1 + (F − 1) more f32 roundings on it, so within a
    flush (1 + 2⁻²⁴)^(F+1) ≤ 1 + γ32_{F+2} covers them together with the f64 rounding of d·φ.  The
    flushed f32 sums are exact in f64 and are added in f64: ⌈n/F⌉ flushes over the row groups plus
    the group-order reduction, at most n − 1 f64 additions on a term.  Hence

        |Ŝ − S| ≤ ((1 + γ32_{F+2})·(1 + γ_{n+2}) − 1)·M,   F = min(n, 256):

    1.5e-5·M at n ≥ 256 and 1.8e-7·M at n = 1 (f32 range assumed: no term under- or overflows)."""
    F = min(int(n), LR_WF_FLUSH)
    return ((1 + lr_gamma(F + 2, LR_U32)) * (1 + lr_gamma(n + 2)) - 1) * M


def phi_mv_oracle(Phi, W):
    """``(Y, Ymag)`` longdouble [n, k]: Y = Φ W and |Φ||W|.  phi_gemv / phi_gemv_f32 sum r fma terms
    in some order (8 per lane, then a wave sum): |Ŷ − Y| ≤ γ_{r+1}·Ymag."""
    np = _np()
    P, Wl = _ld(Phi), _ld(W)
    return P @ Wl, np.abs(P) @ np.abs(Wl)


def phit_oracle(Phi, V):
    """``(O, Omag)`` longdouble [r, k]: O = Φᵀ V and |Φ|ᵀ|V|.  phit_f32 sums n fma terms in some order
    (per thread, per workgroup in LDS, the slot-order reduction): |Ô − O| ≤ γ_{n+1}·Omag."""
    np = _np()
    P, Vl = _ld(Phi), _ld(V)
    return P.T @ Vl, np.abs(P).T @ np.abs(Vl)


def rbf_oracle_f64(A, B, gamma):
    """``(K, dK)`` longdouble [l, m]: K = exp(−γ‖a − b‖²) with d² summed from the differences, and the
    forward bound of rbf_f64's evaluation  t = fl(a_f − b_f); d̂ = fma(t, t, d̂) over f < F;
    K̂ = exp(fl(−γ·d̂)).

    * every t carries one rounding (twice in t²) and the F-step fma chain at most F more on a term:
      d̂ = d²(1 + θ), |θ| ≤ γ_{F+2} (all terms non-negative: no cancellation);
    * fl(−γ·d̂) rounds once more: the exponent is off by δ ≤ γ_{F+2}·γd² + u·γd²(1 + γ_{F+2});
    * exp itself: K̂ = e^x̂(1 + ε), |ε| ≤ E = LR_EXP_ULP·2u (one ulp is at most 2u of the value);
    * a result below the normal range is a subnormal or a flushed 0: 2⁻¹⁰²² absolute there.

    dK = K·((e^δ − 1)(1 + E) + E)  (+ 2⁻¹⁰²² where K < 2⁻¹⁰²¹)."""
    np = _np()
    L = np.longdouble
    A, B = _ld(A), _ld(B)
    F = A.shape[1]
    g = L(gamma)
    d2 = np.zeros((A.shape[0], B.shape[0]), dtype=L)
    for f in range(F):
        t = A[:, f][:, None] - B[:, f][None, :]
        d2 += t * t
    gF = lr_gamma(F + 2)
    with np.errstate(under="ignore"):
        K = np.exp(-g * d2)
        delta = gF * g * d2 + L(LR_U) * g * d2 * (1 + gF)
        E = L(LR_EXP_ULP) * 2 * L(LR_U)
        dK = K * (np.expm1(delta) * (1 + E) + E)
    dK = dK + np.where(K < L(2.0) ** -1021, L(2.0) ** -1022, 0)
    return K, dK


class Certificate:
    """A certificate's verdict: ``ok``, ``why`` (the conditions that failed) and ``worst`` (per
    condition, the largest observed error as a fraction of its bound; ≤ 1 passes)."""
    __slots__ = ("ok", "why", "worst", "extra")

    def __init__(self):
        self.ok, self.why, self.worst, self.extra = True, [], {}, {}

    def check(self, name, err, bound):
        """``err ≤ bound`` everywhere (arrays or scalars; a NaN fails)."""
        np = _np()
        err, bound = np.asarray(err, dtype=np.longdouble), np.asarray(bound, dtype=np.longdouble)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0, err / bound)
        w = float(np.max(ratio)) if ratio.size else 0.0
        self.worst[name] = w
        if not (np.all(err <= bound) and np.isfinite(err).all()):
            self.fail(name)

    def fail(self, name):
        self.ok = False
        self.why.append(name)

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return f"Certificate(ok={self.ok}, why={self.why}, worst={self.worst})"


def entries_within(name, got, want, bound, cert=None):
    """|got − want| ≤ bound per entry, as a :class:`Certificate` (got f64, want / bound longdouble)."""
    np = _np()
    cert = cert or Certificate()
    cert.check(name, np.abs(_ld(got) - want), bound)
    return cert


def chol_jitter(info):
    """The diagonal shift of retry ``info`` of linalg.hip's ladder: 0, then 1e-14·100^(info − 1),
    formed as the kernel forms it (×100.0 in f64 per retry)."""
    if info <= 0:
        return 0.0
    j = LR_JIT0
    for _ in range(int(info) - 1):
        j = j * 100.0
    return j


def chol_certificate(S, L, sc, info):
    """Higham's certificate of chol_spd / chol_spd_mw, in longdouble, from the outputs alone:

    * ``sc``: sc_i = diag(S)_i^-½ to one ulp.  The kernel takes a square root and a reciprocal,
      each correctly rounded: (1 + u)/(1 − u) − 1 ≤ γ_2 = 2⁻⁵²(1 + …), one ulp at the low end of a
      binade, which is what is required (sc_i = 1 where S_ii ≤ 0);
    * ``factor``: |L Lᵀ − (sc·S·sc + jit(info)·I)| ≤ γ_{r+1}·|L||Lᵀ| per entry (Theorem 10.3), with the
      kernel's own sc and :func:`chol_jitter`;
    * ``diag``: L_ii > 0;  ``upper``: the strict upper triangle is exactly 0;  ``info``: 0 ≤ info ≤ 8."""
    np = _np()
    Ll = np.longdouble
    cert = Certificate()
    S0, L0 = np.asarray(S, dtype=np.float64), np.asarray(L, dtype=np.float64)
    r = S0.shape[0]
    Sl, Lf, scl = _ld(S0), _ld(L0), _ld(sc)
    if not (0 <= int(info) <= 8):
        cert.fail("info")
        return cert
    dg = np.diagonal(Sl)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(dg > 0, 1 / np.sqrt(np.where(dg > 0, dg, 1)), Ll(1))
    cert.check("sc", np.abs(scl - want), lr_gamma(2) * np.abs(want))
    T = Sl * scl[:, None] * scl[None, :] + Ll(chol_jitter(info)) * np.eye(r, dtype=Ll)
    # the lower triangle (the part of S the kernel reads), the products taken over column blocks of the
    # lower-triangular factor: a third of the full product's work, the same sums
    Lt = np.tril(Lf)
    LLt, mag = np.zeros((r, r), dtype=Ll), np.zeros((r, r), dtype=Ll)
    for k0 in range(0, r, 64):
        blk = Lt[k0:, k0:k0 + 64]
        LLt[k0:, k0:] += blk @ blk.T
        mag[k0:, k0:] += np.abs(blk) @ np.abs(blk).T
    low = np.tril(np.ones((r, r), dtype=bool))
    cert.check("factor", np.abs(LLt - T)[low], (lr_gamma(r + 1) * mag)[low])
    if not (np.diagonal(L0) > 0).all():
        cert.fail("diag")
    if np.triu(L0, 1).any() or np.isnan(L0).any():
        cert.fail("upper")
    return cert


def chol_solve_certificate(L, sc, B, X):
    """Componentwise backward error of chol_solve's two substitutions, per right-hand side: with
    Y = X/sc,  |(L Lᵀ)Y − sc·B| ≤ γ_{3r+1}·|L||Lᵀ||Y|  per entry (Theorem 8.5 twice: (L + ΔL)(L + ΔL')ᵀ
    with |ΔL| ≤ γ_r|L| gives 2γ_r + γ_r² ≤ γ_{2r+1}; the remaining r cover the two scalings by sc and
    the reciprocal pivots)."""
    np = _np()
    cert = Certificate()
    Lf, scl, Bl, Xl = _ld(L), _ld(sc), _ld(B), _ld(X)
    r = Lf.shape[0]
    Y = Xl / scl[:, None]
    res = np.abs(Lf @ (Lf.T @ Y) - scl[:, None] * Bl)
    bound = lr_gamma(3 * r + 1) * (np.abs(Lf) @ (np.abs(Lf).T @ np.abs(Y)))
    for q in range(Bl.shape[1]):
        cert.check(f"rhs{q}", res[:, q], bound[:, q])
    return cert


class ipm_rows_oracle:
    """One plain numpy f64 function per row kernel of lowrank.hip: the operations and their
    parenthesisation are the kernel comments' (numpy neither contracts nor reorders), so outputs
    are compared bit for bit.  Vectors are f64 [n]; device scalars are Python floats; ``Mh`` / ``My``
    / ``P`` are the already strided columns."""

    @staticmethod
    def resid(c, a, y, P, b, nu, mu):
        """s = c − α,  rd = ((y·P − 1) + b·y − ν) + μ."""
        g = y * P - 1.0
        return c - a, ((g + b * y) - nu) + mu

    @staticmethod
    def pred(a, s, nu, mu, rd, y):
        """D⁻¹ = 1/(ν/α + μ/s), its two-column copy, rν = α·ν, rμ = s·μ, H2 = [((−rd) − rν/α) + rμ/s, y]."""
        np = _np()
        di = 1.0 / (nu / a + mu / s)
        rn, rm = a * nu, s * mu
        h = (-rd - rn / a) + rm / s
        return di, np.stack([di, di], 1), rn, rm, np.stack([h, y], 1)

    @staticmethod
    def corr(a, s, nu, mu, da, dnu, dmu, rd, tau):
        """rν = (α·ν + Δα·Δν) − τ,  rμ = (s·μ − Δα·Δμ) − τ,  h = ((−rd) − rν/α) + rμ/s."""
        rn = (a * nu + da * dnu) - tau
        rm = (s * mu - da * dmu) - tau
        return rn, rm, (-rd - rn / a) + rm / s

    @staticmethod
    def dirs(Mh, My, db, rnu, rmu, nu, mu, a, s):
        """Δα = Mh − db·My,  Δν = (−rν − ν·Δα)/α,  Δμ = (−rμ + μ·Δα)/s."""
        d = Mh - db * My
        return d, (-rnu - nu * d) / a, (-rmu + mu * d) / s

    @staticmethod
    def minv_pre(Dinv, y, U):
        """du = D⁻¹ ∘ U,  V = y ∘ du  (U [n, k])."""
        du = Dinv[:, None] * U
        return du, y[:, None] * du

    @staticmethod
    def minv_post(Dinv, y, du, P):
        """out = du − D⁻¹ ∘ (y ∘ P)."""
        return du - Dinv[:, None] * (y[:, None] * P)

    @staticmethod
    def update(a, nu, mu, da, dnu, dmu, t):
        return a + t * da, nu + t * dnu, mu + t * dmu

    @staticmethod
    def gondzio_rhs(a, s, nu, mu, da, dnu, dmu, alpha, tau):
        """α̃ = min(1.5α + 0.1, 1); the trial products pushed into [0.1τ, 10τ], floored at −10τ."""
        np = _np()
        at = min(1.5 * alpha + 0.1, 1.0)
        lo, hi = 0.1 * tau, 10.0 * tau
        va = (a + at * da) * (nu + at * dnu)
        vs = (s - at * da) * (mu + at * dmu)
        tca = np.maximum(np.minimum(np.maximum(va, lo), hi) - va, -hi)
        tcs = np.maximum(np.minimum(np.maximum(vs, lo), hi) - vs, -hi)
        return tca, tcs, tca / a - tcs / s

    @staticmethod
    def gondzio_apply(Mh, My, dbc, da, dnu, dmu, ta, ts, nu, mu, a, s):
        dac = Mh - dbc * My
        return da + dac, dnu + (ta - nu * dac) / a, dmu + (ts + mu * dac) / s

    @staticmethod
    def select3(ok, x, y):
        """The three ``x`` where the flag is set, else the three ``y`` untouched."""
        return tuple(v.copy() for v in (x if ok else y))

    @staticmethod
    def max_step(pairs, signs):
        """min(1, min over the pairs (v, dv) and rows with sign·dv < 0 of −v/(sign·dv)): the IEEE
        quotient, and a minimum is exact in any order."""
        np = _np()
        m = 1.0
        for (v, dv), sg in zip(pairs, signs):
            a = sg * dv
            neg = a < 0.0
            if neg.any():
                m = min(m, float(np.min(-v[neg] / a[neg])))
        return m

    @staticmethod
    def fill(n, src):
        return _np().full(int(n), src, dtype=_np().float64)

    @staticmethod
    def scale_rows(P32, d):
        """diag(d)·Φ from the f32 copy: one f64 product per entry."""
        np = _np()
        return np.asarray(P32, dtype=np.float32).astype(np.float64) * np.asarray(d, dtype=np.float64)[:, None]


def svc_dual_certificate(Phi, y, c, alpha, rho, rd_tol=LR_RD_LOOSE):
    """KKT certificate of the C-SVC dual  min ½αᵀQα − 1ᵀα, yᵀα = 0, 0 ≤ α ≤ c,  Q = diag(y)ΦΦᵀdiag(y),
    in longdouble, from (α, ρ) alone.  rank(Q) ≤ r, so α is not unique: what is certified is
    w = Φᵀ(y∘α), ρ and the objective.

    The solver's stopping rule (models/svc_lowrank.py ``_ipm_gen``), with b = −ρ, s = c − α,
    multipliers ν, μ ≥ 0 and rd = (y∘Φw − 1) + b·y − ν + μ, is

        (αᵀν + sᵀμ)/(2l) < IPM_TOL,   max|rd| < 1e-8 (or < RD_LOOSE once the gap has converged),
        |yᵀα| < 1e-8·Σc,

    after which α within 1e-9·c of a bound is snapped onto it.  ν and μ are not returned, so the rule
    is restated in (w, ρ): with q = y∘(Φw + b) − 1 the multipliers of least residual are
    ν* = max(q, 0), μ* = max(−q, 0) (these are the hinge slacks ξ = μ* of the primal at (w, ρ)), and
    any ν, μ ≥ 0 with |q − ν + μ| ≤ ε have ν ≥ ν* − ε, μ ≥ μ* − ε, so
    αᵀν* + sᵀμ* ≤ αᵀν + sᵀμ + ε·Σc.  The left side minus b·yᵀα is exactly the duality gap
    P(w, ρ) − D(α), P = ½‖w‖² + Σ c_i ξ_i, D = Σα − ½‖w‖².  Conditions:

    * ``box``: 0 ≤ α ≤ c exactly;
    * ``eq``: |yᵀα| ≤ (1e-8 + 1e-9)·Σc (the rule plus the snap of every point);
    * ``gap``: P − D ≤ 2l·IPM_TOL + rd_tol·Σc + |b|·eq + snap + rounding, where
      - snap: the snap moves α_i by ≤ 1e-9·c_i on points now at a bound, so w by
        ≤ δw = 1e-9·Σ_{at a bound} c_i‖φ_i‖ and q_i by ≤ dq_i = ‖φ_i‖·δw.  The gap is a sum of
        f_i(q_i, α_i) = α_i·max(q_i, 0) + s_i·max(−q_i, 0) − b·y_i·α_i, which does not change at a point
        that is at 0 with q_i > dq_i or at c_i with q_i < −dq_i, and changes by ≤ c_i·dq_i elsewhere;
        the move of α_i itself adds ≤ 1e-9·c_i·(|q_i| + dq_i + |b|) at the points at a bound;
      - rounding: the solver evaluates rd in f64: γ_{l+r+8}·Σc·max_i(|φ_i|·|Φ|ᵀα + 1 + |b|).

    ``extra`` holds w, P, D, gap, gap_bound, the relative gap (P − D)/(1 + |D|) and max|rd*|, the
    residual left when ν*, μ* are restricted by complementarity (informative).  Since D ≤ D* = P* ≤ P
    and P is ½-strongly convex in w, a certified gap also bounds |D − D*| ≤ gap and
    ‖w − w*‖ ≤ √(2·gap)."""
    np = _np()
    L = np.longdouble
    cert = Certificate()
    P, yl, cl, al = _ld(Phi), _ld(y), _ld(c), _ld(alpha)
    l, r = P.shape
    b = -L(rho)
    csum = cl.sum()
    if not ((al >= 0).all() and (al <= cl).all()):
        cert.fail("box")
    eq_bound = (L(LR_IPM_TOL) + L(LR_SNAP)) * csum
    ya = yl @ al
    cert.check("eq", np.abs(ya), eq_bound)
    w = P.T @ (yl * al)
    q = yl * (P @ w + b) - 1
    nus, mus = np.maximum(q, 0), np.maximum(-q, 0)
    s = cl - al
    Pobj = (w @ w) / 2 + (cl * mus).sum()
    Dobj = al.sum() - (w @ w) / 2
    gap = Pobj - Dobj
    nphi = np.sqrt((P * P).sum(1))
    atb = (al == 0) | (al == cl)
    dw = L(LR_SNAP) * (cl * nphi)[atb].sum()
    dq = nphi * dw
    safe = ((al == 0) & (q > dq)) | ((al == cl) & (q < -dq))
    snap = (cl * dq)[~safe].sum() + L(LR_SNAP) * (cl * (np.abs(q) + dq + np.abs(b)))[atb].sum()
    mag = (np.abs(P) @ (np.abs(P).T @ al) + 1 + np.abs(b)).max() if l else L(0)
    rounding = lr_gamma(l + r + 8) * csum * mag
    gap_bound = 2 * l * L(LR_IPM_TOL) + L(rd_tol) * csum + np.abs(b) * eq_bound + snap + rounding
    cert.check("gap", gap, gap_bound)
    cert.extra = {"w": w, "rho": -b, "P": Pobj, "D": Dobj, "gap": gap, "gap_bound": gap_bound, "snap": snap,
                  "rel_gap": gap / (1 + np.abs(Dobj)),
                  "rd": np.abs(np.where(al == 0, np.minimum(q, 0), np.where(al == cl, np.maximum(q, 0), q))).max()
                  if l else L(0)}
    return cert
