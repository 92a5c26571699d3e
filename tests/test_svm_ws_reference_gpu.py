"""svm_ws.hip driven ONE ROUND AT A TIME (ws_init / ws_seed / ws_steps / ws_steps_kc with n_iter = 1 /
ws_finalize) against the numpy oracles of ops/reference.py: after every round the selection, the
box, the untouched points and guards, Σ yα, the published gap and (on the first 8 rounds, every
16th and the last) the true gradient and dual objective are checked against budgets derived from
the code (reference.ws_gupdate_budget and the docstrings below), never against constants.

Shapes are the smallest that reach each instantiation (selector M, working-set size Q, solver
FP / TH, MFMA operand KS, candidate lists), not the workload's; ``workload_round_check`` runs the
end-to-end tests' own problems (tests/test_svm_ws_gpu.py) through the same driver.

Largest observed / budget measured on an MI355X over this module and the workload-size runs
(every helper call prints the running maxima): (e) Σ yα 0.042; (f) objective 0 (it never rose);
(g) gradient 0.12, after a seed 0.013, at workload sizes 0.029; end |gap_true − states.gap| 0.012
of its budget (workload sizes 0.0023), end ρ 0.0044; the offset-30 case's cumulative budget is
1,100 times the centred one's.  At 10,000 × 17 (q = 1024, 21 rounds, 6,788 pairs): true gap
9.701e-4 against the device's 9.673e-4, largest |G_dev − G*| 5.4e-5 against a cumulative budget of
4.7e-3 at that row, |Σ yα| 4.7e-5 against 4.0e-3.  What is left of the gradient budget is about two thirds
the kernel-value term (reference.ws_kernel_error's (F+3)·U·mag chain bound, a worst case over
F + 3 roundings); the accumulation term follows the kernel's real summation tree."""
import numpy as np
import pytest
import torch

from hfens.models import smo
from hfens.ops import reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-3
MAX_INNER = 4096
INNER_FRAC = 0.2
GUARD = 37          # guard points between problems (odd: the next problem starts misaligned)
ZGUARD = 5          # guard rows between problems in zcat (≠ GUARD, so aoff ≠ zoff)
MAX_ROUNDS = 600

_ST = np.dtype([("done", "<i4"), ("outer", "<i4"), ("inner", "<i8"), ("gap", "<f8"), ("nc", "<i4"),
                ("nws", "<i4"), ("nprev", "<i4"), ("pad", "<i4"), ("cyc", "<i8", (6,))])
assert _ST.itemsize == smo._WS_STATE_BYTES

RATIOS = {}      # check → largest observed / budget so far in this process (printed, never asserted)


def _ratio(name, obs, bud):
    r = float(np.max(np.asarray(obs, dtype=np.float64) / np.asarray(bud, dtype=np.float64)))
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _draw(l, npos, F, seed, sep, offset=0.0):
    """Two Gaussian classes ``sep`` apart along the first feature, positives first."""
    rng = np.random.default_rng(seed)
    Z = rng.normal(size=(l, F))
    Z[:, 0] += np.where(np.arange(l) < npos, sep, -sep)
    return (Z + offset).astype(np.float32)


def _feasible_seed(l, npos, Cp, Cn, rng):
    """Random feasible α: about half zeros, the rest at least 5 % of C inside the box, Σ yα = 0 up
    to f64 rounding (the heavier class is scaled down, which keeps it in the box)."""
    C = np.where(np.arange(l) < npos, Cp, Cn)
    a = (0.05 + 0.9 * rng.random(l)) * C
    a[rng.random(l) < 0.5] = 0.0
    sp, sn = a[:npos].sum(), a[npos:].sum()
    if sp > sn:
        a[:npos] *= sn / sp
    else:
        a[npos:] *= sp / sn
    return a


class _Prob:
    def __init__(self, Z, npos, Cp, Cn):
        self.Z, self.l, self.npos, self.Cp, self.Cn = Z, Z.shape[0], int(npos), float(Cp), float(Cn)
        self.pos = np.arange(self.l) < self.npos
        self.y = np.where(self.pos, 1.0, -1.0)
        self.C = np.where(self.pos, self.Cp, self.Cn)
        self.Cmax = max(self.Cp, self.Cn)


def _problems(F, shapes, seed, sep, offset=0.0):
    out = []
    for k, (l, npos) in enumerate(shapes):
        out.append(_Prob(_draw(l, npos, F, seed + k, sep, offset), npos,
                         min(l / (2.0 * npos), 4.0), min(l / (2.0 * (l - npos)), 4.0)))
    return out


class _Driver:
    """The device buffers of one batch, laid out with guards: α, G, ‖z‖² and the keys are NaN /
    0xFFFFFFFF everywhere except the problems' own ranges, and zcat holds the problems in reverse
    order with NaN rows between them, so aoff ≠ zoff."""

    def __init__(self, dev, F, probs, *, kc, q=0, th=256, seeds=None, ngl2e=None):
        from hfens import ops
        self.E, self.dev, self.F, self.probs, self.kc, self.th = ops.ext(), dev, F, probs, kc, th
        self.s = ops.stream_ptr(dev)
        P = self.P = len(probs)
        self.Q = smo.WS_KC_Q if kc else (q or (1024 if F <= 24 else 512))
        self.q_arg = q
        self.ngl2e = np.float32(-(1.0 / F) * R.LOG2E) if ngl2e is None else np.float32(ngl2e)
        self.max_l = max(p.l for p in probs)
        aoffs, off = [], GUARD
        for p in probs:
            aoffs.append(off)
            off += p.l + GUARD
        self.n = n = off
        zoffs, zoff = [0] * P, ZGUARD
        for k in reversed(range(P)):
            zoffs[k] = zoff
            zoff += probs[k].l + ZGUARD
        self.aoffs, self.zoffs = aoffs, zoffs
        zc = np.full((zoff, F), np.nan, np.float32)
        self.guard = np.ones(n, bool)
        arr = np.zeros(P, smo._WS_DT)
        for k, p in enumerate(probs):
            zc[zoffs[k]:zoffs[k] + p.l] = p.Z
            self.guard[aoffs[k]:aoffs[k] + p.l] = False
            arr[k] = (zoffs[k], aoffs[k], p.l, p.npos, p.Cp, p.Cn, self.ngl2e, 0)
        assert all(a != z for a, z in zip(aoffs, zoffs))
        self.zcat = torch.from_numpy(zc).to(dev).contiguous()
        self.pdev = smo._dev_struct(arr, dev)
        nan = float("nan")
        self.zn = torch.full((n,), nan, dtype=torch.float32, device=dev)
        self.alpha = torch.full((n,), nan, dtype=torch.float64, device=dev)
        self.G = torch.full((n,), nan, dtype=torch.float64, device=dev)
        self.keys = torch.full((2 * n,), -1, dtype=torch.int32, device=dev)
        self.states = torch.zeros(P * smo._WS_STATE_BYTES // 4, dtype=torch.int32, device=dev)
        Q, Fp2 = self.Q, 2 * smo._ws_ks(F)
        z = lambda numel, dt: torch.zeros(numel, dtype=dt, device=dev)   # noqa: E731
        self.wsz, self.wsn, self.wdc = z(P * Fp2 * Q, torch.float32), z(P * Q, torch.float32), z(P * Q, torch.float32)
        self.wsprev, self.wsidx = z(P * (Q // 2), torch.int32), z(P * Q, torch.int32)
        self.gkey, self.hist = z(2 * P, torch.int64), z(1, torch.int32)
        self.cand, self.ncand = None, 0
        if kc:
            out = np.zeros(1, dtype=np.int64)
            self.E.ws_kc_cand_len(self.max_l, out.ctypes.data)
            self.ncand = int(out[0])
            if self.ncand:
                self.cand = z(3 * P * self.ncand, torch.int32)
        E = self.E
        E.ws_init(self.pdev.data_ptr(), P, self.max_l, self.zcat.data_ptr(), F, self.zn.data_ptr(),
                  self.alpha.data_ptr(), self.G.data_ptr(), self.states.data_ptr(), self.keys.data_ptr(), n,
                  self.hist.data_ptr(), self.gkey.data_ptr(), self.s)
        if seeds is not None:
            sd = np.full(n, np.nan)
            for k, p in enumerate(probs):
                sd[aoffs[k]:aoffs[k] + p.l] = seeds[k]
            self.aseed = torch.from_numpy(sd).to(dev)
            E.ws_seed(self.pdev.data_ptr(), P, self.max_l, self.zcat.data_ptr(), F, self.zn.data_ptr(),
                      self.aseed.data_ptr(), self.alpha.data_ptr(), self.G.data_ptr(), self.keys.data_ptr(), n,
                      self.gkey.data_ptr(), self.s)

    def round(self):
        E, P, F, n = self.E, self.P, self.F, self.n
        if self.kc:
            E.ws_steps_kc(self.pdev.data_ptr(), P, self.max_l, self.zcat.data_ptr(), F, self.zn.data_ptr(),
                          self.alpha.data_ptr(), self.G.data_ptr(), self.states.data_ptr(), self.wsz.data_ptr(),
                          self.wsn.data_ptr(), self.wdc.data_ptr(), self.wsprev.data_ptr(), self.keys.data_ptr(), n,
                          self.gkey.data_ptr(), self.cand.data_ptr() if self.cand is not None else 0, EPS,
                          MAX_ROUNDS + 1, MAX_INNER, INNER_FRAC, 1, 0, self.s)
        else:
            E.ws_steps(self.pdev.data_ptr(), P, self.max_l, self.zcat.data_ptr(), F, self.zn.data_ptr(),
                       self.alpha.data_ptr(), self.G.data_ptr(), self.states.data_ptr(), self.wsz.data_ptr(),
                       self.wsn.data_ptr(), self.wdc.data_ptr(), self.wsprev.data_ptr(), self.wsidx.data_ptr(),
                       self.keys.data_ptr(), n, self.gkey.data_ptr(), EPS, MAX_ROUNDS + 1, MAX_INNER, INNER_FRAC, 1,
                       0, self.th, self.q_arg, self.s)

    def read(self):
        torch.cuda.synchronize()
        return dict(alpha=self.alpha.cpu().numpy(), G=self.G.cpu().numpy(),
                    st=self.states.cpu().numpy().view(_ST).copy(),
                    wsprev=self.wsprev.cpu().numpy().reshape(self.P, self.Q // 2),
                    wsidx=self.wsidx.cpu().numpy().reshape(self.P, self.Q))

    def check_guards(self, snap):
        g = self.guard
        assert np.isnan(snap["alpha"][g]).all() and np.isnan(snap["G"][g]).all(), "α / G guard written"
        assert np.isnan(self.zn.cpu().numpy()[g]).all(), "‖z‖² guard written"
        k = self.keys.cpu().numpy().reshape(2, self.n)
        assert (k[:, g] == -1).all(), "key guard written"

    def finalize(self):
        P = self.P
        rho = torch.full((P,), float("nan"), dtype=torch.float64, device=self.dev)
        iters = torch.zeros(P, dtype=torch.int32, device=self.dev)
        inner = torch.zeros(P, dtype=torch.int64, device=self.dev)
        gap = torch.zeros(P, dtype=torch.float64, device=self.dev)
        self.E.ws_finalize(self.pdev.data_ptr(), P, self.states.data_ptr(), self.alpha.data_ptr(), self.G.data_ptr(),
                           rho.data_ptr(), iters.data_ptr(), inner.data_ptr(), gap.data_ptr(), self.s)
        torch.cuda.synchronize()
        return rho.cpu().numpy(), iters.cpu().numpy(), inner.cpu().numpy(), gap.cpu().numpy()


def _solve_and_check(dev, F, probs, *, kc=False, q=0, th=256, seeds=None, ngl2e=None, light=False, label=""):
    """Runs the batch to convergence one round at a time and asserts checks (a)–(h) of every round and
    the end checks.  Returns the per-round trace (for bit-identity comparisons) and the largest
    cumulative gradient budget per problem.

    Budgets (U = 2⁻²⁴, Cmax = max(Cp, Cn), pairs = the round's pair updates from ``states.inner``):

    (e) Σ yα.  A pair step keeps y_i α_i + y_j α_j in exact arithmetic; in f32 the unequal-label
        step rounds at most twice (α_i + δ and α_j + δ; clipped: α_i − α_j and C − that), the
        equal-label step at most three times (α_i + α_j, itself ≤ 2·Cmax, counts double; then
        sum − C), every rounding ≤ U·Cmax: ≤ 3·U·Cmax per pair.  The write-back
        a0 + ((double)a − (double)(float)a0) carries the f32 change over exactly (two f64 roundings,
        ≤ 2⁻⁵²·Cmax per slot) EXCEPT for a slot that ends at a bound, which is written as the f64
        0 or C while its f32 twin was (float)a0 → 0 or (float)C: off by |a0 − (float)a0| +
        |C − (float)C| ≤ 2·U·Cmax per clamped slot.
    (f) objective.  A pair step of size δ with a directional derivative known to within e raises
        the true objective by at most |δ|·e (exact line search with a wrong slope s̃ = s + e:
        Δf = δ(e − s̃/2) ≤ |δ||e|, clipping only shortens δ).  Within a round the f32 local
        gradient has drifted after k pairs by ≤ k·U·(Yg + 3·Cmax) per entry (three roundings per
        update: K_j·c_j, the fma, the add to yg), |yg| ≤ Yg = 1 + Σ_{c∉B} α_c + Σ_{c∈B} C_c; and
        the model the solver minimises differs from the truth by the start gradient's error
        (cumulative (g) budget + U·|G| for the f32 copy) and the kernel's (dK).  So
        Δf ≤ Cmax·[pairs²·2U·(Yg + 3·Cmax) + pairs·2·(max budget + U·max|G|) + pairs²·4·dKmax·Cmax].
        Coarse for rounds of thousands of pairs, tight for the short rounds near the end.
    (g) gradient: reference.ws_gupdate_budget per round plus 2⁻⁵²·(1 + |G|) for the f64 add; a seeded
        start contributes the same expression at ncp = 256."""
    D = _Driver(dev, F, probs, kc=kc, q=q, th=th, seeds=seeds, ngl2e=ngl2e)
    Q, P = D.Q, D.P
    snap = D.read()
    D.check_guards(snap)
    trace = []
    S = []
    for k, p in enumerate(probs):
        a = snap["alpha"][D.aoffs[k]:D.aoffs[k] + p.l].copy()
        g = snap["G"][D.aoffs[k]:D.aoffs[k] + p.l].copy()
        znd = D.zn.cpu().numpy()[D.aoffs[k]:D.aoffs[k] + p.l].astype(np.float64)
        zn = (p.Z.astype(np.float64) ** 2).sum(1)
        assert (np.abs(znd - zn) <= (F * U / (1 - F * U)) * zn).all()
        st = dict(alpha=a, G=g, prev=np.zeros(0, np.int64), bud=np.zeros(p.l), sya_bud=0.0, done_at=None,
                  permitted=0.0, final=None, moves=[], f64term=np.zeros(p.l))
        if seeds is None:
            assert (a == 0).all() and (g == -1).all() and not np.signbit(a).any()
        else:
            assert np.array_equal(_bits(a), _bits(seeds[k]))
            st["bud"] = R.ws_gupdate_budget(p.Z, D.ngl2e, a, 256) + 2.0 ** -52 * (1 + np.abs(g))
        o = (R.svc_dual_oracle(p.Z, p.npos, p.Cp, p.Cn, D.ngl2e, a) if not (light and seeds is None)
             else dict(sya=np.longdouble(0), obj=np.longdouble(0)))
        if seeds is not None:
            _ratio("g_seed", np.abs(g - o["G"]), st["bud"])
            assert (np.abs(g - o["G"]) <= st["bud"]).all()
        st["sya0"], st["obj"] = o["sya"], o["obj"]
        st["dkmax"] = None
        S.append(st)
    prev_states = snap["st"]
    assert (prev_states["done"] == 0).all() and (prev_states["nprev"] == 0).all()
    for rnd in range(1, MAX_ROUNDS + 1):
        D.round()
        snap = D.read()
        D.check_guards(snap)
        states = snap["st"]
        trace.append((snap["alpha"].tobytes(), snap["G"].tobytes(),
                      [tuple(int(s[f]) for f in ("done", "outer", "inner", "nc", "nws", "nprev")) + (float(s["gap"]),)
                       for s in states]))
        for k, p in enumerate(probs):
            st, s0, s1 = S[k], prev_states[k], states[k]
            a1 = snap["alpha"][D.aoffs[k]:D.aoffs[k] + p.l]
            g1 = snap["G"][D.aoffs[k]:D.aoffs[k] + p.l]
            tag = f"problem {k} (l={p.l}) round {rnd}"
            if st["done_at"] is not None:
                # a finished problem is left alone while the others continue
                assert np.array_equal(_bits(a1), _bits(st["alpha"])) and np.array_equal(_bits(g1), _bits(st["G"])), tag
                assert s1.tobytes()[:40] == s0.tobytes()[:40], tag
                continue
            # (h) the published gap: the maxima folded by the kernel that wrote G, bit for bit
            kk = R.svc_kkt(st["alpha"], st["G"], p.npos, p.Cp, p.Cn)
            assert float(s1["gap"]) == float(kk["gap"]), (tag, float(s1["gap"]), float(kk["gap"]))
            if s1["done"] and s1["outer"] == s0["outer"]:
                assert np.array_equal(_bits(a1), _bits(st["alpha"])) and np.array_equal(_bits(g1), _bits(st["G"])), tag
                st["done_at"] = rnd
                continue
            assert s1["outer"] == s0["outer"] + 1, tag
            # (a) selection
            up, low, carried = R.ws_select_oracle(st["alpha"], st["G"], p.npos, p.Cp, p.Cn, Q, st["prev"])
            nprev, nws = int(s1["nprev"]), int(s1["nws"])
            new = snap["wsprev"][k, :nprev].astype(np.int64)
            assert nprev == up.size + low.size and nws == nprev + carried.size, (tag, nprev, nws, up.size, low.size)
            assert set(new[:up.size]) == set(up) and set(new[up.size:]) == set(low), tag
            if not kc:
                ws = snap["wsidx"][k, :nws].astype(np.int64)
                assert np.array_equal(ws[:nprev], new) and np.array_equal(ws[nprev:], carried), tag
            B = np.concatenate([new, carried])
            assert np.unique(B).size == B.size and B.min() >= 0 and B.max() < p.l, tag
            inB = np.zeros(p.l, bool)
            inB[B] = True
            # (b) the box, exactly; (c) points outside the working set keep their bits
            assert ((a1 >= 0) & (a1 <= p.C)).all() and not np.signbit(a1).any(), (tag, a1.min(), (a1 - p.C).max())
            assert np.array_equal(_bits(a1[~inB]), _bits(st["alpha"][~inB])), tag
            # (e) Σ yα
            pairs = int(s1["inner"] - s0["inner"])
            assert 0 <= pairs <= MAX_INNER, tag
            d = a1 - st["alpha"]
            changed = d != 0
            nc = int(changed.sum())
            assert int(s1["nc"]) == nc, tag
            nb = int((changed & ((a1 == 0) | (a1 == p.C))).sum())
            st["sya_bud"] += U * p.Cmax * (3 * pairs + 2 * nb) + 2.0 ** -52 * p.Cmax * nws
            sya = (p.y.astype(np.longdouble) * a1.astype(np.longdouble)).sum()
            _ratio("e_sum_y_alpha", abs(sya - st["sya0"]), st["sya_bud"])
            assert abs(sya - st["sya0"]) <= st["sya_bud"], (tag, float(sya - st["sya0"]), st["sya_bud"])
            # (g) budget of this round's gradient update (every round; compared on the check rounds)
            bud0max = float(st["bud"].max())
            ncp = (nc + 31) & ~31
            order = B[changed[B]]            # the staged order of the changed coefficients: slot order
            if nc == 0:
                assert np.array_equal(_bits(g1), _bits(st["G"])), tag
            if light:
                # the round's movement is kept; the budget is evaluated at the end, on the rows that matter
                st["moves"].append((order, d[order], ncp))
                st["f64term"] += 2.0 ** -52 * (1 + np.abs(g1))
                st["alpha"], st["G"], st["prev"], st["final"] = a1.copy(), g1.copy(), new, None
                if s1["done"]:
                    st["done_at"] = rnd
                continue
            st["bud"] = (st["bud"] + R.ws_gupdate_budget(p.Z, D.ngl2e, d, ncp, order=order, npos=p.npos)
                         + 2.0 ** -52 * (1 + np.abs(g1)))
            # (f) what the objective may rise by in this round
            if st["dkmax"] is None:
                n2 = float((p.Z.astype(np.float64) ** 2).sum(1).max())
                nn = F + 3
                x = np.expm1(np.log(2.0) * -float(D.ngl2e) * 4 * n2 * nn * U / (1 - nn * U))
                st["dkmax"] = x + R.EPS_EXP2 + x * R.EPS_EXP2
            Yg = 1 + st["alpha"][~inB].sum() + p.C[inB].sum()
            st["permitted"] += p.Cmax * (pairs ** 2 * 2 * U * (Yg + 3 * p.Cmax)
                                         + pairs * 2 * (bud0max + U * np.abs(st["G"]).max())
                                         + pairs ** 2 * 4 * st["dkmax"] * p.Cmax)
            st["alpha"], st["G"], st["prev"], st["final"] = a1.copy(), g1.copy(), new, None
            if s1["done"]:
                st["done_at"] = rnd
            if rnd <= 8 or rnd % 16 == 0 or s1["done"]:
                _check_true(p, D, st, tag)
        prev_states = states
        if all(st["done_at"] is not None for st in S):
            break
    assert all(st["done_at"] is not None for st in S), "not converged"
    # one more round: every problem is done, nothing may move
    D.round()
    last = D.read()
    assert last["alpha"].tobytes() == snap["alpha"].tobytes() and last["G"].tobytes() == snap["G"].tobytes()
    rho, iters, inner, gap = D.finalize()
    D.check_guards(last)
    figures = []
    for k, p in enumerate(probs):
        st, s1 = S[k], last["st"][k]
        tag = f"problem {k} (l={p.l}) end"
        if light:
            figures.append(_light_end(p, D, st, s1, rho[k], tag))
            continue
        if st["final"] is None:          # (α moved since the last comparison with the oracle)
            _check_true(p, D, st, tag)
        o = st["final"]
        assert s1["done"] == 1 and s1["gap"] < EPS, (tag, s1["gap"])
        assert iters[k] == s1["outer"] and inner[k] == s1["inner"] and gap[k] == s1["gap"], tag
        bmax = float(st["bud"].max())
        _ratio("end_gap", abs(float(o["gap"]) - float(s1["gap"])), 2 * bmax)
        assert abs(float(o["gap"]) - float(s1["gap"])) <= 2 * bmax, (tag, float(o["gap"]), float(s1["gap"]), bmax)
        L = np.longdouble
        kd = R.svc_kkt(st["alpha"].astype(L), st["G"].astype(L), p.npos, p.Cp, p.Cn)
        free = (st["alpha"] > 0) & (st["alpha"] < p.C)
        # (a mean of nfree values of size |yG| carries nfree·2⁻⁵³·mean|yG|: relative to that, not to a ρ near 0)
        scale = max(abs(float(kd["rho"])), float(np.abs(st["G"][free]).mean()) if free.any() else 0.0)
        assert abs(rho[k] - float(kd["rho"])) <= 1e-13 * scale, (tag, rho[k], float(kd["rho"]))
        _ratio("end_rho", abs(rho[k] - float(o["rho"])), bmax)
        assert abs(rho[k] - float(o["rho"])) <= bmax, (tag, rho[k], float(o["rho"]), bmax)
    print("WS_RATIOS", label, {k: float(f"{v:.4g}") for k, v in sorted(RATIOS.items())})
    if light:
        return figures
    return trace, [float(st["bud"].max()) for st in S], [st["done_at"] for st in S]


def _light_end(p, D, st, s1, rho_dev, tag):
    """End checks of a workload-size problem: ONE oracle evaluation, and the exact cumulative
    budget (every round's recorded movement through ws_gupdate_budget's summation-tree form)
    on the rows that decide the claims: the row with the largest |G_dev − G*|, the rows that attain
    the true and the device maxima of the gap, and 60 others.  gap_true ≤ gap_dev + the budgets of
    the two rows attaining the TRUE maxima (each true maximum is at most that row's device value
    plus its budget, which is at most the device maximum plus it), and the other way round."""
    o = R.svc_dual_oracle(p.Z, p.npos, p.Cp, p.Cn, D.ngl2e, st["alpha"])
    Gt = np.asarray(o["G"], dtype=np.float64)
    err = np.abs(st["G"] - Gt)
    a = st["alpha"]
    up = np.where(p.pos, a < p.C, a > 0)
    low = np.where(p.pos, a > 0, a < p.C)

    def arg(G, mask, sign):
        v = np.where(mask, sign * p.y * G, -np.inf)
        return int(np.argmax(v))
    tu, tl, du, dl = arg(Gt, up, -1), arg(Gt, low, 1), arg(st["G"], up, -1), arg(st["G"], low, 1)
    rng = np.random.default_rng(p.l)
    rows = np.unique(np.concatenate([[int(np.argmax(err)), tu, tl, du, dl], rng.choice(p.l, 60, replace=False)]))
    bud = st["f64term"][rows].copy()
    dvec = np.zeros(p.l)
    for order, vals, ncp in st["moves"]:
        if order.size:
            dvec[order] = vals
            bud += R.ws_gupdate_budget(p.Z, D.ngl2e, dvec, ncp, order=order, npos=p.npos, rows=rows)
            dvec[order] = 0.0
    at = dict(zip(rows.tolist(), bud.tolist()))
    _ratio("workload_gradient", err[rows], bud)
    assert (err[rows] <= bud).all(), (tag, float((err[rows] / bud).max()))
    gap_dev, gap_true = float(s1["gap"]), float(o["gap"])
    assert s1["done"] == 1 and gap_dev < EPS, (tag, gap_dev)
    assert gap_true < EPS + at[tu] + at[tl], (tag, gap_true, at[tu], at[tl])
    assert gap_true <= gap_dev + at[tu] + at[tl] and gap_dev <= gap_true + at[du] + at[dl], (tag, gap_true, gap_dev)
    _ratio("workload_gap", abs(gap_true - gap_dev), max(at[tu] + at[tl], at[du] + at[dl]))
    L = np.longdouble
    kd = R.svc_kkt(a.astype(L), st["G"].astype(L), p.npos, p.Cp, p.Cn)
    free = (a > 0) & (a < p.C)
    scale = max(abs(float(kd["rho"])), float(np.abs(st["G"][free]).mean()) if free.any() else 0.0)
    assert abs(rho_dev - float(kd["rho"])) <= 1e-13 * scale, (tag, rho_dev, float(kd["rho"]))
    sya = float(abs(o["sya"] - st["sya0"]))
    assert sya <= st["sya_bud"], (tag, sya, st["sya_bud"])
    fig = dict(l=p.l, rounds=int(s1["outer"]), pairs=int(s1["inner"]), gap_true=gap_true, gap_dev=gap_dev,
               gap_budget=at[tu] + at[tl], G_drift_max=float(err.max()), G_drift_budget=at[int(np.argmax(err))],
               sum_y_alpha=sya, sum_y_alpha_budget=st["sya_bud"])
    print("WS_WORKLOAD", {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in fig.items()})
    return fig


def workload_round_check(dev, Z, y, gamma, kc):
    """One of the end-to-end tests' problems (standardised rows ``Z``, labels ``y`` in {0, 1}, balanced
    class weights, the fitted model's ``gamma``) solved cold through the round driver: every
    per-round check of this module except the per-round oracle, then :func:`_light_end`.  A fit
    keeps no per-round movement, so the sound cumulative budget exists only here."""
    yb = np.asarray(y) > 0
    order = np.argsort(~yb, kind="stable")
    Z32 = np.asarray(Z)[order].astype(np.float32)
    n, npos = yb.size, int(yb.sum())
    p = _Prob(Z32, npos, n / (2.0 * npos), n / (2.0 * (n - npos)))
    return _solve_and_check(dev, Z32.shape[1], [p], kc=kc, ngl2e=np.float32(-gamma * R.LOG2E), light=True,
                            label=f"workload {n}x{Z32.shape[1]} kc={kc}")[0]


def _check_true(p, D, st, tag):
    """(g) and (f) against the true gradient and objective of the device α."""
    o = R.svc_dual_oracle(p.Z, p.npos, p.Cp, p.Cn, D.ngl2e, st["alpha"])
    err = np.abs(st["G"].astype(np.longdouble) - o["G"])
    if st["bud"].max() > 0:
        _ratio("g_gradient", err[st["bud"] > 0], st["bud"][st["bud"] > 0])
    assert (err <= st["bud"]).all(), (tag, float((err - st["bud"]).max()), float(st["bud"].max()))
    if st["permitted"] > 0:
        _ratio("f_objective", max(float(o["obj"] - st["obj"]), 0.0), st["permitted"])
    assert o["obj"] <= st["obj"] + st["permitted"], (tag, float(o["obj"]), float(st["obj"]), st["permitted"])
    st["obj"], st["permitted"], st["final"] = o["obj"], 0.0, o


# ------------------------------------------------------------------------------- the cases
# l edges at F = 17 (npos edges 1, l − 1 and ≈ 0.2·l spread over the problems); sep: class separation
# (large problems are well separated, so few α are non-zero and the oracle stays cheap)
_L_CASES = {
    "l100_257_1025": ([(100, 1), (257, 256), (1025, 205)], 1.0, 0),          # nws < Q; M = 4
    "l4096": ([(4096, 819), (1025, 1024)], 2.0, 0),                            # M = 4 at its edge
    "l4097": ([(4097, 819), (300, 1)], 2.0, 0),                                # M = 16
    "l16384": ([(16384, 3277), (700, 140)], 3.0, 0),                           # M = 16 at its edge
    "l16385_q1024": ([(16385, 3277), (500, 499)], 3.0, 1024),                  # M = 32
}


@pytest.mark.parametrize("name", list(_L_CASES))
def test_rounds_l_edges(dev, name):
    shapes, sep, q = _L_CASES[name]
    _solve_and_check(dev, 17, _problems(17, shapes, 100, sep), q=q, label=name)


def test_finished_problem_is_left_alone(dev):
    """A two-point problem is solved by its first pair; its 600-point batch mate needs several more
    rounds, through all of which the finished problem's α, G and state must keep their bits (the
    ``done_at`` branch of the helper) — asserted to have happened, not left to the shapes."""
    done_at = _solve_and_check(dev, 17, _problems(17, [(2, 1), (600, 120)], 150, 1.0), label="early")[2]
    assert done_at[0] + 2 <= done_at[1], done_at


@pytest.mark.parametrize("F", [1, 7, 8, 9, 16, 17, 18, 19, 24, 25, 32, 33, 48])
def test_rounds_every_feature_width(dev, F):
    """Every KS ∈ {4, 9, 12, 24}, every FP ∈ {4, …, 48}, the odd-F masks of the MFMA operand load and
    Q = 512 above F = 24."""
    _solve_and_check(dev, F, _problems(F, [(600, 120), (333, 200)], 200 + F, 1.0))


def test_rounds_q512(dev):
    _solve_and_check(dev, 17, _problems(17, [(600, 120), (1025, 1)], 300, 1.0), q=512)


def test_inner_threads_512_bit_identical_to_256(dev):
    """The slot set and the max-reductions do not depend on the wave count: α, G and the states of
    every round are the same bits with 8 waves as with 4."""
    probs = _problems(17, [(1500, 300), (600, 599)], 310, 1.0)
    t256 = _solve_and_check(dev, 17, probs, th=256, label="th256")[0]
    t512 = _solve_and_check(dev, 17, probs, th=512, label="th512")[0]
    assert len(t256) == len(t512)
    for r, (x, y) in enumerate(zip(t256, t512)):
        assert x[2] == y[2], (r, x[2], y[2])
        assert x[0] == y[0] and x[1] == y[1], r


@pytest.mark.parametrize("F", [7, 17, 24])
@pytest.mark.parametrize("shapes,sep", [([(300, 60), (131, 130)], 1.0), ([(4097, 819), (300, 1)], 2.0)],
                         ids=["l300", "l4097"])
def test_rounds_kc(dev, F, shapes, sep):
    _solve_and_check(dev, F, _problems(F, shapes, 400 + F, sep), kc=True)


def test_rounds_kc_candidate_lists(dev):
    """16,500 points: three candidate blocks of 8,192, the last nearly empty; check (a) requires the
    two-stage selection to equal the global top-k oracle."""
    _solve_and_check(dev, 17, _problems(17, [(16500, 3300), (400, 80)], 500, 3.0), kc=True)


@pytest.mark.parametrize("F,shapes,kc", [(17, [(250, 50), (130, 100)], False), (17, [(300, 60), (130, 100)], False),
                                         (17, [(3000, 600), (700, 650)], False), (17, [(300, 60), (130, 100)], True),
                                         (7, [(300, 60), (130, 100)], False), (24, [(300, 60), (130, 100)], False),
                                         (33, [(300, 60), (130, 100)], False)],
                         ids=["S1", "S2", "S12", "S2_kc", "F7_KS4", "F24_KS12", "F33_KS24"])
def test_rounds_seeded_start(dev, F, shapes, kc):
    """ws_seed from a feasible random α, half zeros: unsplit (one 256-column chunk, S = 1) and
    split-K (S = 2, S = 12) seeds, and every KS instance of ws_seed_kernel (4, 9, 12, 24)."""
    probs = _problems(F, shapes, 600, 1.0)
    rng = np.random.default_rng(601)
    seeds = [_feasible_seed(p.l, p.npos, p.Cp, p.Cn, rng) for p in probs]
    _solve_and_check(dev, F, probs, kc=kc, seeds=seeds, label=f"seeded F={F}")


def test_adverse_conditioning_budget_grows(dev):
    """Unstandardised features (a common offset of 30): ‖a‖² + ‖b‖² − 2a·b cancels ≈ 900·F against
    distances of ≈ 2·F, and the budget must grow to cover it.  Measured ratio of the largest
    cumulative budgets, offset / centred: about 1,100 (printed)."""
    shapes = [(600, 120), (333, 200)]
    b0 = _solve_and_check(dev, 17, _problems(17, shapes, 700, 1.0), label="centred")[1]
    b1 = _solve_and_check(dev, 17, _problems(17, shapes, 700, 1.0, offset=30.0), label="offset30")[1]
    print("WS_ADVERSE budget growth", max(b1) / max(b0))
    assert max(b1) > 10 * max(b0)


def test_finalize_straight_after_init(dev):
    """No free vectors at α = 0: ub = min yG over {y = +1} = −1, lb = max yG over {y = −1} = +1, ρ = 0."""
    D = _Driver(dev, 17, _problems(17, [(257, 50), (100, 99)], 800, 1.0), kc=False)
    rho, iters, inner, gap = D.finalize()
    assert (rho == 0).all() and (iters == 0).all() and (inner == 0).all()
    D.check_guards(D.read())
