"""The fused stack ops share one source for a row's probability (the tile body of
ops/csrc/stack_model.h) and agree to about 1 ulp; they are not bit-equal by construction, because
the compiler contracts the meta-LR sum per kernel.  ``stack_shapley``'s coalition values do equal
``stack_infer`` on the materialised hybrid rows bit for bit (a row's probability does not depend on
its lane, its tile half, the workgroup width or the SV chunk), and that is what this test holds
with ``torch.equal``.

``stack_partial`` is not held to this.  Its ice against ``stack_infer`` on the hybrid rows (3 cohort
rows; 7 cells, 65 for the second shape; no, one and two substitutions) was measured on an MI355X
with the three copied bodies and again with the one shared body, and misses ``torch.equal`` by one
ulp of the f32 probability in a few entries, the same entries both times: the meta-LR sum
``meta_b + w0·p_svc + w1·p_gbc + w2·p_lg`` is three chained FMAs in ``stack_partial_kernel`` and an FMA, a
packed multiply and two adds in ``stack_infer_kernel``.  Largest differences, (F, m, T,
depth, stumps): (5, 64, 10, 2, False) 6.0e-8 in 1 of 21 entries; (11, 250, 30, 1, True) 1.2e-7 in 29
of 195; (8, 6000, 20, 1, True) 6.0e-8 in 4 of 21; (19, 32, 4, 1, True) 6.0e-8 in 3 of 21.  Forcing
the contraction would move ``stack_infer``'s bits, and a tolerance is what test_partial_gpu.py
already checks, so those four cases are left out rather than loosened."""
import pytest
import torch

from hfens import ops
from test_partial_gpu import _random_pstack

pytestmark = pytest.mark.gpu

# (F, m, T, depth, stumps): the smallest shapes that reach each path of the tile body.  F stops at
# 11 (2^F hybrid rows per patient and background row); the KS = 12 path, (19, 32, 4, 1, True), is
# reached by stack_partial and stack_infer only and went with the partial cases (see above).
SHAPES = [
    (5, 64, 10, 2, False),      # generic tree walk, odd F, KS = 4, X3
    (11, 250, 30, 1, True),     # stumps, KS = 9, X3, mp padded past m
    (8, 6000, 20, 1, True),     # SVs beyond LDS: f32 path with restaging inside the row loop
]
N_BG = 3


@pytest.mark.parametrize("shape", SHAPES)
def test_shapley_values_are_the_f64_mean_of_stack_infer(dev, shape):
    F, m, T, depth, stumps = shape
    pk = _random_pstack(F, m, T, depth, dev, seed=F, stumps=stumps)
    g = torch.Generator().manual_seed(9000 * F)
    x = torch.randn(2, F, generator=g).to(dev)
    bg = torch.randn(N_BG, F, generator=g).to(dev)
    v = ops.stack_shapley(x, bg, pk, return_values=True)[3].cpu()
    nS = 1 << F
    keep = ((torch.arange(nS, device=dev)[:, None] >> torch.arange(F, device=dev)) & 1).bool()   # [2^F, F]
    for p in range(2):
        acc = torch.zeros(nS, dtype=torch.float64)
        for b in range(N_BG):                                    # the kernel's order: b = 0, 1, 2
            acc = acc + ops.stack_infer(torch.where(keep, x[p], bg[b]).contiguous(), pk).cpu().double()
        assert torch.equal(v[p], acc / float(N_BG))
