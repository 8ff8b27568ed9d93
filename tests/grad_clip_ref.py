"""fp64 restatement of the global gradient-norm clipping of csrc/optim.hip (ctrlv_grad_sumsq, ctrlv_grad_finish,
ctrlv_adamw_step_dev) and the inputs and measures of its tests (tests/test_grad_clip_cpu.py, tests/test_grad_clip_gpu.py).  A
helper module, not a conftest.

What is restated is `torch.nn.utils.clip_grad_norm_(params, max_norm)` with norm_type 2 [torch/nn/utils/clip_grad.py]:

    total_norm = sqrt(sum over every gradient element of g * g)
    clip_coef  = min(1, max_norm / (total_norm + 1e-6))
    g         *= clip_coef

with the gradients multiplied by `grad_scale` first (an unscale).  The kernels sum (double)g * (double)g -- exact products -- in
fp64, so their only roundings are the fp64 additions (relative error below n * 2^-53), sqrt and the product with |grad_scale| in
double, and ONE rounding to fp32: the norm is within 1 fp32 ulp of the exact one for every n the tests use."""
import numpy as np
import torch

BLOCK = 4096            # elements per partial sum of ctrlv_grad_sumsq (ctrlv_grad_sumsq_partials(n) = ceil(n / BLOCK))
# tests/test_optim_gpu.py's sizes, plus one block of the stage-1 partition exactly, one element more, two blocks minus one
SIZES = [1, 3, 4, 5, 255, 256, 257, 4099, 2 ** 20 + 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1]


def case(n, steps=3, seed=0):
    """tests/test_optim_gpu.py's `_case`, restated: p0 and `steps` gradients that mix zeros, +-1e4, 1e-20 and ordinary values;
    the kind an element sees changes with the step."""
    gen = torch.Generator().manual_seed(seed + n)
    p0 = (torch.randn(n, generator=gen) * 0.1).float()
    idx = torch.arange(n)
    grads = []
    for s in range(steps):
        g = torch.randn(n, generator=gen).float()
        kind = (idx + s) % 5
        g[kind == 0] = 0.0
        g[kind == 1] = torch.where(g[kind == 1] < 0, -1e4, 1e4).float()
        g[kind == 2] = 1e-20
        grads.append(g)
    return p0, grads


def huge_case(n, seed=0):
    """|g| around 1e18: every square is around 1e36 and an fp32 accumulation overflows from a few hundred elements on; the fp64
    sum stays below 1e43 and the norm, around 1e18 sqrt(n), is an ordinary fp32 number."""
    gen = torch.Generator().manual_seed(seed + n)
    return (torch.randn(n, generator=gen) * 1e18).float()


def total_norm(grads, grad_scale=1.0):
    """sqrt of the fp64 sum of squares over a list of tensors (any dtype, any device), times |grad_scale|: a Python float."""
    s = 0.0
    for g in grads:
        g = g.detach().double().cpu().reshape(-1)
        s += float((g * g).sum())
    return abs(float(grad_scale)) * float(np.sqrt(s))


def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in double."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def clip(grads, max_norm, grad_scale=1.0):
    """(norm, coef, the clipped gradients) in fp64, out of place."""
    norm = total_norm(grads, grad_scale)
    coef = clip_coef(norm, max_norm)
    return norm, coef, [g.detach().double() * float(grad_scale) * coef for g in grads]


def ulps_of(x, ref):
    """|x - ref| in units of the fp32 spacing at |ref| (never below that of the smallest normal number); inf when x is not
    finite.  x: the fp32 result as a Python float; ref: the fp64 reference."""
    x, ref = float(x), float(ref)
    if not np.isfinite(x):
        return float("inf")
    mag = max(abs(ref), float(np.finfo(np.float32).tiny))
    return abs(x - ref) / float(2.0 ** (np.floor(np.log2(mag)) - 23))
