"""fp64 restatements of what csrc/optim.hip and ctrlv_amd/optim.py compute, and the error measure of the parity tests
(tests/test_optim_cpu.py, tests/test_optim_gpu.py).  A helper module, not a conftest.

AdamW is torch.optim.AdamW with amsgrad=False, maximize=False, in torch's operation order.  The EMA update and its decay
schedule are those of diffusers.training_utils.EMAModel [DIFF-0.27.2, not in tree]:

    s = max(0, optimization_step - update_after_step - 1)
    decay = 0                                   for s <= 0
          = (1 + s) / (10 + s)                  without warm-up
          = 1 - (1 + s / inv_gamma) ** -power   with warm-up
    clipped to [min_decay, decay];   shadow -= (1 - decay) * (shadow - param), applied after optimizer.step()

Hyper-parameters of the parity tests are fp32-representable (`f32`): the C entry points take floats, and the three sides of a
comparison -- the kernel, torch's class, this restatement -- must see the same numbers."""
import numpy as np
import torch


def f32(x):
    """x rounded to fp32, as a Python float."""
    return float(np.float32(x))


def adamw_step(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    """Step number t (1-based) on fp64 tensors, out of place: (p, m, v)."""
    g = g * grad_scale
    p = p * (1.0 - lr * weight_decay)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bias1, bias2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    p = p - (lr / bias1) * m / (v.sqrt() / bias2 ** 0.5 + eps)
    return p, m, v


def ema_step(shadow, p, decay):
    return shadow - (1.0 - decay) * (shadow - p)


def ema_decay(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0,
              power=2 / 3):
    s = max(0, optimization_step - update_after_step - 1)
    if s <= 0:
        return 0.0
    cur = 1.0 - (1.0 + s / inv_gamma) ** -power if use_ema_warmup else (1.0 + s) / (10.0 + s)
    return max(min(cur, decay), min_decay)


def ulps(x, ref, scale=None):
    """Largest |x - ref| in units of the fp32 spacing at the magnitude of the parameter.  x: fp32 result; ref: fp64 restatement;
    scale: further fp64 tensors of the same shape that take part in the magnitude (the parameter BEFORE the steps).  The
    parameter's magnitude is the larger of before and after: p * (1 - lr wd) and the subtraction round at the spacing of their
    operands, so where a step all but cancels a parameter no fp32 evaluation of the formula -- torch's included -- can be
    accurate in units of the tiny result.  The spacing never goes below that of the smallest normal number."""
    ref = ref.double().cpu().reshape(-1)
    mag = ref.abs()
    for s in (scale or ()):
        mag = torch.maximum(mag, s.double().cpu().reshape(-1).abs())
    mag = mag.clamp_min(float(np.finfo(np.float32).tiny))
    spacing = torch.exp2(torch.floor(torch.log2(mag)) - 23)
    err = (x.double().cpu().reshape(-1) - ref).abs() / spacing
    return float(err.max()) if err.numel() else 0.0


def within_rule(err_hip, err_torch):
    """The tolerance rule of every parity test: the HIP result's largest error against fp64 may be at most twice that of
    torch.optim.AdamW(foreach=False, fused=False) in fp32 on the device, and never needs to be below 1 ulp."""
    return err_hip <= max(1.0, 2.0 * err_torch)
