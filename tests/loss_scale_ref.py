"""Pure-Python restatement of the loss-scale record of csrc/optim.hip (ctrlv_loss_scale_state, ctrlv_grad_finish_scaled) and
the inputs of its tests (tests/test_loss_scale_cpu.py, tests/test_loss_scale_gpu.py).  A helper module, not a conftest.

What is restated is torch's `_amp_update_scale_` [aten/src/ATen/native/cuda/AmpKernels.cu, amp_update_scale_cuda_kernel]:

    found_inf:                               scale *= backoff_factor;  growth_tracker = 0
    else growth_tracker + 1 == interval:     scale *= growth_factor unless the product is not finite;  growth_tracker = 0
    else:                                    growth_tracker += 1

on an fp32 scale (every product rounded once to fp32), and the multiplier of the gradients that `unscale_` uses,
`_scale.double().reciprocal().float()`, times the host's grad_scale in fp32."""
import math

import numpy as np

F32 = np.float32


def f32(x):
    return float(F32(x))


def unscale(scale, grad_scale=1.0):
    """fp32(grad_scale * fp32(1.0 / (double)scale)): what the gradients are multiplied by, as a Python float."""
    inv = F32(1.0 / float(F32(scale)))
    return float(F32(grad_scale) * inv)


class Record:
    """The host's picture of ctrlv_loss_scale_state plus the running skip count of ctrlv_grad_state."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, growth_tracker=0):
        self.scale = f32(init_scale)
        self.growth_factor, self.backoff_factor = f32(growth_factor), f32(backoff_factor)
        self.growth_interval, self.growth_tracker = int(growth_interval), int(growth_tracker)
        self.unscale = 0.0
        self.skipped_total = 0

    def valid(self):
        return self.scale > 0.0 and math.isfinite(self.scale)

    def step(self, found_inf, grad_scale=1.0):
        """One ctrlv_grad_finish_scaled: the multiplier from the scale BEFORE the update, then the update.  found_inf: the norm
        of the unscaled gradients was not finite.  Returns the skip flag."""
        if not self.valid():                                # validated on the device: skip, scale and tracker left alone
            self.unscale = math.nan
            self.skipped_total += 1
            return 1
        self.unscale = unscale(self.scale, grad_scale)
        skip = 1 if found_inf else 0
        self.skipped_total += skip
        if skip:
            self.scale = float(F32(self.scale) * F32(self.backoff_factor))
            self.growth_tracker = 0
        elif self.growth_tracker + 1 == self.growth_interval:
            with np.errstate(over="ignore"):
                grown = float(F32(self.scale) * F32(self.growth_factor))
            if math.isfinite(grown):
                self.scale = grown
            self.growth_tracker = 0
        else:
            self.growth_tracker += 1
        return skip


# scripted sequences: True = a non-finite gradient in that step
SCRIPTS = {
    # growth exactly at the interval (steps 3, 6), a skip at tracker = interval - 1 (step 9: after two good ones), then growth again
    "interval3": dict(kw=dict(init_scale=1000.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=3),
                      found=[False, False, False, False, False, False, False, False, True, False, False, False]),
    # skips back to back, then recovery
    "skips": dict(kw=dict(init_scale=48000.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=2),
                  found=[True, True, False, True, False, False, False, True, False, False, False, False]),
    # growth refused: scale * growth_factor overflows fp32, the tracker still returns to 0
    "overflow": dict(kw=dict(init_scale=2.5e38, growth_factor=3.0, backoff_factor=0.25, growth_interval=2),
                     found=[False, False, False, False, True, False, False, False, False, False, False, False]),
    # torch's defaults, interval 1: growth on every good step
    "every": dict(kw=dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=1),
                  found=[False, True, False, False, True, True, False, False, False, True, False, False]),
}
