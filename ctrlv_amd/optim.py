"""The optimiser and the EMA of the three training steps (`training.train_step`, `unet_train_step`, `vae_train_step`) on the
kernels of csrc/optim.hip: `AdamW`, a `torch.optim.Optimizer` whose parameters, gradients and moments live in flat fp32
buffers (one launch per parameter group instead of one per tensor), and `EMAModel`, the surface of
`diffusers.training_utils.EMAModel` that tools/train_video_diffusion.py uses (:140, :160-172, :255, :402-422, :550, :595).
The learning-rate scheduler stays the caller's (torch's LambdaLR, which is what diffusers' `get_scheduler` builds).

The kernels run on the GPU only and there is no eager fallback for `AdamW.step`: it raises on CPU parameters.  Construction,
the flat layout, the state dict and the decay schedule work on any device."""
import ctypes
import json
import math
import os
import struct
import weakref

import torch

from . import _lib

ALIGN = 64                  # elements: every parameter starts at a multiple of 64 fp32 elements (256 bytes) of its group's buffer


def _f32(x):
    """x rounded to fp32, as a Python float: the C entry points take floats, the bias corrections are computed from what
    the kernel will actually see."""
    return ctypes.c_float(x).value


def _lib_for_device(t):
    if not t.is_cuda:
        raise _lib.CtrlvHipError("ctrlv_amd.optim: the optimiser kernels run on the GPU; parameters are on " + str(t.device))
    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


_HOMES = {}                 # id of a homed parameter -> (weakref of it, weakref of its optimiser, group index, index in the group)


def _set_home(p, opt, gi, i):
    key = id(p)

    def drop(_ref, key=key):
        _HOMES.pop(key, None)
    _HOMES[key] = (weakref.ref(p, drop), weakref.ref(opt), gi, i)


def home_of(p):
    """(optimiser, group index, index in the group) of a parameter that lives in a `ctrlv_amd.optim.AdamW`, else None.  The entry
    counts only while the parameter's data is still the view it names."""
    h = _HOMES.get(id(p))
    opt = h[1]() if h is not None and h[0]() is p else None
    if opt is None or h[2] >= len(opt._flat):
        return None
    flat = opt._flat[h[2]]
    if h[3] >= len(flat.offsets) or p.dtype != torch.float32 or p.data_ptr() != flat.p.data_ptr() + 4 * flat.offsets[h[3]]:
        return None
    return opt, h[2], h[3]


class _Flat:
    """Flat storage of one parameter group: four fp32 buffers (parameters, gradients, exp_avg, exp_avg_sq) and each
    parameter's (offset, numel) in them.  Padding elements are zero and stay zero under the update (g = m = v = p = 0 gives
    m = v = 0 and p - step * 0 / eps = 0)."""

    def __init__(self, params):
        self.offsets, off = [], 0
        for p in params:
            self.offsets.append(off)
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.numel = off
        self.padding = off - sum(p.numel() for p in params)
        dev = params[0].device if params else torch.device("cpu")
        self.p, self.g, self.m, self.v = (torch.zeros(max(off, 1), dtype=torch.float32, device=dev) for _ in range(4))

    def view(self, buf, i, p):
        return buf[self.offsets[i]:self.offsets[i] + p.numel()].view(p.shape)


class AdamW(torch.optim.Optimizer):
    """`torch.optim.AdamW` (amsgrad=False, maximize=False) as ONE `ctrlv_adamw_step` launch per parameter group.

    Every parameter of a group is re-homed into the group's flat fp32 buffer (`p.data` becomes a view at an offset that is a
    multiple of 64 elements; the Parameter objects, their modules and state-dict keys do not change), `p.grad` is pre-set to the
    matching view of the gradient buffer so that autograd accumulates in place, and `exp_avg` / `exp_avg_sq` are views of two
    more.  `zero_grad()` zeroes the gradient buffer and keeps the views whatever `set_to_none` says.  `param_groups[i]["lr"]`
    edits, `lr_scheduler.step()` and `add_param_group` work as with torch's class; `state_dict()` / `load_state_dict()` use
    torch's layout, so a checkpoint of `torch.optim.AdamW` resumes here and the other way round.

    Differences from torch's class:
      * parameters must be fp32 and stay where they were homed: after `module.to(...)` / `.float()` the next `step()` raises
        ValueError naming the parameter (construct the optimiser after the last move);
      * torch skips a parameter whose gradient is None (no decay, no moment update); here a trainable parameter without a
        gradient is stepped with a ZERO gradient.  `training._backward_and_step` turns None into zeros before the step anyway,
        so the three training steps see no difference.  A parameter with requires_grad=False is skipped, as in torch;
      * a gradient that is not the optimiser's own view (`GradientBuckets._write_back` or a caller assigned a fresh tensor) is
        copied into the view first;
      * betas, eps, lr and weight_decay reach the kernel as fp32; the bias corrections 1 - beta^t are computed in double from
        the fp32 betas, so that the step is the exact AdamW of those (rounded) hyper-parameters.  Each operation is rounded as
        torch's single-tensor path rounds it on the device: with fp32-representable hyper-parameters the tests find no bit of p,
        exp_avg or exp_avg_sq that differs from `torch.optim.AdamW(foreach=False, fused=False)`;
      * every step bumps the version counter of every updated parameter (the kernel writes through a raw pointer): values
        cached on `p._version` (ctrlv_amd.frozen) are rebuilt after a step;
      * `step(max_grad_norm=...)` skips a step whose gradient norm is not finite ON THE DEVICE, and the host cannot know
        without a read: `state[p]["step"]` and the bias corrections count ATTEMPTED steps, skipped ones included
        (`grad_state()["skipped_total"]` tells how many those were).

    `step(ema=ema_model)` fuses the shadow update of a `ctrlv_amd.optim.EMAModel` into the same pass (replaces the
    `ema_unet.step(unet.parameters())` line that follows `optimizer.step()`).

    `step(max_grad_norm=x)` clips the gradients to a global L2 norm of x first, as `accelerator.clip_grad_norm_(params, x)` in
    front of `optimizer.step()` does (`torch.nn.utils.clip_grad_norm_`: one norm over every trainable parameter of every
    group; frozen parameters and padding do not take part): one more read of the gradient buffers sums their squares in
    fp64 (`ctrlv_grad_sumsq`), one small launch forms norm, coefficient and skip flag on the device (`ctrlv_grad_finish`), and
    the AdamW pass multiplies each gradient by the coefficient as it reads it (`ctrlv_adamw_step_dev`).  The gradient buffers
    are not written and nothing is read back; `grad_state()` hands out the record.  A norm that is not finite (an inf or NaN
    gradient) leaves parameters and moments untouched; an attached EMA still averages the unchanged parameters, as
    `ema.step()` after a skipped `optimizer.step()` would.  `max_grad_norm=math.inf` computes norm and flag without clipping;
    None (the default) is the plain step, with no norm at all.

    `step(scaler=loss_scaler)` (a `ctrlv_amd.optim.LossScaler`; what `LossScaler.step(optimizer)` calls) is the step of a
    loss-scaled backward: always the three stages, with the last two in their scaled forms (`ctrlv_grad_finish_scaled`,
    `ctrlv_adamw_step_scaled`).  The finish launch forms the unscale multiplier from the scale on the device, takes norm,
    coefficient and skip flag of the UNSCALED gradients, and updates the scale (backoff on a skip, growth after
    `growth_interval` good steps); the AdamW pass multiplies each gradient by multiplier and coefficient as it reads it.  Without
    `max_grad_norm` the norm is taken without clipping (max_norm = +inf): a loss-scaled step costs the one extra read of the
    gradients that clipping costs, and clipping on top of it costs nothing more.  `grad_scale` stays a host multiplier folded into
    the unscale (the 1 / steps of gradient accumulation); `grad_state()` works as for a clipped step.  The gradient buffers are NOT
    written: `.grad` stays SCALED after the step, unlike after torch's `unscale_`.  Step counts stay ATTEMPTED steps:
    `torch.amp.GradScaler` does not count a skipped step, so after k skips the bias corrections here are those of step t + k."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if not math.isfinite(lr) or lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not eps > 0.0:
            raise ValueError(f"Invalid epsilon value: {eps} (must be positive)")
        if not math.isfinite(weight_decay) or weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys torch's own class keeps per group (amsgrad, maximize, foreach, ... at their defaults): a state dict written
        # here then loads into torch.optim.AdamW of the installed version, whatever keys that version reads
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self._flat = []
        self._ema = None
        self._max_grad_norm = None  # clip_grad_norm(): the default of step(max_grad_norm=None)
        self._grad_state = None     # device record of step(max_grad_norm=...): ctrlv_grad_state as four 32-bit words
        self._partials = None       # fp64 partial sums of squares of all groups; dropped (regrown) by add_param_group
        super().__init__(params, defaults)

    # ---- layout
    def add_param_group(self, param_group):
        if not isinstance(param_group, dict):
            raise TypeError(f"param_group must be a dict, got {type(param_group).__name__}")
        params = param_group["params"]
        params = [params] if isinstance(params, torch.Tensor) else list(params)
        param_group = dict(param_group, params=params)
        if param_group.get("amsgrad") or param_group.get("maximize"):
            raise ValueError("ctrlv_amd.optim.AdamW: amsgrad and maximize are not implemented")
        tensors = [x[1] if isinstance(x, tuple) else x for x in params]
        for i, p in enumerate(tensors):
            what = f"parameter {i} of the new group, shape {tuple(p.shape)},"
            if p.dtype != torch.float32 or p.device != tensors[0].device or p.is_sparse:
                raise ValueError(f"ctrlv_amd.optim.AdamW: {what} is {p.dtype} on {p.device}; the flat buffers hold dense fp32 "
                                 "parameters of one device (`model.float()` first: fp32 masters)")
            home = home_of(p)
            if home is not None and home[0] is not self:
                raise ValueError(f"ctrlv_amd.optim.AdamW: {what} is already homed in another ctrlv_amd.optim.AdamW")
        super().add_param_group(param_group)                 # (refuses a parameter that is already in one of this optimiser's groups)
        params = self.param_groups[-1]["params"]
        flat = _Flat(params)
        gi = len(self._flat)
        with torch.no_grad():
            for i, p in enumerate(params):
                home = flat.view(flat.p, i, p)
                home.copy_(p.detach())
                p.data = home
                gv = flat.view(flat.g, i, p)
                if p.grad is not None:
                    gv.copy_(p.grad)
                if p.requires_grad:
                    p.grad = gv
                _set_home(p, self, gi, i)
        self._flat.append(flat)
        self._partials = None

    def attach_ema(self, ema):
        """Every later `step()` carries `ema` (a `ctrlv_amd.optim.EMAModel`, or None to detach) as `step(ema=ema)` would: for
        callers that do not make the `step()` call themselves (`training.unet_train_step(unet, batch, optimizer)`)."""
        self._ema = ema
        return self

    def clip_grad_norm(self, max_grad_norm):
        """Every later `step()` without a `max_grad_norm` of its own clips to this global norm, as `step(max_grad_norm=...)` would
        (None: no clipping again): for callers that do not make the `step()` call themselves and whose step function takes no such
        argument (`training.vae_train_step(vae, batch, optimizer)`)."""
        if max_grad_norm is not None and not _f32(max_grad_norm) > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (must be positive; math.inf: the norm without clipping)")
        self._max_grad_norm = max_grad_norm
        return self

    def flat_buffers(self, group_index):
        """(parameters, gradients, exp_avg, exp_avg_sq, offsets) of a group: the flat fp32 buffers and each parameter's offset."""
        f = self._flat[group_index]
        return f.p, f.g, f.m, f.v, list(f.offsets)

    def _name(self, gi, i):
        group = self.param_groups[gi] if gi < len(self.param_groups) else None
        names = group.get("param_names") if group else None
        p = group["params"][i] if group else None
        shape = f" of shape {tuple(p.shape)}" if p is not None else ""
        return (f"parameter '{names[i]}'" if names else f"parameter {i} of group {gi}") + shape

    def _check_home(self, gi, i, p):
        flat = self._flat[gi]
        if p.dtype != torch.float32 or p.data_ptr() != flat.p.data_ptr() + 4 * flat.offsets[i] or not p.is_contiguous():
            raise ValueError(f"ctrlv_amd.optim.AdamW.step: {self._name(gi, i)} ({p.dtype}, {p.device}) no longer lives in its "
                             "group's flat buffer -- it was moved or cast (`.to()`, `.float()`, a `.data` assignment) after the "
                             "optimiser was built; build the optimiser after the last move")

    # ---- torch.optim.Optimizer surface
    def zero_grad(self, set_to_none=True):
        """Zeroes the flat gradient buffers; the `.grad` views stay (set_to_none is accepted and ignored)."""
        for gi, group in enumerate(self.param_groups):
            flat = self._flat[gi]
            flat.g.zero_()
            for i, p in enumerate(group["params"]):
                if p.requires_grad and (p.grad is None or p.grad.data_ptr() != flat.g.data_ptr() + 4 * flat.offsets[i]):
                    p.grad = flat.view(flat.g, i, p)

    def _own_gradients(self, gi, group):
        """A gradient that is not the optimiser's view is copied into it (None: zeros), and the view becomes `.grad` again."""
        flat = self._flat[gi]
        for i, p in enumerate(group["params"]):
            if not p.requires_grad:
                continue
            g = p.grad
            if g is not None and g.data_ptr() == flat.g.data_ptr() + 4 * flat.offsets[i] and g.dtype == torch.float32:
                continue
            gv = flat.view(flat.g, i, p)
            if g is None:
                gv.zero_()
            else:
                gv.copy_(g)
            p.grad = gv

    def _runs(self, gi, group):
        """Maximal runs of consecutive trainable parameters with the same step count: [(first, last, steps done)].  One run per
        group unless a parameter is frozen or joined later."""
        runs = []
        for i, p in enumerate(group["params"]):
            if not p.requires_grad:
                continue
            st = self.state[p]
            if "step" not in st:
                flat = self._flat[gi]
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = flat.view(flat.m, i, p)
                st["exp_avg_sq"] = flat.view(flat.v, i, p)
            t = int(st["step"])
            if runs and runs[-1][1] == i - 1 and runs[-1][2] == t:
                runs[-1][1] = i
            else:
                runs.append([i, i, t])
        return runs

    @torch.no_grad()
    def step(self, closure=None, ema=None, grad_scale=1.0, max_grad_norm=None, scaler=None):
        if scaler is not None and not isinstance(scaler, LossScaler):
            raise TypeError(f"ctrlv_amd.optim.AdamW.step: scaler must be a ctrlv_amd.optim.LossScaler, not {type(scaler).__name__} "
                            "(the scale is read and updated on the device; there is no host-read route)")
        if scaler is not None and not scaler.is_enabled():
            scaler = None
        if max_grad_norm is None:
            max_grad_norm = self._max_grad_norm                                      # (None unless clip_grad_norm() set one)
        if max_grad_norm is not None and not _f32(max_grad_norm) > 0.0:             # (false for NaN too) before any device work
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (must be positive; math.inf: the norm without clipping)")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if ema is None:
            ema = self._ema
        ema_decay = ema._begin_fused_step(self) if ema is not None else 0.0
        if max_grad_norm is not None or scaler is not None:
            self._step_clipped(ema, ema_decay, float(grad_scale), math.inf if max_grad_norm is None else float(max_grad_norm), scaler)
            if ema is not None:
                ema._end_fused_step(self)
            return loss
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            flat = self._flat[gi]
            lib = _lib_for_device(flat.p)
            for i, p in enumerate(params):
                self._check_home(gi, i, p)
            self._own_gradients(gi, group)
            lr, wd, eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
            b1, b2 = _f32(group["betas"][0]), _f32(group["betas"][1])
            shadow = ema._shadow_flat(self, gi) if ema is not None else None
            for first, last, t in self._runs(gi, group):
                off = flat.offsets[first]
                n = flat.offsets[last] + params[last].numel() - off
                bias1, bias2 = 1.0 - b1 ** (t + 1), 1.0 - b2 ** (t + 1)
                _lib.check(lib.ctrlv_adamw_step(_ptr(flat.p, off), _ptr(flat.g, off), _ptr(flat.m, off), _ptr(flat.v, off),
                                                _ptr(shadow, off) if shadow is not None else None, n, lr, b1, b2, eps, wd,
                                                bias1, bias2, float(grad_scale), ema_decay, _stream()), "ctrlv_adamw_step", lib)
                for p in params[first:last + 1]:
                    self.state[p]["step"] += 1
            # the kernel wrote through raw pointers: bump each updated parameter's version (a Parameter whose .data was
            # assigned does not share its counter with the flat base), so that values cached on it are rebuilt
            torch.autograd.graph.increment_version([p for p in params if p.requires_grad])
        if ema is not None:
            ema._end_fused_step(self)
        return loss

    def _step_clipped(self, ema, ema_decay, grad_scale, max_grad_norm, scaler=None):
        """`step(max_grad_norm=...)`: the sum of squares of every run of every group into one partials array, one finish, then
        `ctrlv_adamw_step_dev` per run, all on the current stream and without a host read.  With a scaler: the scaled finish and
        `ctrlv_adamw_step_scaled`, which read the unscale multiplier from the scaler's device record."""
        plan, dev, lib = [], None, None
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            flat = self._flat[gi]
            lib = _lib_for_device(flat.p)
            if dev is None:
                dev = flat.p.device
            elif flat.p.device != dev:
                raise ValueError(f"ctrlv_amd.optim.AdamW.step: max_grad_norm takes ONE norm over all groups, and group {gi} lives on "
                                 f"{flat.p.device}, not on {dev}")
            for i, p in enumerate(params):
                self._check_home(gi, i, p)
            self._own_gradients(gi, group)
            plan.append((gi, group, flat, [(flat.offsets[first], flat.offsets[last] + params[last].numel() - flat.offsets[first],
                                            first, last, t) for first, last, t in self._runs(gi, group)]))
        if not any(runs for _, _, _, runs in plan):
            return
        if self._grad_state is None or self._grad_state.device != dev:
            self._grad_state = torch.zeros(4, dtype=torch.int32, device=dev)          # ctrlv_grad_state: norm, coef, skip, skipped_total
        if self._partials is None or self._partials.device != dev:
            # a run of n elements takes ceil(n / 4096) slots: at most numel // 4096 + 1 + (number of parameters) per group,
            # however the runs fall
            cap = sum(f.numel // 4096 + 1 + len(f.offsets) for f in self._flat)
            self._partials = torch.empty(cap, dtype=torch.float64, device=dev)
        partials, state, slot = self._partials, ctypes.c_void_p(self._grad_state.data_ptr()), 0
        for gi, group, flat, runs in plan:
            for off, n, _, _, _ in runs:
                _lib.check(lib.ctrlv_grad_sumsq(_ptr(flat.g, off), n, ctypes.c_void_p(partials.data_ptr()), partials.numel(), slot,
                                                _stream()), "ctrlv_grad_sumsq", lib)
                slot += lib.ctrlv_grad_sumsq_partials(n)
        if scaler is not None:
            ls = ctypes.c_void_p(scaler._record_on(dev).data_ptr())
            _lib.check(lib.ctrlv_grad_finish_scaled(ctypes.c_void_p(partials.data_ptr()), slot, grad_scale, max_grad_norm, ls, state,
                                                    _stream()), "ctrlv_grad_finish_scaled", lib)
        else:
            _lib.check(lib.ctrlv_grad_finish(ctypes.c_void_p(partials.data_ptr()), slot, grad_scale, max_grad_norm, state, _stream()),
                       "ctrlv_grad_finish", lib)
        for gi, group, flat, runs in plan:
            params = group["params"]
            lr, wd, eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
            b1, b2 = _f32(group["betas"][0]), _f32(group["betas"][1])
            shadow = ema._shadow_flat(self, gi) if ema is not None else None
            for off, n, first, last, t in runs:
                bias1, bias2 = 1.0 - b1 ** (t + 1), 1.0 - b2 ** (t + 1)
                bufs = (_ptr(flat.p, off), _ptr(flat.g, off), _ptr(flat.m, off), _ptr(flat.v, off),
                        _ptr(shadow, off) if shadow is not None else None)
                if scaler is not None:
                    _lib.check(lib.ctrlv_adamw_step_scaled(*bufs, n, lr, b1, b2, eps, wd, bias1, bias2, ema_decay, ls, state, _stream()),
                               "ctrlv_adamw_step_scaled", lib)
                else:
                    _lib.check(lib.ctrlv_adamw_step_dev(*bufs, n, lr, b1, b2, eps, wd, bias1, bias2, grad_scale, ema_decay, state,
                                                        _stream()), "ctrlv_adamw_step_dev", lib)
                for p in params[first:last + 1]:
                    self.state[p]["step"] += 1                      # ATTEMPTED steps: the host does not know about a skip
            torch.autograd.graph.increment_version([p for p in params if p.requires_grad])

    def grad_state(self):
        """The record of the last `step(max_grad_norm=...)` or `step(scaler=...)` as 0-dim DEVICE tensors: `norm` (fp32, of the
        gradients times grad_scale -- under a scaler times the unscale multiplier --, over all groups), `coef` (fp32, what the gradients were multiplied by), `skip` (int32, 1: the norm was not
        finite and the step left parameters and moments alone) and `skipped_total` (int32, skipped steps so far).  No
        synchronisation happens here; the tensors are views of the record, which the next such step overwrites -- read or clone
        them when convenient (with the loss, at logging time)."""
        s = self._grad_state
        if s is None:
            raise RuntimeError("ctrlv_amd.optim.AdamW.grad_state: no step(max_grad_norm=...) has run yet")
        return {"norm": s[0].view(torch.float32), "coef": s[1].view(torch.float32), "skip": s[2], "skipped_total": s[3]}

    def load_state_dict(self, state_dict):
        """torch's layout (per-parameter step / exp_avg / exp_avg_sq, param_groups): the moments are copied into the flat
        buffers and become views of them again; `step` is kept on the host."""
        super().load_state_dict(state_dict)
        with torch.no_grad():
            for gi, group in enumerate(self.param_groups):
                flat = self._flat[gi]
                for i, p in enumerate(group["params"]):
                    st = self.state.get(p)
                    if not st:
                        continue
                    for key, buf in (("exp_avg", flat.m), ("exp_avg_sq", flat.v)):
                        view = flat.view(buf, i, p)
                        view.copy_(st[key])
                        st[key] = view
                    st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------ loss scale
class LossScaler:
    """Dynamic loss scaling with the scale ON THE DEVICE: the surface of `torch.amp.GradScaler` that a training loop uses,

        scaler.scale(loss).backward();  scaler.step(optimizer);  scaler.update()

    for a `ctrlv_amd.optim.AdamW`.  The scale, its reciprocal and the growth tracker live in a 32-byte device record
    (`ctrlv_loss_scale_state`, include/ctrlv_hip.h); the optimiser's finish launch unscales, decides the skip and applies
    torch's `_amp_update_scale_` there (skip: scale *= backoff_factor; `growth_interval` unskipped steps in a row: scale *=
    growth_factor unless that overflows), so no step reads the device.  The two factors are held as fp32 in the record (torch
    keeps doubles: 2 and 0.5, or any fp32 number, behave identically).

      * `scale(loss)` multiplies by a 0-dim device view of the scale (the record is created on `loss.device` at first use);
      * `step(optimizer, **kw)` is `optimizer.step(scaler=self, **kw)`; any optimiser but `ctrlv_amd.optim.AdamW` is a TypeError
        (there is no host-read fallback).  `.grad` is NOT unscaled by it: the gradient buffers keep the scaled values;
      * `update()` does nothing -- the update already happened in the finish launch of `step`;
      * `get_scale()` is a HOST READ (a synchronisation): for logging.  `scale_tensor()` / `growth_tracker_tensor()` hand out
        device views without synchronising;
      * `state_dict()` / `load_state_dict()` use exactly torch's keys (scale, growth_factor, backoff_factor, growth_interval,
        _growth_tracker): a checkpoint moves between this class and `torch.amp.GradScaler` in both directions;
      * `enabled=False` makes every method the identity, as in torch.

    The optimiser counts ATTEMPTED steps (see `AdamW`): GradScaler's optimisers do not count a skipped step."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        if enabled:
            if not growth_factor > 1.0:
                raise ValueError("The growth factor must be > 1.0.")
            if not backoff_factor < 1.0:
                raise ValueError("The backoff factor must be < 1.0.")
        self._enabled = bool(enabled)
        self._init_scale, self._init_growth_tracker = float(init_scale), 0
        self._growth_factor, self._backoff_factor = float(growth_factor), float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._record = None         # int32[8] on the device: ctrlv_loss_scale_state

    @classmethod
    def fixed(cls, scale):
        """A scale that never changes (static loss scaling): a growth interval no run reaches and a backoff factor of 1.  A step
        with non-finite gradients is still skipped on the device."""
        self = cls(init_scale=scale, growth_interval=2 ** 31 - 1)
        self._backoff_factor = 1.0
        return self

    # ---- the record
    def _words(self, scale, tracker):
        return list(struct.unpack("<8i", struct.pack("<ffiiffii", _f32(scale), 0.0, int(tracker), self._growth_interval,
                                                     _f32(self._growth_factor), _f32(self._backoff_factor), 0, 0)))

    def _record_on(self, device):
        """The record on `device`: created from the host values at first use, moved (with its current values) if it lives
        elsewhere."""
        device = torch.device(device)
        if self._record is None:
            self._record = torch.tensor(self._words(self._init_scale, self._init_growth_tracker), dtype=torch.int32).to(device)
        elif self._record.device != device:
            self._record = self._record.to(device)
        return self._record

    def _rewrite(self, scale=None, tracker=None):
        """Host values changed: write them into the record, keeping the fields not named (one host read for those)."""
        if self._record is None:
            return
        cur = self._record.cpu()
        scale = float(cur[0:1].view(torch.float32)) if scale is None else scale
        tracker = int(cur[2]) if tracker is None else tracker
        self._record.copy_(torch.tensor(self._words(scale, tracker), dtype=torch.int32))

    def scale_tensor(self):
        """0-dim fp32 DEVICE view of the scale (None before the record exists); no synchronisation."""
        return None if self._record is None else self._record[0].view(torch.float32)

    def growth_tracker_tensor(self):
        """0-dim int32 DEVICE view of the growth tracker (None before the record exists); no synchronisation."""
        return None if self._record is None else self._record[2]

    # ---- GradScaler's loop surface
    def scale(self, outputs):
        """outputs * scale: a tensor, or a (nested) list / tuple of tensors.  No host read."""
        if not self._enabled:
            return outputs
        if isinstance(outputs, torch.Tensor):
            return outputs * self._record_on(outputs.device)[0].view(torch.float32)
        if isinstance(outputs, (list, tuple)):
            return type(outputs)(self.scale(o) for o in outputs)
        raise ValueError("outputs must be a Tensor or an iterable of Tensors")

    def step(self, optimizer, *args, **kwargs):
        """`optimizer.step(scaler=self, ...)`: unscale, finite check, skip and scale update inside the optimiser's launches."""
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        if not isinstance(optimizer, AdamW):
            raise TypeError(f"ctrlv_amd.optim.LossScaler.step: {type(optimizer).__name__} is not a ctrlv_amd.optim.AdamW -- the "
                            "scale lives on the device and only that optimiser reads it there (use torch.amp.GradScaler for others)")
        return optimizer.step(*args, scaler=self, **kwargs)

    def update(self, new_scale=None):
        """Nothing to do: the scale was updated on the device by the step.  new_scale (a float or a 1-element tensor) sets it."""
        if not self._enabled or new_scale is None:
            return
        if isinstance(new_scale, torch.Tensor):
            new_scale = float(new_scale)
        if self._record is None:
            self._init_scale = float(new_scale)
        else:
            self._rewrite(scale=float(new_scale))

    def unscale_(self, optimizer):
        raise NotImplementedError("ctrlv_amd.optim.LossScaler: .grad is never rewritten; clip with step(optimizer, max_grad_norm=...), "
                                  "which takes the norm of the unscaled gradients on the device")

    def get_scale(self):
        """The scale as a Python float.  A HOST READ of the device record (it synchronises): for logging."""
        if not self._enabled:
            return 1.0
        return self._init_scale if self._record is None else float(self._record[0:1].cpu().view(torch.float32))

    def _get_growth_tracker(self):
        if not self._enabled:
            return 0
        return self._init_growth_tracker if self._record is None else int(self._record[2])

    def get_growth_factor(self):
        return self._growth_factor

    def set_growth_factor(self, new_factor):
        self._growth_factor = float(new_factor)
        self._rewrite()

    def get_backoff_factor(self):
        return self._backoff_factor

    def set_backoff_factor(self, new_factor):
        self._backoff_factor = float(new_factor)
        self._rewrite()

    def get_growth_interval(self):
        return self._growth_interval

    def set_growth_interval(self, new_interval):
        self._growth_interval = int(new_interval)
        self._rewrite()

    def is_enabled(self):
        return self._enabled

    def state_dict(self):
        """torch.amp.GradScaler's state dict (a host read of scale and tracker); {} when disabled."""
        if not self._enabled:
            return {}
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self._init_scale = float(state_dict["scale"])
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        self._rewrite(scale=self._init_scale, tracker=self._init_growth_tracker)


def loss_scaler_from_option(option):
    """The --loss-scale option of the tools: "none" -> None, "dynamic" -> LossScaler() (torch's defaults), a number -> that
    scale, fixed (`LossScaler.fixed`)."""
    if option is None or str(option).lower() == "none":
        return None
    if str(option).lower() == "dynamic":
        return LossScaler()
    try:
        scale = float(option)
    except ValueError:
        raise ValueError(f"--loss-scale must be none, dynamic or a positive number, not {option!r}") from None
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"--loss-scale must be none, dynamic or a positive number, not {option!r}")
    return LossScaler.fixed(scale)


# ------------------------------------------------------------------------------------------------------------ EMA
def ema_decay_schedule(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0,
                       power=2 / 3):
    """The decay diffusers' EMAModel.get_decay uses at `optimization_step` [DIFF-0.27.2, not in tree]:
    s = max(0, step - update_after_step - 1); 0 for s <= 0; without warm-up (1 + s) / (10 + s), with warm-up
    1 - (1 + s / inv_gamma) ** -power; clipped to [min_decay, decay]."""
    s = max(0, optimization_step - update_after_step - 1)
    if s <= 0:
        return 0.0
    cur = 1 - (1 + s / inv_gamma) ** -power if use_ema_warmup else (1 + s) / (10 + s)
    return max(min(cur, decay), min_decay)


class EMAModel:
    """Exponential moving average of a model's parameters: the surface of `diffusers.training_utils.EMAModel` that the
    reference's stage-1 script uses.  shadow -= (1 - decay) * (shadow - param) after every optimiser step, with diffusers'
    decay schedule (`ema_decay_schedule`); parameters with requires_grad=False are copied.

    Parameters homed in a `ctrlv_amd.optim.AdamW` get shadows that mirror the optimiser's flat layout (whether the EMA or the
    optimiser was built first: the shadows are re-homed on the first step after): `step(parameters)` is then one
    `ctrlv_ema_step` launch per group, and `optimizer.step(ema=self)` does the update inside the AdamW pass.  Every other
    parameter has a per-tensor shadow updated with torch's foreach ops in the same form."""

    def __init__(self, parameters, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0,
                 power=2 / 3, model_cls=None, model_config=None):
        if isinstance(parameters, torch.nn.Module):
            parameters = parameters.parameters()
        parameters = list(parameters)
        self.shadow_params = [p.clone().detach() for p in parameters]
        self._tracked = parameters      # what `AdamW.step(ema=self)` averages; `step(parameters)` replaces the list
        self.temp_stored_params = None
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_ema_warmup, self.inv_gamma, self.power = use_ema_warmup, inv_gamma, power
        self.optimization_step = 0
        self.cur_decay_value = None
        self.model_cls, self.model_config = model_cls, model_config
        self._flats = {}           # (id of the optimiser, group) -> (weakref of the optimiser, flat shadow buffer)
        self._homes = None         # per shadow: (key, index in the group) when it is a view of a flat shadow buffer, else None

    # ---- schedule
    def get_decay(self, optimization_step):
        return ema_decay_schedule(optimization_step, self.decay, self.min_decay, self.update_after_step, self.use_ema_warmup,
                                  self.inv_gamma, self.power)

    # ---- layout
    def _adopt_layout(self, parameters):
        """Re-home the shadow of every parameter that lives in a ctrlv_amd.optim.AdamW into a flat buffer with that group's
        layout (once; checked again on every step because an optimiser may be built or extended after the EMA)."""
        if len(parameters) != len(self.shadow_params):
            raise ValueError(f"EMAModel: {len(parameters)} parameters for {len(self.shadow_params)} shadow parameters")
        homes = []
        for p in parameters:
            h = home_of(p)
            homes.append(None if h is None or not p.is_cuda else ((id(h[0]), h[1]), h[2], h[0]))
        want = [None if h is None else (h[0], h[1]) for h in homes]
        if want == self._homes:
            return
        with torch.no_grad():
            for k, (h, s) in enumerate(zip(homes, self.shadow_params)):
                if h is None:
                    if self._homes is not None and self._homes[k] is not None:
                        self.shadow_params[k] = s.clone()
                    continue
                key, i, opt = h
                flat = opt._flat[key[1]]
                cur = self._flats.get(key)
                if cur is None or cur[0]() is not opt or cur[1].numel() != flat.p.numel():
                    self._flats[key] = (weakref.ref(opt), torch.zeros_like(flat.p))
                view = flat.view(self._flats[key][1], i, parameters[k])
                if view.data_ptr() != s.data_ptr():
                    view.copy_(s)
                    self.shadow_params[k] = view
        self._homes = want

    def _shadow_flat(self, opt, gi):
        hit = self._flats.get((id(opt), gi))
        return hit[1] if hit is not None and hit[0]() is opt else None

    def _advance(self):
        self.optimization_step += 1
        self.cur_decay_value = self.get_decay(self.optimization_step)
        return self.cur_decay_value

    # ---- update
    @torch.no_grad()
    def step(self, parameters):
        if isinstance(parameters, torch.nn.Module):
            parameters = parameters.parameters()
        parameters = self._tracked = list(parameters)
        self._adopt_layout(parameters)
        decay = self._advance()
        done = set()
        for key, (ref, shadow) in self._flats.items():
            opt = ref()
            if opt is None or not any(h is not None and h[0] == key for h in self._homes):
                continue
            flat = opt._flat[key[1]]
            lib = _lib_for_device(shadow)
            _lib.check(lib.ctrlv_ema_step(_ptr(shadow), _ptr(flat.p), flat.numel, decay, _stream()), "ctrlv_ema_step", lib)
            done.add(key)
        for k, h in enumerate(self._homes):                     # frozen parameters inside a flat launch: a copy, as below
            if h is not None and h[0] in done and not parameters[k].requires_grad:
                self.shadow_params[k].copy_(parameters[k])
        self._foreach([k for k, h in enumerate(self._homes) if h is None or h[0] not in done], parameters, decay)

    def _foreach(self, idx, parameters, decay):
        """diffusers' form on per-tensor shadows: s -= (1 - decay) * (s - p) for trainable parameters, a copy for frozen ones."""
        train = [k for k in idx if parameters[k].requires_grad]
        if train:
            s = [self.shadow_params[k] for k in train]
            diff = torch._foreach_sub(s, [parameters[k] for k in train])
            torch._foreach_mul_(diff, 1.0 - decay)
            torch._foreach_sub_(s, diff)
        for k in idx:
            if not parameters[k].requires_grad:
                self.shadow_params[k].copy_(parameters[k])

    def _begin_fused_step(self, opt):
        """`AdamW.step(ema=self)`: adopt the optimiser's layout for the tracked parameters, advance the schedule."""
        if self._tracked is None:
            raise ValueError("EMAModel: step(ema=...) does not know the averaged parameters of an EMA that was loaded with "
                             "from_pretrained -- call ema.step(parameters) once, or build the EMA from the model's parameters")
        self._adopt_layout(self._tracked)
        return self._advance()

    @torch.no_grad()
    def _end_fused_step(self, opt):
        """What the AdamW pass did not cover: parameters outside this optimiser (foreach), frozen parameters inside it (copy)."""
        params, decay = self._tracked, self.cur_decay_value
        rest = []
        for k, (p, h) in enumerate(zip(params, self._homes)):
            if h is None or h[0][0] != id(opt):
                rest.append(k)
            elif not p.requires_grad:
                self.shadow_params[k].copy_(p)
        other = {}
        for k in rest:
            if self._homes[k] is not None:
                other.setdefault(self._homes[k][0], []).append(k)
        for key in other:                                       # homed in ANOTHER ctrlv optimiser: its flat launch
            ref, shadow = self._flats[key]
            o2 = ref()
            lib = _lib_for_device(shadow)
            _lib.check(lib.ctrlv_ema_step(_ptr(shadow), _ptr(o2._flat[key[1]].p), o2._flat[key[1]].numel, decay, _stream()),
                       "ctrlv_ema_step", lib)
        self._foreach([k for k in rest if self._homes[k] is None], params, decay)

    # ---- the rest of diffusers' surface
    @torch.no_grad()
    def copy_to(self, parameters):
        parameters = list(parameters.parameters() if isinstance(parameters, torch.nn.Module) else parameters)
        for s, p in zip(self.shadow_params, parameters):
            p.data.copy_(s.to(p.device).data)
        if parameters:
            torch.autograd.graph.increment_version(parameters)      # `.data` writes bump nothing: cached forms must rebuild

    def store(self, parameters):
        parameters = parameters.parameters() if isinstance(parameters, torch.nn.Module) else parameters
        self.temp_stored_params = [p.detach().cpu().clone() for p in parameters]

    @torch.no_grad()
    def restore(self, parameters):
        if self.temp_stored_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        parameters = list(parameters.parameters() if isinstance(parameters, torch.nn.Module) else parameters)
        for c, p in zip(self.temp_stored_params, parameters):
            p.data.copy_(c.data)
        if parameters:
            torch.autograd.graph.increment_version(parameters)
        self.temp_stored_params = None

    def to(self, device=None, dtype=None):
        """Moves the shadows (floating ones take `dtype`).  Flat shadows that move become per-tensor ones and are re-homed on
        the next step if their parameters are still in an optimiser on that device."""
        old = self.shadow_params
        new = [s.to(device=device, dtype=dtype) if s.is_floating_point() else s.to(device=device) for s in old]
        if any(n is not s for n, s in zip(new, old)):
            self.shadow_params = [n.clone() if n is s else n for n, s in zip(new, old)]
            self._flats, self._homes = {}, None
        return self

    def state_dict(self):
        return {"decay": self.decay, "min_decay": self.min_decay, "optimization_step": self.optimization_step,
                "update_after_step": self.update_after_step, "use_ema_warmup": self.use_ema_warmup, "inv_gamma": self.inv_gamma,
                "power": self.power, "shadow_params": self.shadow_params}

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        self.decay = sd.get("decay", self.decay)
        if not 0.0 <= self.decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.min_decay = sd.get("min_decay", self.min_decay)
        self.optimization_step = int(sd.get("optimization_step", self.optimization_step))
        self.update_after_step = int(sd.get("update_after_step", self.update_after_step))
        self.use_ema_warmup = bool(sd.get("use_ema_warmup", self.use_ema_warmup))
        self.inv_gamma = sd.get("inv_gamma", self.inv_gamma)
        self.power = sd.get("power", self.power)
        shadow = sd.get("shadow_params")
        if shadow is not None:
            if len(shadow) != len(self.shadow_params) or any(a.shape != b.shape for a, b in zip(shadow, self.shadow_params)):
                raise ValueError("shadow_params do not match this EMAModel's parameters")
            with torch.no_grad():
                for mine, theirs in zip(self.shadow_params, shadow):      # in place: flat views stay views
                    mine.copy_(theirs)

    _SCALARS = ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power")

    def save_pretrained(self, path):
        """The model with the SHADOW weights through modeling_utils (config.json + weights), the EMA's scalars in the config:
        what the reference's `unet_ema` directory holds."""
        if self.model_cls is None or self.model_config is None:
            raise ValueError("`save_pretrained` can only be used if `model_cls` and `model_config` were given")
        model = self.model_cls.from_config(self.model_config)
        sd = self.state_dict()
        sd.pop("shadow_params")
        model.register_to_config(**sd)
        self.copy_to(model.parameters())
        model.save_pretrained(path)

    @classmethod
    def from_pretrained(cls, path, model_cls):
        with open(os.path.join(str(path), model_cls.config_name)) as f:
            cfg = json.load(f)
        model = model_cls.from_pretrained(path)
        ema = cls(model.parameters(), model_cls=model_cls, model_config=model.config)
        ema.load_state_dict({k: cfg[k] for k in cls._SCALARS if k in cfg})
        ema._tracked = None             # (the loaded model is a carrier of the weights only: it is not kept alive)
        return ema
