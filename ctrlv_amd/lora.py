"""LoRA adapters on the UNet's attention projections (the reference's `--enable_lora`: tools/train_video_diffusion.py:126-136,
205-216, src/ctrlv/utils/parser.py:140-144 -- peft `LoraConfig(r=rank, lora_alpha=rank, init_lora_weights="gaussian",
target_modules=["to_k", "to_q", "to_v", "to_out.0"])` added with `unet.add_adapter`).

An adapted `nn.Linear` keeps its own `weight` / `bias` under their diffusers keys and gains two child modules with peft's
names, so the state dict reads `...to_q.lora_A.default.weight` ([r, Cin]) and `...to_q.lora_B.default.weight` ([N, r]).
The layers are parameter containers here (both executors read the tensors directly), so the adapter never runs as a
branch: every consumer reads the MERGED weight W' = W + (lora_alpha / r) . B . A, built by ctrlv_lora_merge
(csrc/lora.hip) -- the C++ plan through `merged_state_dict`, the per-op executor through `merged_weight`, the training step
through the trailing factor inputs of ctrlv_amd.autograd.Gemm (whose backward forms dA / dB with ctrlv_lora_grad).
"""
import math

import torch
from torch import nn

from . import ops

TARGETS_DEFAULT = ("to_q", "to_k", "to_v", "to_out.0")


def _cfg(config, key, default=None):
    if isinstance(config, dict):
        return config.get(key, default)
    return getattr(config, key, default)


def _matches(name, target):
    """peft's suffix rule: the module name is the target or ends with '.' + target"""
    return name == target or name.endswith("." + target)


def add_adapter(model, config, adapter_name="default"):
    """Inject rank-r factors into every nn.Linear whose name matches a target (suffix match, as peft), freeze every other
    parameter.  Init (peft's LoraLayer.reset_lora_parameters, from knowledge of peft -- it is not a dependency):
    init_lora_weights="gaussian": A ~ N(0, (1/r)^2); True: kaiming_uniform_(A, a=sqrt(5)); B = 0 in both cases."""
    if getattr(model, "_lora", None) is not None:
        raise ValueError(f"an adapter ({model._lora['name']!r}) is already attached; ctrlv_amd supports one adapter")
    r = int(_cfg(config, "r", 8))
    alpha = _cfg(config, "lora_alpha", 8)
    alpha = r if alpha is None else float(alpha)
    dropout = float(_cfg(config, "lora_dropout", 0.0) or 0.0)
    init = _cfg(config, "init_lora_weights", True)
    targets = _cfg(config, "target_modules", None) or TARGETS_DEFAULT
    if isinstance(targets, str):
        targets = [targets]
    if dropout != 0.0:
        raise ValueError("lora_dropout != 0 is not supported (the adapter is merged into the weight, there is no branch to "
                         "drop out)")
    if r <= 0 or r % 4 or r > 64:
        raise ValueError(f"LoRA rank r must be a multiple of 4 in [4, 64] (got {r})")
    if init not in (True, "gaussian"):
        raise ValueError(f"init_lora_weights={init!r} is not supported (True or 'gaussian')")
    found = {t: [] for t in targets}
    for name, mod in model.named_modules():
        if isinstance(mod, nn.Linear):
            for t in targets:
                if _matches(name, t):
                    found[t].append((name, mod))
    missing = [t for t, v in found.items() if not v]
    if missing:
        raise ValueError(f"target_modules {missing} match no nn.Linear of {type(model).__name__}")
    # only the attention projections are read through the merge by BOTH executors and the training forward: a factor on
    # any other layer would never train and would make the two executors disagree
    other = sorted({n for v in found.values() for n, _ in v if not any(_matches(n, t) for t in TARGETS_DEFAULT)})
    if other:
        raise ValueError(f"target_modules match {other[:3]}{'...' if len(other) > 3 else ''}: ctrlv_amd adapts the attention "
                         f"projections {list(TARGETS_DEFAULT)} only")
    adapted = []
    for t in targets:
        for name, lin in found[t]:
            if hasattr(lin, "lora_A"):
                continue
            w = lin.weight
            a = nn.Linear(lin.in_features, r, bias=False, device=w.device, dtype=w.dtype)
            b = nn.Linear(r, lin.out_features, bias=False, device=w.device, dtype=w.dtype)
            with torch.no_grad():
                if init == "gaussian":
                    nn.init.normal_(a.weight, std=1.0 / r)
                else:
                    nn.init.kaiming_uniform_(a.weight, a=math.sqrt(5))
                b.weight.zero_()
            lin.add_module("lora_A", nn.ModuleDict({adapter_name: a}))
            lin.add_module("lora_B", nn.ModuleDict({adapter_name: b}))
            lin.lora_scaling = alpha / r
            lin.lora_adapter = adapter_name
            adapted.append(name)
    object.__setattr__(model, "_lora", dict(name=adapter_name, r=r, lora_alpha=alpha, modules=adapted))
    for p in model.parameters():
        p.requires_grad_(False)
    for f in factor_parameters(model):
        f.requires_grad_(True)
    model._packed = False                       # (drops both executors' packings)
    return model


def factors(linear):
    """(A, B, scale) of an adapted nn.Linear, None for a plain one."""
    if not hasattr(linear, "lora_A"):
        return None
    name = linear.lora_adapter
    return linear.lora_A[name].weight, linear.lora_B[name].weight, linear.lora_scaling


def factor_parameters(model):
    out = []
    for m in model.modules():
        f = factors(m) if isinstance(m, nn.Linear) else None
        if f is not None:
            out += [f[0], f[1]]
    return out


def merged_weight(linear, scale_mult=1.0):
    """The weight every executor uses: W' = W + s . B . A (ctrlv_lora_merge, fp32) in W's dtype, or W itself."""
    f = factors(linear)
    if f is None:
        return linear.weight
    a, b, s = f
    w = linear.weight
    if not w.is_cuda:
        raise RuntimeError("ctrlv_amd: merging a LoRA adapter runs on a HIP device (ctrlv_lora_merge); the model is on "
                           f"{w.device}")
    return ops.lora_merge(w, a, b, s * scale_mult).to(w.dtype)


def merged_state_dict(model):
    """model.state_dict() with every adapted base weight replaced by its merged form and the factor keys dropped: what the
    C++ plan loads (its key lookup is unchanged)."""
    sd = model.state_dict()
    for name, mod in model.named_modules():
        if isinstance(mod, nn.Linear) and factors(mod) is not None:
            a = mod.lora_adapter
            sd[name + ".weight"] = merged_weight(mod).detach()
            sd.pop(f"{name}.lora_A.{a}.weight", None)
            sd.pop(f"{name}.lora_B.{a}.weight", None)
    return sd


def has_adapter(model):
    return getattr(model, "_lora", None) is not None


def fuse(model, lora_scale=1.0):
    """Write W' (scale lora_scale . lora_alpha / r) into the base weights through ctrlv_lora_merge and remove the adapter:
    the model is a plain diffusers-key UNet again (what stage 2's ControlNetModel.from_unet and from_pretrained read)."""
    if not has_adapter(model):
        raise ValueError("fuse_lora: the model has no adapter")
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, nn.Linear) and factors(mod) is not None:
                mod.weight.copy_(merged_weight(mod, lora_scale))
                del mod.lora_A, mod.lora_B
                del mod.lora_scaling, mod.lora_adapter
    object.__setattr__(model, "_lora", None)
    model._packed = False
    return model
