"""`CLIPVisionModelWithProjection.forward` on the HIP kernels: `image_encoder(pixel_values).image_embeds`, the first thing every
pipeline call does (pipeline_video_control.py:220) and every step of the reference's video training loops
(`encode_video_image`, src/ctrlv/utils/util.py:97-125).

Same approach as vae_encoder_hip.py: the module's parameters (transformers' state-dict layout; a transformers module and
ctrlv_amd's own class alike -- everything is reached by attribute name) are executed through the C ABI:

    pixels --clip_patch_rows--> [n P, 640] --gemm--> patch rows --clip_tokens (+class, +position)--> layernorm (pre_layrnorm)
    per layer:  layernorm -> gemm (q|k|v, one launch) -> attention_tokens -> gemm (out_proj, +residual)
                layernorm -> gemm (fc1) -> act_rows -> gemm (fc2, +residual)
    class rows -> layernorm (post_layernorm) -> gemm (visual_projection)

8 launches per layer.  `encode_plan` is the same walk as ONE C call (csrc/clip_plan.hip: ctrlv_clip_forward) with fc1 and the
activation in one launch -- 7 per layer.  The residual trunk stays in the element type (the 16-bit torch module's own storage); out_proj / fc2 add
the residual in the GEMM epilogue (fp32, one rounding)."""
import os

import torch

from .. import ops, packing
from ..frozen import frozen, frozen_module

# The HIP route is the default only where it was measured no slower than the module's torch forward at batch 1 in both
# element types (tools/clip_bench.py).  It was not (profiles/clip_encode_bench.jsonl, one MI355X: 8.1 ms against 6.2 ms in bf16,
# 8.1 against 6.1 in fp16), so the route is OPT-IN: CTRLV_CLIP_HIP=1 selects it, unset / 0 = torch forward.
# The one-call plan (CTRLV_CLIP_HIP=plan, encode_plan) meets that rule in bf16 (6.50 against 6.70 ms) and misses it in fp16 (6.35
# against 6.24), and is the slowest route at 8 images (13.2 ms): opt-in as well.
DEFAULT_ON = False


def enabled():
    v = os.environ.get("CTRLV_CLIP_HIP")
    return DEFAULT_ON if v is None else v != "0"


def route(model=None, pixel_values=None):
    """Which forward serves a call: "torch", "ops" (the per-op executor `encode`: CTRLV_CLIP_HIP=1) or "plan" (`encode_plan`,
    one C call: CTRLV_CLIP_HIP=plan).  With a module and an input, a HIP route is named only where `supports()` holds."""
    if not enabled():
        return "torch"
    if model is not None and not supports(model, pixel_values):
        return "torch"
    return "plan" if os.environ.get("CTRLV_CLIP_HIP") == "plan" else "ops"


def _parts(model):
    """The modules the executor reads, or None when `model` is not a CLIP vision tower with a projection."""
    try:
        vm = model.vision_model
        emb = vm.embeddings
        layers = list(vm.encoder.layers)
        got = (emb.class_embedding, emb.patch_embedding.weight, emb.position_embedding.weight, vm.pre_layrnorm.weight,
               vm.post_layernorm.weight, model.visual_projection.weight)
        for l in layers:
            got += (l.layer_norm1.weight, l.layer_norm2.weight, l.mlp.fc1.weight, l.mlp.fc2.weight, l.self_attn.q_proj.weight,
                    l.self_attn.k_proj.weight, l.self_attn.v_proj.weight, l.self_attn.out_proj.weight)
    except AttributeError:
        return None
    if not layers or any(not isinstance(t, torch.Tensor) for t in got):
        return None
    return vm, emb, layers


def _cfg(model, name, default=None):
    cfg = getattr(model, "config", None)
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


def _heads(model, layer):
    return getattr(layer.self_attn, "num_heads", None) or _cfg(model, "num_attention_heads")


def supports(model, pixel_values):
    """Whether `encode(model, pixel_values)` serves this call: a CLIP vision tower (duck-typed) with 16-bit parameters on a HIP
    device, no gradient wanted, an image of the position table's size, gelu / quick_gelu, and the kernels' size rules --
    hidden and intermediate sizes multiples of 64 (the GEMM's K), hidden <= 2048 (LayerNorm), projection a multiple of 32,
    head_dim a multiple of 16 in [16, 128], at most 4096 tokens."""
    parts = _parts(model)
    if parts is None or not isinstance(pixel_values, torch.Tensor):
        return False
    vm, emb, layers = parts
    w = emb.patch_embedding.weight
    if not (pixel_values.is_cuda and w.is_cuda and w.dtype in (torch.float16, torch.bfloat16)):
        return False
    if pixel_values.dim() != 4 or pixel_values.shape[1] != 3 or pixel_values.shape[0] < 1:
        return False
    if pixel_values.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        return False
    params = list(model.parameters())
    if any(p.dtype != w.dtype or p.device != w.device for p in params):
        return False
    if torch.is_grad_enabled() and (pixel_values.requires_grad or any(p.requires_grad for p in params)):
        return False
    if w.dim() != 4 or w.shape[1] != 3 or w.shape[2] != w.shape[3] or getattr(emb.patch_embedding, "bias", None) is not None:
        return False
    hidden, patch = w.shape[0], w.shape[2]
    H, W = pixel_values.shape[2], pixel_values.shape[3]
    tokens = emb.position_embedding.weight.shape[0]
    if H != W or H % patch or (H // patch) * (W // patch) + 1 != tokens or tokens > 4096:
        return False
    if _cfg(model, "hidden_act") not in ops.ACT_KINDS:
        return False
    heads = _heads(model, layers[0])
    if not heads or hidden % heads:
        return False
    hd = hidden // heads
    inter = layers[0].mlp.fc1.weight.shape[0]
    proj = model.visual_projection.weight.shape[0]
    if hd % 16 or not 16 <= hd <= 128 or hidden % 64 or hidden > 2048 or inter % 64 or proj % 32:
        return False
    if getattr(model.visual_projection, "bias", None) is not None:
        return False
    return all(_heads(model, l) == heads and l.mlp.fc1.weight.shape[0] == inter for l in layers)


def _f32(p):
    return frozen([p], "clip_f32", lambda: p.detach().float().contiguous())


def _lin(p):
    return frozen([p], "clip_linear", lambda: _packed(p, lambda: packing.pack_linear(p)))


def _packed(p, build):
    with packing.element_dtype(p.dtype):
        return build()


def _qkv(a):
    ws = [a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]
    bs = [a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]
    w = frozen(ws, "clip_qkv", lambda: _packed(ws[0], lambda: packing.pack_qkv(*ws)))
    b = frozen(bs, "clip_qkv_bias", lambda: torch.cat([t.detach().float() for t in bs]).contiguous())
    return w, b


def launches(num_layers):
    """Kernel launches of one `encode` call (the torch gather of the class rows not counted)."""
    return 4 + 8 * num_layers + 2


@torch.no_grad()
def encode(model, pixel_values, return_hidden=False):
    """image_embeds [n, projection_dim] in the model's dtype (with return_hidden: also last_hidden_state [n, tokens, hidden],
    the encoder output before post_layernorm, as transformers defines it)."""
    if not supports(model, pixel_values):
        raise ValueError("HIP CLIP encode: unsupported module / input (see clip_vision_hip.supports)")
    vm, emb, layers = _parts(model)
    w = emb.patch_embedding.weight
    el, dev = w.dtype, w.device
    C, patch = w.shape[0], w.shape[2]
    n = pixel_values.shape[0]
    S = emb.position_embedding.weight.shape[0]
    P = S - 1
    M = n * S
    heads = _heads(model, layers[0])
    act = _cfg(model, "hidden_act")

    def rows(m, c):
        return torch.empty(m, c, dtype=el, device=dev)

    # patch embedding: the stride-`patch` convolution without bias = one GEMM over (c, dy, dx) patch rows
    kp = (3 * patch * patch + 63) // 64 * 64
    pr = ops.clip_patch_rows(pixel_values.contiguous(), patch, rows(n * P, kp))
    pe = rows(n * P, C)
    ops.gemm(pr, _lin(w), pe, N=C, cin=kp)
    tok = ops.clip_tokens(pe, _f32(emb.class_embedding), _f32(emb.position_embedding.weight), n, rows(M, C))
    x = ops.layernorm(tok, _f32(vm.pre_layrnorm.weight), _f32(vm.pre_layrnorm.bias), vm.pre_layrnorm.eps, rows(M, C))
    del pr, pe, tok

    inter = layers[0].mlp.fc1.weight.shape[0]
    hn, qkv, att, u, x2 = rows(M, C), rows(M, 3 * C), rows(M, C), rows(M, inter), rows(M, C)
    for l in layers:
        a = l.self_attn
        ops.layernorm(x, _f32(l.layer_norm1.weight), _f32(l.layer_norm1.bias), l.layer_norm1.eps, hn)
        wqkv, bqkv = _qkv(a)
        ops.gemm(hn, wqkv, qkv, N=3 * C, cin=C, bias=bqkv)
        ops.attention_tokens(qkv, att, n, S, C, C // heads)
        ops.gemm(att, _lin(a.out_proj.weight), x2, N=C, cin=C, bias=_f32(a.out_proj.bias), R1=x)
        x, x2 = x2, x
        ops.layernorm(x, _f32(l.layer_norm2.weight), _f32(l.layer_norm2.bias), l.layer_norm2.eps, hn)
        ops.gemm(hn, _lin(l.mlp.fc1.weight), u, N=inter, cin=C, bias=_f32(l.mlp.fc1.bias))
        ops.act_rows(u, act)
        ops.gemm(u, _lin(l.mlp.fc2.weight), x2, N=C, cin=inter, bias=_f32(l.mlp.fc2.bias), R1=x)
        x, x2 = x2, x

    hidden = x.view(n, S, C)
    cls = hidden[:, 0].contiguous()                                 # the class rows: M = n for the projection
    pn = ops.layernorm(cls, _f32(vm.post_layernorm.weight), _f32(vm.post_layernorm.bias), vm.post_layernorm.eps, rows(n, C))
    wp = model.visual_projection.weight
    embeds = rows(n, wp.shape[0])
    ops.gemm(pn, _lin(wp), embeds, N=wp.shape[0], cin=C)
    return (embeds, hidden) if return_hidden else embeds


def plan_launches(num_layers):
    """Kernels of one `encode_plan` call (plus one memset node and one strided copy node)."""
    return 4 + 7 * num_layers + 2


def _plan(model):
    """The module's ClipPlan, kept while every parameter keeps its version, storage and dtype (frozen.frozen_module: the plan
    has no gradient path, so a module whose parameters require grad is cached as well -- rebuilding it is 1.3 GB of packing)."""
    from ..plan import ClipPlan

    def build():
        vm, emb, layers = _parts(model)
        w = emb.patch_embedding.weight
        ln = vm.pre_layrnorm
        cfg = dict(hidden_size=w.shape[0], intermediate_size=layers[0].mlp.fc1.weight.shape[0], num_hidden_layers=len(layers),
                   num_attention_heads=_heads(model, layers[0]), patch_size=w.shape[2],
                   image_size=int(round((emb.position_embedding.weight.shape[0] - 1) ** 0.5)) * w.shape[2],
                   projection_dim=model.visual_projection.weight.shape[0], hidden_act=_cfg(model, "hidden_act"),
                   layer_norm_eps=ln.eps)
        plan = ClipPlan(cfg, w.device, w.dtype)
        plan.load_state_dict({k: v for k, v in model.state_dict().items() if not k.endswith("position_ids")})
        return plan
    return frozen_module(model, "clip_plan", build)


@torch.no_grad()
def encode_plan(model, pixel_values, return_hidden=False):
    """`encode` through the C plan: one ctrlv_clip_forward call on the module's cached ClipPlan (same gate, same outputs)."""
    if not supports(model, pixel_values):
        raise ValueError("HIP CLIP encode: unsupported module / input (see clip_vision_hip.supports)")
    eps = {l.eps for l in _norms(model)}
    if len(eps) != 1:
        raise ValueError("HIP CLIP encode_plan: the plan takes ONE layer_norm_eps")
    return _plan(model).forward(pixel_values, return_hidden=return_hidden)


def _norms(model):
    vm, _, layers = _parts(model)
    return [vm.pre_layrnorm, vm.post_layernorm] + [n for l in layers for n in (l.layer_norm1, l.layer_norm2)]
