"""`CLIPVisionModelWithProjection` without transformers: the image encoder of SVD (`image_encoder/`, ViT-H/14), whose
`image_embeds` open every pipeline call (pipeline_video_control.py:220) and every step of the reference's two video training
loops (`encode_video_image`, src/ctrlv/utils/util.py:97-125).

Parameters are registered under transformers' state-dict keys (`vision_model.embeddings.class_embedding`,
`vision_model.pre_layrnorm.weight` -- transformers' spelling --, `vision_model.encoder.layers.N.self_attn.q_proj.weight`, ...,
`visual_projection.weight`), in transformers' order, so `image_encoder/model.safetensors` loads by name.  `forward` runs the
HIP executor (clip_vision_hip.py) where it is switched on (CTRLV_CLIP_HIP=1, or =plan for the one-call C plan: opt-in, see there) and serves the call, and the
plain torch forward below otherwise: that one is the CPU path and the checker."""
import json
import os
import types

import torch
import torch.nn.functional as F
from torch import nn

from .modeling_utils import CONFIG_NAME, HipModelMixin

WEIGHTS_NAME = "pytorch_model.bin"
SAFETENSORS_WEIGHTS_NAME = "model.safetensors"


def _act(name):
    if name == "gelu":
        return F.gelu
    if name == "quick_gelu":
        return lambda x: x * torch.sigmoid(1.702 * x)
    raise ValueError(f"CLIPVisionModelWithProjection: hidden_act '{name}' (gelu / quick_gelu)")


class _Embeddings(nn.Module):
    def __init__(self, hidden, image_size, patch):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.randn(hidden))
        self.patch_embedding = nn.Conv2d(3, hidden, kernel_size=patch, stride=patch, bias=False)
        self.position_embedding = nn.Embedding((image_size // patch) ** 2 + 1, hidden)

    def forward(self, pixel_values):
        w = self.patch_embedding.weight
        x = self.patch_embedding(pixel_values.to(w.dtype)).flatten(2).transpose(1, 2)
        cls = self.class_embedding.expand(x.shape[0], 1, -1)
        return torch.cat([cls, x], 1) + self.position_embedding.weight


class _Attention(nn.Module):
    def __init__(self, hidden, heads):
        super().__init__()
        self.num_heads = heads
        self.k_proj = nn.Linear(hidden, hidden)
        self.v_proj = nn.Linear(hidden, hidden)
        self.q_proj = nn.Linear(hidden, hidden)
        self.out_proj = nn.Linear(hidden, hidden)

    def forward(self, x):
        n, s, c = x.shape
        h = self.num_heads
        q, k, v = (p(x).view(n, s, h, c // h).transpose(1, 2) for p in (self.q_proj, self.k_proj, self.v_proj))
        o = F.scaled_dot_product_attention(q, k, v)
        return self.out_proj(o.transpose(1, 2).reshape(n, s, c))


class _MLP(nn.Module):
    def __init__(self, hidden, inter, act):
        super().__init__()
        self.fc1 = nn.Linear(hidden, inter)
        self.fc2 = nn.Linear(inter, hidden)
        self._act = _act(act)

    def forward(self, x):
        return self.fc2(self._act(self.fc1(x)))


class _Layer(nn.Module):
    def __init__(self, hidden, inter, heads, act, eps):
        super().__init__()
        self.self_attn = _Attention(hidden, heads)
        self.layer_norm1 = nn.LayerNorm(hidden, eps=eps)
        self.mlp = _MLP(hidden, inter, act)
        self.layer_norm2 = nn.LayerNorm(hidden, eps=eps)

    def forward(self, x):
        x = x + self.self_attn(self.layer_norm1(x))
        return x + self.mlp(self.layer_norm2(x))


class _Encoder(nn.Module):
    def __init__(self, n, *a):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(*a) for _ in range(n)])


class _VisionTransformer(nn.Module):
    def __init__(self, hidden, inter, layers, heads, image_size, patch, act, eps):
        super().__init__()
        self.embeddings = _Embeddings(hidden, image_size, patch)
        self.pre_layrnorm = nn.LayerNorm(hidden, eps=eps)
        self.encoder = _Encoder(layers, hidden, inter, heads, act, eps)
        self.post_layernorm = nn.LayerNorm(hidden, eps=eps)


class CLIPVisionModelWithProjection(HipModelMixin):
    """Config fields carry transformers' names (CLIPVisionConfig)."""
    _class_name = "CLIPVisionModelWithProjection"

    def __init__(self, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=224,
                 patch_size=32, projection_dim=512, hidden_act="quick_gelu", layer_norm_eps=1e-5):
        super().__init__()
        if hidden_size % num_attention_heads or image_size % patch_size:
            raise ValueError(f"CLIPVisionModelWithProjection: hidden_size {hidden_size} / heads {num_attention_heads}, "
                             f"image_size {image_size} / patch_size {patch_size}")
        _act(hidden_act)
        self.register_to_config(hidden_size=hidden_size, intermediate_size=intermediate_size, num_hidden_layers=num_hidden_layers,
                                num_attention_heads=num_attention_heads, image_size=image_size, patch_size=patch_size,
                                projection_dim=projection_dim, hidden_act=hidden_act, layer_norm_eps=layer_norm_eps)
        self.vision_model = _VisionTransformer(hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, image_size,
                                               patch_size, hidden_act, layer_norm_eps)
        self.visual_projection = nn.Linear(hidden_size, projection_dim, bias=False)

    # ---- forward ---------------------------------------------------------------------------------------------------
    def torch_forward(self, pixel_values):
        """Plain PyTorch: the CPU path and the checker of the HIP executor (same rounding points in a 16-bit dtype)."""
        vm = self.vision_model
        x = vm.pre_layrnorm(vm.embeddings(pixel_values))
        for layer in vm.encoder.layers:
            x = layer(x)
        embeds = self.visual_projection(vm.post_layernorm(x[:, 0]))
        return types.SimpleNamespace(image_embeds=embeds, last_hidden_state=x)

    def forward(self, pixel_values):
        from . import clip_vision_hip
        r = clip_vision_hip.route(self, pixel_values)
        if r != "torch":
            run = clip_vision_hip.encode_plan if r == "plan" else clip_vision_hip.encode
            embeds, hidden = run(self, pixel_values, return_hidden=True)
            return types.SimpleNamespace(image_embeds=embeds, last_hidden_state=hidden)
        return self.torch_forward(pixel_values)

    # ---- (de)serialisation: transformers' file names and config ------------------------------------------------------
    def save_pretrained(self, save_directory, safe_serialization=True, variant=None, **_):
        os.makedirs(save_directory, exist_ok=True)
        cfg = {"architectures": [self._class_name], "model_type": "clip_vision_model"}
        cfg.update(self.config)
        with open(os.path.join(save_directory, CONFIG_NAME), "w") as f:
            json.dump(cfg, f, indent=2, sort_keys=True)
        sd = {k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}
        name = SAFETENSORS_WEIGHTS_NAME if safe_serialization else WEIGHTS_NAME
        if variant:
            stem, ext = name.rsplit(".", 1)
            name = f"{stem}.{variant}.{ext}"
        if safe_serialization:
            from safetensors.torch import save_file
            save_file(sd, os.path.join(save_directory, name), metadata={"format": "pt"})
        else:
            torch.save(sd, os.path.join(save_directory, name))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, variant=None, torch_dtype=None, **_):
        root = str(pretrained_model_name_or_path)
        if subfolder:
            root = os.path.join(root, subfolder)
        cfg_path = os.path.join(root, CONFIG_NAME)
        if not os.path.isfile(cfg_path):
            raise EnvironmentError(f"{cfg_path} not found.  ctrlv_amd loads models from a local directory only (no hub download).")
        with open(cfg_path) as f:
            config = json.load(f)
        config = dict(config.get("vision_config") or {}, **{k: v for k, v in config.items() if k != "vision_config"})
        model = cls.from_config(config)
        cands = []
        for base in (SAFETENSORS_WEIGHTS_NAME, WEIGHTS_NAME):
            if variant:
                stem, ext = base.rsplit(".", 1)
                cands.append(f"{stem}.{variant}.{ext}")
            cands.append(base)
        for name in cands:
            path = os.path.join(root, name)
            if os.path.isfile(path):
                if name.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    sd = load_file(path)
                else:
                    sd = torch.load(path, map_location="cpu", weights_only=True)
                break
        else:
            raise EnvironmentError(f"no weights file ({' / '.join(cands)}) under {root}")
        sd.pop("vision_model.embeddings.position_ids", None)          # a buffer old checkpoints carry: arange(P + 1)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        if missing or unexpected:
            raise ValueError(f"{cls.__name__}.from_pretrained: missing keys {missing[:5]}... unexpected {unexpected[:5]}...")
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        model.eval()
        return model.requires_grad_(False)                            # frozen in every loop of the reference
