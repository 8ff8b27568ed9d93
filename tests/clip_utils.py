"""Shared by tests/golden/make_clip_golden.py, tests/test_clip_cpu.py and tests/test_clip_gpu.py: the CLIP vision configs under
test and the seeded weight rule (the fixture tests/golden/clip_vectors.npz stores transformers' outputs for exactly these)."""
import math
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_vectors.npz")

# A: head_dim 80 (ViT-H's), 17 tokens, erf-GELU, 3 images.  B: head_dim 64, 26 tokens, quick-GELU, 1 image.
CONFIG_A = dict(hidden_size=320, intermediate_size=640, num_hidden_layers=2, num_attention_heads=4, image_size=56, patch_size=14,
                projection_dim=64, hidden_act="gelu", layer_norm_eps=1e-5)
CONFIG_B = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=70, patch_size=14,
                projection_dim=64, hidden_act="quick_gelu", layer_norm_eps=1e-5)
CONFIGS = {"A": (CONFIG_A, 3, 11), "B": (CONFIG_B, 1, 12)}          # name -> (config, images, seed)
# SVD's image encoder (laion CLIP ViT-H/14)
CONFIG_VIT_H = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, image_size=224,
                    patch_size=14, projection_dim=1024, hidden_act="gelu", layer_norm_eps=1e-5)


def seeded_state_dict(model, seed):
    """fp32 tensors for every key of `model.state_dict()`, drawn in state-dict order from ONE generator: matrices (and the
    patch convolution) uniform +-1/sqrt(fan_in), q_proj / k_proj x 3 (so that the softmax is not flat); norm weights 1 + 0.1
    randn, norm biases 0.1 randn; every other vector 0.1 randn."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in model.state_dict().items():
        if k.endswith("position_ids"):
            continue
        shape = tuple(v.shape)
        is_norm = "norm" in k.split(".")[-2]
        if len(shape) >= 2 and not is_norm:
            fan_in = math.prod(shape[1:])
            t = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
            if ".q_proj." in k or ".k_proj." in k:
                t = t * 3
        elif is_norm and k.endswith("weight"):
            t = 1 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.1 * torch.randn(shape, generator=g)
        out[k] = t
    return out


def seeded_pixels(config, n, seed):
    s = config["image_size"]
    return torch.randn(n, 3, s, s, generator=torch.Generator().manual_seed(seed + 1000))


def build_own(config, seed, dtype=torch.float32, device="cpu"):
    from ctrlv_amd.models import CLIPVisionModelWithProjection
    m = CLIPVisionModelWithProjection(**config)
    m.load_state_dict(seeded_state_dict(m, seed))
    return m.to(device=device, dtype=dtype).eval().requires_grad_(False)


def build_transformers(config, seed):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**config))
    missing, unexpected = m.load_state_dict(seeded_state_dict(m, seed), strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return m.eval().requires_grad_(False)


def load_golden():
    import numpy as np
    z = np.load(GOLDEN)
    return {name: {f: torch.from_numpy(z[f"{name}_{f}"]) for f in ("pixel_values", "image_embeds", "last_hidden_state")}
            for name in CONFIGS}
