"""Writes tests/golden/clip_vectors.npz: transformers' CLIPVisionModelWithProjection (fp32, CPU) on the two seeded configs of
tests/clip_utils.py -- pixel_values, image_embeds and last_hidden_state per config.  Run from the repository root:

    python tests/golden/make_clip_golden.py [--keys]

--keys also prints the state-dict keys transformers creates (what ctrlv_amd/models/clip_vision.py registers)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import clip_utils as U  # noqa: E402


def main():
    out = {}
    for name, (cfg, n, seed) in U.CONFIGS.items():
        m = U.build_transformers(cfg, seed)
        if "--keys" in sys.argv:
            for k, v in m.state_dict().items():
                print(name, k, tuple(v.shape))
        px = U.seeded_pixels(cfg, n, seed)
        with torch.no_grad():
            r = m(pixel_values=px)
        print(f"{name}: image_embeds std {r.image_embeds.std():.3f}  last_hidden_state std {r.last_hidden_state.std():.3f}")
        out[f"{name}_pixel_values"] = px.numpy()
        out[f"{name}_image_embeds"] = r.image_embeds.float().numpy()
        out[f"{name}_last_hidden_state"] = r.last_hidden_state.float().numpy()
    np.savez_compressed(U.GOLDEN, **out)
    print("wrote", U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
