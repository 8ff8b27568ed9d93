"""The whole-clip driver (include/ctrlv_hip.h: ctrlv_pipeline_*, csrc/pipeline.hip) where no GPU is needed: the symbols, the
host-side validation of ctrlv_pipeline_create and of a `ctrlv_clip_request` -- every refusal names its field and comes before
anything would be launched --, and the pure route predicate of the pipelines.

The workspace SIZE of a request is the sum of the borrowed plans' own workspace answers, and those exist only for plans whose
weights are loaded (ctrlv_plan_workspace_bytes: "not loaded"), which needs a device: the too-small-workspace refusal and the
monotonicity of ctrlv_pipeline_workspace_bytes are checked in tests/test_pipeline_plan_gpu.py
(test_workspace_bytes_and_the_too_small_workspace)."""
import ctypes

import pytest
import torch

import __graft_entry__ as g

NEW = ("ctrlv_resize_antialias", "ctrlv_pixels_prepare", "ctrlv_frames_to_u8", "ctrlv_pipeline_create",
       "ctrlv_pipeline_set_overlap", "ctrlv_pipeline_workspace_bytes", "ctrlv_pipeline_generate", "ctrlv_pipeline_destroy")
CLIP_CFG = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=128, patch_size=16,
                projection_dim=64, hidden_act="gelu", layer_norm_eps=1e-5)
VAE_CFG = dict(in_channels=3, out_channels=3, latent_channels=4, layers_per_block=2, block_out_channels=(128, 256, 512, 512),
               scaling_factor=0.18215)


@pytest.fixture(scope="module")
def libs():
    g.build()
    from ctrlv_amd import _lib
    return {torch.bfloat16: _lib.load(torch.bfloat16), torch.float16: _lib.load(torch.float16)}


@pytest.fixture(scope="module")
def plans(libs):
    """Unloaded plans of the tiny models in the bf16 library: create needs no GPU."""
    import ctrlv_ref as R
    from ctrlv_amd.plan import ClipPlan, Plan, VaePlan
    cfg = dict(R.TINY_CONFIG)
    ccfg = {k: v for k, v in cfg.items() if k not in ("out_channels", "up_block_types")}
    return Plan("unet", cfg, "cpu"), Plan("controlnet", ccfg, "cpu"), VaePlan(VAE_CFG, "cpu"), ClipPlan(CLIP_CFG, "cpu")


def _create(lib, unet, cn, vae, clip):
    h = ctypes.c_void_p()
    rc = lib.ctrlv_pipeline_create(unet._h if unet else None, cn._h if cn else None, vae._h if vae else None,
                                   clip._h if clip else None, 0, ctypes.byref(h))
    return rc, h


def test_both_libraries_export_the_new_symbols_at_abi_22(libs):
    from ctrlv_amd import _lib
    for dt, lib in libs.items():
        assert lib.ctrlv_abi_version() == 22 == _lib.ABI_VERSION
        for name in NEW:
            assert name in _lib.SIGNATURES and getattr(lib, name) is not None, (dt, name)


def test_create_rejects_a_null_plan_and_accepts_a_null_controlnet(libs, plans):
    from ctrlv_amd import _lib
    lib = libs[torch.bfloat16]
    unet, cn, vae, clip = plans
    for args, word in (((None, cn, vae, clip), "UNet"), ((unet, cn, None, clip), "VAE"), ((unet, cn, vae, None), "CLIP")):
        rc, h = _create(lib, *args)
        assert rc == -1 and not h.value and word in _lib.last_error(lib), (word, _lib.last_error(lib))
    rc, h = _create(lib, cn, cn, vae, clip)                    # a ControlNet plan is not a UNet plan
    assert rc == -1 and "UNet plan" in _lib.last_error(lib)
    for args in ((unet, None, vae, clip), (unet, cn, vae, clip)):
        rc, h = _create(lib, *args)
        assert rc == 0 and h.value, _lib.last_error(lib)
        assert lib.ctrlv_pipeline_set_overlap(h, 0) == 0 and lib.ctrlv_pipeline_set_overlap(h, 1) == 0
        assert lib.ctrlv_pipeline_set_overlap(h, 2) == -1
        assert lib.ctrlv_pipeline_destroy(h) == 0
    assert lib.ctrlv_pipeline_destroy(None) == 0


def _request(_lib, keep, **over):
    """A request every field of which passes validation (pointers are never dereferenced on the host except sigmas /
    timesteps, which are host arrays)."""
    r = _lib.ClipRequest()
    r.n_clips, r.num_frames, r.height, r.width = 1, 3, 128, 192
    r.image_u8, r.cond, r.cond_channels, r.cond_dtype = 0x1000, 0x2000, 3, 0
    r.noise_aug_strength, r.num_steps = 0.02, 2
    r.latents, r.out_latents = 0x3000, 0x4000
    sig = (ctypes.c_float * 3)(*over.pop("sigmas", (700.0, 5.0, 0.0)))
    ts = (ctypes.c_float * 2)(1.6, 0.4)
    keep += [sig, ts]
    r.sigmas, r.timesteps = sig, ts
    r.fps, r.motion_bucket_id = 7, 127
    r.min_guidance, r.max_guidance, r.conditioning_scale, r.decode_chunk = 1.0, 3.0, 1.0, 2
    r.out_frames_u8 = 0x5000
    for k, v in over.items():
        setattr(r, k, v)
    return r


def test_a_bad_request_is_refused_by_name_before_anything_else(libs, plans):
    """generate and workspace_bytes alike; the valid request reaches the next gate ("not loaded": these plans have no
    weights), which proves that every field check sits in front of it."""
    from ctrlv_amd import _lib
    lib = libs[torch.bfloat16]
    unet, cn, vae, clip = plans
    rc, h = _create(lib, unet, cn, vae, clip)
    assert rc == 0
    rc, h_svd = _create(lib, unet, None, vae, clip)
    assert rc == 0
    keep = []
    ws = ctypes.c_void_p(0x100000)

    def refused(r, word, pipe=h):
        assert lib.ctrlv_pipeline_workspace_bytes(pipe, ctypes.byref(r)) == 0
        m1 = _lib.last_error(lib)
        rc = lib.ctrlv_pipeline_generate(pipe, ctypes.byref(r), ws, 1 << 40, None)
        m2 = _lib.last_error(lib)
        assert rc < 0 and word in m1 and word in m2, (word, rc, m1, m2)
        return rc

    refused(_request(_lib, keep), "not loaded")
    refused(_lib.ClipRequest(), "n_clips")                                     # a cleared request
    refused(_request(_lib, keep, num_frames=33), "num_frames")
    refused(_request(_lib, keep, cond=None), "cond is null")
    refused(_request(_lib, keep, cond=None), "not loaded", pipe=h_svd)         # ... fine without a ControlNet
    for ch in (0, 1, 5, 8):
        refused(_request(_lib, keep, cond_channels=ch), "cond_channels")
    refused(_request(_lib, keep, cond_channels=4), "not loaded")
    refused(_request(_lib, keep, cond_dtype=3), "cond_dtype")
    m = 8 * 2 ** (unet._cfg.n_blocks - 1)                                      # 8 for the VAE times the UNet's levels
    refused(_request(_lib, keep, height=128 + m // 2), "height")
    refused(_request(_lib, keep, width=192 + 8), "width")
    refused(_request(_lib, keep, height=0), "height")
    refused(_request(_lib, keep, sigmas=(5.0, 5.0, 0.0)), "sigmas")            # not decreasing
    refused(_request(_lib, keep, sigmas=(5.0, 7.0, 0.0)), "sigmas")
    refused(_request(_lib, keep, sigmas=(5.0, 0.0, 0.0)), "sigmas")            # a zero sigma in front of the last
    refused(_request(_lib, keep, num_steps=0), "num_steps")
    refused(_request(_lib, keep, decode_chunk=0), "decode_chunk")
    refused(_request(_lib, keep, image_u8=None), "image_u8")
    refused(_request(_lib, keep, latents=None), "latents")
    refused(_request(_lib, keep, out_latents=None), "out_latents")
    refused(_request(_lib, keep, height=2048, width=2048), "latent pixels")    # the VAE attention's limit
    assert lib.ctrlv_pipeline_generate(h, None, ws, 1 << 40, None) == -1 and "null request" in _lib.last_error(lib)
    assert lib.ctrlv_pipeline_destroy(h) == 0 and lib.ctrlv_pipeline_destroy(h_svd) == 0


def test_resize_host_validation(libs):
    """ks // 2 >= H or W (reflect padding undefined) and a factor above 8 are shape errors of the host, through
    ctrlv_last_error; so is an output dtype that is not fp32 or the library's element type."""
    from ctrlv_amd import _lib
    for dt, lib in libs.items():
        code = 2 if dt == torch.bfloat16 else 1
        p = ctypes.c_void_p(0x1000)
        call = lambda H, W, h, w, dd=0: lib.ctrlv_resize_antialias(p, 0, 1, H, W, p, dd, h, w, None, None, None)   # noqa: E731
        assert call(64, 513, 8, 64) == -2 and "factor above 8" in _lib.last_error(lib)
        assert call(513, 64, 64, 8) == -2 and "factor above 8" in _lib.last_error(lib)
        assert call(1, 16, 1, 16) == -2 and "reflect" in _lib.last_error(lib)          # ks = 3: one row of padding, H = 1
        assert call(16, 1, 16, 1) == -2 and "reflect" in _lib.last_error(lib)
        assert call(64, 64, 32, 32, 3 - code) == -4 and "dtype" in _lib.last_error(lib)
        assert call(0, 64, 32, 32) == -2


def test_the_route_predicate_is_pure_host_logic():
    from PIL import Image
    from ctrlv_amd.pipelines.pipeline_utils import pipeline_route
    im = Image.new("RGB", (16, 8))
    on = {"CTRLV_PIPELINE": "plan"}
    assert pipeline_route(im, None, "pil", True, env=on) == "plan"
    assert pipeline_route([im, im], None, "latent", lambda: True, env=on) == "plan"
    for ot in ("np", "pt", "pil", "latent"):
        assert pipeline_route(im, None, ot, True, env=on) == "plan"
    asked = []
    serve = lambda: (asked.append(1), True)[1]        # noqa: E731
    assert pipeline_route(im, None, "pil", serve, env={}) == "python"                       # unset: as today
    assert pipeline_route(im, None, "pil", serve, env={"CTRLV_PIPELINE": "1"}) == "python"
    assert pipeline_route(im, lambda *a: {}, "pil", serve, env=on) == "python"              # a per-step callback
    assert pipeline_route(torch.zeros(1, 3, 8, 16), None, "pil", serve, env=on) == "python"  # a tensor image
    assert pipeline_route([im, torch.zeros(3, 8, 16)], None, "pil", serve, env=on) == "python"
    assert pipeline_route([], None, "pil", serve, env=on) == "python"
    assert pipeline_route(im, None, "video", serve, env=on) == "python"
    assert not asked                                       # the plans are asked last, and only where everything else holds
    assert pipeline_route(im, None, "pil", False, env=on) == "python"
    assert pipeline_route(im, None, "pil", lambda: False, env=on) == "python"


def test_the_request_mirror_has_the_c_layout():
    """Offsets of the ctypes mirror against the C struct's natural layout (the fields in header order, each aligned to its
    size): a field added on one side only moves everything behind it."""
    from ctrlv_amd import _lib
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctrlv_hip.h")).read()
    body = src[src.index("typedef struct ctrlv_clip_request {"):src.index("} ctrlv_clip_request;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            names.append(re.sub(r"\[\d+\]", "", part.strip().split()[-1].lstrip("*")))
    assert names == [f[0] for f in _lib.ClipRequest._fields_]
    assert ctypes.sizeof(_lib.ClipRequest) % 8 == 0
