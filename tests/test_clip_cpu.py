"""The CLIP vision tower without a GPU: ctrlv_amd's own CLIPVisionModelWithProjection against transformers (keys, shapes, the
torch forward, checkpoints), the loader fallbacks of the pipelines, the minimal feature extractor, the executor's `supports()`
truth table and the host-side argument checks of the four entry points of csrc/clip.hip.

Oracle: transformers' CLIPVisionModelWithProjection in fp32 on the CPU -- live where the library is importable, and recorded in
tests/golden/clip_vectors.npz (tests/golden/make_clip_golden.py) for the two configs of tests/clip_utils.py.  Bound of the fp32
torch forward: rel-L2 <= 1e-5 (same operations, fp32 round-off only)."""
import ctypes
import json
import os
import sys

import pytest
import torch

import __graft_entry__ as g
from tests import clip_utils as U
from tests.fakes import FakeCLIP
from tests.parity_utils import rel_l2


def _have_transformers():
    try:
        import transformers  # noqa: F401
        return True
    except ImportError:
        return False


needs_transformers = pytest.mark.skipif(not _have_transformers(), reason="transformers is not installed")


@pytest.fixture(scope="module")
def golden():
    return U.load_golden()


def _own(cfg, device=None):
    from ctrlv_amd.models import CLIPVisionModelWithProjection
    if device is None:
        return CLIPVisionModelWithProjection(**cfg)
    with torch.device(device):
        return CLIPVisionModelWithProjection(**cfg)


@needs_transformers
@pytest.mark.parametrize("name", ["A", "B", "vit_h"])
def test_state_dict_keys_and_shapes_equal_transformers(name):
    from transformers import CLIPVisionConfig
    from transformers import CLIPVisionModelWithProjection as T
    cfg = U.CONFIG_VIT_H if name == "vit_h" else U.CONFIGS[name][0]
    with torch.device("meta"):
        ref = T(CLIPVisionConfig(**cfg))
    own = _own(cfg, "meta")
    a = [(k, tuple(v.shape)) for k, v in ref.state_dict().items() if not k.endswith("position_ids")]
    b = [(k, tuple(v.shape)) for k, v in own.state_dict().items()]
    assert a == b                          # the same keys in the same order (the seeded rule draws in this order)
    assert len(b) == 8 + 16 * cfg["num_hidden_layers"]


def test_state_dict_keys_of_vit_h_are_transformers_names():
    """Without transformers: the names SVD's image_encoder/model.safetensors carries."""
    own = _own(dict(U.CONFIG_VIT_H, num_hidden_layers=1), "meta")
    sd = {k: tuple(v.shape) for k, v in own.state_dict().items()}
    assert sd["vision_model.embeddings.class_embedding"] == (1280,)
    assert sd["vision_model.embeddings.patch_embedding.weight"] == (1280, 3, 14, 14)
    assert sd["vision_model.embeddings.position_embedding.weight"] == (257, 1280)
    assert sd["vision_model.pre_layrnorm.weight"] == (1280,)
    assert sd["vision_model.encoder.layers.0.self_attn.q_proj.weight"] == (1280, 1280)
    assert sd["vision_model.encoder.layers.0.mlp.fc1.bias"] == (5120,)
    assert sd["vision_model.post_layernorm.bias"] == (1280,)
    assert sd["visual_projection.weight"] == (1024, 1280)
    assert "vision_model.embeddings.patch_embedding.bias" not in sd and "visual_projection.bias" not in sd


@pytest.mark.parametrize("name", ["A", "B"])
def test_torch_forward_reproduces_the_golden(golden, name):
    cfg, n, seed = U.CONFIGS[name]
    m = U.build_own(cfg, seed)
    with torch.no_grad():
        r = m(golden[name]["pixel_values"])
    assert r.image_embeds.shape == (n, cfg["projection_dim"])
    for f in ("image_embeds", "last_hidden_state"):
        e = rel_l2(getattr(r, f), golden[name][f])
        print(f"  {name} {f}: rel-L2 {e:.3e}")
        assert e <= 1e-5


@needs_transformers
@pytest.mark.parametrize("name", ["A", "B", "vit_h_2_layers"])
def test_torch_forward_against_live_transformers(name):
    if name == "vit_h_2_layers":
        cfg, n, seed = dict(U.CONFIG_VIT_H, num_hidden_layers=2), 1, 13
    else:
        cfg, n, seed = U.CONFIGS[name]
    ref, own = U.build_transformers(cfg, seed), U.build_own(cfg, seed)
    px = U.seeded_pixels(cfg, n, seed)
    with torch.no_grad():
        a, b = ref(pixel_values=px), own(px)
    for f in ("image_embeds", "last_hidden_state"):
        e = rel_l2(getattr(b, f), getattr(a, f))
        print(f"  {name} {f}: rel-L2 {e:.3e}")
        assert e <= 1e-5


def test_save_and_from_pretrained_round_trip(tmp_path):
    from ctrlv_amd.models import CLIPVisionModelWithProjection
    cfg, _, seed = U.CONFIGS["B"]
    m = U.build_own(cfg, seed)
    m.save_pretrained(tmp_path / "enc")
    assert (tmp_path / "enc" / "model.safetensors").is_file() and (tmp_path / "enc" / "config.json").is_file()
    m2 = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="enc", torch_dtype=torch.bfloat16)
    assert m2.dtype == torch.bfloat16 and m2.device.type == "cpu" and dict(m2.config) == dict(m.config)
    assert not any(p.requires_grad for p in m2.parameters())
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a.to(torch.bfloat16), b)
    # a variant file, and the torch.save form
    m.save_pretrained(tmp_path / "v", variant="fp16")
    assert (tmp_path / "v" / "model.fp16.safetensors").is_file()
    CLIPVisionModelWithProjection.from_pretrained(tmp_path / "v", variant="fp16")
    m.save_pretrained(tmp_path / "b", safe_serialization=False)
    m3 = CLIPVisionModelWithProjection.from_pretrained(tmp_path / "b")
    assert torch.equal(m3.visual_projection.weight, m.visual_projection.weight)
    with pytest.raises(EnvironmentError):
        CLIPVisionModelWithProjection.from_pretrained(tmp_path / "nothing")


def test_from_pretrained_ignores_position_ids_and_rejects_other_keys(tmp_path):
    from safetensors.torch import save_file

    from ctrlv_amd.models import CLIPVisionModelWithProjection
    cfg, _, seed = U.CONFIGS["B"]
    m = U.build_own(cfg, seed)
    m.save_pretrained(tmp_path / "old")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["vision_model.embeddings.position_ids"] = torch.arange(26).unsqueeze(0)          # what old checkpoints carry
    save_file(sd, str(tmp_path / "old" / "model.safetensors"))
    m2 = CLIPVisionModelWithProjection.from_pretrained(tmp_path / "old")
    assert torch.equal(m2.vision_model.embeddings.class_embedding, m.vision_model.embeddings.class_embedding)
    sd["vision_model.something_else"] = torch.zeros(1)
    save_file(sd, str(tmp_path / "old" / "model.safetensors"))
    with pytest.raises(ValueError, match="unexpected"):
        CLIPVisionModelWithProjection.from_pretrained(tmp_path / "old")


@needs_transformers
def test_from_pretrained_reads_a_transformers_saved_directory(tmp_path, golden):
    from ctrlv_amd.models import CLIPVisionModelWithProjection
    cfg, _, seed = U.CONFIGS["A"]
    U.build_transformers(cfg, seed).save_pretrained(str(tmp_path / "image_encoder"))
    m = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="image_encoder")
    assert {k: m.config[k] for k in cfg} == cfg
    with torch.no_grad():
        r = m(golden["A"]["pixel_values"])
    assert rel_l2(r.image_embeds, golden["A"]["image_embeds"]) <= 1e-5


def test_loaders_fall_back_without_transformers(tmp_path, monkeypatch):
    from ctrlv_amd.models import CLIPVisionModelWithProjection
    from ctrlv_amd.pipelines import pipeline_utils as PU
    cfg, _, seed = U.CONFIGS["B"]
    U.build_own(cfg, seed).save_pretrained(tmp_path / "image_encoder")
    os.makedirs(tmp_path / "feature_extractor")
    with open(tmp_path / "feature_extractor" / "preprocessor_config.json", "w") as f:
        json.dump({"image_mean": [0.5, 0.4, 0.3], "image_std": [0.2, 0.3, 0.4], "do_resize": True, "size": 224}, f)
    monkeypatch.setitem(sys.modules, "transformers", None)                  # `import transformers` now raises ImportError
    enc = PU._load_image_encoder(str(tmp_path / "image_encoder"), torch_dtype=torch.float32, variant=None)
    assert type(enc) is CLIPVisionModelWithProjection
    fe = PU._load_feature_extractor(str(tmp_path / "feature_extractor"), torch_dtype=None, variant=None)
    assert type(fe) is PU.MinimalCLIPImageProcessor and fe.image_mean == [0.5, 0.4, 0.3] and fe.image_std == [0.2, 0.3, 0.4]


@needs_transformers
def test_loaders_prefer_transformers_when_it_is_there(tmp_path):
    import transformers

    from ctrlv_amd.pipelines import pipeline_utils as PU
    cfg, _, seed = U.CONFIGS["B"]
    U.build_own(cfg, seed).save_pretrained(tmp_path / "image_encoder")
    enc = PU._load_image_encoder(str(tmp_path / "image_encoder"))
    assert isinstance(enc, transformers.CLIPVisionModelWithProjection)


def test_minimal_feature_extractor_serves_one_call_only():
    from ctrlv_amd.pipelines.pipeline_utils import MinimalCLIPImageProcessor
    fe = MinimalCLIPImageProcessor()
    x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(0))
    kw = dict(do_normalize=True, do_center_crop=False, do_resize=False, do_rescale=False, return_tensors="pt")
    y = fe(images=x, **kw).pixel_values
    mean, std = torch.tensor(fe.image_mean).view(1, 3, 1, 1), torch.tensor(fe.image_std).view(1, 3, 1, 1)
    assert y.dtype == torch.float32 and torch.equal(y, (x - mean) / std)
    for bad in (dict(kw, do_resize=True), dict(kw, do_center_crop=True), dict(kw, do_rescale=True), dict(kw, do_normalize=False),
                dict(kw, return_tensors="np"), dict(kw, size=224), {}):
        with pytest.raises(NotImplementedError):
            fe(images=x, **bad)
    with pytest.raises(NotImplementedError):
        fe(images=[x[0]], **kw)


@needs_transformers
def test_minimal_feature_extractor_against_clip_image_processor():
    from transformers import CLIPImageProcessor

    from ctrlv_amd.pipelines.pipeline_utils import MinimalCLIPImageProcessor
    ref, fe = CLIPImageProcessor(), MinimalCLIPImageProcessor()
    assert fe.image_mean == pytest.approx(ref.image_mean) and fe.image_std == pytest.approx(ref.image_std)
    x = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    kw = dict(do_normalize=True, do_center_crop=False, do_resize=False, do_rescale=False, return_tensors="pt")
    a, b = ref(images=x, **kw).pixel_values, fe(images=x, **kw).pixel_values
    assert a.shape == b.shape and a.dtype == b.dtype
    assert (a - b).abs().max().item() <= 1e-6             # fp32 round-off of (x - mean) / std, |values| < 3


def test_supports_truth_table(monkeypatch):
    """Without a device nothing is served (CPU tensors); the size rules are checked with `is_cuda` patched to True."""
    from ctrlv_amd.models import clip_vision_hip as H
    cfg = U.CONFIGS["A"][0]
    m = _own(cfg).to(torch.bfloat16).requires_grad_(False)
    px = torch.zeros(1, 3, 56, 56)
    assert not H.supports(m, px)                                   # CPU tensors
    assert not H.supports(FakeCLIP(64), px)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))

    def ok(cfg_over=None, px=px, dtype=torch.bfloat16, model=None):
        mm = model if model is not None else _own(dict(cfg, **(cfg_over or {}))).to(dtype).requires_grad_(False)
        return H.supports(mm, px)

    assert ok()
    assert ok(dict(hidden_act="quick_gelu")) and ok(dtype=torch.float16)
    assert ok(U.CONFIGS["B"][0], px=torch.zeros(2, 3, 70, 70))
    assert not ok(dict(hidden_size=288, num_attention_heads=4, intermediate_size=576))       # head_dim 72
    assert not ok(dict(hidden_size=100, num_attention_heads=1))                                # hidden 100
    assert not ok(px=torch.zeros(1, 3, 70, 70))                                                # not the table's image size
    assert not ok(px=torch.zeros(1, 3, 28, 112))
    assert not ok(dict(intermediate_size=600)) and not ok(dict(projection_dim=48))
    assert not ok(dtype=torch.float32)                                                         # not an element type
    assert not ok(model=FakeCLIP(64))
    assert not ok(px=torch.zeros(3, 56, 56)) and not ok(px=None)
    bad_act = _own(cfg).to(torch.bfloat16).requires_grad_(False)
    bad_act.register_to_config(hidden_act="relu")
    assert not H.supports(bad_act, px)
    trainable = _own(cfg).to(torch.bfloat16)
    with torch.enable_grad():
        assert not H.supports(trainable, px)
    with torch.no_grad():
        assert H.supports(trainable, px)
    with pytest.raises(ValueError, match="hidden_act"):
        _own(dict(cfg, hidden_act="relu"))


def test_route_switch_reads_the_environment(monkeypatch):
    from ctrlv_amd.models import clip_vision_hip as H
    monkeypatch.setenv("CTRLV_CLIP_HIP", "0")
    assert not H.enabled()
    monkeypatch.setenv("CTRLV_CLIP_HIP", "1")
    assert H.enabled()
    monkeypatch.delenv("CTRLV_CLIP_HIP")
    assert H.enabled() == H.DEFAULT_ON
    # a CPU module never takes the HIP route, whatever the switch says
    cfg, n, seed = U.CONFIGS["B"]
    monkeypatch.setenv("CTRLV_CLIP_HIP", "1")
    r = U.build_own(cfg, seed)(U.seeded_pixels(cfg, n, seed))
    assert r.image_embeds.shape == (n, 64) and r.last_hidden_state.shape == (n, 26, 128)


def test_host_side_argument_errors_of_the_clip_entry_points():
    g.build()
    from ctrlv_amd import _lib
    p, bad = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    for lib in (_lib.load(), _lib.load(torch.float16)):
        cases = [
            (lambda: lib.ctrlv_attention_tokens(None, p, 1, 17, 320, 80, None), "null"),
            (lambda: lib.ctrlv_attention_tokens(bad, p, 1, 17, 320, 80, None), "16-byte"),
            (lambda: lib.ctrlv_attention_tokens(p, p, 1, 17, 288, 72, None), "head_dim=72 must be a multiple of 16"),
            (lambda: lib.ctrlv_attention_tokens(p, p, 1, 17, 288, 144, None), "multiple of 16"),
            (lambda: lib.ctrlv_attention_tokens(p, p, 1, 17, 8, 8, None), "multiple of 16"),
            (lambda: lib.ctrlv_attention_tokens(p, p, 1, 17, 330, 80, None), "multiple of head_dim"),
            (lambda: lib.ctrlv_attention_tokens(p, p, 1, 0, 320, 80, None), "S=0"),
            (lambda: lib.ctrlv_attention_tokens(p, p, 1, 4097, 320, 80, None), "S=4097"),
            (lambda: lib.ctrlv_attention_tokens(p, p, 0, 17, 320, 80, None), "n_img"),
            (lambda: lib.ctrlv_clip_patch_rows(None, 0, 1, 56, 56, 14, p, 640, None), "null"),
            (lambda: lib.ctrlv_clip_patch_rows(p, 3, 1, 56, 56, 14, p, 640, None), "dtype code 3"),
            (lambda: lib.ctrlv_clip_patch_rows(p, 0, 1, 57, 56, 14, p, 640, None), "whole patches"),
            (lambda: lib.ctrlv_clip_patch_rows(p, 0, 1, 56, 56, 14, p, 584, None), "patch\\^2 = 588"),
            (lambda: lib.ctrlv_clip_patch_rows(p, 0, 1, 56, 56, 14, p, 636, None), "multiple of 8"),
            (lambda: lib.ctrlv_clip_tokens(p, None, p, 1, 16, 320, p, None), "null"),
            (lambda: lib.ctrlv_clip_tokens(p, p, p, 1, 16, 324, p, None), "C=324"),
            (lambda: lib.ctrlv_clip_tokens(p, p, p, 1, 0, 320, p, None), "P=0"),
            (lambda: lib.ctrlv_act_rows(None, 4, 64, 64, 0, None), "null"),
            (lambda: lib.ctrlv_act_rows(p, 4, 64, 64, 2, None), "kind 2"),
            (lambda: lib.ctrlv_act_rows(p, 4, 60, 64, 0, None), "N=60"),
            (lambda: lib.ctrlv_act_rows(p, 4, 64, 56, 0, None), "ld >= N"),
            (lambda: lib.ctrlv_act_rows(bad, 4, 64, 64, 0, None), "16-byte"),
        ]
        for call, what in cases:
            with pytest.raises(ValueError, match=what):
                _lib.check(call(), "clip entry point")


def test_ops_wrappers_refuse_cpu_tensors():
    from ctrlv_amd import _lib, ops
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.CtrlvHipError, match="no CPU path"):
        ops.act_rows(x, "gelu")
    with pytest.raises(_lib.CtrlvHipError, match="no CPU path"):
        ops.attention_tokens(torch.zeros(4, 192, dtype=torch.bfloat16), x, 1, 4, 64, 16)
    with pytest.raises(_lib.CtrlvHipError, match="no CPU path"):
        ops.clip_patch_rows(torch.zeros(1, 3, 14, 14), 14, torch.zeros(1, 640, dtype=torch.bfloat16))
    with pytest.raises(_lib.CtrlvHipError, match="no CPU path"):
        ops.clip_tokens(x, torch.zeros(64), torch.zeros(5, 64), 1, torch.zeros(5, 64, dtype=torch.bfloat16))


def test_abi_version_is_unchanged_by_the_additive_entry_points():
    from ctrlv_amd import _lib
    assert _lib.ABI_VERSION == 22
    for name in ("ctrlv_attention_tokens", "ctrlv_clip_patch_rows", "ctrlv_clip_tokens", "ctrlv_act_rows"):
        assert name in _lib.SIGNATURES
    src = open(os.path.join(g.ROOT, "include", "ctrlv_hip.h")).read()
    assert "ADDITIVE entry points do not" in src
    assert "clip.hip" in g.HIP_SOURCES
