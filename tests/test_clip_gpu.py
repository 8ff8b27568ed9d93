"""GPU tests of the CLIP vision tower on the HIP kernels (csrc/clip.hip, ctrlv_amd/models/clip_vision_hip.py), bf16 elements
(tests/test_clip_f16_gpu.py executes this file's source with EL = torch.float16, as test_ops_f16_gpu.py does).

Bounds.
  attention_tokens   fp32 SDPA on the element-rounded inputs; the bounds the project's other attention cores are held to:
                     parity_err < tol(5e-3), tol(6e-3) for the large-score case (tests/test_ops_gpu.py).
  clip_patch_rows,   exact: a conversion / an fp32 sum rounded once.
  clip_tokens
  act_rows           <= 1 ulp of the element type against F.gelu / x sigmoid(1.702 x) evaluated in fp32 and rounded (where the
                     fp32 evaluation is done: see test_act_rows).
  model              NOT a fixed number: the module's own torch forward on the GPU in the same 16-bit dtype gives the error a
                     16-bit evaluation has against fp32 (rel-L2 of image_embeds and of last_hidden_state); the HIP path must be
                     within 1.5x of it.  Both paths round at the same points, so the two errors are two draws of one quantity; a
                     structural mistake (missing scale, unmasked tail, wrong GELU form, position row off by one) shows as >= 10x.
                     Measured figures: DESIGN.md 3.12.
The key tile and the query block of attention_tokens are both 32: S = 31 / 32 / 33 are the T - 1 / T / T + 1 cases."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import clip_utils as U
from tests.parity_utils import parity_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EL = torch.bfloat16


def tol(bf16_bound):
    """tests/test_ops_gpu.py tol(): the stated bf16 bound, a sixth of it for fp16 elements."""
    return bf16_bound if EL == torch.bfloat16 else bf16_bound / 6.0


def g(seed=0):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    return U.load_golden()


# ------------------------------------------------------------------------------------------------ attention_tokens
def _attn_ref(qkv, n_img, S, C, d):
    """fp32 SDPA on the (already rounded) rows."""
    f = qkv.float().reshape(n_img, S, 3, C // d, d)
    q, k, v = (f[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    return F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n_img * S, C)


def _attn_run(ops, qkv, n_img, S, C, d):
    out = torch.empty(n_img * S, C, dtype=EL, device=DEV)
    ops.attention_tokens(qkv.to(DEV), out, n_img, S, C, d)
    return out


# (S, head_dim, heads, n_img): every S of {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 577} (31 / 32 / 33 = T - 1, T, T + 1 of the
# 32-key tile and the 32-query block), every head_dim of {16, 64, 80, 128}, heads and images of {1, 3}
ATTN_CASES = [(1, 16, 1, 1), (1, 80, 1, 3), (15, 64, 3, 1), (16, 80, 1, 3), (17, 128, 1, 1), (31, 80, 3, 1), (32, 16, 3, 3),
              (32, 80, 1, 1), (33, 64, 1, 1), (33, 80, 3, 3), (63, 128, 3, 1), (64, 80, 1, 1), (65, 16, 1, 3), (257, 80, 3, 3),
              (257, 64, 1, 1), (257, 128, 1, 1), (577, 80, 1, 1), (577, 16, 3, 1)]


@pytest.mark.parametrize("S,d,heads,n_img", ATTN_CASES)
def test_attention_tokens(ops, S, d, heads, n_img):
    C = heads * d
    qkv = torch.randn(n_img * S, 3 * C, generator=g(S + d)).to(EL)
    out = _attn_run(ops, qkv, n_img, S, C, d)
    assert parity_err(out, _attn_ref(qkv, n_img, S, C, d), f"attention_tokens S={S} d={d}") < tol(5e-3)


@pytest.mark.parametrize("S,kpk", [(257, 250), (65, 64)])
def test_attention_tokens_peaked(ops, S, kpk):
    """One late key dominates: the running max jumps in the last tile (S = 65: in the one-key ragged tile)."""
    d, C = 80, 80
    qkv = torch.randn(S, 3 * C, generator=g(1))
    qkv[:, :d] *= 3.0
    qkv[kpk, d:2 * d] = qkv[7, :d] * 4.0            # key kpk aligned with query 7
    qkv = qkv.to(EL)
    out = _attn_run(ops, qkv, 1, S, C, d)
    assert parity_err(out, _attn_ref(qkv, 1, S, C, d), "peaked") < tol(5e-3)


@pytest.mark.parametrize("scale", [6.0, 40.0])
def test_attention_tokens_large_scores(ops, scale):
    """Logits of magnitude ~scale^2 (exp2 overflows without the running max), growing along the key axis so that the max is
    raised tile after tile, and a run of identical large keys."""
    S, d, C = 257, 80, 80
    qkv = torch.randn(S, 3 * C, generator=g(3))
    ramp = torch.linspace(0.2, 1.0, S)[:, None]
    qkv[:, :d] *= scale
    qkv[:, d:2 * d] = (qkv[:, d:2 * d] * ramp + 0.5 * ramp) * scale
    qkv[S // 2:S // 2 + 40, d:2 * d] = qkv[S // 2, d:2 * d]
    qkv = qkv.to(EL)
    out = _attn_run(ops, qkv, 1, S, C, d)
    assert torch.isfinite(out.float()).all()
    assert parity_err(out, _attn_ref(qkv, 1, S, C, d), "large scores") < tol(6e-3)


@pytest.mark.parametrize("S", [17, 33, 257])
def test_attention_tokens_tail_mask_and_bounds(ops, S):
    """qkv / out are views inside larger device buffers: the rows around qkv are NaN (a key tail that is read past S and not
    masked, or a V row that is not zeroed, turns the result into NaN), the rows around out hold a sentinel.  A second image made
    of NaN follows the first: the first image's result must not see it.  Every read stays inside the allocation."""
    d, heads, pad = 80, 2, 40
    C = heads * d
    rows = torch.randn(S, 3 * C, generator=g(S)).to(EL)
    big = torch.full((pad + 2 * S + pad, 3 * C), float("nan"), dtype=EL, device=DEV)
    big[pad:pad + S] = rows.to(DEV)
    sentinel = 777.0
    obig = torch.full((pad + 2 * S + pad, C), sentinel, dtype=EL, device=DEV)
    qkv, out = big[pad:pad + 2 * S], obig[pad:pad + 2 * S]
    assert qkv.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    ops.attention_tokens(qkv, out, 2, S, C, d)
    torch.cuda.synchronize()
    first = out[:S]
    assert torch.isfinite(first.float()).all()
    assert parity_err(first, _attn_ref(rows, 1, S, C, d), "tail") < tol(5e-3)
    assert (obig[:pad] == sentinel).all() and (obig[pad + 2 * S:] == sentinel).all()
    # ... and with ONE image the rows behind it (the NaN image) are not written at all
    obig.fill_(sentinel)
    ops.attention_tokens(qkv, out, 1, S, C, d)
    torch.cuda.synchronize()
    assert torch.equal(out[:S], first)
    assert (obig[:pad] == sentinel).all() and (obig[pad + S:] == sentinel).all()


def test_attention_tokens_is_deterministic_and_independent_of_the_batch(ops):
    S, d, heads = 257, 80, 2
    C = heads * d
    qkv = torch.randn(3 * S, 3 * C, generator=g(5)).to(EL).to(DEV)
    a = _attn_run(ops, qkv, 3, S, C, d)
    b = _attn_run(ops, qkv, 3, S, C, d)
    one = _attn_run(ops, qkv[:S].contiguous(), 1, S, C, d)
    assert torch.equal(a, b)
    assert torch.equal(a[:S], one)


# ------------------------------------------------------------------------------------------------ layout kernels
@pytest.mark.parametrize("src", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("patch,H,W,ld", [(14, 28, 56, 640), (14, 56, 56, 592), (16, 32, 48, 832)])
def test_clip_patch_rows(ops, src, patch, H, W, ld):
    n = 2
    px = torch.randn(n, 3, H, W, generator=g(patch + H)).to(src)
    P, k = (H // patch) * (W // patch), 3 * patch * patch
    want = F.unfold(px.float(), kernel_size=patch, stride=patch).transpose(1, 2).reshape(n * P, k).to(EL)   # (c, dy, dx) columns
    rows = torch.full((n * P, ld), 5.0, dtype=EL, device=DEV)
    ops.clip_patch_rows(px.to(DEV), patch, rows)
    assert torch.equal(rows[:, :k].cpu(), want)
    assert (rows[:, k:] == 0).all()                         # the pad columns are written, as zeros


def test_clip_tokens(ops):
    n, P, C = 3, 16, 328
    pe = torch.randn(n * P, C, generator=g(1)).to(EL)
    cls, pos = torch.randn(C, generator=g(2)), torch.randn(P + 1, C, generator=g(3))
    want = (torch.cat([cls.expand(n, 1, C), pe.float().view(n, P, C)], 1) + pos).to(EL).reshape(n * (P + 1), C)
    out = torch.empty(n * (P + 1), C, dtype=EL, device=DEV)
    ops.clip_tokens(pe.to(DEV), cls.to(DEV), pos.to(DEV), n, out)
    assert torch.equal(out.cpu(), want)


def _ordinal(t):
    """Element bit patterns on one monotonic integer axis (-0 and +0 coincide): |difference| = distance in ulps."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _act_ref(xf, kind):
    return F.gelu(xf) if kind == "gelu" else xf * torch.sigmoid(1.702 * xf)


@pytest.mark.parametrize("kind", ["gelu", "quick_gelu"])
def test_act_rows(ops, kind):
    """<= 1 ulp of the element type against the fp32 evaluation, rounded once.

    The fp32 reference is evaluated ON THE DEVICE (torch's own fp32 kernel: what the 16-bit torch module computes there before
    its one rounding).  For quick-GELU the CPU evaluation is asserted as well.  For the erf form it is asserted for x >= -3 only
    and printed for the rest: 0.5 x (1 + erf(x / sqrt 2)) cancels in the negative tail, where one fp32 ulp of erf (6e-8) is a
    large fraction of 1 + erf, so two correct erff implementations differ there by many element ulps -- measured on MI355X
    against the host's: 128 bf16 ulps at x = -5.34375 on one host CPU (-3.19e-07 on the device, -1.59e-07 on the CPU, exact
    -2.5e-07: one quantum of 1 + erf either side of the truth), 5 ulps at x = -5 on another; 0 ulps against the device's own
    fp32 evaluation both times."""
    M, N, ld = 37, 72, 88
    x = (torch.randn(M, N, generator=g(7)) * 3.0)
    tiny = [1e-7, -3e-6, 6e-5] if EL == torch.float16 else [1e-39, -5e-39, 2e-38]         # the element type's subnormal range
    special = torch.tensor([0.0, -0.0, 50.0, -50.0, 1e4, -1e4, 6e4, -6e4, 1.0, -1.0, 5.0, -5.0] + tiny)
    x[0, :special.numel()] = special
    x = x.to(EL)
    want_dev = _act_ref(x.to(DEV).float(), kind).to(EL).cpu()
    want_cpu = _act_ref(x.float(), kind).to(EL)
    buf = torch.full((M, ld), 9.0, dtype=EL, device=DEV)
    buf[:, :N] = x.to(DEV)
    ops.act_rows(buf[:, :N], kind)
    got = buf.cpu()
    assert (got[:, N:] == 9.0).all()                        # the gap columns of the pitch are untouched
    got = got[:, :N]
    assert torch.isfinite(got.float()).all()
    dist = {}
    for name, want in (("device fp32", want_dev), ("CPU fp32", want_cpu)):
        d = (_ordinal(got) - _ordinal(want)).abs()
        w = d.argmax()
        print(f"  act_rows {kind} vs {name}: max {int(d.max())} ulp at x = {float(x.flatten()[w])}: got {float(got.flatten()[w])}"
              f" want {float(want.flatten()[w])}")
        dist[name] = d
    assert int(dist["device fp32"].max()) <= 1
    well = torch.ones_like(x, dtype=torch.bool) if kind == "quick_gelu" else x.float() >= -3.0
    assert int(dist["CPU fp32"][well].max()) <= 1


# ------------------------------------------------------------------------------------------------ the model
def _check_model(m, px, ref_embeds, ref_hidden, what):
    """HIP encode vs the module's own 16-bit torch forward on the same device, both against the fp32 result."""
    from ctrlv_amd.models import clip_vision_hip as H
    assert H.supports(m, px)
    with torch.no_grad():
        t = m.torch_forward(px)
        e, h = H.encode(m, px, return_hidden=True)
    assert e.dtype == EL and e.shape == ref_embeds.shape and h.shape == ref_hidden.shape
    figs = {}
    for name, got, tor, ref in (("image_embeds", e, t.image_embeds, ref_embeds), ("last_hidden_state", h, t.last_hidden_state, ref_hidden)):
        err_hip, err_torch = rel_l2(got, ref), rel_l2(tor, ref)
        print(f"  {what} {name}: HIP rel-L2 {err_hip:.3e}   torch {str(EL)[6:]} rel-L2 {err_torch:.3e}   ratio {err_hip / err_torch:.2f}")
        figs[name] = (err_hip, err_torch)
    for name, (err_hip, err_torch) in figs.items():
        assert err_hip <= 1.5 * err_torch, (what, name, err_hip, err_torch)
    # image 0 alone: the same bits as in the batch
    with torch.no_grad():
        e0 = H.encode(m, px[:1])
    assert torch.equal(e0[0], e[0])
    return e


@pytest.mark.parametrize("name", ["A", "B"])
def test_model_parity_with_the_golden(hip_lib, golden, name):
    cfg, n, seed = U.CONFIGS[name]
    m = U.build_own(cfg, seed, EL, DEV)
    gd = golden[name]
    _check_model(m, gd["pixel_values"].to(DEV), gd["image_embeds"], gd["last_hidden_state"], name)


def test_model_parity_at_vit_h_widths(hip_lib):
    """ViT-H/14 widths (1280 / 5120 / 16 heads of 80 / 257 tokens / projection 1024) at 2 layers, 2 images, against the class's
    own fp32 forward on the CPU."""
    cfg, seed = dict(U.CONFIG_VIT_H, num_hidden_layers=2), 21
    ref = U.build_own(cfg, seed)
    px = U.seeded_pixels(cfg, 2, seed)
    with torch.no_grad():
        r = ref.torch_forward(px)
    m = ref.to(device=DEV, dtype=EL)
    _check_model(m, px.to(DEV), r.image_embeds, r.last_hidden_state, "ViT-H x 2 layers")


def test_model_forward_takes_the_hip_route_and_the_switch_turns_it_off(hip_lib, golden, monkeypatch):
    from ctrlv_amd.models import clip_vision_hip as H
    cfg, n, seed = U.CONFIGS["A"]
    m = U.build_own(cfg, seed, EL, DEV)
    px = golden["A"]["pixel_values"].to(DEV)
    with torch.no_grad():
        monkeypatch.setenv("CTRLV_CLIP_HIP", "1")
        a = m(px)
        assert torch.equal(a.image_embeds, H.encode(m, px))
        monkeypatch.setenv("CTRLV_CLIP_HIP", "0")
        b = m(px)
        assert torch.equal(b.image_embeds, m.torch_forward(px).image_embeds)
    assert a.last_hidden_state.shape == b.last_hidden_state.shape == (n, 17, 320)


def test_transformers_module_runs_on_the_same_executor(hip_lib, golden):
    """A transformers CLIPVisionModelWithProjection is served as it is (duck typing): the same bits as the project's class."""
    pytest.importorskip("transformers")
    from ctrlv_amd.models import clip_vision_hip as H
    cfg, n, seed = U.CONFIGS["B"]
    t = U.build_transformers(cfg, seed).to(device=DEV, dtype=EL)
    m = U.build_own(cfg, seed, EL, DEV)
    px = golden["B"]["pixel_values"].to(DEV)
    assert H.supports(t, px)
    with torch.no_grad():
        assert torch.equal(H.encode(t, px), H.encode(m, px))


# ------------------------------------------------------------------------------------------------ the pipeline
PIPE_CLIP = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=128, patch_size=16,
                 projection_dim=64, hidden_act="gelu", layer_norm_eps=1e-5)        # 65 tokens; projection = cross_attention_dim


@torch.no_grad()
def test_pipeline_encodes_the_image_on_the_hip_kernels(hip_lib, monkeypatch):
    import ctrlv_ref as R
    from ctrlv_amd.pipelines import StableVideoControlPipeline
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from tests.fakes import FakeVAE, fake_feature_extractor
    from tests.parity_utils import make_pair
    cfg = dict(R.TINY_CONFIG)
    assert cfg["cross_attention_dim"] == PIPE_CLIP["projection_dim"]
    _, _, hu, hc = make_pair(cfg, DEV, dtype=EL)
    ref = U.build_own(PIPE_CLIP, 31)
    clip = U.build_own(PIPE_CLIP, 31, EL, DEV)
    pipe = StableVideoControlPipeline(FakeVAE().to(DEV, EL), clip, hu, hc, EulerDiscreteScheduler(), fake_feature_extractor)
    pipe.set_progress_bar_config(disable=True)
    gen = torch.Generator().manual_seed(11)
    image = torch.rand(1, 3, 128, 128, generator=gen) * 2 - 1
    cond = torch.rand(1, 3, 3, 128, 128, generator=gen) * 2 - 1
    want = ref.torch_forward(image.to(EL).float()).image_embeds
    monkeypatch.setenv("CTRLV_CLIP_HIP", "1")
    on = pipe._encode_image(image.to(DEV, EL), DEV, 1, True)
    monkeypatch.setenv("CTRLV_CLIP_HIP", "0")
    off = pipe._encode_image(image.to(DEV, EL), DEV, 1, True)
    assert on.shape == off.shape == (2, 1, 64) and on.dtype == EL
    assert (on[0] == 0).all() and (off[0] == 0).all()                  # the CFG negative half is exact zeros
    err_on, err_off = rel_l2(on[1, 0], want[0]), rel_l2(off[1, 0], want[0])
    print(f"  pipeline image_embeds: HIP rel-L2 {err_on:.3e}   torch rel-L2 {err_off:.3e}")
    assert err_on <= 1.5 * err_off
    monkeypatch.setenv("CTRLV_CLIP_HIP", "1")
    fr = pipe(image.to(DEV, EL), cond_images=cond.to(DEV), height=128, width=128, num_frames=3, num_inference_steps=2,
              output_type="pt").frames
    assert fr.shape == (1, 3, 3, 128, 128) and torch.isfinite(fr.float()).all()
