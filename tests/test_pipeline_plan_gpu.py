"""The whole-clip driver on the device (include/ctrlv_hip.h: ctrlv_pipeline_generate; csrc/pipeline.hip, csrc/pipeline_io.hip):
the three I/O kernels against reference-executed vectors / the torch expressions they restate, the driver against the same
kernels called one by one (bit for bit), from a foreign host through raw ctypes, and the opt-in pipeline route
(CTRLV_PIPELINE=plan).  Tiny models (R.TINY_CONFIG), the default AutoencoderKLTemporalDecoder, a two-layer CLIP tower; 1 clip x 3
frames x 128 x 192 pixels (latent 16 x 24), 2 steps.

Element types: the kernels and the driver are checked in both builds.  In the fp16 build the reference composition calls the
fp16 library's VAE plan directly (`vae_plan(vae, dtype=fp16)`): vae_encoder_hip.encode_plan / vae_decoder_hip.decode_plan route
to the bf16 library, whose plan a driver of the fp16 library cannot borrow."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_helpers.npz"))
PIPE_CLIP = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=128, patch_size=16,
                 projection_dim=64, hidden_act="gelu", layer_norm_eps=1e-5)        # 65 tokens; projection = cross_attention_dim
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
N, F, H, W, STEPS = 1, 3, 128, 192, 2


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def el(request, hip_lib):
    return request.param


# ------------------------------------------------------------------------------------------------------------- the I/O kernels
def test_resize_against_reference_executed_vectors(el):
    """The four resize cases of tests/golden/ref_helpers.npz (the reference's own _resize_with_antialiasing): 80x128 -> 56^2,
    144x256 -> 56^2, 97x131 -> 64x48, 50x56 -> 56^2.  fp32 output within 2e-5 (<= 15 + 15 blur taps and 16 bicubic taps of
    fp32 products with absolute weight sum <= 1.9: < 1e-5, doubled for the differing exp); the element-type output is that
    value rounded to nearest even, bit for bit; the normalising epilogue is the torch formula on the fp32 output within 1 ulp."""
    from ctrlv_amd import ops
    mean = torch.tensor(MEAN, device=DEV).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=DEV).view(1, 3, 1, 1)
    for i in range(4):
        x, want = torch.from_numpy(G[f"resize{i}_in"]).to(DEV), torch.from_numpy(G[f"resize{i}_out"])
        size = tuple(int(v) for v in G[f"resize{i}_size"])
        got = ops.resize_antialias(x, size)
        got_el = ops.resize_antialias(x, size, out_dtype=el)
        got_n = ops.resize_antialias(x, size, mean=MEAN, std=STD)
        torch.cuda.synchronize()
        err = float((got.cpu() - want).abs().max())
        print(f"  resize{i} {tuple(x.shape)} -> {size}: max abs error {err:.3e}")
        assert got.shape == want.shape and got.dtype == torch.float32
        assert err <= 2e-5, (i, err)
        assert got_el.dtype == el and torch.equal(got_el, got.to(el)), i
        ref_n = ((got + 1.0) / 2.0 - mean) / std
        ulp = torch.maximum(ref_n.abs(), torch.tensor(2.0 ** -126, device=DEV)).log2().floor().sub(23).exp2()
        assert bool(((got_n - ref_n).abs() <= ulp).all()), (i, float((got_n - ref_n).abs().max()))


def test_resize_reads_uint8_like_the_float_path(el):
    """uint8 input = the fp32 path on (v / 255) * 2 - 1 (formed on the host: true division), bit for bit; a strong down-scale
    (13 taps per axis, several tiles), the identity size and an up-scale."""
    from ctrlv_amd import ops
    u8 = torch.randint(0, 256, (2, 61, 90, 3), generator=gen(2), dtype=torch.uint8)
    x = (torch.from_numpy(u8.numpy().astype(np.float32) / 255.0).permute(0, 3, 1, 2) * 2.0 - 1.0).contiguous().to(DEV)
    u8 = u8.to(DEV)
    for size in ((56, 56), (8, 12), (61, 90), (64, 100)):
        a, b = ops.resize_antialias(u8, size), ops.resize_antialias(x, size)
        assert torch.equal(a, b), size
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) < 1.5


def test_resize_at_the_largest_factor_takes_the_short_tile(el):
    """520 x 1040 -> 65 x 130 (factor 8, 15 taps per axis): an 8-row output tile's source rows would need more than 64 KiB of
    LDS, so the launch takes 4-row tiles.  Against the torch restatement on the host (itself within 2e-6 of the reference's
    vectors, tests/test_ref_helpers.py), same 2e-5 bound; the image is 2 tiles wide and 17 high with a partial last column tile."""
    from ctrlv_amd import ops
    from ctrlv_amd.pipelines.pipeline_utils import _resize_with_antialiasing
    x = torch.rand(1, 3, 520, 1040, generator=gen(6)) * 2 - 1
    want = _resize_with_antialiasing(x, (65, 130))
    got = ops.resize_antialias(x.to(DEV), (65, 130)).cpu()
    err = float((got - want).abs().max())
    print(f"  resize 520x1040 -> 65x130: max abs error {err:.3e}")
    assert err <= 2e-5, err


@pytest.mark.parametrize("with_noise", [False, True])
def test_pixels_prepare_is_the_torch_expression(el, with_noise):
    from ctrlv_amd import ops
    u8 = torch.randint(0, 256, (2, 17, 23, 3), generator=gen(3), dtype=torch.uint8)
    noise = torch.randn(2, 3, 17, 23, generator=gen(4)) if with_noise else None
    x = 2.0 * (torch.from_numpy(u8.numpy().astype(np.float32) / 255.0).permute(0, 3, 1, 2)) - 1.0     # VaeImageProcessor.preprocess
    if with_noise:
        x = x + 0.02 * noise                                                                          # prepare_clip
    got = ops.pixels_prepare(u8.to(DEV), noise.to(DEV) if with_noise else None, 0.02, dtype=el)
    assert got.dtype == el and torch.equal(got.cpu(), x.to(el))


def test_frames_to_u8_is_postprocess_and_round(el):
    from ctrlv_amd import ops
    from ctrlv_amd.pipelines.pipeline_utils import VaeImageProcessor
    x = ((torch.rand(6, 3, 17, 23, generator=gen(5)) * 3.0) - 1.5).to(el)
    x[0, 0, 0, :4] = torch.tensor([-1.0, 1.0, 0.0, 2.0 / 255.0 - 1.0]).to(el)
    img = VaeImageProcessor().postprocess(x.float(), output_type="np")                  # (6, 17, 23, 3) in [0, 1]
    want = (img * 255).round().astype("uint8")
    got = ops.frames_to_u8(x.to(DEV))
    assert got.shape == (6, 17, 23, 3) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.min() == 0 and want.max() == 255                                         # the clamped range is exercised


# ------------------------------------------------------------------------------------------------------------------ the models
class Setup:
    pass


@pytest.fixture(scope="module")
def setup(el):
    return build_setup(el)


def build_setup(el):
    import ctrlv_ref as R
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder, clip_vision_hip
    from ctrlv_amd.plan import PipelinePlan, vae_plan
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from tests import clip_utils as U
    from tests.parity_utils import make_pair
    s = Setup()
    s.el = el
    s.cfg = dict(R.TINY_CONFIG)
    assert s.cfg["cross_attention_dim"] == PIPE_CLIP["projection_dim"]
    _, _, s.hu, s.hc = make_pair(s.cfg, DEV, dtype=el)
    torch.manual_seed(5)
    s.vae = AutoencoderKLTemporalDecoder().eval().to(DEV, el)
    s.clip = U.build_own(PIPE_CLIP, 31, el, DEV)
    s.sched = EulerDiscreteScheduler()
    s.sched.set_timesteps(STEPS, device=DEV)
    s.sigmas, s.timesteps = list(s.sched._sigmas_host), list(s.sched._timesteps_host)
    probe = torch.empty(0, device=DEV)
    s.vplan = vae_plan(s.vae, dtype=el)
    s.plans = (s.hu._ensure_plan(probe), s.hc._ensure_plan(probe), s.vplan, clip_vision_hip._plan(s.clip))
    s.pipe = PipelinePlan(*s.plans)
    s.pipe_svd = PipelinePlan(s.plans[0], None, s.plans[2], s.plans[3])
    g0 = gen(11)
    s.image = torch.randint(0, 256, (2, H, W, 3), generator=g0, dtype=torch.uint8).to(DEV)
    s.cond = (torch.rand(2, F, 3, H, W, generator=g0) * 2 - 1).to(DEV)                                # fp32 pixels
    s.cond_lat = torch.randn(2, F, 4, H // 8, W // 8, generator=g0).to(DEV, el)
    s.aug = torch.randn(2, 3, H, W, generator=g0).to(DEV)
    s.lat = (torch.randn(2, F, 4, H // 8, W // 8, generator=g0) * s.sched.init_noise_sigma).to(DEV)
    return s


def _venc(s, x):
    from ctrlv_amd.models import vae_encoder_hip
    if s.el == torch.bfloat16:
        return vae_encoder_hip.encode_plan(s.vae, x, moments=False)[0]
    return s.vplan.encode(x, moments=False)[0]


def _vdec(s, z, nf):
    from ctrlv_amd.models import vae_decoder_hip
    if s.el == torch.bfloat16:
        return vae_decoder_hip.decode_plan(s.vae, z, nf)
    return s.vplan.decode(z, nf)


def compose(s, n, *, use_cn=True, cfg=True, cond="pixels", chunk=2, strength=0.02, scale=0.8):
    """What ctrlv_pipeline_generate enqueues, call by call: the ops wrappers, clip_vision_hip.encode_plan, the VAE plan, an
    eager DenoiseStepper, the VAE plan, the uint8 kernel."""
    from ctrlv_amd import ops
    from ctrlv_amd.models import clip_vision_hip
    from ctrlv_amd.pipelines.pipeline_utils import DenoiseStepper
    el = s.el
    image, aug, lat = s.image[:n], s.aug[:n], s.lat[:n]
    size = PIPE_CLIP["image_size"]
    px = ops.resize_antialias(image, (size, size), mean=MEAN, std=STD, out_dtype=el)
    ehs = clip_vision_hip.encode_plan(s.clip, px).unsqueeze(1)
    first = _venc(s, ops.pixels_prepare(image, aug, strength, dtype=el))
    if cfg:
        ehs = torch.cat([torch.zeros_like(ehs), ehs])
        first = torch.cat([torch.zeros_like(first), first])
    image_latents = first.unsqueeze(1).repeat(1, F, 1, 1, 1)
    cond_em = None
    if use_cn:
        if cond == "pixels":
            cond_em = _venc(s, s.cond[:n].to(el).flatten(0, 1)).reshape(n, F, 4, H // 8, W // 8)
        else:
            cond_em = s.cond_lat[:n]
        if cfg:
            cond_em = torch.cat([torch.zeros_like(cond_em), cond_em])
    ids = torch.tensor([[7 - 1, 127, strength]], dtype=el).repeat(2 * n if cfg else n, 1).to(DEV)
    max_g = 3.0 if cfg else 1.0
    st = DenoiseStepper(s.hu, s.hc if use_cn else None, s.sched, lat, image_latents, ehs, ids, cond_em, 1.0, max_g, scale,
                        do_cfg=cfg, use_hip_graph=False)
    for i in range(STEPS):
        st.step(i)
    out_lat = st.latents
    inv = float(np.float32(1.0 / float(np.float32(s.vae.config.scaling_factor))))
    z = out_lat.to(el).flatten(0, 1) * inv
    frames = torch.cat([_vdec(s, z[i:i + chunk], z[i:i + chunk].shape[0]) for i in range(0, z.shape[0], chunk)])
    u8 = ops.frames_to_u8(frames).reshape(n, F, H, W, 3)
    torch.cuda.synchronize()
    return out_lat, frames, u8


def drive(s, n, *, use_cn=True, cfg=True, cond="pixels", chunk=2, strength=0.02, scale=0.8, overlap=True):
    pipe = s.pipe if use_cn else s.pipe_svd
    pipe.set_overlap(overlap)
    c = None if not use_cn else (s.cond[:n] if cond == "pixels" else s.cond_lat[:n])
    out = pipe.generate(s.image[:n], s.lat[:n], s.sigmas, s.timesteps, cond=c, aug_noise=s.aug[:n], noise_aug_strength=strength,
                        fps=7, motion_bucket_id=127, min_guidance=1.0, max_guidance=3.0 if cfg else 1.0,
                        conditioning_scale=scale, decode_chunk=chunk)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4 else torch.uint8))


def same(got, want):
    for a, b, what in zip(got, want, ("out_latents", "out_frames", "out_frames_u8")):
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert torch.equal(bits(a), bits(b)), (what, float((a.float() - b.float()).abs().max()))


VARIANTS = {
    "base": dict(),                                  # CFG on, ControlNet on, 3-channel cond, chunks of 2 and 1, overlap on
    "no_controlnet": dict(use_cn=False),
    "cfg_off": dict(cfg=False),
    "cond_latents": dict(cond="latents"),
    "two_clips": dict(n=2),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_driver_is_the_same_kernels_called_one_by_one(setup, variant):
    kw = dict(VARIANTS[variant])
    n = kw.pop("n", N)
    want = compose(setup, n, **kw)
    got = drive(setup, n, **kw)
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0
    same(got, want)


def test_overlap_off_and_on_give_the_same_bits(setup):
    on = drive(setup, N, overlap=True)
    off = drive(setup, N, overlap=False)
    same(off, on)
    setup.pipe.set_overlap(True)


def test_workspace_bytes_and_the_too_small_workspace(setup):
    """Pure host arithmetic on loaded plans: non-decreasing in n_clips / num_frames / the image size / decode_chunk, unchanged by
    num_steps; a workspace one byte short is CTRLV_E_WORKSPACE, the message carries the needed size, nothing is launched."""
    from ctrlv_amd import _lib
    s = setup
    lib = s.pipe._lib

    def need(n=1, f=F, h=H, w=W, steps=STEPS, chunk=2, pipe=s.pipe, frames=True):
        image = torch.empty(n, h, w, 3, dtype=torch.uint8, device=DEV)
        lat = torch.empty(n, f, 4, h // 8, w // 8, device=DEV)
        cond = torch.empty(n, f, 3, h, w, device=DEV)
        sig = [float(steps + 1 - i) for i in range(steps + 1)]
        r, keep = pipe.request(image, lat, sig, [1.0] * steps, cond=cond, decode_chunk=chunk, out_latents=lat,
                               out_frames_u8=image if frames else None)
        return pipe.workspace_bytes(r), r, keep

    base = need()[0]
    assert base > 0 and base % 256 == 0
    assert need(steps=1)[0] == base == need(steps=50)[0]
    assert need(n=2)[0] >= base and need(f=4)[0] >= base >= need(f=2)[0]
    assert need(h=2 * H)[0] >= base and need(chunk=3)[0] >= base >= need(chunk=1)[0]
    assert need(frames=False)[0] <= base and need(pipe=s.pipe_svd)[0] <= base
    nb, r, keep = need()
    out = torch.full((1, F, 4, H // 8, W // 8), 7.0, device=DEV)
    r.out_latents = out.data_ptr()
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ctrlv_pipeline_generate(s.pipe._h, ctypes.byref(r), ws.data_ptr(), nb - 1, st) == -5
    assert str(nb) in _lib.last_error(lib) and "ws_bytes" in _lib.last_error(lib)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="num_frames"):
        need(f=33)


# ---------------------------------------------------------------------------------------------------------------- foreign host
def _tensor_descs(_lib, module_or_sd):
    sd = module_or_sd if isinstance(module_or_sd, dict) else module_or_sd.state_dict()
    host = [(k, v.detach().float().cpu().contiguous()) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()]
    arr = (_lib.TensorDesc * len(host))()
    for i, (k, v) in enumerate(host):
        arr[i].name, arr[i].data, arr[i].dtype, arr[i].on_device, arr[i].numel = k.encode(), v.data_ptr(), 0, 0, v.numel()
    return arr, host


def test_pipeline_from_a_foreign_host(setup):
    """Raw ctypes only: the four plans created and loaded from HOST fp32 weights (rounding an fp32 copy of a 16-bit value is
    exact), the pipeline, the workspace query, generate on a non-default stream.  Bit-equal to PipelinePlan; 4 KiB of pattern
    behind the workspace survive; a second generate gives the same bits."""
    from ctrlv_amd import _lib
    from ctrlv_amd.plan import CLIP_ACTS, config_struct
    s = setup
    lib = _lib.load(s.el)
    want = drive(s, N)
    handles = []
    for kind, m in (("unet", s.hu), ("controlnet", s.hc)):
        c = config_struct(kind, m.config, m.time_context_order)
        h = ctypes.c_void_p()
        assert lib.ctrlv_plan_create(ctypes.byref(c), 0, ctypes.byref(h)) == 0, _lib.last_error(lib)
        arr, host = _tensor_descs(_lib, m)
        assert lib.ctrlv_plan_load_weights(h, arr, len(host)) == 0, _lib.last_error(lib)
        handles.append(h)
    vc = _lib.VaeConfig()
    vc.in_channels, vc.out_channels, vc.latent_channels, vc.layers_per_block, vc.n_blocks = 3, 3, 4, 2, 4
    for i, ch in enumerate((128, 256, 512, 512)):
        vc.block_out_channels[i] = ch
    vc.scaling_factor = 0.18215
    hv = ctypes.c_void_p()
    assert lib.ctrlv_vae_plan_create(ctypes.byref(vc), 0, ctypes.byref(hv)) == 0, _lib.last_error(lib)
    arr, host = _tensor_descs(_lib, s.vae)
    assert lib.ctrlv_vae_plan_load_weights(hv, arr, len(host)) == 0, _lib.last_error(lib)
    cc = _lib.ClipConfig()
    for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
              "projection_dim"):
        setattr(cc, k, PIPE_CLIP[k])
    cc.hidden_act, cc.layer_norm_eps = CLIP_ACTS[PIPE_CLIP["hidden_act"]], PIPE_CLIP["layer_norm_eps"]
    hc = ctypes.c_void_p()
    assert lib.ctrlv_clip_plan_create(ctypes.byref(cc), 0, ctypes.byref(hc)) == 0, _lib.last_error(lib)
    arr, host = _tensor_descs(_lib, {k: v for k, v in s.clip.state_dict().items() if not k.endswith("position_ids")})
    assert lib.ctrlv_clip_plan_load_weights(hc, arr, len(host)) == 0, _lib.last_error(lib)
    hp = ctypes.c_void_p()
    assert lib.ctrlv_pipeline_create(handles[0], handles[1], hv, hc, 0, ctypes.byref(hp)) == 0, _lib.last_error(lib)

    out_lat = torch.zeros(N, F, 4, H // 8, W // 8, device=DEV)
    out_fr = torch.zeros(N * F, 3, H, W, dtype=s.el, device=DEV)
    out_u8 = torch.zeros(N, F, H, W, 3, dtype=torch.uint8, device=DEV)
    r = _lib.ClipRequest()
    r.n_clips, r.num_frames, r.height, r.width = N, F, H, W
    image, cond, aug, lat = s.image[:N].contiguous(), s.cond[:N].contiguous(), s.aug[:N].contiguous(), s.lat[:N].contiguous()
    r.image_u8, r.cond, r.cond_channels, r.cond_dtype = image.data_ptr(), cond.data_ptr(), 3, 0
    r.aug_noise, r.noise_aug_strength, r.num_steps, r.latents = aug.data_ptr(), 0.02, STEPS, lat.data_ptr()
    sig, ts = (ctypes.c_float * (STEPS + 1))(*s.sigmas), (ctypes.c_float * STEPS)(*s.timesteps)
    r.sigmas, r.timesteps = sig, ts
    r.fps, r.motion_bucket_id, r.min_guidance, r.max_guidance, r.conditioning_scale, r.decode_chunk = 7, 127, 1.0, 3.0, 0.8, 2
    r.out_latents, r.out_frames, r.out_frames_u8 = out_lat.data_ptr(), out_fr.data_ptr(), out_u8.data_ptr()
    need = lib.ctrlv_pipeline_workspace_bytes(hp, ctypes.byref(r))
    assert need > 0 and need % 256 == 0, _lib.last_error(lib)
    buf = torch.empty(need + 4096, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf[need:] = 0xA5
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    st = ctypes.c_void_p(stream.cuda_stream)
    assert lib.ctrlv_pipeline_generate(hp, ctypes.byref(r), buf.data_ptr(), need, st) == 0, _lib.last_error(lib)
    stream.synchronize()
    torch.cuda.synchronize()
    same((out_lat, out_fr, out_u8), want)
    assert bool((buf[need:] == 0xA5).all())
    first = (out_lat.clone(), out_fr.clone(), out_u8.clone())
    for t in (out_lat, out_fr, out_u8):
        t.zero_()
    torch.cuda.synchronize()
    assert lib.ctrlv_pipeline_generate(hp, ctypes.byref(r), buf.data_ptr(), need, st) == 0, _lib.last_error(lib)
    stream.synchronize()
    torch.cuda.synchronize()
    same((out_lat, out_fr, out_u8), first)
    assert bool((buf[need:] == 0xA5).all())
    assert lib.ctrlv_pipeline_destroy(hp) == 0
    assert lib.ctrlv_clip_plan_destroy(hc) == 0 and lib.ctrlv_vae_plan_destroy(hv) == 0
    assert lib.ctrlv_plan_destroy(handles[0]) == 0 and lib.ctrlv_plan_destroy(handles[1]) == 0


# ---------------------------------------------------------------------------------------------------------------- Python route
def test_the_pipeline_route(hip_lib, monkeypatch):
    """StableVideoControlPipeline with PIL inputs at the working size and a seeded CPU generator: CTRLV_PIPELINE=plan against the
    same call with the variable unset (both under CTRLV_VAE_HIP=plan, CTRLV_CLIP_HIP=plan).  parity_err < 3e-2, the project's
    bound for a pipeline-level route comparison (test_pipeline_under_the_plan_route); the arithmetic that differs is the resize,
    at the 1e-5 level before rounding.  With a callback or a tensor image the driver is not entered."""
    import ctrlv_ref as R
    from PIL import Image
    from ctrlv_amd import plan as plan_mod
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.pipelines import StableVideoControlPipeline
    from ctrlv_amd.pipelines.pipeline_utils import MinimalCLIPImageProcessor
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from tests import clip_utils as U
    from tests.parity_utils import make_pair
    BF = torch.bfloat16
    cfg = dict(R.TINY_CONFIG)
    _, _, hu, hc = make_pair(cfg, DEV)
    torch.manual_seed(5)
    vae = AutoencoderKLTemporalDecoder().eval().to(DEV, BF)
    clip = U.build_own(dict(PIPE_CLIP, image_size=224), 31, BF, DEV)           # the pipelines resize a PIL image to 224 x 224
    pipe = StableVideoControlPipeline(vae, clip, hu, hc, EulerDiscreteScheduler(), MinimalCLIPImageProcessor())
    pipe.set_progress_bar_config(disable=True)
    g0 = gen(11)
    image = Image.fromarray(torch.randint(0, 256, (H, W, 3), generator=g0, dtype=torch.uint8).numpy())
    cond = (torch.rand(1, F, 3, H, W, generator=g0) * 2 - 1).to(DEV)
    calls = []
    real = plan_mod.PipelinePlan.generate
    monkeypatch.setattr(plan_mod.PipelinePlan, "generate", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    monkeypatch.setenv("CTRLV_VAE_HIP", "plan")
    monkeypatch.setenv("CTRLV_CLIP_HIP", "plan")

    def run(img=image, **kw):
        return pipe(img, cond_images=cond, height=H, width=W, num_frames=F, num_inference_steps=STEPS, decode_chunk_size=2,
                    generator=gen(7), output_type="pt", **kw).frames.float().cpu()

    monkeypatch.delenv("CTRLV_PIPELINE", raising=False)
    ref = run()
    assert not calls
    monkeypatch.setenv("CTRLV_PIPELINE", "plan")
    got = run()
    assert len(calls) == 1
    assert got.shape == ref.shape == (1, F, 3, H, W) and got.min() >= 0 and got.max() <= 1
    assert parity_err(got, ref, "pipeline frames, one C call vs the Python pipeline") < 3e-2
    run(callback_on_step_end=lambda p, i, t, kw: {})
    assert len(calls) == 1                                          # a per-step callback: the Python loop
    tensor_image = torch.from_numpy(np.asarray(image).astype(np.float32) / 255.0).permute(2, 0, 1)[None].to(DEV, BF) * 2 - 1
    took = pipe._generate_plan(
        tensor_image, cond, lambda h, w: None, height=H, width=W, num_frames=F, decode_chunk_size=2, fps=7, motion_bucket_id=127,
        noise_aug_strength=0.02, num_videos_per_prompt=1, generator=gen(7), latents=None, latent_channels=8,
        min_guidance_scale=1.0, max_guidance_scale=3.0, num_inference_steps=STEPS, control_condition_scale=1.0,
        output_type="pt", return_dict=True, callback_on_step_end=None)
    assert took is None and len(calls) == 1                         # a tensor image: the route is not taken
    pil = pipe(image, cond_images=cond, height=H, width=W, num_frames=F, num_inference_steps=STEPS, decode_chunk_size=2,
               generator=gen(7), output_type="pil").frames
    assert len(calls) == 2 and len(pil) == 1 and len(pil[0]) == F and pil[0][0].size == (W, H)
    assert np.abs(np.asarray(pil[0][0]).astype(np.float32) / 255.0 - got[0, 0].permute(1, 2, 0).numpy()).max() <= 0.5 / 255 + 1e-6
