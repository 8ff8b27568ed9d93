"""Seeded clips on the device (include/ctrlv_hip.h, "Seeded clips"; csrc/pipeline_io.hip, csrc/pipeline.hip): ctrlv_randn
against the float64 restatement of tests/seeded_ref.py and against torch's element rounding, ctrlv_resize_lanczos_u8 against PIL,
ctrlv_pipeline_prepare / ctrlv_pipeline_generate_seeded against the same entry points fed by hand, from a foreign host, and
`DeviceSeed` through the pipelines.  The models, the geometry (1 and 2 clips x 3 frames x 128 x 192, 2 steps) and the fixture
pattern are those of tests/test_pipeline_plan_gpu.py; the source image is 97 x 131."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import guarded as Gd
from tests import seeded_ref as R
from tests.test_pipeline_plan_gpu import DEV, F, H, PIPE_CLIP, STEPS, W, build_setup, same

pytestmark = pytest.mark.gpu
SEED = 0xDEADBEEFCAFEF00D
SH, SW = 97, 131                     # the source image's size
K = 1                                # conditioning box frames of the box predictor
LANCZOS_SHAPES = (((375, 1242), (320, 512)), ((720, 1280), (576, 1024)), ((97, 131), (64, 96)), ((64, 96), (128, 192)),
                  ((50, 70), (50, 35)))


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def el(request, hip_lib):
    return request.param


# -------------------------------------------------------------------------------------------------------------------- randn
# The kernel's error against exact arithmetic on the same fp32 uniforms, from the documented bounds of the device functions it
# calls (HIP math API: logf 1 ulp, sqrtf 1 ulp, sincospif 1 ulp; 1 ulp <= 2^-23 relative):
#   L = logf(u)              relative error e1, |e1| <= 2^-23;  -2 L is exact
#   r = sqrtf(-2 L)          sqrt halves e1 and adds its own rounding: <= 2^-24 + 2^-23
#   (c, s) = sincospif(2 u)  the argument is exact in fp32; relative error <= 2^-23
#   z = r c                  one rounding: <= 2^-24
# in sum |dz| <= 3 * 2^-23 |z| <= 6 * 2^-24 r < 6 ulp(r), ulp(x) = 2^(floor(log2 x) - 23) > 2^-24 x.  The float64 restatement's
# own error is 2^-29 of that.  The bound is stated against max(r, 1).
RANDN_ULPS = 6


@pytest.mark.parametrize("n_clips", [1, 3])
def test_randn_against_the_float64_restatement(hip_lib, n_clips):
    from ctrlv_amd import ops
    worst = 0.0
    for per in (1, 3, 4, 5, 1027, 3 * 128 * 192):
        got = ops.randn(SEED, (n_clips, per), clip0=2, call=1, stream_id=1, device=DEV)
        torch.cuda.synchronize()
        z, r = R.randn(SEED, n_clips, per, clip0=2, call=1, stream_id=1)
        ulp = np.exp2(np.floor(np.log2(np.maximum(r, 1.0))) - 23)
        err = np.abs(got.cpu().numpy().astype(np.float64) - z) / ulp
        worst = max(worst, float(err.max()))
        assert got.shape == (n_clips, per) and got.dtype == torch.float32
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= R.MAX_ABS
        assert float(err.max()) <= RANDN_ULPS, (per, float(err.max()))
    print(f"  randn n_clips={n_clips}: largest error {worst:.3f} ulp of max(r, 1) (bound {RANDN_ULPS})")


def test_randn_element_rounding_is_torchs(el):
    """round_dtype = 1 is (z32.to(el) * scale) as torch forms it on the device from the kernel's own fp32 z32 of the same
    counters: what prepare_latents computes for an element-typed randn times the scheduler's Python float."""
    from ctrlv_amd import ops
    scale = math.sqrt(700.0 ** 2 + 1.0)
    for shape in ((2, 3, 4, 16, 24), (3, 1027)):
        z32 = ops.randn(SEED, shape, call=3, stream_id=1, device=DEV)
        want = z32.to(el) * scale
        got32 = ops.randn(SEED, shape, call=3, stream_id=1, scale=scale, round_el=True, el=el, device=DEV)
        got_el = ops.randn(SEED, shape, call=3, stream_id=1, scale=scale, round_el=True, dtype=el, device=DEV)
        assert got32.dtype == torch.float32 and torch.equal(got32, want.float())
        assert got_el.dtype == el and torch.equal(got_el, want)
        plain = ops.randn(SEED, shape, call=3, stream_id=1, scale=0.5, dtype=el, device=DEV)        # round_dtype 0, stored as el
        assert torch.equal(plain, (z32 * 0.5).to(el))


def test_randn_is_keyed_per_clip_and_blind_to_alignment(el):
    from ctrlv_amd import ops
    for dtype in (torch.float32, el):
        for per in (1027, 4 * 260):
            kw = dict(call=2, stream_id=1, dtype=dtype, device=DEV)
            three = ops.randn(SEED, (3, per), clip0=5, **kw)
            for i in range(3):                                   # a clip alone, whatever the batch it is drawn in
                assert torch.equal(three[i], ops.randn(SEED, (1, per), clip0=5 + i, **kw)[0]), (dtype, per, i)
            assert torch.equal(three, ops.randn(SEED, (3, per), clip0=5, **kw))                       # determinism
            # `out` 4 bytes (fp32) / 2 and 4 bytes (elements) off a 16-byte boundary, sentinels around it
            for off in ((1,) if dtype == torch.float32 else (1, 2)):
                buf = Gd.fill_(torch.empty(3 * per + 64, dtype=dtype, device=DEV), "sentinel")
                before = buf.clone()
                assert buf.data_ptr() % 16 == 0
                view = buf[off:off + 3 * per].view(3, per)
                ops.randn(SEED, (3, per), clip0=5, out=view, **kw)
                torch.cuda.synchronize()
                assert torch.equal(view, three), (dtype, per, off)
                assert torch.equal(Gd.as_int(buf[:off]), Gd.as_int(before[:off]))
                assert torch.equal(Gd.as_int(buf[off + 3 * per:]), Gd.as_int(before[off + 3 * per:]))
    base = ops.randn(SEED, (2, 1027), device=DEV)
    for other in (dict(seed=SEED ^ 1), dict(seed=SEED ^ (1 << 63)), dict(call=1), dict(stream_id=1), dict(clip0=1)):
        kw = dict(dict(seed=SEED), **other)
        assert not torch.equal(base, ops.randn(kw.pop("seed"), (2, 1027), device=DEV, **kw)), other


# ------------------------------------------------------------------------------------------------------------------ Lanczos
@pytest.mark.parametrize("src,dst", LANCZOS_SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in LANCZOS_SHAPES])
def test_lanczos_is_pil_byte_for_byte_and_writes_nowhere_else(hip_lib, src, dst):
    from PIL import Image
    from ctrlv_amd import _lib, ops
    rng = np.random.default_rng(src[1] * 3 + dst[0])
    img = rng.integers(0, 256, size=(2, src[0], src[1], 3), dtype=np.uint8)
    img[0, :8, :8] = 255                                         # saturated corners: the overshoot of the negative lobes clips
    img[1, -8:, -8:] = 0
    want = torch.from_numpy(np.stack([np.asarray(Image.fromarray(im).resize((dst[1], dst[0]), resample=Image.LANCZOS))
                                      for im in img]))
    x = torch.from_numpy(img).to(DEV)
    got = ops.resize_lanczos_u8(x, *dst)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    # the same call into guard-banded dst and ws: nothing outside is written, every output byte is
    need = _lib.load().ctrlv_resize_lanczos_ws_bytes(2, src[0], src[1], dst[0], dst[1])
    obuf, oflat = Gd.guarded_flat(want.numel(), torch.uint8, DEV)
    wbuf, wflat = Gd.guarded_flat(need, torch.uint8, DEV)
    assert wflat.data_ptr() % 16 == 0
    o0, w0 = obuf.clone(), wbuf.clone()
    ops.resize_lanczos_u8(x, *dst, out=oflat.view(want.shape), workspace=wflat)
    torch.cuda.synchronize()
    Gd.check_written_only_inside(o0, obuf, oflat.view(1, -1), expected=want.view(1, -1), what="resize_lanczos_u8 dst")
    changed = Gd.as_int(wbuf) != Gd.as_int(w0)
    lo = wflat.storage_offset() - wbuf.storage_offset()
    changed.view(-1)[lo:lo + need] = False
    assert not bool(changed.any()), "resize_lanczos_u8 wrote outside its workspace"
    assert torch.equal(oflat.view(want.shape).cpu(), want)


# ------------------------------------------------------------------------------------------------------------------- driver
@pytest.fixture(scope="module")
def setup(el):
    s = build_setup(el)
    s.src = torch.randint(0, 256, (2, SH, SW, 3), generator=torch.Generator().manual_seed(21), dtype=torch.uint8).to(DEV)
    return s


KW = dict(noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0, max_guidance=3.0, conditioning_scale=0.8,
          decode_chunk=2)


def by_hand(s, n, call=0, clip0=0, seed=SEED):
    """What prepare fills, through the wrappers of the single entry points."""
    from ctrlv_amd import ops
    from ctrlv_amd.plan import euler_schedule
    img = ops.resize_lanczos_u8(s.src[:n], H, W)
    aug = ops.randn(seed, (n, 3, H, W), clip0=clip0, call=call, stream_id=0, device=DEV)
    sig, ts, ins = euler_schedule(STEPS)
    lat = ops.randn(seed, (n, F, 4, H // 8, W // 8), clip0=clip0, call=call, stream_id=1, scale=ins, round_el=True, el=s.el,
                    device=DEV)
    return img, aug, lat, sig, ts


@pytest.mark.parametrize("n", [1, 2])
def test_generate_seeded_is_generate_fed_by_hand(setup, n):
    s = setup
    img, aug, lat, sig, ts = by_hand(s, n, call=4, clip0=3)
    assert sig == list(s.sigmas) and max(abs(a - b) for a, b in zip(ts, s.timesteps)) <= 2.0 ** -22      # ln 700 / 4 < 2
    want = s.pipe.generate(img, lat, sig, ts, cond=s.cond[:n], aug_noise=aug, **KW)
    got = s.pipe.generate(s.src[:n], seed=SEED, clip_index0=3, call=4, num_steps=STEPS, num_frames=F, height=H, width=W,
                          cond=s.cond[:n], **KW)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0
    same(got, want)
    # a host that brings its own latents still takes the rest; an image at the working size is used as it is
    own = s.pipe.generate(img, latents=lat, seed=SEED, clip_index0=3, call=4, num_steps=STEPS, cond=s.cond[:n], **KW)
    torch.cuda.synchronize()
    same(own, want)


@pytest.mark.parametrize("n", [1, 2])
def test_predict_boxes_and_the_chain_with_a_seed(setup, n):
    from ctrlv_amd.plan import boxes_to_video
    s = setup
    boxes = s.cond[:n]
    img, aug0, lat0, sig, ts = by_hand(s, n, call=0)
    _, aug1, lat1, _, _ = by_hand(s, n, call=1)
    want = s.pipe_svd.predict_boxes(img, lat0, sig, ts, boxes, K, aug_noise=aug0, **KW)
    got = s.pipe_svd.predict_boxes(s.src[:n], None, None, None, boxes, K, seed=SEED, num_steps=STEPS, height=H, width=W, **KW)
    torch.cuda.synchronize()
    same(got, want)
    size = dict(KW, height=H, width=W)
    want = boxes_to_video(s.pipe_svd, s.pipe, img, lat0, lat1, (sig, ts), (sig, ts), boxes, K, box_aug_noise=aug0,
                          video_aug_noise=aug1, box_kw=KW, video_kw=KW)
    got = boxes_to_video(s.pipe_svd, s.pipe, s.src[:n], None, None, None, None, boxes, K, seed=SEED, num_steps=STEPS,
                         box_kw=size, video_kw=size)
    torch.cuda.synchronize()
    same(got[:3], want[:3])
    assert torch.equal(got[3], want[3])


def _filled(ws, ptr, shape):
    off = int(ptr) - ws.data_ptr()
    numel = int(np.prod(shape))
    assert 0 <= off and off + 4 * numel <= ws.numel()
    return ws[off:off + 4 * numel].view(torch.float32).view(shape)


def test_prepared_noise_is_keyed_per_clip_and_the_sizes_add_up(setup):
    s = setup
    pipe, lib = s.pipe, s.pipe._lib
    kw = dict(num_steps=STEPS, num_frames=F, height=H, width=W, cond=s.cond, **KW)
    keep2 = pipe._stage_request("test", s.src, seed=SEED, **kw)
    r2, s2 = keep2.request, keep2.seed_request
    f2, ws2 = pipe.prepare(r2, s2)
    keep1 = pipe._stage_request("test", s.src[1:], seed=SEED, clip_index0=1, **dict(kw, cond=s.cond[1:]))
    r1, s1 = keep1.request, keep1.seed_request
    f1, ws1 = pipe.prepare(r1, s1)
    torch.cuda.synchronize()
    for name, shape in (("latents", (F, 4, H // 8, W // 8)), ("aug_noise", (3, H, W))):
        two = _filled(ws2, getattr(f2, name), (2,) + shape)
        one = _filled(ws1, getattr(f1, name), (1,) + shape)
        assert torch.equal(two[1], one[0]), name
        assert not torch.equal(two[0], two[1]) and bool(torch.isfinite(two).all())
    assert [f2.sigmas[i] for i in range(STEPS + 1)] == list(s.sigmas) and f2.num_steps == STEPS
    assert f2.cond == r2.cond and f2.out_latents == r2.out_latents and f2.image_u8 != s2.src_image_u8
    # seeded workspace = prepare's bytes (a multiple of the 256-byte alignment) + generate's for the filled request
    prep = lib.ctrlv_pipeline_prepare_bytes(pipe._h, ctypes.byref(r2), ctypes.byref(s2))
    assert prep == ws2.numel() and prep % 256 == 0
    rest = lib.ctrlv_pipeline_workspace_bytes(pipe._h, ctypes.byref(f2))
    assert rest > 0 and lib.ctrlv_pipeline_seeded_workspace_bytes(pipe._h, ctypes.byref(r2), ctypes.byref(s2)) == prep + rest
    # the prepared request is an ordinary one: generate takes it
    out = pipe._workspace(rest)
    assert lib.ctrlv_pipeline_generate(pipe._h, ctypes.byref(f2), out.data_ptr(), out.numel(), pipe._stream()) == 0
    torch.cuda.synchronize()
    del keep1, keep2


def test_seeded_clip_from_a_foreign_host(setup):
    """Raw ctypes only, on the pipeline the module already loaded: image bytes at 97 x 131 plus a seed, the structs filled field
    by field, no host arrays (the pipeline keeps the schedule), the size query, the call on a non-default stream.  Bit-equal to
    the Python wrapper; 4 KiB of pattern behind the workspace survive."""
    from ctrlv_amd import _lib
    s = setup
    lib = _lib.load(s.el)
    want = s.pipe.generate(s.src[:1], seed=SEED, num_steps=STEPS, num_frames=F, height=H, width=W, cond=s.cond[:1], **KW)
    torch.cuda.synchronize()
    out_lat = torch.zeros(1, F, 4, H // 8, W // 8, device=DEV)
    out_fr = torch.zeros(F, 3, H, W, dtype=s.el, device=DEV)
    out_u8 = torch.zeros(1, F, H, W, 3, dtype=torch.uint8, device=DEV)
    src, cond = s.src[:1].contiguous(), s.cond[:1].contiguous()
    r = _lib.ClipRequest()
    r.n_clips, r.num_frames, r.height, r.width = 1, F, H, W
    r.cond, r.cond_channels, r.cond_dtype = cond.data_ptr(), 3, 0
    r.noise_aug_strength, r.num_steps = 0.02, STEPS
    r.fps, r.motion_bucket_id, r.min_guidance, r.max_guidance, r.conditioning_scale, r.decode_chunk = 7, 127, 1.0, 3.0, 0.8, 2
    r.out_latents, r.out_frames, r.out_frames_u8 = out_lat.data_ptr(), out_fr.data_ptr(), out_u8.data_ptr()
    q = _lib.SeedRequest()
    q.seed, q.src_image_u8, q.src_height, q.src_width = SEED, src.data_ptr(), SH, SW
    need = lib.ctrlv_pipeline_seeded_workspace_bytes(s.pipe._h, ctypes.byref(r), ctypes.byref(q))
    assert need > 0 and need % 256 == 0, _lib.last_error(lib)
    buf = torch.empty(need + 4096, dtype=torch.uint8, device=DEV)
    buf[need:] = 0xA5
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    st = ctypes.c_void_p(stream.cuda_stream)
    assert lib.ctrlv_pipeline_generate_seeded(s.pipe._h, ctypes.byref(r), ctypes.byref(q), buf.data_ptr(), need - 1, st) == -5
    assert lib.ctrlv_pipeline_generate_seeded(s.pipe._h, ctypes.byref(r), ctypes.byref(q), buf.data_ptr(), need, st) == 0, \
        _lib.last_error(lib)
    stream.synchronize()
    torch.cuda.synchronize()
    same((out_lat, out_fr, out_u8), want)
    assert bool((buf[need:] == 0xA5).all())


# ---------------------------------------------------------------------------------------------------------------- DeviceSeed
def test_device_seed_through_the_pipelines(hip_lib, monkeypatch):
    """StableVideoControlPipeline (bf16, the element type the route serves) with a PIL image at 97 x 131: generator=DeviceSeed
    on CTRLV_PIPELINE=plan is PipelinePlan.generate(seed=...) on the image's own bytes; on the default route it raises by
    name.  A torch generator on the plan route still draws on the host in the order it always did: the call equals
    PipelinePlan.generate fed with PIL's resize, randn_tensor twice and the scheduler's tables."""
    import ctrlv_ref as Ref
    from PIL import Image
    import ctrlv_amd
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.pipelines import StableVideoControlPipeline
    from ctrlv_amd.pipelines.pipeline_utils import MinimalCLIPImageProcessor, randn_tensor
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from tests import clip_utils as U
    from tests.parity_utils import make_pair
    BF = torch.bfloat16
    _, _, hu, hc = make_pair(dict(Ref.TINY_CONFIG), DEV)
    torch.manual_seed(5)
    vae = AutoencoderKLTemporalDecoder().eval().to(DEV, BF)
    clip = U.build_own(dict(PIPE_CLIP, image_size=224), 31, BF, DEV)
    pipe = StableVideoControlPipeline(vae, clip, hu, hc, EulerDiscreteScheduler(), MinimalCLIPImageProcessor())
    pipe.set_progress_bar_config(disable=True)
    g0 = torch.Generator().manual_seed(11)
    host = torch.randint(0, 256, (SH, SW, 3), generator=g0, dtype=torch.uint8)
    image = Image.fromarray(host.numpy())
    cond = (torch.rand(1, F, 3, H, W, generator=g0) * 2 - 1).to(DEV)
    monkeypatch.setenv("CTRLV_VAE_HIP", "plan")
    monkeypatch.setenv("CTRLV_CLIP_HIP", "plan")

    def run(generator, output_type):
        return pipe(image, cond_images=cond, height=H, width=W, num_frames=F, num_inference_steps=STEPS, decode_chunk_size=2,
                    generator=generator, output_type=output_type).frames

    monkeypatch.delenv("CTRLV_PIPELINE", raising=False)
    with pytest.raises(ValueError, match="CTRLV_PIPELINE=plan"):
        run(ctrlv_amd.DeviceSeed(5), "latent")
    monkeypatch.setenv("CTRLV_PIPELINE", "plan")
    fe = pipe.feature_extractor
    kw = dict(cond=cond, noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0, max_guidance=3.0,
              conditioning_scale=1.0, decode_chunk=2, clip_mean=fe.image_mean, clip_std=fe.image_std)
    pp = pipe._pipeline_plan()
    assert pp is not None
    want = pp.generate(host[None].to(DEV), seed=5, clip_index0=2, num_steps=STEPS, num_frames=F, height=H, width=W, **kw)
    torch.cuda.synchronize()
    lat = run(ctrlv_amd.DeviceSeed(5, clip_index0=2), "latent")
    assert lat.dtype == BF and torch.equal(lat, want[0].to(BF))
    pil = run(ctrlv_amd.DeviceSeed(5, clip_index0=2), "pil")
    assert len(pil) == 1 and len(pil[0]) == F and pil[0][0].size == (W, H)
    assert np.array_equal(np.stack([np.asarray(f) for f in pil[0]]), want[2][0].cpu().numpy())
    # a torch generator on the plan route: the host-side draws and PIL's resize, as before
    gen = torch.Generator().manual_seed(7)
    got = run(gen, "latent")
    gen = torch.Generator().manual_seed(7)
    resized = torch.from_numpy(np.asarray(image.resize((W, H), resample=Image.LANCZOS))[None].copy()).to(DEV)
    aug = randn_tensor((1, 3, H, W), generator=gen, device=torch.device(DEV), dtype=torch.float32)
    sched = EulerDiscreteScheduler()
    sched.set_timesteps(STEPS, device=DEV)
    lat0 = randn_tensor((1, F, 4, H // 8, W // 8), generator=gen, device=torch.device(DEV), dtype=BF) * sched.init_noise_sigma
    ref = pp.generate(resized, lat0.float(), list(sched._sigmas_host), list(sched._timesteps_host), aug_noise=aug, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got, ref[0].to(BF))
