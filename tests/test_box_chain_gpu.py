"""The box predictor and the boxes-to-video chain on the device (include/ctrlv_hip.h: ctrlv_pipeline_predict_boxes,
ctrlv_pipeline_boxes_to_video; csrc/pipeline.hip), bit for bit against the same kernels called one by one.  Models, inputs and
the composition are those of tests/test_pipeline_plan_gpu.py (tiny models, 1 clip x 3 frames x 128 x 192, 2 steps), reused by
import; the box frames are that module's ControlNet condition tensors.

The composition of the box predictor is `compose` without a ControlNet, with the box latents written into `image_latents` the way
VideoDiffusionPipeline.__call__ writes them (cat[zeros, latents] with guidance; frames [0, K) and the last one): the stepper
`compose` builds is handed the overwritten tensor."""
import contextlib
import ctypes

import pytest
import torch

from tests.test_pipeline_plan_gpu import DEV, F, H, N, STEPS, W, _venc, bits, build_setup, compose, same

pytestmark = pytest.mark.gpu
THRESHOLD = 50.0


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def el(request, hip_lib):
    return request.param


@pytest.fixture(scope="module")
def setup(el):
    return build_setup(el)


def _boxes(s, n, kind):
    return s.cond[:n] if kind == "pixels" else s.cond_lat[:n]


@contextlib.contextmanager
def _stepper_with_boxes(s, n, K, cfg, kind):
    """pipeline_video_diffusion.py:200-206 on the image_latents `compose` hands its DenoiseStepper."""
    from ctrlv_amd.pipelines import pipeline_utils as PU
    real = PU.DenoiseStepper

    def stepper(unet, controlnet, sched, latents, image_latents, *a, **kw):
        lat = s.cond_lat[:n] if kind == "latents" else \
            _venc(s, s.cond[:n].to(s.el).flatten(0, 1)).reshape(n, F, 4, H // 8, W // 8)
        if cfg:
            lat = torch.cat([torch.zeros_like(lat), lat])
        image_latents = image_latents.clone()
        lat = lat.to(image_latents.dtype)
        image_latents[:, 0:K] = lat[:, 0:K]
        image_latents[:, -1] = lat[:, -1]
        return real(unet, controlnet, sched, latents, image_latents, *a, **kw)

    PU.DenoiseStepper = stepper
    try:
        yield
    finally:
        PU.DenoiseStepper = real


def compose_boxes(s, n, *, K, cfg=True, kind="pixels"):
    with _stepper_with_boxes(s, n, K, cfg, kind):
        lat, frames, u8 = compose(s, n, use_cn=False, cfg=cfg)
    return lat, frames, u8


def predict(s, n, *, K, cfg=True, kind="pixels", **kw):
    out = s.pipe_svd.predict_boxes(s.image[:n], s.lat[:n], s.sigmas, s.timesteps, _boxes(s, n, kind), K, aug_noise=s.aug[:n],
                                   noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0,
                                   max_guidance=3.0 if cfg else 1.0, decode_chunk=2, **kw)
    torch.cuda.synchronize()
    return out


VARIANTS = {
    "K1": dict(K=1),                                        # frames 0 and 2 taken: two encoder calls per clip
    "K0": dict(K=0),                                        # the last frame only
    "K3": dict(K=3),                                        # K = F: every frame, one encoder call
    "K1_cfg_off": dict(K=1, cfg=False),
    "K1_latents": dict(K=1, kind="latents"),
    "K0_latents_cfg_off": dict(K=0, kind="latents", cfg=False),
    "K1_two_clips": dict(K=1, n=2),
    "K3_latents_two_clips": dict(K=3, kind="latents", n=2),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_predict_boxes_is_the_same_kernels_called_one_by_one(setup, variant):
    """... and encoding only the taken frames gives the bits of encoding all F (the composition encodes all F); out_frames is
    the composition's frames clamped to [-1, 1], out_frames_u8 its bytes unchanged."""
    kw = dict(VARIANTS[variant])
    n = kw.pop("n", N)
    lat, frames, u8 = compose_boxes(setup, n, **kw)
    got = predict(setup, n, **kw)
    print(f"  {variant}: decoded frames in [{float(frames.min()):.3f}, {float(frames.max()):.3f}]")
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0
    assert float(got[1].min()) >= -1.0 and float(got[1].max()) <= 1.0
    same(got, (lat, frames.clamp(-1, 1), u8))
    if variant == "K0":                                      # even the one frame of K = 0 reaches the model
        plain = compose(setup, n, use_cn=False, cfg=True)
        assert not torch.equal(bits(plain[0]), bits(lat))


def test_the_clamp_is_applied_to_out_frames_only(setup):
    """A box condition far outside [-1, 1] as latents drives the decoded frames out of range: out_frames is clamped, the
    bytes are those of the unclamped frames (ctrlv_frames_to_u8 clamps itself), and without out_frames nothing changes."""
    s = setup
    big = (s.cond_lat[:N].float() * 40).to(s.el)
    keep = s.cond_lat
    s.cond_lat = torch.cat([big, keep[N:]])
    try:
        lat, frames, u8 = compose_boxes(s, N, K=3, kind="latents")
        got = predict(s, N, K=3, kind="latents")
        only_u8 = predict(s, N, K=3, kind="latents", frames=False)
    finally:
        s.cond_lat = keep
    print(f"  decoded frames in [{float(frames.min()):.3f}, {float(frames.max()):.3f}]")
    assert float(frames.float().abs().max()) > 1.0, "the input no longer drives the frames out of range: scale it up"
    assert float(got[1].min()) >= -1.0 and float(got[1].max()) <= 1.0
    same(got, (lat, frames.clamp(-1, 1), u8))
    assert only_u8[1] is None and torch.equal(only_u8[2], u8) and torch.equal(bits(only_u8[0]), bits(lat))


def _by_hand(s, n, K):
    from ctrlv_amd import ops
    _, frames, _ = predict(s, n, K=K, frames_u8=False)
    _, cond, clean = ops.box_frames_post(frames, F, THRESHOLD, pt=False)
    out = s.pipe.generate(s.image[:n], s.lat[:n], s.sigmas, s.timesteps, cond=cond.view(n, F, 3, H, W), aug_noise=s.aug[:n],
                          noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0, max_guidance=3.0,
                          conditioning_scale=0.8, decode_chunk=2)
    torch.cuda.synchronize()
    return out, clean


def _chain(s, n, K, **kw):
    from ctrlv_amd.plan import boxes_to_video
    sched = (s.sigmas, s.timesteps)
    common = dict(noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0, max_guidance=3.0, decode_chunk=2)
    out = boxes_to_video(s.pipe_svd, s.pipe, s.image[:n], s.lat[:n], s.lat[:n], sched, sched, s.cond[:n], K,
                         box_aug_noise=s.aug[:n], video_aug_noise=s.aug[:n], clean_threshold=THRESHOLD, box_kw=common,
                         video_kw=dict(common, conditioning_scale=0.8), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n", [1, 2])
def test_boxes_to_video_is_the_three_calls_by_hand(setup, n):
    want, clean = _by_hand(setup, n, 1)
    got = _chain(setup, n, 1)
    same(got[:3], want)
    assert got[3].shape == (n, F, 3, H, W) and torch.equal(got[3], clean)
    assert bool(got[3].any())


def _requests(s, n=N, K=1, cond=None):
    """(boxes request, box condition, video request, keep) around fresh outputs."""
    from ctrlv_amd.plan import PipelinePlan
    image, lat = s.image[:n].contiguous(), s.lat[:n].contiguous()
    outs = dict(lat_b=torch.full_like(lat, 7.0), lat_v=torch.full_like(lat, 7.0),
                fr=torch.zeros(n * F, 3, H, W, dtype=s.el, device=DEV), u8=torch.zeros(n, F, H, W, 3, dtype=torch.uint8, device=DEV),
                clean=torch.zeros(n, F, 3, H, W, dtype=torch.uint8, device=DEV))
    common = dict(aug_noise=s.aug[:n].contiguous(), noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0,
                  max_guidance=3.0, decode_chunk=2)
    rb, kb = s.pipe_svd.request(image, lat, s.sigmas, s.timesteps, out_latents=outs["lat_b"], **common)
    rv, kv = s.pipe.request(image, lat, s.sigmas, s.timesteps, cond=cond, conditioning_scale=0.8, out_latents=outs["lat_v"],
                            out_frames=outs["fr"], out_frames_u8=outs["u8"], **common)
    boxes = s.cond[:n].contiguous()
    return rb, PipelinePlan.box_condition(boxes, K), rv, (kb, kv, boxes), outs


def test_workspace_queries_and_the_too_small_workspace(setup):
    """Both queries answer the size their call accepts (one byte less is CTRLV_E_WORKSPACE with the needed size in the message and
    nothing launched) and 0, with ctrlv_last_error set, for a request the call refuses."""
    from ctrlv_amd import _lib
    s = setup
    lib = s.pipe._lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rb, bc, rv, keep, outs = _requests(s)
    rb.out_frames = outs["fr"].data_ptr()
    need = lib.ctrlv_pipeline_boxes_workspace_bytes(s.pipe_svd._h, ctypes.byref(rb), ctypes.byref(bc))
    assert need > 0 and need % 256 == 0
    assert need >= lib.ctrlv_pipeline_workspace_bytes(s.pipe_svd._h, ctypes.byref(rb))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.ctrlv_pipeline_predict_boxes(s.pipe_svd._h, ctypes.byref(rb), ctypes.byref(bc), ws.data_ptr(), need - 1, st) == -5
    assert str(need) in _lib.last_error(lib) and "ws_bytes" in _lib.last_error(lib)
    assert lib.ctrlv_pipeline_predict_boxes(s.pipe_svd._h, ctypes.byref(rb), ctypes.byref(bc), ws.data_ptr(), need, st) == 0
    torch.cuda.synchronize()
    assert bool((outs["lat_b"] != 7.0).any())
    bc.num_cond_frames = F + 1
    assert lib.ctrlv_pipeline_boxes_workspace_bytes(s.pipe_svd._h, ctypes.byref(rb), ctypes.byref(bc)) == 0
    assert "num_cond_frames" in _lib.last_error(lib)
    assert lib.ctrlv_pipeline_boxes_workspace_bytes(s.pipe._h, ctypes.byref(rb), ctypes.byref(bc)) == 0
    assert "has a ControlNet" in _lib.last_error(lib)

    rb, bc, rv, keep, outs = _requests(s)
    q = _lib.TwoStageRequest()
    q.boxes, q.box_cond, q.video, q.out_box_frames_u8, q.clean_threshold = rb, bc, rv, outs["clean"].data_ptr(), THRESHOLD
    need = lib.ctrlv_pipeline_chain_workspace_bytes(s.pipe_svd._h, s.pipe._h, ctypes.byref(q))
    assert need > 0 and need % 256 == 0, _lib.last_error(lib)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.ctrlv_pipeline_boxes_to_video(s.pipe_svd._h, s.pipe._h, ctypes.byref(q), ws.data_ptr(), need - 1, st) == -5
    assert str(need) in _lib.last_error(lib) and "ws_bytes" in _lib.last_error(lib)
    torch.cuda.synchronize()
    assert bool((outs["lat_b"] == 7.0).all()) and bool((outs["lat_v"] == 7.0).all()) and not bool(outs["clean"].any())
    q.video.num_frames = F - 1
    assert lib.ctrlv_pipeline_chain_workspace_bytes(s.pipe_svd._h, s.pipe._h, ctypes.byref(q)) == 0
    assert "geometry" in _lib.last_error(lib)
    q.video.num_frames = F
    assert lib.ctrlv_pipeline_chain_workspace_bytes(s.pipe._h, s.pipe._h, ctypes.byref(q)) == 0
    assert "has a ControlNet" in _lib.last_error(lib)


def test_the_chain_from_a_foreign_host(setup):
    """Raw ctypes only, on the plans the module already loaded: two pipelines created through the C ABI, the request struct
    filled field by field, the workspace query, the call on a non-default stream.  Bit-equal to the calls by hand; 4 KiB of
    pattern behind the workspace survive; a second call gives the same bits."""
    from ctrlv_amd import _lib
    s = setup
    lib = _lib.load(s.el)
    want, clean = _by_hand(s, N, 1)
    unet, cn, vae, clip = (p._h for p in s.plans)
    hb, hv = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.ctrlv_pipeline_create(unet, None, vae, clip, 0, ctypes.byref(hb)) == 0, _lib.last_error(lib)
    assert lib.ctrlv_pipeline_create(unet, cn, vae, clip, 0, ctypes.byref(hv)) == 0, _lib.last_error(lib)
    image, boxes, aug, lat = (t[:N].contiguous() for t in (s.image, s.cond, s.aug, s.lat))
    out_lat_b, out_lat = torch.zeros_like(lat), torch.zeros_like(lat)
    out_fr = torch.zeros(N * F, 3, H, W, dtype=s.el, device=DEV)
    out_u8 = torch.zeros(N, F, H, W, 3, dtype=torch.uint8, device=DEV)
    out_clean = torch.zeros(N, F, 3, H, W, dtype=torch.uint8, device=DEV)
    sig, ts = (ctypes.c_float * (STEPS + 1))(*s.sigmas), (ctypes.c_float * STEPS)(*s.timesteps)
    q = _lib.TwoStageRequest()
    for r, o in ((q.boxes, out_lat_b), (q.video, out_lat)):
        r.n_clips, r.num_frames, r.height, r.width = N, F, H, W
        r.image_u8, r.aug_noise, r.noise_aug_strength, r.num_steps, r.latents = image.data_ptr(), aug.data_ptr(), 0.02, STEPS, lat.data_ptr()
        r.sigmas, r.timesteps = sig, ts
        r.fps, r.motion_bucket_id, r.min_guidance, r.max_guidance, r.conditioning_scale, r.decode_chunk = 7, 127, 1.0, 3.0, 0.8, 2
        r.out_latents = o.data_ptr()
    q.video.out_frames, q.video.out_frames_u8 = out_fr.data_ptr(), out_u8.data_ptr()
    q.box_cond.frames, q.box_cond.channels, q.box_cond.dtype, q.box_cond.num_cond_frames = boxes.data_ptr(), 3, 0, 1
    q.out_box_frames_u8, q.clean_threshold = out_clean.data_ptr(), THRESHOLD
    need = lib.ctrlv_pipeline_chain_workspace_bytes(hb, hv, ctypes.byref(q))
    assert need > 0 and need % 256 == 0, _lib.last_error(lib)
    buf = torch.empty(need + 4096, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf[need:] = 0xA5
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    st = ctypes.c_void_p(stream.cuda_stream)
    outs = (out_lat, out_fr, out_u8)
    for _ in range(2):
        for t in outs + (out_clean,):
            t.zero_()
        torch.cuda.synchronize()
        assert lib.ctrlv_pipeline_boxes_to_video(hb, hv, ctypes.byref(q), buf.data_ptr(), need, st) == 0, _lib.last_error(lib)
        stream.synchronize()
        torch.cuda.synchronize()
        same(outs, want)
        assert torch.equal(out_clean, clean) and bool((buf[need:] == 0xA5).all())
    assert lib.ctrlv_pipeline_destroy(hb) == 0 and lib.ctrlv_pipeline_destroy(hv) == 0


def test_the_pipeline_route_takes_box_frames(hip_lib, monkeypatch):
    """VideoDiffusionPipeline with a PIL image and tensor bbox_images: CTRLV_PIPELINE=plan goes through predict_boxes and gives
    what the Python route gives (both under CTRLV_VAE_HIP=plan, CTRLV_CLIP_HIP=plan) within the project's bound for a
    pipeline-level route comparison, 3e-2 (tests/test_pipeline_plan_gpu.py: test_the_pipeline_route); unset, it is not entered."""
    import ctrlv_ref as R
    from PIL import Image
    from ctrlv_amd import plan as plan_mod
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.pipelines import VideoDiffusionPipeline
    from ctrlv_amd.pipelines.pipeline_utils import MinimalCLIPImageProcessor
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from tests import clip_utils as U
    from tests.parity_utils import make_pair, parity_err
    from tests.test_pipeline_plan_gpu import PIPE_CLIP, gen
    BF = torch.bfloat16
    _, _, hu, _ = make_pair(dict(R.TINY_CONFIG), DEV)
    torch.manual_seed(5)
    vae = AutoencoderKLTemporalDecoder().eval().to(DEV, BF)
    clip = U.build_own(dict(PIPE_CLIP, image_size=224), 31, BF, DEV)
    pipe = VideoDiffusionPipeline(vae, clip, hu, EulerDiscreteScheduler(), MinimalCLIPImageProcessor())
    pipe.set_progress_bar_config(disable=True)
    g0 = gen(11)
    image = Image.fromarray(torch.randint(0, 256, (H, W, 3), generator=g0, dtype=torch.uint8).numpy())
    boxes = (torch.rand(1, F, 3, H, W, generator=g0) * 2 - 1).to(DEV)
    calls = []
    real = plan_mod.PipelinePlan.predict_boxes
    monkeypatch.setattr(plan_mod.PipelinePlan, "predict_boxes", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    monkeypatch.setenv("CTRLV_VAE_HIP", "plan")
    monkeypatch.setenv("CTRLV_CLIP_HIP", "plan")

    def run(**kw):
        return pipe(image, bbox_images=boxes, height=H, width=W, num_frames=F, num_inference_steps=STEPS, decode_chunk_size=2,
                    generator=gen(7), output_type="pt", num_cond_bbox_frames=1, **kw).frames.float().cpu()

    monkeypatch.delenv("CTRLV_PIPELINE", raising=False)
    ref = run()
    assert not calls
    monkeypatch.setenv("CTRLV_PIPELINE", "plan")
    got = run()
    assert len(calls) == 1
    assert got.shape == ref.shape == (1, F, 3, H, W) and got.min() >= 0 and got.max() <= 1
    assert parity_err(got, ref, "box predictor frames, one C call vs the Python pipeline") < 3e-2
