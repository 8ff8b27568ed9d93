"""Seeded clips where no GPU is needed (include/ctrlv_hip.h, "Seeded clips"): the numpy restatements of tests/seeded_ref.py
against their own ground truth -- Random123's known answers, the moments of a normal sample, PIL's Lanczos resize --, the
host-only ctrlv_euler_schedule against the Python scheduler, and the refusals of the new entry points, every one named and in
front of any launch.

Workspace sizes: ctrlv_pipeline_prepare_bytes is arithmetic on the plans' configurations and is checked here;
ctrlv_pipeline_workspace_bytes exists only for plans whose weights are loaded (tests/test_pipeline_plan_cpu.py), so the identity
seeded = prepare + generate's is checked on the device (tests/test_seeded_gpu.py) and here only that the query refuses like
its parts."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as g
from tests import seeded_ref as R

CLIP_CFG = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=128, patch_size=16,
                projection_dim=64, hidden_act="gelu", layer_norm_eps=1e-5)
VAE_CFG = dict(in_channels=3, out_channels=3, latent_channels=4, layers_per_block=2, block_out_channels=(128, 256, 512, 512),
               scaling_factor=0.18215)
NEW = ("ctrlv_randn", "ctrlv_euler_schedule", "ctrlv_resize_lanczos_ws_bytes", "ctrlv_resize_lanczos_u8",
       "ctrlv_pipeline_prepare_bytes", "ctrlv_pipeline_prepare", "ctrlv_pipeline_seeded_workspace_bytes",
       "ctrlv_pipeline_generate_seeded")
LANCZOS_SHAPES = (((375, 1242), (320, 512)), ((720, 1280), (576, 1024)), ((97, 131), (64, 96)), ((64, 96), (128, 192)),
                  ((50, 70), (50, 35)))


@pytest.fixture(scope="module")
def libs():
    g.build()
    from ctrlv_amd import _lib
    return {torch.bfloat16: _lib.load(torch.bfloat16), torch.float16: _lib.load(torch.float16)}


# ------------------------------------------------------------------------------------------------------------------- Philox
def test_philox_known_answers():
    ones = 0xFFFFFFFF
    for counter, key, want in (
            ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
            ((ones,) * 4, (ones, ones), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
            ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
             (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = R.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
        assert tuple(int(v[0]) for v in got) == want, [hex(int(v[0])) for v in got]


def test_uniforms_round_once_and_stay_in_the_half_open_interval():
    x = np.array([0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint64)
    u = R.uniforms(x)
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -33) and u[-1] == np.float32(1.0) and (u > 0).all()
    for xi, ui in zip(x, u):                        # against exact rational arithmetic: the nearest fp32, never two roundings
        exact = (2 * int(xi) + 1) / 2 ** 33        # (a Python float division of two ints is correctly rounded to double,
        assert ui == np.float32(exact)              # and the double holds the 33-bit numerator exactly)
    assert math.sqrt(-2.0 * math.log(2.0 ** -33)) == pytest.approx(R.MAX_ABS)


@pytest.mark.parametrize("seed", [0, 1234, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("stream_id", [0, 1])
def test_moments_within_four_standard_errors(seed, stream_id):
    """N = 2^20 samples of clip 0: mean, variance, skewness, excess kurtosis, the lag-1 product mean and the product mean with
    clip 1 of the same stream, each within 4 standard errors of a standard normal's."""
    N = 1 << 20
    z, _ = R.randn(seed, 2, N, stream_id=stream_id)
    a, b = z[0], z[1]
    m = a.mean()
    d = a - m
    var = (d * d).mean()
    stats = {
        "mean": (m, 1 / math.sqrt(N)),
        "variance": (var - 1.0, math.sqrt(2 / N)),
        "skewness": ((d ** 3).mean() / var ** 1.5, math.sqrt(6 / N)),
        "excess kurtosis": ((d ** 4).mean() / var ** 2 - 3.0, math.sqrt(24 / N)),
        "lag-1 product": ((a[:-1] * a[1:]).mean(), 1 / math.sqrt(N)),
        "product with clip 1": ((a * b).mean(), 1 / math.sqrt(N)),
    }
    for name, (v, se) in stats.items():
        print(f"  seed {seed:#x} stream {stream_id} {name}: {v / se:+.2f} standard errors")
        assert abs(v) <= 4 * se, (name, v, se)
    assert np.abs(z).max() <= R.MAX_ABS


# ----------------------------------------------------------------------------------------------------------------- schedule
def _schedule(lib, n, lo=0.0, hi=0.0):
    sig, ts, ins = (ctypes.c_float * (n + 1))(), (ctypes.c_float * n)(), ctypes.c_double()
    rc = lib.ctrlv_euler_schedule(n, lo, hi, sig, ts, ctypes.byref(ins))
    return rc, np.array(sig, dtype=np.float32), np.array(ts, dtype=np.float32), ins.value


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_the_library_loads_without_a_gpu_and_exports_the_new_symbols(libs):
    from ctrlv_amd import _lib
    for dt, lib in libs.items():
        assert lib.ctrlv_abi_version() == 22 == _lib.ABI_VERSION
        for name in NEW:
            assert name in _lib.SIGNATURES and getattr(lib, name) is not None, (dt, name)


def test_schedule_against_the_python_scheduler(libs):
    """num_steps 1 .. 200: sigmas bit-equal, timesteps within one fp32 ulp (torch takes the logarithm in fp32, the library in
    double: two roundings of one real number), sigmas[n] == 0, init_noise_sigma the scheduler's property as a double."""
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    lib = libs[torch.bfloat16]
    sched = EulerDiscreteScheduler()
    worst = 0
    for n in range(1, 201):
        rc, sig, ts, ins = _schedule(lib, n)
        assert rc == 0
        sched.set_timesteps(n)
        want_sig, want_ts = sched.sigmas.numpy(), sched.timesteps.numpy()
        assert np.array_equal(sig.view(np.int32), want_sig.view(np.int32)), n
        assert sig[n] == 0.0
        worst = max(worst, int(_ulps(ts, want_ts).max()))
        assert ins == sched.init_noise_sigma, (n, ins, sched.init_noise_sigma)
    print(f"  largest timestep difference over 20100 values: {worst} ulp")
    assert worst <= 1


def test_schedule_against_the_golden_tables(libs):
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "scheduler_tables.npz"))
    for lib in libs.values():
        for n in (25, 30, 50):
            rc, sig, ts, ins = _schedule(lib, n)
            assert rc == 0
            assert np.array_equal(sig.view(np.int32), gold[f"sigmas_{n}"].view(np.int32))
            assert int(_ulps(ts, gold[f"timesteps_{n}"]).max()) <= 1
            assert np.float32(ins) == gold[f"init_noise_sigma_{n}"]


def test_schedule_wrapper_and_refusals(libs):
    from ctrlv_amd import _lib
    from ctrlv_amd.plan import euler_schedule
    sig, ts, ins = euler_schedule(25)
    assert len(sig) == 26 and len(ts) == 25 and sig[0] == 700.0 and sig[-1] == 0.0 and ins == math.sqrt(490001.0)
    sig2, _, _ = euler_schedule(4, 0.5, 80.0)
    assert sig2[0] == 80.0 and sig2[3] == 0.5 and sig2[4] == 0.0 and all(a > b for a, b in zip(sig2, sig2[1:]))
    lib = libs[torch.bfloat16]
    for n in (0, -3, 1025):
        sig, ts = (ctypes.c_float * 2)(), (ctypes.c_float * 1)()
        assert lib.ctrlv_euler_schedule(n, 0.0, 0.0, sig, ts, None) == -2 and "num_steps" in _lib.last_error(lib)
        with pytest.raises(ValueError, match="num_steps"):
            euler_schedule(n)
    sig, ts = (ctypes.c_float * 3)(), (ctypes.c_float * 2)()
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (-1.0, 5.0), (0.0, 5.0), (1.0, float("inf")), (float("nan"), 5.0)):
        assert lib.ctrlv_euler_schedule(2, lo, hi, sig, ts, None) == -1 and "sigma_min" in _lib.last_error(lib), (lo, hi)
    assert lib.ctrlv_euler_schedule(2, 0.0, 0.0, None, ts, None) == -1 and "null" in _lib.last_error(lib)
    assert lib.ctrlv_euler_schedule(2, 0.0, 0.0, sig, None, None) == -1 and "null" in _lib.last_error(lib)


# ------------------------------------------------------------------------------------------------------------------ Lanczos
@pytest.mark.parametrize("src,dst", LANCZOS_SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in LANCZOS_SHAPES])
def test_lanczos_restatement_is_pil_byte_for_byte(src, dst):
    from PIL import Image
    rng = np.random.default_rng(src[0] * 7 + dst[1])
    img = rng.integers(0, 256, size=(src[0], src[1], 3), dtype=np.uint8)
    img[:8, :8] = 255                              # saturated corners: the negative lobes overshoot, clip8 is exercised
    img[-8:, -8:] = 0
    want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), resample=Image.LANCZOS))
    got = R.resize_lanczos_u8(img, *dst)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert int((got != want).sum()) == 0


# ----------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def pipes(libs):
    """Pipelines on unloaded plans of the tiny models (bf16 library): create and every host-side check need no GPU."""
    import ctrlv_ref as Ref
    from ctrlv_amd.plan import ClipPlan, Plan, VaePlan
    cfg = dict(Ref.TINY_CONFIG)
    ccfg = {k: v for k, v in cfg.items() if k not in ("out_channels", "up_block_types")}
    plans = Plan("unet", cfg, "cpu"), Plan("controlnet", ccfg, "cpu"), VaePlan(VAE_CFG, "cpu"), ClipPlan(CLIP_CFG, "cpu")
    lib = libs[torch.bfloat16]
    out = []
    for cn in (plans[1], None):
        h = ctypes.c_void_p()
        assert lib.ctrlv_pipeline_create(plans[0]._h, cn._h if cn else None, plans[2]._h, plans[3]._h, 0, ctypes.byref(h)) == 0
        out.append(h)
    yield lib, out[0], out[1], plans
    for h in out:
        lib.ctrlv_pipeline_destroy(h)


def _pair(_lib, keep, steps=2, **over):
    """A (request, seed request) pair prepare accepts: everything prepare can fill is left NULL."""
    r = _lib.ClipRequest()
    r.n_clips, r.num_frames, r.height, r.width = 1, 3, 128, 192
    r.cond, r.cond_channels, r.cond_dtype = 0x2000, 3, 0
    r.noise_aug_strength, r.num_steps = 0.02, steps
    r.out_latents, r.out_frames_u8 = 0x4000, 0x5000
    r.fps, r.motion_bucket_id = 7, 127
    r.min_guidance, r.max_guidance, r.conditioning_scale, r.decode_chunk = 1.0, 3.0, 1.0, 2
    s = _lib.SeedRequest()
    s.seed = 7
    s.src_image_u8, s.src_height, s.src_width = 0x1000, 97, 131
    n = min(max(steps, 1), 1024)
    sig, ts = (ctypes.c_float * (n + 1))(), (ctypes.c_float * n)()
    keep += [sig, ts]
    s.sigmas_host, s.timesteps_host = sig, ts
    for k, v in over.items():
        setattr(s if hasattr(s, k) and not hasattr(r, k) else r, k, v)
    return r, s


def test_prepare_refuses_by_name_before_any_launch(pipes):
    """prepare_bytes, prepare, seeded_workspace_bytes and generate_seeded alike.  The accepted pair reaches check_workspace in
    prepare (a workspace that is too small: CTRLV_E_WORKSPACE with the needed size) and "not loaded" in the seeded entries,
    which proves that every field check sits in front of the first launch."""
    from ctrlv_amd import _lib
    lib, h, h_svd, _ = pipes
    keep = []
    ws = ctypes.c_void_p(0x100000)

    def refused(r, s, word, code=None):
        out = _lib.ClipRequest()
        assert lib.ctrlv_pipeline_prepare_bytes(h, ctypes.byref(r), ctypes.byref(s)) == 0
        m0 = _lib.last_error(lib)
        rc1 = lib.ctrlv_pipeline_prepare(h, ctypes.byref(r), ctypes.byref(s), ctypes.byref(out), ws, 1 << 40, None)
        m1 = _lib.last_error(lib)
        assert lib.ctrlv_pipeline_seeded_workspace_bytes(h, ctypes.byref(r), ctypes.byref(s)) == 0
        m2 = _lib.last_error(lib)
        rc3 = lib.ctrlv_pipeline_generate_seeded(h, ctypes.byref(r), ctypes.byref(s), ws, 1 << 40, None)
        m3 = _lib.last_error(lib)
        assert rc1 < 0 and rc3 < 0 and all(word in m for m in (m0, m1, m2, m3)), (word, rc1, rc3, m0, m1, m2, m3)
        if code is not None:
            assert rc1 == code == rc3
        assert not out.latents and not out.n_clips               # nothing was handed out

    r, s = _pair(_lib, keep)
    need = lib.ctrlv_pipeline_prepare_bytes(h, ctypes.byref(r), ctypes.byref(s))
    # the Lanczos workspace, the resized image, aug_noise (1, 3, 128, 192) fp32 and latents (1, 3, 4, 16, 24) fp32, each a
    # multiple of 256 bytes
    up = lambda v: (v + 255) // 256 * 256                        # noqa: E731
    assert need == up(lib.ctrlv_resize_lanczos_ws_bytes(1, 97, 131, 128, 192)) + up(128 * 192 * 3) + up(3 * 128 * 192 * 4) + \
        up(3 * 4 * 16 * 24 * 4)
    out = _lib.ClipRequest()
    assert lib.ctrlv_pipeline_prepare(h, ctypes.byref(r), ctypes.byref(s), ctypes.byref(out), ws, need - 1, None) == -5
    assert str(need) in _lib.last_error(lib) and "prep" in _lib.last_error(lib)
    assert lib.ctrlv_pipeline_prepare(h, ctypes.byref(r), ctypes.byref(s), ctypes.byref(out), None, need, None) == -1
    # the seeded entries go on to the plans' own workspace answers: these plans have no weights
    assert lib.ctrlv_pipeline_seeded_workspace_bytes(h, ctypes.byref(r), ctypes.byref(s)) == 0 and "not loaded" in _lib.last_error(lib)
    assert lib.ctrlv_pipeline_generate_seeded(h, ctypes.byref(r), ctypes.byref(s), ws, 1 << 40, None) < 0
    assert "not loaded" in _lib.last_error(lib)
    # what the caller brings shrinks the workspace; an image at the working size is a pointer copy
    r2, s2 = _pair(_lib, keep, src_height=128, src_width=192)
    assert lib.ctrlv_pipeline_prepare_bytes(h, ctypes.byref(r2), ctypes.byref(s2)) == up(3 * 128 * 192 * 4) + up(3 * 4 * 16 * 24 * 4)
    r3, s3 = _pair(_lib, keep, aug_noise=0x6000, latents=0x7000, src_height=128, src_width=192)
    assert lib.ctrlv_pipeline_prepare_bytes(h, ctypes.byref(r3), ctypes.byref(s3)) == 256

    refused(*_pair(_lib, keep, reserved=1), "reserved", -1)
    r, s = _pair(_lib, keep)
    s.sigmas_host = None
    out = _lib.ClipRequest()
    assert lib.ctrlv_pipeline_prepare(h, ctypes.byref(r), ctypes.byref(s), ctypes.byref(out), ws, 1 << 40, None) == -1
    assert "sigmas_host" in _lib.last_error(lib)                 # (generate_seeded keeps the arrays itself: not refused there)
    refused(*_pair(_lib, keep, src_height=0), "without sizes", -2)
    refused(*_pair(_lib, keep, src_width=0), "without sizes", -2)
    refused(*_pair(_lib, keep, src_height=128 * 16 + 1), "down-scale above 16", -2)
    refused(*_pair(_lib, keep, src_width=192 * 16 + 1), "down-scale above 16", -2)
    refused(*_pair(_lib, keep, steps=0), "num_steps", -2)
    refused(*_pair(_lib, keep, steps=1025), "num_steps", -2)
    refused(*_pair(_lib, keep, image_u8=0x8000), "both set", -1)
    refused(*_pair(_lib, keep, src_image_u8=None), "image_u8 is null", -1)
    refused(*_pair(_lib, keep, num_frames=33), "num_frames", -2)
    refused(*_pair(_lib, keep, height=120), "height", -2)
    refused(*_pair(_lib, keep, out_latents=None), "out_latents", -1)
    # a ControlNet request without cond is prepared (stage 2 of the chain receives it there); generate_seeded refuses it
    r, s = _pair(_lib, keep, cond=None)
    assert lib.ctrlv_pipeline_prepare_bytes(h, ctypes.byref(r), ctypes.byref(s)) == need
    assert lib.ctrlv_pipeline_generate_seeded(h, ctypes.byref(r), ctypes.byref(s), ws, 1 << 40, None) == -1
    assert "cond is null" in _lib.last_error(lib)
    assert lib.ctrlv_pipeline_prepare_bytes(h_svd, ctypes.byref(r), ctypes.byref(s)) == need
    assert lib.ctrlv_pipeline_prepare(h, None, ctypes.byref(s), ctypes.byref(out), ws, 1 << 40, None) == -1
    assert lib.ctrlv_pipeline_prepare(h, ctypes.byref(r), None, ctypes.byref(out), ws, 1 << 40, None) == -1
    assert lib.ctrlv_pipeline_prepare(h, ctypes.byref(r), ctypes.byref(s), None, ws, 1 << 40, None) == -1


def test_randn_and_lanczos_refuse_on_the_host(libs):
    from ctrlv_amd import _lib
    p = ctypes.c_void_p(0x1000)
    for dt, lib in libs.items():
        code = 2 if dt == torch.bfloat16 else 1
        call = lambda n=1, per=16, out=p, od=0, rd=0, scale=1.0: lib.ctrlv_randn(7, 0, 0, 0, n, per, scale, rd, out, od, None)   # noqa: E731
        assert call(per=(1 << 34) + 1) == -2 and "counter's range" in _lib.last_error(lib)
        assert call(per=0) == -2 and call(n=0) == -2 and "n_clips" in _lib.last_error(lib)
        assert call(out=None) == -1 and "null" in _lib.last_error(lib)
        assert call(od=3 - code) == -4 and "dtype" in _lib.last_error(lib)
        assert call(rd=2) == -1 and "round_dtype" in _lib.last_error(lib)
        assert call(scale=float("inf")) == -1 and "scale" in _lib.last_error(lib)
        assert call(out=ctypes.c_void_p(0x1002)) == -1 and "aligned" in _lib.last_error(lib)
        rz = lambda H, W, h, w, n=1, ws=p, nb=1 << 40: lib.ctrlv_resize_lanczos_u8(p, n, H, W, p, h, w, ws, nb, None)   # noqa: E731
        for shape in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0)):
            assert rz(*shape) == -2 and "zero dimension" in _lib.last_error(lib)
            assert lib.ctrlv_resize_lanczos_ws_bytes(1, *shape) == 0
        assert rz(8, 8, 8, 8, n=0) == -2 and "zero dimension" in _lib.last_error(lib)
        assert rz(129, 8, 8, 8) == -2 and "down-scale above 16" in _lib.last_error(lib)
        assert rz(8, 161, 8, 10) == -2 and "down-scale above 16" in _lib.last_error(lib)
        assert lib.ctrlv_resize_lanczos_ws_bytes(1, 128, 8, 8, 8) > 0                 # exactly 16 is served
        need = lib.ctrlv_resize_lanczos_ws_bytes(2, 97, 131, 64, 96)
        # tables: per output index 2 bounds + 2 ceil(3 in / out) + 1 = 11 weights on either axis; the intermediate (2, 97, 96, 3)
        assert need == (4 * (96 * 13 + 64 * 13) + 255) // 256 * 256 + (2 * 97 * 96 * 3 + 255) // 256 * 256
        assert rz(97, 131, 64, 96, n=2, nb=need - 1) == -5 and str(need) in _lib.last_error(lib)
        assert rz(97, 131, 64, 96, ws=None) == -1 and rz(97, 131, 64, 96, ws=ctypes.c_void_p(0x1008)) == -1


def test_device_seed_is_refused_on_the_default_route_by_name():
    """prepare_clip is the first thing the default route does: the refusal comes before any model or random draw."""
    import ctrlv_amd
    from ctrlv_amd.pipelines.pipeline_utils import SVDPipelineBase
    s = ctrlv_amd.DeviceSeed(2 ** 64 + 5, clip_index0=3)
    assert (s.seed, s.clip_index0) == (5, 3)
    with pytest.raises(ValueError):
        ctrlv_amd.DeviceSeed(1, clip_index0=-1)
    with pytest.raises(ValueError, match="CTRLV_PIPELINE=plan"):
        SVDPipelineBase.prepare_clip(object(), None, None, height=8, width=8, num_frames=1, decode_chunk_size=1, fps=7,
                                     motion_bucket_id=127, noise_aug_strength=0.02, num_videos_per_prompt=1, generator=s,
                                     latents=None, latent_channels=8, min_guidance_scale=1.0, max_guidance_scale=3.0,
                                     num_inference_steps=2)
