"""The VAE plan (csrc/vae_plan.hip: ctrlv_vae_encode / ctrlv_vae_decode, one C call each) against the per-op Python executors
(bit for bit where the walks are the same: `to_v.bias` zero, see include/ctrlv_hip.h), against the CPU oracle
(oracle/ctrlv_ref/vae.py; the project's VAE bound parity_err < 2.5e-2), from a foreign host through raw ctypes, under HIP-graph
capture, after an in-place parameter update, and inside the pipeline under CTRLV_VAE_HIP=plan.  Production widths
(128/256/512/512), mix factors 0.4, bf16-rounded parameters: the construction of tests/test_vae_gpu.py."""
import copy
import ctypes

import pytest
import torch

from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SMALL_LIMIT = 3 * 64 * 64 * 128 * 2 + 1       # the limit of test_vae_decode_two_clips_and_limits: 256-channel tensors do not fit


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def vae(hip_lib):
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    torch.manual_seed(5)
    m = AutoencoderKLTemporalDecoder().eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("mix_factor"):
                p.fill_(0.4)                          # exercise both branches of the AlphaBlender
            p.copy_(p.to(BF).float())
    return m


@pytest.fixture(scope="module")
def dev_vae(vae):
    """On the device in bf16, `to_v.bias` as initialised (non-zero)."""
    m = copy.deepcopy(vae).to(DEV, BF)
    assert float(m.decoder.mid_block.attentions[0].to_v.bias.abs().max()) > 0
    return m


@pytest.fixture(scope="module")
def dev_vae0(vae):
    """The same with both attentions' `to_v.bias` zeroed: the folded output bias is exact, the two routes compute the same bits."""
    m = copy.deepcopy(vae).to(DEV, BF)
    with torch.no_grad():
        m.decoder.mid_block.attentions[0].to_v.bias.zero_()
        m.encoder.mid_block.attentions[0].to_v.bias.zero_()
    return m


def _z(n, h, w, seed=3):
    return torch.randn(n, 4, h, w, generator=g(seed)).to(BF)


# ------------------------------------------------------------------------------------------------------------ T3 / T4: decode
@pytest.mark.parametrize("n,h,w", [(3, 8, 8), (3, 16, 24)])
def test_decode_plan_is_the_per_op_walk(dev_vae0, n, h, w):
    from ctrlv_amd.models import vae_decoder_hip as vh
    z = _z(n, h, w).to(DEV)
    want = vh.decode(dev_vae0.decoder, z, n)
    got = vh.decode_plan(dev_vae0, z, n)
    torch.cuda.synchronize()
    assert got.shape == (n, 3, 8 * h, 8 * w) and got.dtype == BF
    assert torch.equal(got, want)
    assert torch.equal(vh.decode_plan(dev_vae0, z, n), got)          # and the same bits again


def test_decode_plan_two_clips_and_the_offset_limit(dev_vae0):
    from ctrlv_amd.models import vae_decoder_hip as vh
    z = _z(4, 8, 8, seed=9).to(DEV)
    both = vh.decode_plan(dev_vae0, z, 2)
    first, second = vh.decode_plan(dev_vae0, z[:2], 2), vh.decode_plan(dev_vae0, z[2:], 2)
    assert torch.equal(both, torch.cat([first, second]))
    assert torch.equal(both, vh.decode(dev_vae0.decoder, z, 2))
    with pytest.raises(ValueError, match="whole clips|multiple of num_frames"):
        vh.decode_plan(dev_vae0, z[:3], 2)
    # frame ranges of the per-frame ops under a tiny limit: the bits of the default limit
    ref = vh.decode_plan(dev_vae0, z[:3], 3)
    assert len(vh._frame_batches(3, 64 * 64, 256)) == 1
    small = vh.decode_plan(dev_vae0, z[:3], 3, offset_limit_bytes=SMALL_LIMIT)
    assert torch.equal(small, ref)
    # ... and a clip whose whole-clip tensors exceed that limit is a shape error of the C call, before any launch
    from ctrlv_amd.plan import vae_plan
    with pytest.raises(ValueError, match="offset limit"):
        vae_plan(dev_vae0, SMALL_LIMIT).decode(z, 4)


def test_decode_plan_parity_with_the_oracle(vae, dev_vae):
    """T4: random to_v.bias (the fold is rounded, not exact): against the CPU oracle; the per-op route's error printed beside."""
    import ctrlv_ref as R
    from ctrlv_amd.models import vae_decoder_hip as vh
    n, h, w = 3, 8, 8
    z = _z(n, h, w)
    with torch.no_grad():
        ref = R.vae.decode({k: v.detach() for k, v in vae.state_dict().items()}, z.float(), n)
    got = vh.decode_plan(dev_vae, z.to(DEV), n)
    per_op = vh.decode(dev_vae.decoder, z.to(DEV), n)
    torch.cuda.synchronize()
    parity_err(per_op.float().cpu(), ref, "per-op route")
    assert parity_err(got.float().cpu(), ref, "plan") < 2.5e-2


# ------------------------------------------------------------------------------------------------------------------ T5: encode
@pytest.mark.parametrize("n,H,W", [(2, 128, 192), (1, 64, 64)])
def test_encode_plan(vae, dev_vae0, n, H, W):
    import ctrlv_ref as R
    from ctrlv_amd import ops
    from ctrlv_amd.models import vae_encoder_hip as ve
    x = (torch.rand(n, 3, H, W, generator=g(4)) * 2 - 1).to(BF)
    xd = x.to(DEV)
    sf = dev_vae0.config.scaling_factor
    noise = torch.randn(n, 4, H // 8, W // 8, generator=g(6))
    lat, mom = ve.encode_plan(dev_vae0, xd, scale=sf)
    lat_n, none = ve.encode_plan(dev_vae0, xd, noise=noise.to(DEV), scale=sf, moments=False)
    # the pre-posterior walk is the per-op twin's: the posterior kernel applied by hand to the twin's rows gives the same bits
    rows = ve.encode(dev_vae0.encoder, xd, native_down=True, rows=True)
    qw = dev_vae0.quant_conv.weight.detach().float().reshape(8, 8).contiguous()
    qb = dev_vae0.quant_conv.bias.detach().float().contiguous()
    mom_t, lat_t = ops.vae_posterior(rows, n, 4, (H // 8) * (W // 8), qw, qb, None, sf, torch.empty_like(mom), torch.empty_like(lat))
    torch.cuda.synchronize()
    assert none is None and mom.shape == (n, 8, H // 8, W // 8) and lat.shape == (n, 4, H // 8, W // 8)
    assert torch.equal(mom, mom_t) and torch.equal(lat, lat_t)
    sd = {k: v.detach() for k, v in dev_vae0.state_dict().items()}
    with torch.no_grad():
        ref_q = R.vae.encode_moments({k: v.float().cpu() for k, v in sd.items()}, x.float())
    mean, logvar = torch.chunk(ref_q, 2, dim=1)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    assert parity_err(mom.float().cpu(), ref_q, "plan moments") < 2.5e-2
    assert parity_err(lat.float().cpu(), sf * mean, "plan latents (mode)") < 2.5e-2
    assert parity_err(lat_n.float().cpu(), sf * (mean + std * noise), "plan latents (mean + std * noise)") < 2.5e-2


# ------------------------------------------------------------------------------------------------------------ T6: foreign host
def _raw_plan(lib, _lib, m):
    cfg = _lib.VaeConfig()
    cfg.in_channels, cfg.out_channels, cfg.latent_channels, cfg.layers_per_block, cfg.n_blocks = 3, 3, 4, 2, 4
    for i, c in enumerate((128, 256, 512, 512)):
        cfg.block_out_channels[i] = c
    cfg.scaling_factor = 0.18215
    h = ctypes.c_void_p()
    assert lib.ctrlv_vae_plan_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0, _lib.last_error(lib)
    assert lib.ctrlv_vae_plan_workspace_bytes(h, 1, 3, 3, 8, 8) == 0 and "not loaded" in _lib.last_error(lib)
    host = [(k, v.detach().float().cpu().contiguous()) for k, v in m.state_dict().items()]       # HOST fp32
    arr = (_lib.TensorDesc * len(host))()
    for i, (k, v) in enumerate(host):
        arr[i].name, arr[i].data, arr[i].dtype, arr[i].on_device, arr[i].numel = k.encode(), v.data_ptr(), 0, 0, v.numel()
    assert lib.ctrlv_vae_plan_load_weights(h, arr, len(host)) == 0, _lib.last_error(lib)
    return h


def test_vae_plan_from_a_foreign_host(hip_lib, dev_vae):
    """create -> load from host fp32 -> workspace -> decode / encode through raw ctypes only: bit-equal to VaePlan on the same
    module (loaded from its bf16 device tensors: rounding an fp32 copy of a bf16 value is exact).  A workspace one byte short is
    CTRLV_E_WORKSPACE and nothing is written."""
    from ctrlv_amd import _lib
    from ctrlv_amd.models import vae_decoder_hip as vh
    from ctrlv_amd.models import vae_encoder_hip as ve
    lib = _lib.load()
    n, h, w = 3, 8, 8
    z = _z(n, h, w).to(DEV)
    x = (torch.rand(1, 3, 64, 64, generator=g(4)) * 2 - 1).to(DEV, BF)
    want = vh.decode_plan(dev_vae, z, n)
    want_lat, want_mom = ve.encode_plan(dev_vae, x, scale=0.5)
    hnd = _raw_plan(lib, _lib, dev_vae)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = lib.ctrlv_vae_plan_workspace_bytes(hnd, 1, n, n, h, w)
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((n, 3, 8 * h, 8 * w), 7.0, dtype=BF, device=DEV)
    assert lib.ctrlv_vae_decode(hnd, z.data_ptr(), 2, n, n, h, w, out.data_ptr(), 2, ws.data_ptr(), need - 1, st) == -5
    assert "needed" in _lib.last_error(lib)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert lib.ctrlv_vae_decode(hnd, z.data_ptr(), 2, n, n, h, w, out.data_ptr(), 2, ws.data_ptr(), need, st) == 0, _lib.last_error(lib)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # encode
    need_e = lib.ctrlv_vae_plan_workspace_bytes(hnd, 0, 1, 0, 64, 64)
    assert need_e > 0
    ws = torch.empty(need_e, dtype=torch.uint8, device=DEV)
    lat = torch.full((1, 4, 8, 8), 7.0, dtype=BF, device=DEV)
    mom = torch.full((1, 8, 8, 8), 7.0, dtype=BF, device=DEV)
    args = (hnd, x.data_ptr(), 2, 1, 64, 64, None, 0.5, lat.data_ptr(), mom.data_ptr(), 2, ws.data_ptr())
    assert lib.ctrlv_vae_encode(*args, need_e - 1, st) == -5
    torch.cuda.synchronize()
    assert bool((lat == 7.0).all()) and bool((mom == 7.0).all())
    assert lib.ctrlv_vae_encode(*args, need_e, st) == 0, _lib.last_error(lib)
    torch.cuda.synchronize()
    assert torch.equal(lat, want_lat) and torch.equal(mom, want_mom)
    # shapes outside the rules are refused by the C calls themselves
    assert lib.ctrlv_vae_decode(hnd, z.data_ptr(), 2, n, 2, h, w, out.data_ptr(), 2, ws.data_ptr(), need, st) == -2
    assert lib.ctrlv_vae_plan_workspace_bytes(hnd, 1, 1, 1, 6, 6) == 0 and "multiple of 64" in _lib.last_error(lib)
    assert lib.ctrlv_vae_plan_workspace_bytes(hnd, 0, 1, 0, 60, 64) == 0 and "multiples of 8" in _lib.last_error(lib)
    # a missing tensor is an error, and the plan is unloaded by the failed load
    arr = (_lib.TensorDesc * 1)()
    arr[0].name, arr[0].data, arr[0].dtype, arr[0].on_device, arr[0].numel = b"quant_conv.bias", 0x1000, 0, 1, 8
    assert lib.ctrlv_vae_plan_load_weights(hnd, arr, 1) < 0 and "missing tensor" in _lib.last_error(lib)
    assert lib.ctrlv_vae_plan_destroy(hnd) == 0


# ------------------------------------------------------------------------------------------------- workspace against the per-op peak
def test_decode_workspace_is_within_a_tenth_of_the_per_op_peak(dev_vae):
    """workspace_bytes(decode, 25 frames, 72 x 128) against torch.cuda.max_memory_allocated of the per-op call above what was
    allocated before it (its output included): the walk and its liveness are the same, so at most 1.10 x -- the margin is
    256-byte alignment and first-fit fragmentation.  One warm call first: the per-op route's persistent scratch is not the
    call's."""
    from ctrlv_amd.models import vae_decoder_hip as vh
    from ctrlv_amd.plan import vae_plan
    z = _z(25, 72, 128).to(DEV)
    vh.decode(dev_vae.decoder, z, 25)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = vh.decode(dev_vae.decoder, z, 25)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    ws = vae_plan(dev_vae).workspace_bytes("decode", 25, 25, 72, 128)
    print(f"  decode 25 x 72 x 128: plan workspace {ws} B, per-op peak {peak} B, ratio {ws / peak:.4f}")
    assert ws <= 1.10 * peak


# ---------------------------------------------------------------------------------------------------------- T7: graph capture
def test_vae_decode_is_graph_capturable(dev_vae):
    from ctrlv_amd.plan import vae_plan
    n, h, w = 3, 8, 8
    z1, z2 = _z(n, h, w, 3).to(DEV), _z(n, h, w, 77).to(DEV)
    plan = vae_plan(dev_vae)
    want1, want2 = plan.decode(z1, n).clone(), plan.decode(z2, n).clone()
    assert not torch.equal(want1, want2)
    buf = z1.clone()
    ws = torch.empty(plan.workspace_bytes("decode", n, n, h, w), dtype=torch.uint8, device=DEV)
    out = torch.empty_like(want1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.decode(buf, n, workspace=ws, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want1)
    buf.copy_(z2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2)


# ------------------------------------------------------------------------------------------------- T8: in-place parameter update
def test_decode_plan_follows_an_in_place_parameter_update(dev_vae0):
    from ctrlv_amd.models import vae_decoder_hip as vh
    from ctrlv_amd.plan import vae_plan
    m = copy.deepcopy(dev_vae0)
    z = _z(3, 8, 8).to(DEV)
    before = vh.decode_plan(m, z, 3).clone()
    assert vae_plan(m) is vae_plan(m)                               # cached
    with torch.no_grad():
        m.decoder.conv_out.bias.add_(1)
    after = vh.decode_plan(m, z, 3)
    assert not torch.equal(before, after)
    assert torch.equal(after, vh.decode(m.decoder, z, 3))


# ------------------------------------------------------------------------------------------------------------- T9: the pipeline
@torch.no_grad()
def test_pipeline_under_the_plan_route(dev_vae, monkeypatch):
    """The construction of test_pipeline_with_real_vae_hip_vs_torch (tiny UNet / ControlNet, 3 frames, 128 x 128, 2 steps) with
    CTRLV_VAE_HIP=plan against the same call with CTRLV_VAE_HIP=0."""
    import ctrlv_ref as R
    from ctrlv_amd.models import vae_decoder_hip as vh
    from ctrlv_amd.pipelines import StableVideoControlPipeline
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    from tests.fakes import FakeCLIP, fake_feature_extractor
    from tests.parity_utils import make_pair
    cfg = dict(R.TINY_CONFIG)
    _, _, hu, hc = make_pair(cfg, DEV)
    clip = FakeCLIP(cfg["cross_attention_dim"]).to(DEV, BF)
    pipe = StableVideoControlPipeline(dev_vae, clip, hu, hc, EulerDiscreteScheduler(), fake_feature_extractor)
    pipe.set_progress_bar_config(disable=True)
    gen = g(11)
    image = (torch.rand(1, 3, 128, 128, generator=gen) * 2 - 1).to(DEV, BF)
    cond = (torch.rand(1, 3, 3, 128, 128, generator=gen) * 2 - 1).to(DEV)
    lat = torch.randn(1, 3, 4, 16, 16, generator=gen).to(DEV, BF)
    calls = []
    real_dec, real_enc = vh.decode_plan, __import__("ctrlv_amd.models.vae_encoder_hip", fromlist=["x"]).encode_plan
    monkeypatch.setattr(vh, "decode_plan", lambda *a, **k: (calls.append("decode"), real_dec(*a, **k))[1])
    monkeypatch.setattr("ctrlv_amd.models.vae_encoder_hip.encode_plan", lambda *a, **k: (calls.append("encode"), real_enc(*a, **k))[1])

    def run():
        return pipe(image, cond_images=cond, height=128, width=128, num_frames=3, num_inference_steps=2,
                    decode_chunk_size=2, latents=lat.clone(), noise_aug_strength=0.0, output_type="pt").frames.float().cpu()

    monkeypatch.setenv("CTRLV_VAE_HIP", "plan")
    got = run()
    assert "decode" in calls and "encode" in calls
    n_plan = len(calls)
    monkeypatch.setenv("CTRLV_VAE_HIP", "0")
    ref = run()
    assert len(calls) == n_plan                                     # the torch route never enters the plan
    assert got.shape == (1, 3, 3, 128, 128) and got.min() >= 0 and got.max() <= 1
    assert parity_err(got, ref, "pipeline frames, VAE plan vs torch VAE") < 3e-2
