"""The training-batch driver on the device (include/ctrlv_hip.h: ctrlv_train_batch_prepare; csrc/train_batch_plan.hip): every
output against the same calls made by hand, bit for bit, for the three modes and in both element builds; the loss of train_step /
unet_train_step on the prepared batch against the loss on the classic dict built from the same tensors; reproducibility from
(seed, step).  The default AutoencoderKLTemporalDecoder, a two-layer CLIP tower, R.TINY_CONFIG models; 2 clips x 3 frames.

Geometry: 128 x 128 pixels (latent 16 x 16).  The VAE plan's mid-block attention takes latent pixel counts that are multiples of
64, so 64 x 64 pixels is the smallest frame ctrlv_vae_encode accepts (32 x 32 is refused by name, asserted below); 128 x 128 is
the size the training-step tests run the tiny UNet at (its four levels halve a 16 x 16 latent down to 2 x 2)."""
import numpy as np
import pytest
import torch

from tests import train_batch_ref as T
from tests.test_pipeline_plan_gpu import MEAN, PIPE_CLIP, STD
from tests.test_train_batch_cpu import CALL, DP, SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, F, H, W, K = 2, 3, 128, 128, 1
MODES = ("controlnet", "unet", "boxes")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def first_clip():
    """The first clip index >= 5 at which the two clips of the batch fall into different dropout regions, neither of them the
    region where nothing is dropped -- read off the numpy restatement, so both masks do something in every test below."""
    table = np.arange(1000, dtype=np.float32)
    d = T.draws(SEED, 64, table, table, clip0=5, call=CALL, dropout_prob=DP)
    pair = list(zip(d["prompt_keep"], d["image_mask"]))
    for i in range(63):
        if pair[i] != pair[i + 1] and (1.0, 1.0) not in (pair[i], pair[i + 1]):
            return 5 + i
    raise AssertionError("no such pair of clips")


CLIP0 = first_clip()


class Setup:
    pass


_SETUPS = {}


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def setup(request, hip_lib):
    return build_setup(request.param)


@pytest.fixture(scope="module")
def setup_bf16(hip_lib):
    """The training steps run in bf16 elements: the loss tests take that build's setup."""
    return build_setup(torch.bfloat16)


def build_setup(el):
    if el in _SETUPS:
        return _SETUPS[el]
    from ctrlv_amd import DeviceSeed
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder, clip_vision_hip
    from ctrlv_amd.plan import TrainBatchPlan, vae_plan
    from tests import clip_utils as U
    s = _SETUPS[el] = Setup()
    s.el = el
    torch.manual_seed(5)
    s.vae = AutoencoderKLTemporalDecoder().eval().to(DEV, el)
    s.clip = U.build_own(PIPE_CLIP, 31, el, DEV)
    s.vplan, s.cplan = vae_plan(s.vae, dtype=el), clip_vision_hip._plan(s.clip)
    s.plan = TrainBatchPlan(s.vplan, s.cplan)
    s.seed = DeviceSeed(SEED, clip_index0=CLIP0)
    g0 = gen(21)
    s.clips = (torch.rand(N, F, 3, H, W, generator=g0) * 2.4 - 1.2).clamp(-1, 1).to(DEV)              # fp32, both ends reached
    s.boxes = (torch.rand(N, F, 3, H, W, generator=g0) * 2 - 1).to(DEV, el)                           # elements
    return s


def compose(s, mode, step=CALL, dp=DP):
    """What ctrlv_train_batch_prepare enqueues, call by call: ops.resize_antialias(clamp=True), ClipPlan.forward,
    ops.train_draws, ops.randn, VaePlan.encode(noise=...), ops.train_assemble."""
    from ctrlv_amd import ops
    el, seed, clip0 = s.el, s.seed.seed, s.seed.clip_index0
    L, h, w = 4, H // 8, W // 8
    size = PIPE_CLIP["image_size"]
    img = s.clips[:, 0].float().contiguous()
    px = ops.resize_antialias(img, (size, size), mean=MEAN, std=STD, out_dtype=el, clamp=True)
    emb = s.cplan.forward(px)
    d = ops.train_draws(seed, N, s.plan.sigma_table, s.plan.timestep_table, clip0=clip0, call=step, dropout_prob=dp, el=el)
    ehs = (d["prompt_keep"].view(N, 1) * emb.float()).to(el).unsqueeze(1)

    def enc(x, stream_id, scale):
        m = x.shape[0]
        z = ops.randn(seed, (N, m // N, L, h, w), clip0=clip0, call=step, stream_id=stream_id, device=DEV)
        lat = s.vplan.encode(x, noise=z.view(m, L, h, w), scale=scale, moments=False, out_dtype=torch.float32)[0]
        return lat.view(N, m // N, L, h, w) if m != N else lat

    sf = float(s.vae.config.scaling_factor)
    cond = None
    if mode == "boxes":
        cond = enc(s.boxes.flatten(0, 1), 4, 1.0)
        target = cond * sf
    else:
        target = enc(s.clips.flatten(0, 1), 4, sf)
    image = enc(img, 5, 1.0)
    out = {"target_latents": target, "encoder_hidden_states": ehs, "sigmas": d["sigmas"], "timesteps": d["timesteps"],
           "indices": d["indices"], "random_p": d["random_p"]}
    if mode == "controlnet":
        out["control_cond"] = enc(s.boxes.flatten(0, 1), 6, 1.0)
    out["noisy_latents"], out["sample"], out["noise"] = ops.train_assemble(
        target, d["sigmas"], image, image_mask=d["image_mask"], cond_frames=cond, layout=1 if mode == "boxes" else 0,
        num_cond_frames=K, seed=seed, clip0=clip0, call=step, sample_dtype=el, return_noise=True, el=el)
    torch.cuda.synchronize()
    s.last = dict(image=image, cond=cond, draws=d)
    return out


def drive(s, mode, step=CALL, dp=DP, **kw):
    out = s.plan.prepare(s.clips, None if mode == "unet" else s.boxes, mode=mode, seed=s.seed, step=step, num_cond_frames=K,
                         dropout_prob=dp, return_noise=True, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", MODES)
def test_driver_is_the_same_calls_made_by_hand(setup, mode):
    want, got = compose(setup, mode), drive(setup, mode)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(bits(got[k]), bits(want[k])), (k, float((got[k].float() - want[k].float()).abs().max()))
    assert bool(torch.isfinite(got["sample"].float()).all()) and float(got["noisy_latents"].abs().max()) > 0
    d = setup.last["draws"]
    assert float(d["prompt_keep"].min()) == 0.0 or float(d["image_mask"].min()) == 0.0          # the dropout did something
    # an fp32 sample is the same values before the element rounding
    wide = drive(setup, mode, sample_dtype=torch.float32)["sample"]
    assert wide.dtype == torch.float32 and torch.equal(bits(wide.to(setup.el)), bits(got["sample"]))


def test_same_seed_and_step_same_bits_another_step_other_noise(setup):
    a, b, c = drive(setup, "controlnet"), drive(setup, "controlnet"), drive(setup, "controlnet", step=CALL + 1)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
    for k in ("noise", "target_latents", "control_cond", "random_p", "noisy_latents"):
        assert not torch.equal(a[k], c[k]), k
    # and clip 1 of this batch is clip 0 of the batch that starts one clip later
    from ctrlv_amd import DeviceSeed
    one = setup.plan.prepare(setup.clips[1:], setup.boxes[1:], mode="controlnet", seed=DeviceSeed(SEED, clip_index0=CLIP0 + 1),
                             step=CALL, dropout_prob=DP, return_noise=True)
    for k in ("noise", "sigmas", "timesteps", "indices", "random_p"):
        assert torch.equal(bits(a[k][1:]), bits(one[k])), k


def test_a_frame_the_vae_refuses_is_refused_by_name(setup):
    small = torch.zeros(1, 3, 3, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="latent pixels"):
        setup.plan.prepare(small, None, mode="unet", seed=setup.seed, step=0)
    with pytest.raises(ValueError, match="box_frames is null"):
        setup.plan.prepare(setup.clips, None, mode="controlnet", seed=setup.seed, step=0)


# ------------------------------------------------------------------------------------------------------------------- the losses
def _classic(s, mode, batch):
    """The dict the training steps have always taken, from the same target, noise, sigmas and conditioning."""
    d, image, cond = s.last["draws"], s.last["image"], s.last["cond"]
    c = image.unsqueeze(1).repeat(1, F, 1, 1, 1)
    if mode == "boxes":
        c[:, :K] = cond[:, :K]
        c[:, F - 1] = cond[:, F - 1]
    classic = {"latents": batch["latents"], "noise": batch["noise"], "sigmas": batch["sigmas"],
               "image_latents": d["image_mask"].view(N, 1, 1, 1, 1) * c,
               "encoder_hidden_states": batch["encoder_hidden_states"], "added_time_ids": batch["added_time_ids"]}
    if mode == "controlnet":
        classic["control_cond"] = batch["control_cond"]
    return classic


@pytest.mark.parametrize("mode", MODES)
def test_the_loss_on_the_prepared_batch_is_the_loss_on_the_classic_dict(setup_bf16, mode):
    """train_step (mode "controlnet") / unet_train_step (the others) with optimizer=None, bf16 elements (the training steps'
    element type).  Printed before the assertion: both losses and the largest timestep difference between the scheduler's table
    (what the prepared batch carries) and 0.25 log(sigma) as the classic path forms it on the device."""
    import ctrlv_ref as R
    from ctrlv_amd.training import _noised_inputs, prepare_batch, train_step, unet_train_step
    from tests.parity_utils import make_pair
    s = setup_bf16
    compose(s, mode)                                     # (the by-hand image latent, cond frames and draws: s.last)
    batch = prepare_batch(s.plan, s.clips, None if mode == "unet" else s.boxes, mode=mode, seed=s.seed, step=CALL,
                          num_cond_frames=K, dropout_prob=DP, return_noise=True)
    classic = _classic(s, mode, batch)
    a, b = _noised_inputs(batch), _noised_inputs(classic)
    torch.cuda.synchronize()
    dt = float((a[3] - b[3]).abs().max())
    print(f"  {mode}: timesteps table vs device log, max abs difference {dt:.3e}; sigmas {batch['sigmas'].tolist()}")
    assert torch.equal(bits(a[2]), bits(b[2])) and torch.equal(bits(a[4]), bits(b[4]))      # noisy latents and the model input
    _, _, hu, hc = make_pair(dict(R.TINY_CONFIG), DEV, seed=3)
    with torch.enable_grad():
        if mode == "controlnet":
            hc.float()
            for p in hc.parameters():
                p.requires_grad_(True)
            for p in hu.parameters():
                p.requires_grad_(False)
            step = lambda bt: train_step(hc, hu, bt, optimizer=None, conditioning_scale=0.8)        # noqa: E731
        else:
            hu.float()
            for p in hu.parameters():
                p.requires_grad_(True)
            step = lambda bt: unet_train_step(hu, bt, optimizer=None)                               # noqa: E731
        l1, l2 = step(batch), step(classic)
    torch.cuda.synchronize()
    print(f"  {mode}: loss on the prepared batch {float(l1):.9g}, on the classic dict {float(l2):.9g}")
    assert bool(torch.isfinite(l1)) and torch.equal(bits(l1.reshape(1)), bits(l2.reshape(1)))
