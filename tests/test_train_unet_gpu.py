"""Stage-1 training step (the whole UNet fine-tuned; reference: tools/train_video_diffusion.py:515-541) on the HIP kernels:
ctrlv_amd.training.unet_train_step against torch.autograd on the oracle UNet.  Checked: the loss, the gradient of EVERY
UNet parameter, the temporal-only mode and the switch into it, inference after an optimizer step, gradient checkpointing,
and the full-size step (finite, bit-reproducible, learning).

Bounds are those of the cfg5 step (tests/test_train_gpu.py): the same step in plain torch bf16 on the GPU is the
yardstick; all gradients concatenated < 3e-2 and < 1.5x the yardstick, each parameter < 8e-2 and < 3x the yardstick
(floor 2e-2: a few tiny-width norm gradients have a yardstick far below bf16 resolution).  The scalar mix factors are
cancelling sums over whole activation tensors and are judged on the absolute error against the largest mix-factor
gradient, as in the cfg5 test."""
import copy
import math

import pytest
import torch

from tests.parity_utils import make_pair, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _batch(config, B, F, h, w, seed=5, drop=()):
    """A stage-1 batch; samples in `drop` carry what the caller's conditioning dropout gives them (zero CLIP token and
    zero conditioning-frame latents, tools/train_video_diffusion.py:489-513)."""
    g = torch.Generator().manual_seed(seed)
    bf = lambda x: x.to(torch.bfloat16).float()   # noqa: E731
    dc = config["cross_attention_dim"]
    b = dict(latents=bf(torch.randn(B, F, 4, h, w, generator=g)), noise=bf(torch.randn(B, F, 4, h, w, generator=g)),
             sigmas=torch.tensor([1.3] * B), image_latents=bf(torch.randn(B, 1, 4, h, w, generator=g)).repeat(1, F, 1, 1, 1),
             encoder_hidden_states=bf(torch.randn(B, 1, dc, generator=g)),
             added_time_ids=torch.tensor([[6.0, 127.0, 0.02]] * B))
    for i in drop:
        b["encoder_hidden_states"][i] = 0
        b["image_latents"][i] = 0
    return b


def _oracle_unet_step(ou, b):
    """The reference's stage-1 step (train_video_diffusion.py:515-531) on an oracle UNet in whatever dtype / device it
    lives: fp32 CPU = the reference result, bf16 on the GPU = the yardstick."""
    p0 = next(ou.parameters())
    b = {k: v.to(device=p0.device, dtype=p0.dtype) for k, v in b.items()}
    lat, noise, sig = b["latents"], b["noise"], b["sigmas"]
    B = lat.shape[0]
    s5 = sig.reshape(B, 1, 1, 1, 1)
    noisy = lat + noise * s5
    inp = noisy / (s5 * s5 + 1) ** 0.5
    sample = torch.cat([inp, b["image_latents"]], dim=2).to(torch.bfloat16).to(p0.dtype)
    t = 0.25 * torch.log(sig.float())[0]
    pred = ou(sample, t, b["encoder_hidden_states"], b["added_time_ids"])[0]
    c_out, c_skip = -s5 / (s5 * s5 + 1) ** 0.5, 1 / (s5 * s5 + 1)
    den = pred * c_out + c_skip * noisy
    wgt = (1 + s5 ** 2) * s5 ** -2.0
    loss = (wgt.float() * (den.float() - lat.float()) ** 2).reshape(B, -1).mean(dim=1).mean()
    loss.backward()
    return loss.detach()


def _set_mode(model, mode):
    """the reference's two modes on an oracle / HIP UNet: 'all' or 'temporal' (names with temporal_transformer_block)"""
    for n, p in model.named_parameters():
        p.requires_grad_(mode == "all" or "temporal_transformer_block" in n)
        p.grad = None


def _check_grads(hu, ou, yu, b_loss, tag, per_param_bound=8e-2):
    """HIP gradients of `hu` against the oracle `ou`, next to the yardstick `yu` (all after their backward)."""
    loss, loss_ref = b_loss
    print(f"  [{tag}] loss: HIP {loss:.6f}  oracle {loss_ref:.6f}")
    assert math.isfinite(loss) and abs(loss - loss_ref) <= 5e-3 * abs(loss_ref)
    refp, yp = dict(ou.named_parameters()), dict(yu.named_parameters())
    gmax = max(float(q.grad.abs().max()) for q in refp.values() if q.grad is not None)
    errs, got, ref, yard = {}, [], [], []
    for name, p in hu.named_parameters():
        rg = refp[name].grad
        if not refp[name].requires_grad:
            assert not p.requires_grad and p.grad is None, name
            continue
        if rg is None or float(rg.abs().max()) <= 1e-6 * gmax:
            assert p.grad is not None, name
            if ".attn2.to_q." in name or ".attn2.to_k." in name or (".norm2." in name and "transformer_block" in name):
                assert float(p.grad.abs().max()) == 0.0, name      # one-key cross-attention: no gradient path, zeros
            else:                                                  # (vanishing, e.g. the mid block's temporal q / k at
                assert float(p.grad.abs().max()) <= 1e-5 * gmax, name    # 3 x 5 pixels): tiny as well
            continue
        assert p.grad is not None, name
        pg = p.grad.float().cpu().reshape(rg.shape)
        errs[name] = rel_l2(pg, rg)
        got.append(pg.reshape(-1)); ref.append(rg.reshape(-1)); yard.append(yp[name].grad.float().cpu().reshape(-1))
    tot, ytot = rel_l2(torch.cat(got), torch.cat(ref)), rel_l2(torch.cat(yard), torch.cat(ref))
    ypar = {n: rel_l2(yp[n].grad.float().cpu().reshape(refp[n].grad.shape), refp[n].grad) for n in errs}
    for n, v in sorted(errs.items(), key=lambda kv: -kv[1])[:6]:
        print(f"  {v:.2e} (torch bf16: {ypar[n]:.2e})  d/d {n}")
    print(f"  {len(errs)} parameter gradients, concatenated: rel-L2 {tot:.2e}   (torch bf16: {ytot:.2e})")
    assert tot < 3e-2 and tot < 1.5 * ytot
    mix = [n for n in errs if n.endswith("mix_factor")]
    mixmax = max((float(refp[n].grad.abs().max()) for n in mix), default=0.0)
    hp = dict(hu.named_parameters())
    for n, v in errs.items():
        if n.endswith("mix_factor"):
            ae = float((hp[n].grad.float().cpu().reshape(-1) - refp[n].grad.reshape(-1)).abs().max())
            assert ae < 5e-2 * mixmax, (n, ae, mixmax)
        else:
            assert v < per_param_bound and v < max(3.0 * ypar[n], 2e-2), (n, v, ypar[n])
    return errs


def _run_parity(ou, hu, b, mode, tag, per_param_bound=8e-2):
    from ctrlv_amd.training import unet_train_step
    _set_mode(ou, mode)
    with torch.enable_grad():
        loss_ref = float(_oracle_unet_step(ou, b))
        hu.float()
        _set_mode(hu, mode)
        loss = float(unet_train_step(hu, {k: v.to(DEV) for k, v in b.items()}))
        torch.cuda.synchronize()
        yu = copy.deepcopy(ou).to(DEV, torch.bfloat16)
        _set_mode(yu, mode)
        _oracle_unet_step(yu, b)
    return _check_grads(hu, ou, yu, (loss, loss_ref), tag, per_param_bound)


@pytest.mark.parametrize("B", [1, 2])
def test_unet_train_step_matches_oracle_autograd(hip_lib, B):
    """All-mode (the demo scripts): loss and the gradient of every UNet parameter.  B = 2 has sample 0 hit by conditioning
    dropout (zero CLIP token and conditioning frame) and runs the (s, b) temporal-context quirk of diffusers 0.27.2."""
    import ctrlv_ref as R
    config = dict(R.TINY_CONFIG)
    ou, _, hu, _ = make_pair(config, DEV, seed=3)
    b = _batch(config, B, 3, 16, 16, drop=(0,) if B == 2 else ())
    errs = _run_parity(ou, hu, b, "all", f"all, B={B}")
    assert len(errs) > 300                       # (every layer type of the UNet is in the comparison)
    assert any(n.startswith("conv_out.") for n in errs) and any(".upsamplers.0.conv." in n for n in errs)


def test_unet_temporal_only_mode_and_the_switch_into_it(hip_lib):
    """unet.enable_grad(temporal_transformer_block=True): exactly those parameters get gradients, matching the oracle;
    after an AdamW step every other parameter is bit-unchanged.  Switching a model that trained in all-mode to
    temporal-only (backprop_temporal_blocks_start_iter, train_video_diffusion.py:379-388) gives the gradients of a fresh
    temporal-only model with the same weights, bit for bit."""
    import ctrlv_ref as R
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    from ctrlv_amd.training import unet_train_step
    config = dict(R.TINY_CONFIG)
    ou, _, hu, _ = make_pair(config, DEV, seed=7)
    b = _batch(config, 2, 3, 16, 16, seed=8, drop=(1,))
    _run_parity(ou, hu, b, "temporal", "temporal")
    trained = {n for n, p in hu.named_parameters() if p.grad is not None}
    assert trained == {n for n, _ in hu.named_parameters() if "temporal_transformer_block" in n}
    # an AdamW step moves the temporal transformer blocks only
    before = {n: p.detach().clone() for n, p in hu.named_parameters()}
    opt = torch.optim.AdamW(hu.get_parameters_with_grad(), lr=1e-3, weight_decay=1e-2)
    opt.step()
    for n, p in hu.named_parameters():
        if n in trained:
            assert not torch.equal(before[n], p.detach()) or float(p.grad.abs().max()) == 0.0, n
        else:
            assert torch.equal(before[n], p.detach()), n
    # all-mode for one optimizer step, then the switch
    bd = {k: v.to(DEV) for k, v in b.items()}
    hu.enable_grad(all=True)
    for p in hu.parameters():
        p.grad = None
    opt = torch.optim.AdamW(hu.get_parameters_with_grad(), lr=1e-3, weight_decay=1e-2)
    unet_train_step(hu, bd, opt)
    hu.enable_grad(temporal_transformer_block=True)
    loss_sw = unet_train_step(hu, bd)
    g_sw = {n: p.grad.clone() for n, p in hu.named_parameters() if p.grad is not None}
    fresh = UNetSpatioTemporalConditionModel(**config).to(DEV, torch.float32).eval()
    fresh.load_state_dict(hu.state_dict())
    fresh.enable_grad(temporal_transformer_block=True)
    loss_fr = unet_train_step(fresh, bd)
    g_fr = {n: p.grad for n, p in fresh.named_parameters() if p.grad is not None}
    assert set(g_sw) == set(g_fr) == trained
    assert torch.equal(loss_sw, loss_fr)
    for n in g_sw:
        assert torch.equal(g_sw[n], g_fr[n]), n


def test_unet_train_step_production_widths(hip_lib):
    """SVD widths (320/640/1280/1280, 5/10/20/20 heads, cross-attention 1024) on a small latent, 24 x 40 at 4 frames:
    N = 320 / 640 tiles, K up to 10240, the 640-channel upsampler conv on the LDS-DMA ring, conv_out's N = 4."""
    import ctrlv_ref as R
    cfg = dict(R.SVD_CONFIG, num_frames=4)
    ou, _, hu, _ = make_pair(cfg, DEV, seed=21, lean=True)
    b = _batch(cfg, 1, 4, 24, 40, seed=22)
    _run_parity(ou, hu, b, "all", "SVD widths 24x40")


def test_forward_after_unet_optimizer_steps_uses_the_updated_weights(hip_lib):
    """After AdamW steps, inference through the C++ plan and through the per-op executor equals a freshly built UNet
    loaded from the updated state_dict(), bit for bit (the packed forms of both executors follow the update)."""
    import ctrlv_ref as R
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    from ctrlv_amd.training import unet_train_step
    from tests.parity_utils import make_inputs
    config = dict(R.TINY_CONFIG)
    _, _, hu, _ = make_pair(config, DEV, seed=6)
    hu.float()
    sample, t, ehs, ids, _ = make_inputs(config, 1, 3, 16, 16)
    dev = lambda x: x.to(device=DEV, dtype=torch.float32)   # noqa: E731

    def fwd(model, executor):
        model.executor = executor
        with torch.no_grad():
            out = model(dev(sample), t.to(DEV), dev(ehs), ids.to(DEV), return_dict=False)[0]
        torch.cuda.synchronize()
        return out.clone()

    before = {ex: fwd(hu, ex) for ex in ("plan", "python")}
    hu.enable_grad(all=True)
    opt = torch.optim.AdamW(hu.get_parameters_with_grad(), lr=3e-3, weight_decay=1e-2)
    bd = {k: v.to(DEV) for k, v in _batch(config, 1, 3, 16, 16, seed=9).items()}
    for _ in range(2):
        unet_train_step(hu, bd, opt)
    fresh = UNetSpatioTemporalConditionModel(**config).to(DEV, torch.float32).eval()
    fresh.load_state_dict(hu.state_dict())
    for ex in ("plan", "python"):
        after, ref = fwd(hu, ex), fwd(fresh, ex)
        assert not torch.equal(after, before[ex]), ex
        assert torch.equal(after, ref), ex


def test_unet_gradient_checkpointing_same_step_less_memory(hip_lib):
    """unet.enable_gradient_checkpointing(): the GEGLU intermediates are recomputed by the forward's own launch, so the
    loss and every gradient are bit-identical to the plain step, at a lower peak."""
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    config = dict(R.TINY_CONFIG)
    _, _, hu, _ = make_pair(config, DEV, seed=3)
    hu.float()
    hu.enable_grad(all=True)
    b = {k: v.to(DEV) for k, v in _batch(config, 2, 4, 32, 32, drop=(1,)).items()}
    unet_train_step(hu, b)                 # warm-up: packed-weight caches and scratch buffers are allocated once
    res = {}
    for ck in (True, False):
        (hu.enable_gradient_checkpointing if ck else hu.disable_gradient_checkpointing)()
        for p in hu.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = unet_train_step(hu, b)
        torch.cuda.synchronize()
        res[ck] = (float(loss), [p.grad.clone() for p in hu.parameters()], torch.cuda.max_memory_allocated() - base)
    (l0, g0, m0), (l1, g1, m1) = res[False], res[True]
    print(f"  peak above the resident set: plain {m0 / 2**20:.1f} MiB, checkpointed {m1 / 2**20:.1f} MiB")
    assert l0 == l1 and math.isfinite(l0)
    assert all(torch.equal(a, c) for a, c in zip(g0, g1))
    assert m1 < m0


@pytest.mark.parametrize("hw", [(40, 64), (72, 128)])
def test_unet_train_step_full_size(hip_lib, hw):
    """B = 1, F = 25, SVD widths at the stage-1 training latent (320 x 512 -> 40 x 64) and at 576 x 1024 (72 x 128), all
    parameters trainable, checkpointed: loss and every gradient finite, two steps bit-identical, the loss goes down over
    three AdamW steps (the loss after them is below the loss before).  Logs the peak device memory."""
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    from ctrlv_amd.training import unet_train_step
    from ctrlv_amd.utils import build_on_device, random_init_
    h, w = hw
    F = 25
    unet = build_on_device(UNetSpatioTemporalConditionModel, DEV, dtype=torch.float32, num_frames=F)
    random_init_(unet, seed=0)
    unet.enable_grad(all=True)
    unet.enable_gradient_checkpointing()
    g = torch.Generator(device=DEV).manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)      # noqa: E731
    b = dict(latents=rn(1, F, 4, h, w), noise=rn(1, F, 4, h, w), sigmas=torch.tensor([1.5], device=DEV),
             image_latents=rn(1, 1, 4, h, w).repeat(1, F, 1, 1, 1), encoder_hidden_states=rn(1, 1, 1024),
             added_time_ids=torch.tensor([[6.0, 127.0, 0.02]], device=DEV))
    try:
        torch.cuda.reset_peak_memory_stats()
        runs = []
        for _ in range(2):
            for p in unet.parameters():
                p.grad = None
            loss = unet_train_step(unet, b)
            torch.cuda.synchronize()
            runs.append((loss.clone(), [p.grad.clone() for p in unet.parameters()]))
        peak = torch.cuda.max_memory_allocated() / 2**30
        (l0, g0), (l1, g1) = runs
        assert math.isfinite(float(l0))
        assert all(bool(torch.isfinite(x).all()) for x in g0)
        assert torch.equal(l0, l1)
        assert all(torch.equal(a, c) for a, c in zip(g0, g1))
        del runs, g0, g1
        for p in unet.parameters():
            p.grad = None
        opt = torch.optim.AdamW(unet.get_parameters_with_grad(), lr=1e-5, weight_decay=1e-2)
        losses = [float(unet_train_step(unet, b, opt)) for _ in range(3)] + [float(unet_train_step(unet, b))]
        print(f"  {h}x{w}, F={F}: peak {peak:.1f} GiB (checkpointed), losses {losses}")
        assert all(math.isfinite(v) for v in losses)
        assert losses[3] < losses[0]
    finally:
        del unet
        torch.cuda.empty_cache()
