"""Fine-tuning of the VAE temporal decoder on the HIP kernels (ctrlv_amd.training.vae_train_step; reference:
tools/train_vae_finetuning.py:303-320): the two new kernels against torch, the training walk against the inference
executor (same bits forward) and against torch.autograd on the CPU oracle of the VAE (oracle/ctrlv_ref/vae.py), the step.

Production widths (128/256/512/512) at tiny latents, parameters rounded to bf16, mix factors 0.4, as tests/test_vae_gpu.py.
Bounds: kernels -- the project's element-type bound (parity_err <= 3e-3 in bf16, a sixth of it for fp16) and 1e-4 for fp32
outputs; blocks -- rel-L2 <= 3e-2 per gradient (tests/test_backward_gpu.py); whole decoder -- the rule set of
tests/test_train_unet_gpu._check_grads with the same step through the torch modules in bf16 on the GPU as the yardstick
(concatenated < 1.5x the yardstick, each parameter < 3x its yardstick with the 2e-2 floor, vanishing reference gradients
held to 1e-5 of the largest, mix factors on the absolute error against the largest mix-factor gradient), plus absolute
caps set from the measured values (see test_vae_decoder_every_gradient)."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from tests.parity_utils import parity_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def g(seed=0):
    return torch.Generator().manual_seed(seed)


def bf(x):
    return x.to(torch.bfloat16).float()


def rows(x):            # (N, C, H, W) -> [N*H*W, C]
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def nchw(r, n, h, w):
    return r.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


@pytest.fixture(scope="module")
def vae(hip_lib):
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    torch.manual_seed(5)
    m = AutoencoderKLTemporalDecoder().eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("mix_factor"):
                p.fill_(0.4)
            p.copy_(p.to(torch.bfloat16).float())
    return m


def _trainable(vae_cpu):
    """fp32 copy on the device, decoder trainable, the rest frozen (the reference's setting)"""
    m = copy.deepcopy(vae_cpu).to(DEV)
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("decoder."))
        p.grad = None
    return m


def _oracle_sd(vae_cpu):
    sd = {k: v.detach().clone() for k, v in vae_cpu.state_dict().items()}
    for k, v in sd.items():
        if k.startswith("decoder."):
            v.requires_grad_(True)
    return sd


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("el", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("S,peaked", [(64, False), (192, False), (2560, False), (192, True)])
def test_softmax_rows_bwd(ops, S, peaked, el):
    """dS = scale * P o (dP - rowsum(P o dP)) against fp32 torch on the same rounded P; `peaked`: scores large enough that
    the rows are nearly one-hot (dP - rowsum cancels).  The output is pre-filled with NaN: every element is written."""
    tol = 3e-3 if el == torch.bfloat16 else 3e-3 / 6.0
    scores = torch.randn(S, S, generator=g(S)) * (14.0 if peaked else 1.5)
    P = torch.softmax(scores, dim=-1).to(el)
    if peaked:
        assert float(P.float().max(dim=-1).values.median()) > 0.9
    dP = torch.randn(S, S, generator=g(S + 1))
    scale = 512 ** -0.5
    Pf = P.float()
    ref = scale * Pf * (dP - (Pf * dP).sum(-1, keepdim=True))
    ds = torch.full((S, S), float("nan"), dtype=el, device=DEV)
    ops.softmax_rows_bwd(P.to(DEV), dP.to(DEV), scale, ds)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ds.float()).all())
    assert parity_err(ds.float().cpu(), ref, f"softmax_rows_bwd S={S} peaked={peaked} {el}") < tol


@pytest.mark.parametrize("el", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,clip", [(1, 1), (2, 2), (5, 5), (4, 2), (3, 1)])
@pytest.mark.parametrize("H,W", [(8, 8), (24, 40)])
def test_time_conv_rows_to_nchw_bwd(ops, n, clip, H, W, el):
    """Against F.conv3d autograd: one clip of 1 / 2 / 5 frames, two clips of 2, three clips of 1.  fp32 outputs at 1e-4,
    dRows at the element-type bound with its padding column zero, outer taps exactly zero at one frame per clip, the
    parameter gradients bit-identical across two runs."""
    tol = 3e-3 if el == torch.bfloat16 else 3e-3 / 6.0
    co, HW = 3, H * W
    y = torch.randn(n * HW, 4, generator=g(2)).to(el)                     # (column 3: padding, ignored by the forward)
    wt = torch.randn(co, co, 3, generator=g(3))
    dout = torch.randn(n, co, H, W, generator=g(4))
    x5 = y.float()[:, :co].reshape(n // clip, clip, H, W, co).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    w5 = wt[:, :, :, None, None].clone().requires_grad_(True)
    b = torch.randn(co, generator=g(5)).requires_grad_(True)
    out = F.conv3d(x5, w5, b, padding=(1, 0, 0))                          # (clips, C, F, H, W)
    out.backward(dout.reshape(n // clip, clip, co, H, W).permute(0, 2, 1, 3, 4))
    ref_rows = x5.grad.permute(0, 2, 3, 4, 1).reshape(n * HW, co)
    runs = []
    for _ in range(2):
        drows = torch.full((n * HW, 4), float("nan"), dtype=el, device=DEV)
        dw = torch.full((co, co, 3), float("nan"), device=DEV)
        db = torch.full((co,), float("nan"), device=DEV)
        ops.time_conv_rows_to_nchw_bwd(dout.to(DEV), y.to(DEV), n, clip, co, HW, wt.to(DEV), drows, dw, db)
        torch.cuda.synchronize()
        runs.append((drows, dw, db))
    drows, dw, db = runs[0]
    assert torch.equal(dw, runs[1][1]) and torch.equal(db, runs[1][2]) and torch.equal(drows, runs[1][0])
    assert parity_err(dw.cpu(), w5.grad[:, :, :, 0, 0], "dWeight") < 1e-4
    assert parity_err(db.cpu(), b.grad, "dBias") < 1e-4
    assert parity_err(drows[:, :co].float().cpu(), ref_rows, "dRows") < tol
    assert float(drows[:, co:].float().abs().max()) == 0.0
    if clip == 1:
        assert float(dw[:, :, 0].abs().max()) == 0.0 and float(dw[:, :, 2].abs().max()) == 0.0
        assert float(w5.grad[:, :, 0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ forward identity
@pytest.mark.parametrize("n,nf,h,w", [(3, 3, 8, 8), (4, 2, 8, 8), (4, 1, 8, 8)])
def test_train_forward_is_the_inference_executor_bit_for_bit(vae, n, nf, h, w):
    from ctrlv_amd.models import vae_decoder_hip as vh
    from ctrlv_amd.training import vae_decoder_train_forward
    m = _trainable(vae)
    z = bf(torch.randn(n, 4, h, w, generator=g(3))).to(DEV)
    with torch.no_grad():
        ref = vh.decode(m.decoder, z, nf)
    got = vae_decoder_train_forward(m.decoder, z, nf)
    torch.cuda.synchronize()
    assert got.shape == (n, 3, 8 * h, 8 * w) and got.dtype == torch.float32 and got.requires_grad
    assert torch.equal(got.detach().to(ref.dtype), ref)
    zb = z.to(torch.bfloat16)
    with torch.no_grad():
        ref16 = vh.decode(m.decoder, zb, nf)
    assert torch.equal(vae_decoder_train_forward(m.decoder, zb, nf).detach().to(torch.bfloat16), ref16)


@pytest.mark.parametrize("which", ["shortcut", "plain"])
def test_res_block_forward_identity_and_gradients(vae, which):
    """One SpatioTemporalResBlock of the decoder (512 -> 256 with conv_shortcut / 128 -> 128): the training forward equals
    vae_decoder_hip._res bit for bit (one clip of 3, and two clips of 2 against the per-clip launches); gradients of the
    input and of every parameter against the oracle's autograd, rel-L2 <= 3e-2."""
    import ctrlv_ref as R
    from ctrlv_amd.autograd import vae_res_block_train_forward
    from ctrlv_amd.models import vae_decoder_hip as vh
    m = _trainable(vae)
    i, j = (2, 0) if which == "shortcut" else (3, 1)
    blk = m.decoder.up_blocks[i].resnets[j]
    key = f"decoder.up_blocks.{i}.resnets.{j}"
    cout, cin = blk.spatial_res_block.conv1.weight.shape[:2]
    assert (blk.spatial_res_block.conv_shortcut is not None) == (which == "shortcut")
    n, H, W = 3, 8, 8
    x = bf(torch.randn(4, cin, H, W, generator=g(11)))
    sc = vh._Scratch(DEV)
    pk = vh._pack_res(blk)
    xr = rows(x).to(DEV, torch.bfloat16)
    with torch.no_grad():
        ref3 = vh._res(pk, xr[:n * H * W], n, H, W, sc).clone()
        ref22 = torch.cat([vh._res(pk, xr[:2 * H * W], 2, H, W, sc).clone(), vh._res(pk, xr[2 * H * W:], 2, H, W, sc).clone()])
        assert torch.equal(vae_res_block_train_forward(blk, xr, 2, 2, H, W), ref22)
    xh = xr[:n * H * W].clone().requires_grad_(True)
    yh = vae_res_block_train_forward(blk, xh, 1, n, H, W)
    assert torch.equal(yh.detach(), ref3)
    # ---- gradients: the oracle block on the same parameters (upstream gradient as in tests/test_backward_gpu.py)
    sd = {k: v for k, v in _oracle_sd(vae).items() if k.startswith(key + ".")}
    xo = x[:n].clone().requires_grad_(True)
    yo = R.vae.spatio_temporal_resblock(sd, key, xo, n)
    dy = bf(yo.detach() + 0.5 * torch.randn(n, cout, H, W, generator=g(7)))
    yo.backward(dy)
    yh.backward(rows(dy).to(DEV, torch.bfloat16))
    torch.cuda.synchronize()
    errs = {"x": rel_l2(nchw(xh.grad.float().cpu(), n, H, W), xo.grad)}
    for name, p in blk.named_parameters():
        assert p.grad is not None, name
        rg = sd[f"{key}.{name}"].grad
        errs[name] = rel_l2(p.grad.float().cpu().reshape(rg.shape), rg)
    for k, v in errs.items():
        print(f"  {v:.2e}  d/d {k}")
    assert max(errs.values()) < 3e-2, errs


@pytest.mark.parametrize("H,W", [(8, 8), (16, 12)])
def test_attention_forward_identity_and_gradients(vae, H, W):
    """The mid block's head-dim-512 attention: forward bits of vae_decoder_hip._attn; gradients of the input and of every
    parameter against the oracle's autograd, rel-L2 <= 3e-2.  to_k.bias has no gradient (the softmax removes a per-row
    shift of the scores): the oracle leaves rounding noise, the HIP path returns exact zeros."""
    import ctrlv_ref as R
    from ctrlv_amd.autograd import vae_attention_train_forward
    from ctrlv_amd.models import vae_decoder_hip as vh
    m = _trainable(vae)
    a = m.decoder.mid_block.attentions[0]
    key = "decoder.mid_block.attentions.0"
    n, C = 2, 512
    x = bf(torch.randn(n, C, H, W, generator=g(13)) * 2.0)
    xr = rows(x).to(DEV, torch.bfloat16)
    with torch.no_grad():
        ref = vh._attn(vh.pack_attn(a), xr, n, H, W, vh._Scratch(DEV)).clone()
    xh = xr.clone().requires_grad_(True)
    yh = vae_attention_train_forward(a, xh, n, H, W)
    assert torch.equal(yh.detach(), ref)
    sd = {k: v for k, v in _oracle_sd(vae).items() if k.startswith(key + ".")}
    xo = x.clone().requires_grad_(True)
    yo = R.vae.attention(sd, key, xo)
    dy = bf(torch.randn(n, C, H, W, generator=g(7)))
    yo.backward(dy)
    yh.backward(rows(dy).to(DEV, torch.bfloat16))
    torch.cuda.synchronize()
    gmax = max(float(v.grad.abs().max()) for v in sd.values())
    errs = {"x": rel_l2(nchw(xh.grad.float().cpu(), n, H, W), xo.grad)}
    for name, p in a.named_parameters():
        assert p.grad is not None, name
        rg = sd[f"{key}.{name}"].grad
        if float(rg.abs().max()) <= 1e-6 * gmax:
            assert name == "to_k.bias" and float(p.grad.abs().max()) <= 1e-5 * gmax, name
            continue
        errs[name] = rel_l2(p.grad.float().cpu().reshape(rg.shape), rg)
    for k, v in errs.items():
        print(f"  {v:.2e}  d/d {k}")
    assert "to_k.bias" not in errs
    assert max(errs.values()) < 3e-2, errs


# ------------------------------------------------------------------------------------------------ whole decoder
def _decoder_losses_and_grads(vae_cpu, z, target, nf):
    """(oracle sd with grads, HIP model, yardstick model, (loss, loss_ref)): loss = mse(clamp(decode(z), -1, 1), target)."""
    import ctrlv_ref as R
    from ctrlv_amd.training import vae_decoder_train_forward
    sd = _oracle_sd(vae_cpu)
    pred = R.vae.decode(sd, z, nf)
    print(f"  oracle: {float(((pred < -1) | (pred > 1)).float().mean()):.1e} of the outputs clamped")
    loss_ref = F.mse_loss(pred.clamp(-1, 1), target)
    loss_ref.backward()
    hm = _trainable(vae_cpu)
    loss = F.mse_loss(vae_decoder_train_forward(hm.decoder, z.to(DEV), nf).clamp(-1, 1), target.to(DEV))
    loss.backward()
    ym = copy.deepcopy(vae_cpu).to(DEV, torch.bfloat16)
    for p in ym.parameters():
        p.grad = None
    py = ym.decoder(z.to(DEV, torch.bfloat16), nf)
    F.mse_loss(py.clamp(-1, 1).float(), target.to(DEV)).backward()
    torch.cuda.synchronize()
    return sd, hm, ym, (float(loss.detach()), float(loss_ref.detach()))


# Absolute caps of test_vae_decoder_every_gradient: below 1.5x the values measured on an MI355X (2.18e-2 concatenated,
# 3.84e-2 for the worst single parameter: docstring there), and far below the LoRA test's per-parameter 2.2e-1.
CAP_TOTAL = 3.2e-2
CAP_PARAM = 5.7e-2


def _check_grads(hm, sd, ym, b_loss, tag, cap_total=CAP_TOTAL, cap_param=CAP_PARAM):
    """The rule set of tests/test_train_unet_gpu._check_grads on the decoder: HIP gradients of `hm.decoder` against the
    oracle's (`sd`, keys decoder.*), next to the yardstick `ym` (torch modules, bf16, GPU)."""
    loss, loss_ref = b_loss
    print(f"  [{tag}] loss: HIP {loss:.6f}  oracle {loss_ref:.6f}")
    assert math.isfinite(loss) and abs(loss - loss_ref) <= 5e-3 * abs(loss_ref)
    ref = {k[len("decoder."):]: v.grad for k, v in sd.items() if k.startswith("decoder.")}
    assert all(v is not None for v in ref.values())                  # (the oracle leaves no parameter without a gradient)
    yp = dict(ym.decoder.named_parameters())
    gmax = max(float(v.abs().max()) for v in ref.values())
    errs, got, rf, yard = {}, [], [], []
    hp = dict(hm.decoder.named_parameters())
    assert set(hp) == set(ref)
    for name, p in hp.items():
        rg = ref[name]
        assert p.grad is not None, name
        if float(rg.abs().max()) <= 1e-6 * gmax:
            assert float(p.grad.abs().max()) <= 1e-5 * gmax, name
            print(f"  vanishing reference gradient ({float(rg.abs().max()):.1e}): {name}, HIP {float(p.grad.abs().max()):.1e}")
            continue
        pg = p.grad.float().cpu().reshape(rg.shape)
        errs[name] = rel_l2(pg, rg)
        got.append(pg.reshape(-1)); rf.append(rg.reshape(-1)); yard.append(yp[name].grad.float().cpu().reshape(-1))
    tot, ytot = rel_l2(torch.cat(got), torch.cat(rf)), rel_l2(torch.cat(yard), torch.cat(rf))
    ypar = {n: rel_l2(yp[n].grad.float().cpu().reshape(ref[n].shape), ref[n]) for n in errs}
    for n, v in sorted(errs.items(), key=lambda kv: -kv[1])[:8]:
        print(f"  {v:.2e} (torch bf16: {ypar[n]:.2e})  d/d {n}")
    worst = max(v for n, v in errs.items() if not n.endswith("mix_factor"))
    print(f"  {len(errs)} parameter gradients, concatenated: rel-L2 {tot:.2e}   (torch bf16: {ytot:.2e});  worst single "
          f"parameter {worst:.2e}")
    assert tot < cap_total and tot < 1.5 * ytot
    mix = [n for n in errs if n.endswith("mix_factor")]
    mixmax = max(float(ref[n].abs().max()) for n in mix)
    for n, v in errs.items():
        if n.endswith("mix_factor"):
            ae = float((hp[n].grad.float().cpu().reshape(-1) - ref[n].reshape(-1)).abs().max())
            print(f"  mix factor {n}: abs err {ae:.2e} of max {mixmax:.2e}")
            assert ae < 5e-2 * mixmax, (n, ae, mixmax)
        else:
            assert v < cap_param and v < max(3.0 * ypar[n], 2e-2), (n, v, ypar[n])
    return errs


def test_vae_decoder_every_gradient(vae):
    """3 frames as one clip, 8x8 latent, target uniform in [-1, 1]: the loss and the gradient of EVERY decoder parameter
    against the oracle's autograd, next to the torch-module bf16 yardstick.
    Measured on an MI355X: loss 0.384468 against the oracle's 0.384451 (5.4e-5 of the outputs clamped); 265 gradients
    concatenated rel-L2 2.18e-2 (torch bf16 yardstick: 3.32e-2); worst single parameter 3.84e-2 (the attention's to_k.weight;
    yardstick 5.37e-2); mix factors: worst absolute error 2.0e-5 against the largest mix-factor gradient 1.06e-3 (1.9 %;
    in relative terms up to 2.9e-1, the yardstick up to 2.2); to_k.bias: oracle 3.1e-12, here exact zeros."""
    z = bf(torch.randn(3, 4, 8, 8, generator=g(3)))
    target = torch.rand(3, 3, 64, 64, generator=g(4)) * 2 - 1
    sd, hm, ym, b_loss = _decoder_losses_and_grads(vae, z, target, 3)
    errs = _check_grads(hm, sd, ym, b_loss, "3 frames, 8x8")
    assert len(errs) >= len(list(hm.decoder.parameters())) - 2
    assert "mid_block.attentions.0.to_k.bias" not in errs and any(n.startswith("time_conv_out.") for n in errs)


def test_vae_decoder_one_frame_per_clip(vae):
    """num_frames = 1 (the reference's setting), 4 images of 8x8 latents: the loss against the oracle's, and the outer taps
    of every temporal conv weight and of time_conv_out get exactly zero gradient (as in the oracle)."""
    import ctrlv_ref as R
    from ctrlv_amd.training import vae_decoder_train_forward
    z = bf(torch.randn(4, 4, 8, 8, generator=g(6)))
    target = torch.rand(4, 3, 64, 64, generator=g(7)) * 2 - 1
    sd = _oracle_sd(vae)
    loss_ref = F.mse_loss(R.vae.decode(sd, z, 1).clamp(-1, 1), target)
    loss_ref.backward()
    hm = _trainable(vae)
    loss = F.mse_loss(vae_decoder_train_forward(hm.decoder, z.to(DEV), 1).clamp(-1, 1), target.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    loss, loss_ref = float(loss.detach()), float(loss_ref.detach())
    print(f"  loss: HIP {loss:.6f}  oracle {loss_ref:.6f}")
    assert abs(loss - loss_ref) <= 5e-3 * abs(loss_ref)
    seen = 0
    for name, p in hm.decoder.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        if p.dim() == 5:
            rg = sd["decoder." + name].grad
            assert float(rg[:, :, 0].abs().max()) == 0.0 and float(rg[:, :, 2].abs().max()) == 0.0, name
            assert float(p.grad[:, :, 0].abs().max()) == 0.0 and float(p.grad[:, :, 2].abs().max()) == 0.0, name
            assert float(p.grad[:, :, 1].abs().max()) > 0.0, name
            seen += 1
    assert seen == 2 * 14 + 1                                   # two temporal convs in each of 14 res blocks + time_conv_out


# ------------------------------------------------------------------------------------------------ the step
def test_vae_train_step(vae):
    """Two AdamW steps on the decoder: encoder / quant_conv untouched, every decoder parameter moves, bit-reproducible
    gradients, inference after the steps follows the update, gradient accumulation adds up to the single step."""
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.training import vae_train_step
    m = _trainable(vae)
    px = (torch.rand(4, 3, 64, 64, generator=g(21)) * 2 - 1).to(DEV)
    batch = {"pixel_values": px}
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)   # noqa: E731
    # (gradients of a first step, twice on fresh copies: the same bits)
    grads = []
    for _ in range(2):
        c = _trainable(vae)
        loss0 = vae_train_step(c, batch, num_frames=2, generator=gen())
        grads.append({n: p.grad.clone() for n, p in c.decoder.named_parameters()})
        assert all(p.grad is None for p in c.encoder.parameters()) and all(p.grad is None for p in c.quant_conv.parameters())
    assert all(torch.equal(grads[0][n], grads[1][n]) for n in grads[0])
    # (accumulation: two half-weight micro-batches of the same batch = the single step)
    c = _trainable(vae)
    vae_train_step(c, batch, num_frames=2, generator=gen(), accumulate=True, loss_scale=0.5)
    vae_train_step(c, batch, num_frames=2, generator=gen(), accumulate=True, loss_scale=0.5)
    for n, p in c.decoder.named_parameters():
        assert rel_l2(p.grad, grads[0][n]) <= 1e-6 or float(grads[0][n].abs().max()) == 0.0, n
    del c, grads
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = torch.optim.AdamW([p for p in m.decoder.parameters()], lr=1e-3, weight_decay=1e-2)
    l1 = vae_train_step(m, batch, opt, num_frames=2, generator=gen())
    l2 = vae_train_step(m, batch, opt, num_frames=2, generator=gen())
    torch.cuda.synchronize()
    print(f"  losses {float(loss0):.5f} / {float(l1):.5f} -> {float(l2):.5f}")
    assert torch.equal(l1, loss0) and math.isfinite(float(l2))
    for n, p in m.named_parameters():
        if n.startswith("decoder."):
            assert not torch.equal(before[n], p.detach()), n
        else:
            assert torch.equal(before[n], p.detach()) and p.grad is None, n
    fresh = AutoencoderKLTemporalDecoder().to(DEV).eval()
    fresh.load_state_dict(m.state_dict())
    z = bf(torch.randn(4, 4, 8, 8, generator=g(3))).to(DEV)
    with torch.no_grad():
        after, ref = m.decode(z, num_frames=2).sample, fresh.decode(z, num_frames=2).sample
    assert torch.equal(after, ref)
    with pytest.raises(ValueError):
        vae_train_step(m, batch, num_frames=3)
    with pytest.raises(ValueError):
        vae_train_step(m, {"pixel_values": px[:, :, :40, :40]}, num_frames=2)
