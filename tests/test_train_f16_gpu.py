"""The training steps with fp16 ELEMENTS and a dynamic loss scale on the device (the reference's --mixed_precision fp16):
`unet_train_step` / `train_step` with compute_dtype=torch.float16 and a `ctrlv_amd.optim.LossScaler`.

Tiny configuration, F = 3, 16 x 16 latents, the batches and the gradient rules of tests/test_train_unet_gpu.py,
tests/test_train_gpu.py and tests/test_lora_gpu.py.  On top of those rules the fp16 route's concatenated rel-L2 against the
oracle's fp32 autograd must be NO LARGER than the bf16 route's on the same batch (the bf16 route runs in the same test); the two
figures are printed.  Power-of-two loss scales and the element-type switch are checked bit for bit.

Measured on an MI355X (concatenated rel-L2 of all parameter gradients, fp16 route / bf16 route): see DESIGN 3.9."""
import copy
import math

import pytest
import torch

from tests import loss_scale_ref as L
from tests.parity_utils import make_pair, rel_l2
from tests.test_train_unet_gpu import _batch, _check_grads, _oracle_unet_step, _set_mode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = torch.float16
S10 = 2.0 ** 10


def _scaler(**kw):
    from ctrlv_amd.optim import LossScaler
    return LossScaler(**dict(dict(init_scale=S10, growth_interval=10 ** 9), **kw))


def _adamw(params, **kw):
    from ctrlv_amd.optim import AdamW
    return AdamW(list(params), **dict(dict(lr=1e-4, weight_decay=1e-2), **kw))


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _concat_err(grads, refp, names):
    got = torch.cat([grads[n].float().cpu().reshape(-1) for n in names])
    return rel_l2(got, torch.cat([refp[n].grad.reshape(-1) for n in names]))


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("B", [1, 2])
def test_unet_step_f16_matches_oracle_and_is_no_worse_than_bf16(hip_lib, B):
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    config = dict(R.TINY_CONFIG)
    ou, _, hu, _ = make_pair(config, DEV, seed=3)
    b = _batch(config, B, 3, 16, 16, drop=(0,) if B == 2 else ())
    bd = {k: v.to(DEV) for k, v in b.items()}
    _set_mode(ou, "all")
    with torch.enable_grad():
        loss_ref = float(_oracle_unet_step(ou, b))
        hu.float()
        _set_mode(hu, "all")
        opt = _adamw(hu.get_parameters_with_grad())
        loss_bf = float(unet_train_step(hu, bd))                                  # the bf16 route: the code as it was
        g_bf = _grads(hu)
        opt.zero_grad()
        scaler = _scaler()
        loss = float(unet_train_step(hu, bd, None, compute_dtype=H, scaler=scaler))
        g16 = {n: g * 2.0 ** -10 for n, g in _grads(hu).items()}
        scaler.step(opt)
        scaler.update()
        st = {k: v.clone() for k, v in opt.grad_state().items()}
        yu = copy.deepcopy(ou).to(DEV, torch.bfloat16)
        _set_mode(yu, "all")
        _oracle_unet_step(yu, b)
    torch.cuda.synchronize()
    assert int(st["skip"]) == 0 and int(st["skipped_total"]) == 0 and math.isfinite(float(st["norm"]))
    assert scaler.get_scale() == S10
    for n, p in hu.named_parameters():
        p.grad.copy_(g16[n])
    errs = _check_grads(hu, ou, yu, (loss, loss_ref), f"fp16 elements, all, B={B}")
    assert len(errs) > 300
    refp = dict(ou.named_parameters())
    tot16, totbf = _concat_err(g16, refp, list(errs)), _concat_err(g_bf, refp, list(errs))
    print(f"  B={B}: concatenated rel-L2 against the fp32 oracle: fp16 route {tot16:.3e}   bf16 route {totbf:.3e}   "
          f"(ratio {tot16 / totbf:.3f}); loss fp16 {loss:.6f} bf16 {loss_bf:.6f} oracle {loss_ref:.6f}")
    assert tot16 <= totbf, (tot16, totbf)


def _check_controlnet_grads(grads, oc, yc, tag):
    """tests/test_train_gpu.py's rules: concatenated < 3e-2 and < 1.5x the torch-bf16 yardstick; per parameter < 8e-2 and
    < max(2x yardstick, 2e-2); mix factors on the absolute error against the largest mix-factor gradient."""
    refp, yp = dict(oc.named_parameters()), dict(yc.named_parameters())
    gmax = max(float(q.grad.abs().max()) for q in refp.values() if q.grad is not None)
    errs = {}
    for name, rp in refp.items():
        rg = rp.grad
        if rg is None or float(rg.abs().max()) <= 1e-6 * gmax:
            assert name not in grads or float(grads[name].abs().max()) == 0.0, name
            continue
        assert name in grads, name
        errs[name] = rel_l2(grads[name].float().cpu().reshape(rg.shape), rg)
    yard = {n: rel_l2(yp[n].grad.float().cpu(), refp[n].grad) for n in errs}
    ytot = _concat_err({n: yp[n].grad for n in errs}, refp, list(errs))
    tot = _concat_err(grads, refp, list(errs))
    print(f"  [{tag}] {len(errs)} parameter gradients, all concatenated: rel-L2 {tot:.2e}   (torch bf16: {ytot:.2e})")
    assert tot < 3e-2 and tot < 1.5 * ytot
    mixmax = max(float(refp[n].grad.abs().max()) for n in errs if n.endswith("mix_factor"))
    for n, v in errs.items():
        if n.endswith("mix_factor"):
            ae = float((grads[n].float().cpu().reshape(-1) - refp[n].grad.reshape(-1)).abs().max())
            assert ae < 5e-2 * mixmax, (n, ae, mixmax)
        else:
            assert v < 8e-2 and v < max(2.0 * yard[n], 2e-2), (n, v, yard[n])
    return errs, tot


def test_controlnet_step_f16_matches_oracle_and_is_no_worse_than_bf16(hip_lib):
    """ControlNet trainable, UNet frozen; the frozen UNet is held in the element type of the route (bf16 / fp16 copies of the
    same bf16-representable weights)."""
    import ctrlv_ref as R
    from ctrlv_amd.training import train_step
    from tests.test_train_gpu import _batch as _cbatch, _oracle_step
    config = dict(R.TINY_CONFIG)
    ou, oc, hu, hc = make_pair(config, DEV, seed=3)
    _, _, hu16, _ = make_pair(config, DEV, seed=3)
    hu16.half()
    b = _cbatch(config, 1, 3, 16, 16)
    bd = {k: v.to(DEV) for k, v in b.items()}
    with torch.enable_grad():
        loss_ref = float(_oracle_step(ou, oc, b, 0.8))
        hc.float()
        for p in hc.parameters():
            p.requires_grad_(True)
        for m in (hu, hu16):
            for p in m.parameters():
                p.requires_grad_(False)
        opt = _adamw(hc.parameters())
        loss_bf = float(train_step(hc, hu, bd, optimizer=None, conditioning_scale=0.8))
        g_bf = _grads(hc)
        opt.zero_grad()
        scaler = _scaler()
        loss = float(train_step(hc, hu16, bd, optimizer=None, conditioning_scale=0.8, compute_dtype=H, scaler=scaler))
        g16 = {n: g * 2.0 ** -10 for n, g in _grads(hc).items()}
        scaler.step(opt)
        st = {k: v.clone() for k, v in opt.grad_state().items()}
        yu, yc = copy.deepcopy(ou).to(DEV, torch.bfloat16), copy.deepcopy(oc).to(DEV, torch.bfloat16)
        for q in yc.parameters():
            q.grad = None
        _oracle_step(yu, yc, b, 0.8)
    torch.cuda.synchronize()
    print(f"  loss: fp16 route {loss:.6f}  bf16 route {loss_bf:.6f}  oracle {loss_ref:.6f}")
    assert math.isfinite(loss) and abs(loss - loss_ref) <= 5e-3 * abs(loss_ref)
    assert int(st["skip"]) == 0 and all(p.grad is None for m in (hu, hu16) for p in m.parameters())
    errs, tot16 = _check_controlnet_grads(g16, oc, yc, "fp16 elements")
    totbf = _concat_err(g_bf, dict(oc.named_parameters()), list(errs))
    print(f"  concatenated rel-L2 against the fp32 oracle: fp16 route {tot16:.3e}   bf16 route {totbf:.3e}   (ratio {tot16 / totbf:.3f})")
    assert tot16 <= totbf, (tot16, totbf)
    with pytest.raises(ValueError, match="compute_dtype"):
        train_step(hc, hu, bd, optimizer=None, compute_dtype=H)                   # a bf16-held frozen UNet under fp16 elements


# ------------------------------------------------------------------------------------------------ 2. bit for bit
def _fresh_unet(config, seed=6, mode="all"):
    _, _, hu, _ = make_pair(config, DEV, seed=seed)
    hu.float()
    _set_mode(hu, mode)
    return hu


def test_power_of_two_scale_on_the_bf16_route_is_exact(hip_lib):
    """The backward is linear in the upstream gradient, fp32 and bf16 share an exponent range, and a power of two commutes with
    every rounding: p.grad * 2^-10 under LossScaler(2^10) equals the scaler-free p.grad, and so do the parameters after the step."""
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    config = dict(R.TINY_CONFIG)
    bd = {k: v.to(DEV) for k, v in _batch(config, 2, 3, 16, 16, seed=9, drop=(1,)).items()}
    out = []
    for scaled in (False, True):
        hu = _fresh_unet(config)
        opt = _adamw(hu.get_parameters_with_grad(), lr=1e-3)
        scaler = _scaler() if scaled else None
        unet_train_step(hu, bd, None, scaler=scaler)
        grads = {n: g * (2.0 ** -10 if scaled else 1.0) for n, g in _grads(hu).items()}
        opt.zero_grad()
        loss = unet_train_step(hu, bd, opt, scaler=scaler)
        out.append((grads, {n: p.detach().clone() for n, p in hu.named_parameters()}, loss.clone()))
        if scaled:
            assert int(opt.grad_state()["skip"]) == 0 and scaler.get_scale() == S10
    torch.cuda.synchronize()
    (g0, p0, l0), (g1, p1, l1) = out
    assert torch.equal(l0, l1) and set(g0) == set(g1) and len(g0) > 300
    differ = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not differ, differ[:8]
    moved = [n for n in p0 if not torch.equal(p0[n], p1[n])]
    assert not moved, moved[:8]
    assert sum(float(g.abs().max()) > 0 for g in g0.values()) > 300


def test_none_is_todays_step_and_the_two_types_do_not_share_cached_forms(hip_lib):
    """compute_dtype=None without a scaler is the step without the arguments, bit for bit.  In temporal-only mode (the spatial
    layers are FROZEN fp32 parameters: their packed forms are cached) the same model stepped bf16, fp16, bf16, fp16 gives each
    type the bits a model gives that has only ever run in that type."""
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    config = dict(R.TINY_CONFIG)
    bd = {k: v.to(DEV) for k, v in _batch(config, 2, 3, 16, 16, seed=8, drop=(1,)).items()}

    def run(hu, **kw):
        for p in hu.parameters():
            p.grad = None
        loss = unet_train_step(hu, bd, **kw)
        return loss.clone(), _grads(hu)

    def same(a, b):
        return torch.equal(a[0], b[0]) and set(a[1]) == set(b[1]) and all(torch.equal(a[1][n], b[1][n]) for n in a[1])

    hu = _fresh_unet(config, mode="temporal")
    today = run(hu)
    assert same(today, run(hu, compute_dtype=None, scaler=None)) and same(today, run(hu, compute_dtype=torch.bfloat16))
    h1 = run(hu, compute_dtype=H)
    b2 = run(hu)
    h2 = run(hu, compute_dtype=H)
    only16 = run(_fresh_unet(config, mode="temporal"), compute_dtype=H)
    torch.cuda.synchronize()
    assert same(today, b2) and same(h1, h2) and same(h1, only16)
    assert not same(today, h1) and all(bool(torch.isfinite(g).all()) for g in h1[1].values())
    assert len(today[1]) > 20 and all("temporal_transformer_block" in n for n in today[1])


def test_gradient_checkpointing_gives_the_same_f16_gradients(hip_lib):
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    config = dict(R.TINY_CONFIG)
    bd = {k: v.to(DEV) for k, v in _batch(config, 1, 3, 16, 16, seed=9).items()}
    out = []
    for ckpt in (False, True):
        hu = _fresh_unet(config)
        if ckpt:
            hu.enable_gradient_checkpointing()
        loss = unet_train_step(hu, bd, None, compute_dtype=H, scaler=_scaler())
        out.append((loss.clone(), _grads(hu)))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and set(out[0][1]) == set(out[1][1]) and len(out[0][1]) > 300
    differ = [n for n in out[0][1] if not torch.equal(out[0][1][n], out[1][1][n])]
    assert not differ, differ[:8]
    assert all(bool(torch.isfinite(g).all()) for g in out[0][1].values())


# ------------------------------------------------------------------------------------------------ 3. the dynamics
def test_dynamic_scale_backs_off_until_a_step_is_applied(hip_lib):
    """init_scale 2^24, growth_interval 2, 8 steps of the tiny fp16 step.  Whenever the record says skip, the parameters kept
    their bits and the scale halved; the whole trajectory of scale and tracker is the restatement's for the skips observed; by
    the last step a step has been applied and the loss is finite.  The test reads nothing from the device inside the loop: it
    clones the records, and compares at the end.  A non-finite gradient value is ordinary data here."""
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    config = dict(R.TINY_CONFIG)
    bd = {k: v.to(DEV) for k, v in _batch(config, 1, 3, 16, 16, seed=9).items()}
    hu = _fresh_unet(config)
    params = list(hu.get_parameters_with_grad())
    opt = _adamw(params, lr=1e-4)
    kw = dict(init_scale=2.0 ** 24, growth_interval=2)
    scaler = _scaler(**kw)
    trail = [(None, None, [p.detach().clone() for p in params], None)]
    for _ in range(8):
        loss = unet_train_step(hu, bd, opt, compute_dtype=H, scaler=scaler, max_grad_norm=1.0)
        trail.append((scaler._record.clone(), {k: v.clone() for k, v in opt.grad_state().items()},
                      [p.detach().clone() for p in params], loss.clone()))
    torch.cuda.synchronize()
    rec = L.Record(**kw)
    skips = []
    for k in range(1, 9):
        ls, st, ps, loss = trail[k]
        skip = int(st["skip"])
        skips.append(skip)
        before = rec.scale
        assert rec.step(bool(skip)) == skip
        kept = all(torch.equal(a, b) for a, b in zip(trail[k - 1][2], ps))
        assert float(ls[0].view(torch.float32)) == rec.scale and int(ls[2]) == rec.growth_tracker, (k, skips)
        assert int(st["skipped_total"]) == rec.skipped_total
        if skip:
            assert kept and rec.scale == before / 2 and not math.isfinite(float(st["norm"])), k
        else:
            assert not kept and math.isfinite(float(st["norm"])) and 0.0 < float(st["coef"]) <= 1.0, k
    print(f"\n  skips {skips}; scale 2^24 -> {rec.scale:g}; losses {[round(float(t[3]), 5) for t in trail[1:]]}")
    assert 0 in skips and math.isfinite(float(trail[8][3]))
    assert float(opt.state[params[0]]["step"]) == 8.0                              # attempted steps
    assert all(bool(torch.isfinite(p).all()) for p in params)


# ------------------------------------------------------------------------------------------------ 4. LoRA mode
def test_lora_step_f16(hip_lib):
    """One LoRA-mode step with fp16 elements: finite factor gradients within tests/test_lora_gpu.py's rule."""
    import ctrlv_ref as R
    from ctrlv_amd.training import unet_train_step
    from tests.test_lora_gpu import _cfg, _random_B, _wrap_oracle
    config = dict(R.TINY_CONFIG)
    ou, _, hu, _ = make_pair(config, DEV, seed=3)
    hu.float()
    hu.add_adapter(_cfg(r=4, alpha=8))
    _random_B(hu)
    b = _batch(config, 1, 3, 16, 16)
    yu = copy.deepcopy(ou).to(DEV, torch.bfloat16)
    of, yf = _wrap_oracle(ou, hu, 4, 2.0), _wrap_oracle(yu, hu, 4, 2.0)
    with torch.enable_grad():
        loss_ref = float(_oracle_unet_step(ou, b))
        _oracle_unet_step(yu, b)
        loss = float(unet_train_step(hu, {k: v.to(DEV) for k, v in b.items()}, None, compute_dtype=H, scaler=_scaler()))
    torch.cuda.synchronize()
    assert math.isfinite(loss) and abs(loss - loss_ref) <= 5e-3 * abs(loss_ref), (loss, loss_ref)
    hp = dict(hu.named_parameters())
    got, ref, yst = [], [], []
    for n in of:
        assert hp[n].grad is not None and bool(torch.isfinite(hp[n].grad).all()), n
        gp = hp[n].grad * 2.0 ** -10
        if ".attn2.to_q." in n or ".attn2.to_k." in n:
            assert float(gp.abs().max()) == 0.0, n
            continue
        e, ye = rel_l2(gp, of[n].grad), rel_l2(yf[n].grad.float().cpu(), of[n].grad)
        assert e < 2.2e-1 and e < max(3.5 * ye, 2e-2), (n, e, ye)
        got.append(gp.float().cpu().reshape(-1)); ref.append(of[n].grad.reshape(-1)); yst.append(yf[n].grad.float().cpu().reshape(-1))
    tot, ytot = rel_l2(torch.cat(got), torch.cat(ref)), rel_l2(torch.cat(yst), torch.cat(ref))
    print(f"  LoRA, fp16 elements: loss {loss:.6f} vs {loss_ref:.6f}; {len(got)} factor gradients rel-L2 {tot:.2e} (torch bf16 {ytot:.2e})")
    assert len(got) == 512 - 128 and tot < 3e-2 and tot < 1.5 * ytot
