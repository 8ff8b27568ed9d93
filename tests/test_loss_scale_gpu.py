"""Dynamic loss scaling on the GPU: ctrlv_grad_finish_scaled / ctrlv_adamw_step_scaled (csrc/optim.hip) and
`ctrlv_amd.optim.LossScaler` with `AdamW.step(scaler=...)`.

Everything is compared bit for bit: the scaled finish against ctrlv_grad_finish called with the host-computed multiplier, the
record's trajectory against the pure-Python restatement (tests/loss_scale_ref.py, itself checked against torch.amp.GradScaler
on the CPU), the scaled step against ctrlv_adamw_step_dev, a power-of-two scale against no scale at all."""
import ctypes
import math
import struct

import pytest
import torch

from tests import grad_clip_ref as G
from tests import loss_scale_ref as L
from tests import optim_ref as R
from tests.guarded import as_int, check_written_only_inside, guarded_flat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, B1, B2, EPS, WD = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(1e-2)
ONE_BITS = 0x3F800000


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def _record(scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, tracker=0, unscale=0.0):
    """ctrlv_loss_scale_state as int32[8] on the device."""
    words = struct.unpack("<8i", struct.pack("<ffiiffii", scale, unscale, tracker, growth_interval, growth_factor, backoff_factor, 0, 0))
    return torch.tensor(words, dtype=torch.int32, device=DEV)


def _f(t, i):
    return t[i].view(torch.float32)


def _sumsq(lib, g, partials=None, slot0=0):
    from ctrlv_amd import _lib
    n = g.numel()
    slots = lib.ctrlv_grad_sumsq_partials(n)
    if partials is None:
        partials = torch.full((slot0 + slots,), math.nan, dtype=torch.float64, device=DEV)
    _lib.check(lib.ctrlv_grad_sumsq(_ptr(g), n, _ptr(partials), partials.numel(), slot0, _stream()), "ctrlv_grad_sumsq", lib)
    return partials, slots


def _finish_scaled(lib, partials, slots, ls, state, grad_scale=1.0, max_norm=math.inf, slot0=0):
    from ctrlv_amd import _lib
    _lib.check(lib.ctrlv_grad_finish_scaled(ctypes.c_void_p(partials.data_ptr() + 8 * slot0), slots, grad_scale, max_norm, _ptr(ls),
                                            _ptr(state), _stream()), "ctrlv_grad_finish_scaled", lib)


def _step_scaled(lib, p, g, m, v, e, t, ls, state, ema_decay=0.0):
    from ctrlv_amd import _lib
    _lib.check(lib.ctrlv_adamw_step_scaled(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), p.numel(), LR, B1, B2, EPS, WD, 1.0 - B1 ** t,
                                           1.0 - B2 ** t, ema_decay, _ptr(ls), _ptr(state), _stream()), "ctrlv_adamw_step_scaled", lib)


# ------------------------------------------------------------------------------------------------ 1. the finish
@pytest.mark.parametrize("scale,grad_scale,max_norm", [(1000.0, 1.0, 1.0), (48000.0, R.f32(1.0 / 3.0), math.inf), (2.0 ** 16, 0.25, 1e-3)])
@pytest.mark.parametrize("n", G.SIZES)
def test_finish_scaled_writes_the_bits_of_finish_with_the_host_unscale(hip_lib, n, scale, grad_scale, max_norm):
    from ctrlv_amd import _lib
    g = (G.case(n, steps=1)[1][0] * 64.0).to(DEV)
    unscale = L.unscale(scale, grad_scale)
    partials, slots = _sumsq(hip_lib, g)
    ls, state, plain = _record(scale=scale, growth_interval=5), torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    _finish_scaled(hip_lib, partials, slots, ls, state, grad_scale, max_norm)
    _lib.check(hip_lib.ctrlv_grad_finish(_ptr(partials), slots, unscale, max_norm, _ptr(plain), _stream()), "ctrlv_grad_finish", hip_lib)
    torch.cuda.synchronize()
    assert state.tolist() == plain.tolist(), (state.tolist(), plain.tolist())
    assert int(state[2]) == 0 and math.isfinite(float(_f(state, 0)))
    assert (float(_f(state, 0)) > 0.0) == (n > 1)                               # (the case's only element at n = 1 is a zero)
    assert int(ls[1]) == _bits(unscale)                                          # the multiplier, as the host forms it
    assert int(ls[0]) == _bits(scale) and int(ls[2]) == 1 and ls[3:].tolist() == _record(scale=scale, growth_interval=5)[3:].tolist()
    if max_norm == 1e-3 and n > 1:
        assert float(_f(state, 1)) < 1.0                                        # the clip was active


POSITIONS = {4099: [0, 4098, 4095, 4096]}          # first, last (the n % 4 tail), the last of block 0, the first of block 1


@pytest.mark.parametrize("name", sorted(L.SCRIPTS))
def test_scripted_sequence_follows_the_restatement(hip_lib, name):
    """12 steps, an inf or a NaN injected at a chosen element where the script says so: scale, growth tracker, multiplier, skip and
    skipped_total equal the CPU restatement after EVERY step.  Nothing is read from the device before the end."""
    n = 4099
    script = L.SCRIPTS[name]
    rec = L.Record(**script["kw"])
    kw = script["kw"]
    ls = _record(scale=kw["init_scale"], growth_factor=kw["growth_factor"], backoff_factor=kw["backoff_factor"],
                 growth_interval=kw["growth_interval"])
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    grads = G.case(n, steps=3)[1]
    seen, want, bad_no = [], [], 0
    for k, found in enumerate(script["found"]):
        g = grads[k % 3].clone()
        if found:
            g[POSITIONS[n][bad_no % 4]] = (math.inf, math.nan, -math.inf)[bad_no % 3]
            bad_no += 1
        partials, slots = _sumsq(hip_lib, g.to(DEV))
        _finish_scaled(hip_lib, partials, slots, ls, state, grad_scale=0.5)
        seen.append((ls.clone(), state.clone()))
        skip = rec.step(found, grad_scale=0.5)
        want.append((_bits(rec.scale), _bits(rec.unscale), rec.growth_tracker, skip, rec.skipped_total))
    torch.cuda.synchronize()
    assert bad_no == sum(script["found"]) >= 1
    for k, ((l, s), w) in enumerate(zip(seen, want)):
        got = (int(l[0]), int(l[1]), int(l[2]), int(s[2]), int(s[3]))
        assert got == w, (name, k, got, w)
        assert math.isfinite(float(_f(s, 0))) == (w[3] == 0)
        assert l[3:].tolist() == ls[3:].tolist()                                 # interval, factors and reserved words are only read


@pytest.mark.parametrize("bad", [0.0, -4.0, math.inf, math.nan])
def test_an_unusable_scale_skips_and_is_left_alone(hip_lib, bad):
    n = 257
    p0, grads = G.case(n)
    g = grads[0].to(DEV)
    ls, state = _record(scale=bad, growth_interval=1, tracker=0), torch.zeros(4, dtype=torch.int32, device=DEV)
    before = ls.clone()
    partials, slots = _sumsq(hip_lib, g)
    _finish_scaled(hip_lib, partials, slots, ls, state)
    p, m, v = p0.to(DEV).clone(), torch.full((n,), 0.5, device=DEV), torch.full((n,), 0.25, device=DEV)
    _step_scaled(hip_lib, p, g, m, v, None, 1, ls, state)
    torch.cuda.synchronize()
    assert int(state[2]) == 1 and int(state[3]) == 1 and math.isnan(float(_f(state, 0)))
    assert math.isnan(float(_f(ls, 1))) and ls[[0, 2, 3, 4, 5, 6, 7]].tolist() == before[[0, 2, 3, 4, 5, 6, 7]].tolist()
    assert torch.equal(p, p0.to(DEV)) and float(m.min()) == float(m.max()) == 0.5 and float(v.min()) == float(v.max()) == 0.25


# ------------------------------------------------------------------------------------------------ 2. the step
@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("n", G.SIZES)
def test_step_scaled_equals_step_dev_when_unscale_is_grad_scale(hip_lib, n, with_ema):
    from ctrlv_amd import _lib
    p0, grads = G.case(n)
    gs, coef = R.f32(1.0 / 1000.0), R.f32(0.75)
    state = torch.tensor([0, _bits(coef), 0, 0], dtype=torch.int32, device=DEV)
    ls = _record(scale=1000.0, unscale=gs, tracker=3)
    ls0 = ls.clone()
    grads = [g.to(DEV) for g in grads]
    out = []
    for scaled in (False, True):
        p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        e = (p0 * 1.5).to(DEV) if with_ema else None
        for t, g in enumerate(grads, 1):
            if scaled:
                _step_scaled(hip_lib, p, g, m, v, e, t, ls, state, R.f32(0.75))
            else:
                _lib.check(hip_lib.ctrlv_adamw_step_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), n, LR, B1, B2, EPS, WD, 1.0 - B1 ** t,
                                                        1.0 - B2 ** t, gs, R.f32(0.75), _ptr(state), _stream()), "ctrlv_adamw_step_dev", hip_lib)
        torch.cuda.synchronize()
        out.append((p, m, v) + ((e,) if with_ema else ()))
    for a, b, name in zip(out[0], out[1], ("p", "m", "v", "shadow")):
        assert torch.equal(a, b), name
    assert not torch.equal(out[1][0], p0.to(DEV))
    assert torch.equal(ls, ls0) and state.tolist() == [0, _bits(coef), 0, 0]     # both records are only read
    assert all(torch.equal(g, h.to(DEV)) for g, h in zip(grads, G.case(n)[1]))   # g is never written


@pytest.mark.parametrize("bad", [math.inf, math.nan])
@pytest.mark.parametrize("n,pos", [(4099, 0), (4099, 4098), (4099, 4095), (4099, 4096), (5, 4), (2 ** 20 + 1, 2 ** 20)])
def test_skipped_step(hip_lib, n, pos, bad):
    """p, m and v keep their bits, the shadow moves as ctrlv_ema_step moves it, the scale is multiplied by the backoff factor."""
    from ctrlv_amd import _lib
    p0, grads = G.case(n)
    g = grads[0].clone()
    g[pos] = bad
    g = g.to(DEV)
    g0 = g.clone()
    p, m, v = p0.to(DEV).clone(), grads[1].to(DEV) * 0.1, grads[2].to(DEV).abs()
    e = (p0 * 1.5).to(DEV)
    kept = [t.clone() for t in (p, m, v)]
    shadow = e.clone()
    ls, state = _record(scale=3000.0, backoff_factor=0.25, growth_interval=3, tracker=2), torch.zeros(4, dtype=torch.int32, device=DEV)
    partials, slots = _sumsq(hip_lib, g)
    _finish_scaled(hip_lib, partials, slots, ls, state, max_norm=1.0)
    _step_scaled(hip_lib, p, g, m, v, e, 2, ls, state, R.f32(0.9))
    _lib.check(hip_lib.ctrlv_ema_step(_ptr(shadow), _ptr(kept[0]), n, R.f32(0.9), _stream()), "ctrlv_ema_step", hip_lib)
    torch.cuda.synchronize()
    for a, b, name in zip((p, m, v, e), kept + [shadow], ("p", "m", "v", "shadow")):
        assert torch.equal(as_int(a), as_int(b)), name
    assert not torch.equal(e, (p0 * 1.5).to(DEV))
    assert int(state[2]) == 1 and int(state[3]) == 1
    assert float(_f(ls, 0)) == 750.0 and int(ls[2]) == 0 and int(ls[1]) == _bits(L.unscale(3000.0))
    assert torch.equal(as_int(g), as_int(g0))


@pytest.mark.parametrize("n", G.SIZES)
def test_guard_bands(hip_lib, n):
    """The three stages write the record (32 bytes), the grad record (16), the run's partials and p, m, v, shadow -- and nothing
    around any of them; g keeps its bits."""
    slots, slot0 = (n + G.BLOCK - 1) // G.BLOCK, 2
    p0, grads = G.case(n)
    g_buf, g = guarded_flat(n, torch.float32, DEV, fill="poison")
    g.copy_((grads[0] * 1000.0).to(DEV))
    bufs = {}
    for name, init in (("p", p0), ("m", grads[1] * 0.1), ("v", grads[2].abs()), ("shadow", p0 * 1.5)):
        bufs[name] = guarded_flat(n, torch.float32, DEV, fill="sentinel")
        bufs[name][1].copy_(init.to(DEV))
    p_buf, p32 = guarded_flat(2 * (slot0 + slots + 3), torch.float32, DEV, fill="sentinel")    # fp64 slots as pairs of words
    s_buf, s32 = guarded_flat(4, torch.float32, DEV, fill="sentinel")
    l_buf, l32 = guarded_flat(8, torch.float32, DEV, fill="sentinel")
    partials, state, ls = p32.view(torch.float64), s32.view(torch.int32), l32.view(torch.int32)
    assert all(t.data_ptr() % 16 == 0 for t in (g, state, ls, *(b[1] for b in bufs.values()))) and partials.data_ptr() % 8 == 0
    state[3] = 0
    ls.copy_(_record(scale=1000.0, growth_interval=2, tracker=1, growth_factor=3.0))
    before = {"g": g_buf.clone(), "partials": p_buf.clone(), "state": s_buf.clone(), "ls": l_buf.clone(),
              **{k: b[0].clone() for k, b in bufs.items()}}
    _sumsq(hip_lib, g, partials=partials, slot0=slot0)
    _finish_scaled(hip_lib, partials, slots, ls, state, max_norm=1.0, slot0=slot0)
    _step_scaled(hip_lib, bufs["p"][1], g, bufs["m"][1], bufs["v"][1], bufs["shadow"][1], 1, ls, state, R.f32(0.5))
    torch.cuda.synchronize()
    assert torch.equal(as_int(g_buf), as_int(before["g"]))
    check_written_only_inside(before["state"], s_buf, s32.view(1, 4), what="state")
    check_written_only_inside(before["ls"], l_buf, l32.view(1, 8), what="loss-scale record")
    for k, (buf, view) in bufs.items():
        check_written_only_inside(before[k], buf, view.view(1, n), what=k)
        assert not torch.equal(as_int(buf), as_int(before[k])), k                # the step was applied
    changed = as_int(p_buf) != as_int(before["partials"])
    inside = torch.zeros_like(changed)
    inside[1, 64 + 2 * slot0:64 + 2 * (slot0 + slots)] = True
    assert not bool((changed & ~inside).any())
    assert bool(torch.isfinite(partials[slot0:slot0 + slots]).all())
    assert int(state[2]) == 0 and float(_f(ls, 0)) == 3000.0 and int(ls[2]) == 0 and int(ls[1]) == _bits(L.unscale(1000.0))


# ------------------------------------------------------------------------------------------------ 3. the classes
@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
@pytest.mark.parametrize("n", [5, 4099, 2 * G.BLOCK - 1])
def test_power_of_two_scale_is_exact(hip_lib, n, max_grad_norm):
    """Gradients times 2^10 under LossScaler(init_scale=2^10) give the p, m, v of the unscaled step: a power of two commutes with
    every rounding, the norm's included (fp64 squares scale by 2^20 exactly)."""
    from ctrlv_amd.optim import AdamW, LossScaler
    p0, grads = G.case(n)
    kw = dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    pa, pb = torch.nn.Parameter(p0.to(DEV).clone()), torch.nn.Parameter(p0.to(DEV).clone())
    oa, ob = AdamW([pa], **kw), AdamW([pb], **kw)
    scaler = LossScaler(init_scale=2.0 ** 10, growth_interval=10 ** 9)
    for g in grads:
        pa.grad.copy_(g.to(DEV))
        oa.step(max_grad_norm=max_grad_norm)
        pb.grad.copy_(g.to(DEV) * 1024.0)
        scaler.step(ob, max_grad_norm=max_grad_norm)
        scaler.update()
        assert torch.equal(pb.grad, g.to(DEV) * 1024.0)                           # .grad stays scaled
    torch.cuda.synchronize()
    for name, a, b in (("p", pa.detach(), pb.detach()), ("exp_avg", oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]),
                       ("exp_avg_sq", oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert not torch.equal(pa.detach(), p0.to(DEV))
    st = ob.grad_state()
    assert int(st["skip"]) == 0 and int(st["skipped_total"]) == 0 and scaler.get_scale() == 1024.0
    assert int(scaler.growth_tracker_tensor()) == 3 and float(ob.state[pb]["step"]) == 3.0
    if max_grad_norm is not None:
        assert int(st["norm"].view(torch.int32)) == int(oa.grad_state()["norm"].view(torch.int32))
        assert int(st["coef"].view(torch.int32)) == int(oa.grad_state()["coef"].view(torch.int32))
        if n >= 5:
            assert float(st["coef"]) < 1.0
    else:
        assert float(st["coef"]) == 1.0


SHAPES = [(5,), (4099,), (320, 3, 3), (2 * G.BLOCK + 3,)]        # two groups; a frozen parameter splits the first into two runs


def _module(seed=1):
    gen = torch.Generator().manual_seed(seed)
    m = torch.nn.Module()
    for i, shape in enumerate(SHAPES):
        m.register_parameter(f"w{i}", torch.nn.Parameter(torch.randn(*shape, generator=gen) * 0.1))
    m.register_parameter("frozen", torch.nn.Parameter(torch.randn(9, generator=gen), requires_grad=False))
    return m.to(DEV)


def _groups(m):
    return [{"params": [m.w0, m.frozen, m.w1], "lr": R.f32(1e-3), "weight_decay": R.f32(1e-2)},
            {"params": [m.w2, m.w3], "lr": R.f32(3e-4), "weight_decay": 0.0}]


def test_two_groups_skip_growth_and_state_dict_round_trip(hip_lib):
    """Step 1 finite, 2 with a NaN (skip, backoff), 3 and 4 finite (growth at interval 2); the state dict then moves into a FRESH
    scaler, and step 5 under it is bit-identical to step 5 under the original."""
    from ctrlv_amd.optim import AdamW, EMAModel, LossScaler
    gen = torch.Generator().manual_seed(7)
    steps = [[torch.randn(*s, generator=gen) * (10.0 ** (i - 1)) for i, s in enumerate(SHAPES)] for _ in range(5)]
    steps[1][3][G.BLOCK] = math.nan
    kw = dict(init_scale=3000.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=2)
    out = []
    for fresh in (False, True):
        m = _module()
        ema = EMAModel(m.parameters())
        opt = AdamW(_groups(m), betas=(B1, B2), eps=EPS)
        scaler = LossScaler(**kw)
        scaler.scale(torch.zeros((), device=DEV))
        trail = []
        for k, grads in enumerate(steps):
            if k == 4 and fresh:
                sd = scaler.state_dict()
                scaler = LossScaler()
                scaler.load_state_dict(sd)
                assert scaler.state_dict() == sd == dict(scale=2250.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=2,
                                                         _growth_tracker=0)
                scaler.scale(torch.zeros((), device=DEV))
            for i, g in enumerate(grads):
                getattr(m, f"w{i}").grad.copy_(g.to(DEV) * scaler.scale_tensor())          # a scaled backward's gradients
            before = [p.detach().clone() for p in m.parameters()]
            scaler.step(opt, ema=ema, max_grad_norm=1.0, grad_scale=0.5)
            scaler.update()
            trail.append((scaler.scale_tensor().clone(), scaler.growth_tracker_tensor().clone(), opt.grad_state()["skip"].clone(),
                          [torch.equal(a, p.detach()) for a, p in zip(before, m.parameters())]))
            opt.zero_grad()
        torch.cuda.synchronize()
        assert [(float(s), int(t), int(k)) for s, t, k, _ in trail] == [(3000.0, 1, 0), (750.0, 0, 1), (750.0, 1, 0), (2250.0, 0, 0),
                                                                        (2250.0, 1, 0)]
        assert all(trail[1][3]) and not any(trail[0][3][:4]) and not any(trail[4][3][:4])         # the skip kept every bit
        assert int(opt.grad_state()["skipped_total"]) == 1 and float(opt.state[m.w0]["step"]) == 5.0   # ATTEMPTED steps
        out.append([p.detach().clone() for p in m.parameters()] + [s.clone() for s in ema.shadow_params]
                   + [t.clone() for gi in range(2) for t in opt.flat_buffers(gi)[2:4]] + [scaler._record.clone()])
    assert len(out[0]) == len(out[1]) and all(torch.equal(a, b) for a, b in zip(out[0], out[1]))


def test_disabled_scaler_is_the_plain_step(hip_lib):
    from ctrlv_amd.optim import AdamW, LossScaler
    p0, grads = G.case(257)
    kw = dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    pa, pb = torch.nn.Parameter(p0.to(DEV).clone()), torch.nn.Parameter(p0.to(DEV).clone())
    oa, ob = AdamW([pa], **kw), AdamW([pb], **kw)
    off = LossScaler(enabled=False)
    pa.grad.copy_(grads[0].to(DEV))
    pb.grad.copy_(grads[0].to(DEV))
    oa.step()
    off.step(ob)
    ob.step(scaler=off)
    pa.grad.copy_(grads[0].to(DEV))
    oa.step()
    torch.cuda.synchronize()
    assert torch.equal(pa.detach(), pb.detach()) and off._record is None
    with pytest.raises(RuntimeError, match="grad_state"):
        ob.grad_state()
