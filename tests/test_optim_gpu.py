"""ctrlv_adamw_step / ctrlv_ema_step (csrc/optim.hip) and ctrlv_amd.optim.AdamW / EMAModel on the GPU.

Tolerance rule of every AdamW parity test: both sides -- the HIP result and torch.optim.AdamW(foreach=False, fused=False) in
fp32 on the device -- are measured against the fp64 restatement (tests/optim_ref.py) on the same inputs; the HIP result's largest
error in ulps of p (optim_ref.ulps: the fp32 spacing at the larger of |p| before and after the steps) may be at most twice
torch's and never needs to be below 1 ulp.  Each test prints its (hip, torch) pair.  Hyper-parameters are fp32-representable
(optim_ref.f32): the C entry points take floats and the three sides must see the same numbers.

EMA bound (left to this file by the issue, derived here): one update e - (1 - d) * (e - p) in fp32 costs at most 2 ulps at the
magnitude max(|e|, |p|): 1/2 for the subtraction (times 1 - d <= 1), 1/2 for the final rounding, and at most 1 for 1 - d reaching
the kernel through an fp32 `decay` (an absolute error of 2^-25 on a factor that multiplies |e - p| <= 2 max(|e|, |p|)).  k updates
with exact fp64 inputs at every step: 2 k ulps."""
import ctypes
import math

import pytest
import torch

from tests import optim_ref as R
from tests.guarded import as_int, check_written_only_inside, guarded_flat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, B1, B2, EPS = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8)
SIZES = [1, 3, 4, 5, 255, 256, 257, 4099, 2 ** 20 + 1]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hip_adamw(lib, p, g, m, v, ema, n, t, wd, lr=LR, ema_decay=0.0):
    from ctrlv_amd import _lib
    _lib.check(lib.ctrlv_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), n, lr, B1, B2, EPS, wd, 1.0 - B1 ** t, 1.0 - B2 ** t,
                                    1.0, ema_decay, _stream()), "ctrlv_adamw_step", lib)


def _hip_ema(lib, ema, p, n, decay):
    from ctrlv_amd import _lib
    _lib.check(lib.ctrlv_ema_step(_ptr(ema), _ptr(p), n, decay, _stream()), "ctrlv_ema_step", lib)


def _case(n, steps=3, seed=0):
    """p0 and `steps` gradients that mix zeros, +-1e4, 1e-20 and ordinary values; the kind an element sees changes with the step."""
    gen = torch.Generator().manual_seed(seed + n)
    p0 = (torch.randn(n, generator=gen) * 0.1).float()
    idx = torch.arange(n)
    grads = []
    for s in range(steps):
        g = torch.randn(n, generator=gen).float()
        kind = (idx + s) % 5
        g[kind == 0] = 0.0
        g[kind == 1] = torch.where(g[kind == 1] < 0, -1e4, 1e4).float()
        g[kind == 2] = 1e-20
        grads.append(g)
    return p0, grads


def _fp64(p0, grads, wd, lr=LR):
    p, m, v = p0.double(), torch.zeros_like(p0, dtype=torch.float64), torch.zeros_like(p0, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        p, m, v = R.adamw_step(p, g.double(), m, v, t, lr, B1, B2, EPS, wd)
    return p, m, v


def _torch_adamw(p0, grads, wd, lr=LR):
    p = torch.nn.Parameter(p0.to(DEV).clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False, fused=False)
    for g in grads:
        p.grad = g.to(DEV).clone()
        opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


# ------------------------------------------------------------------------------------------------ 1. kernel against fp64
@pytest.mark.parametrize("wd", [0.0, R.f32(1e-2)])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_fp64(hip_lib, n, wd):
    p0, grads = _case(n)
    ref_p, ref_m, ref_v = _fp64(p0, grads, wd)
    tp, tm, tv = _torch_adamw(p0, grads, wd)
    p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for t, g in enumerate(grads, 1):
        _hip_adamw(hip_lib, p, g.to(DEV), m, v, None, n, t, wd)
    torch.cuda.synchronize()
    e_hip, e_torch = R.ulps(p, ref_p, [p0]), R.ulps(tp, ref_p, [p0])
    print(f"  n={n} wd={wd}: max error in ulps of p after 3 steps: hip {e_hip:.3f}  torch {e_torch:.3f}   "
          f"(elements whose bits differ from torch's: p {int((p != tp).sum())}, m {int((m != tm).sum())}, v {int((v != tv).sum())})")
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())
    assert R.within_rule(e_hip, e_torch), (e_hip, e_torch)
    # the moments, at the magnitude of their operands (m is a convex combination of the g, v of the g * g; 1e-20 ** 2 lives among
    # the subnormals, where the spacing is constant).  Per step m rounds twice (1 ulp) and v three times (1.5), and 1 - beta reaches
    # the kernel as an fp32 number (1 more): 2 and 2.5 ulps per step, 8 covers three steps of either.
    gmax = torch.stack([g.abs() for g in grads]).max(0).values.double()
    e_m, e_v = R.ulps(m, ref_m, [gmax]), R.ulps(v, ref_v, [gmax * gmax])
    print(f"    moments: exp_avg {e_m:.3f}  exp_avg_sq {e_v:.3f} ulps (bound 8); torch {R.ulps(tm, ref_m, [gmax]):.3f} {R.ulps(tv, ref_v, [gmax * gmax]):.3f}")
    assert e_m <= 8.0 and e_v <= 8.0, (e_m, e_v)


# ------------------------------------------------------------------------------------------------ 2. guard bands
@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_guard_bands(hip_lib, n, with_ema):
    """No byte outside [0, n) of any of the five buffers changes; the gradient buffer does not change at all."""
    p0, grads = _case(n, steps=1)
    bufs = {k: guarded_flat(n, torch.float32, DEV, fill="sentinel") for k in ("p", "g", "m", "v", "ema")}
    bufs["p"][1].copy_(p0.to(DEV))
    bufs["g"][1].copy_(grads[0].to(DEV))
    bufs["m"][1].copy_((p0 * 0.5).to(DEV))
    bufs["v"][1].copy_((p0 * p0).to(DEV))
    bufs["ema"][1].copy_((p0 * 1.5).to(DEV))
    for k in bufs:
        assert bufs[k][1].data_ptr() % 16 == 0
    before = {k: b.clone() for k, (b, _) in bufs.items()}
    _hip_adamw(hip_lib, bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1], bufs["ema"][1] if with_ema else None, n, 2, R.f32(1e-2),
               ema_decay=R.f32(0.75))
    if with_ema:
        _hip_ema(hip_lib, bufs["ema"][1], bufs["p"][1], n, R.f32(0.5))
    torch.cuda.synchronize()
    for k in ("p", "m", "v") + (("ema",) if with_ema else ()):
        check_written_only_inside(before[k], bufs[k][0], bufs[k][1].view(1, n), what=k)
        assert not torch.equal(bufs[k][1], before[k][1, 64:64 + n]), k
    for k in ("g",) + (() if with_ema else ("ema",)):
        assert torch.equal(as_int(bufs[k][0]), as_int(before[k])), k


# ------------------------------------------------------------------------------------------------ 3. determinism and fusion
@pytest.mark.parametrize("n", [5, 4099, 2 ** 20 + 1])
def test_determinism_and_fusion(hip_lib, n):
    p0, grads = _case(n)
    decays = [0.0, R.f32(2 / 11), R.f32(0.9999)]

    def run(fused):
        p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        e = p.clone()
        for t, (g, d) in enumerate(zip(grads, decays), 1):
            if fused:
                _hip_adamw(hip_lib, p, g.to(DEV), m, v, e, n, t, R.f32(1e-2), ema_decay=d)
            else:
                _hip_adamw(hip_lib, p, g.to(DEV), m, v, None, n, t, R.f32(1e-2))
                _hip_ema(hip_lib, e, p, n, d)
        torch.cuda.synchronize()
        return p, m, v, e

    a, b, c = run(True), run(True), run(False)
    for x, y, z, name in zip(a, b, c, ("p", "m", "v", "ema")):
        assert torch.equal(x, y), f"{name}: two runs differ"
        assert torch.equal(x, z), f"{name}: fused differs from AdamW followed by ctrlv_ema_step"
    assert not torch.equal(a[3], a[0])                      # the shadow lags the parameter


# ------------------------------------------------------------------------------------------------ 4. the class against torch's
SHAPES = [(1,), (3,), (320, 3, 3), (7, 5)]


def _module(seed=1, frozen=True):
    gen = torch.Generator().manual_seed(seed)
    m = torch.nn.Module()
    for i, shape in enumerate(SHAPES):
        m.register_parameter(f"w{i}", torch.nn.Parameter(torch.randn(*shape, generator=gen) * 0.1))
    if frozen:
        m.register_parameter("frozen", torch.nn.Parameter(torch.randn(9, generator=gen), requires_grad=False))
    return m.to(DEV)


def _groups(m):
    ps = dict(m.named_parameters())
    first = [ps["w0"], ps["w1"]] + ([ps["frozen"]] if "frozen" in ps else [])
    return [{"params": first, "lr": R.f32(1e-3), "weight_decay": R.f32(1e-2)},
            {"params": [ps["w2"], ps["w3"]], "lr": R.f32(3e-4), "weight_decay": 0.0}]


def _grads(steps, seed=2):
    gen = torch.Generator().manual_seed(seed)
    return [[torch.randn(*s, generator=gen) * (10.0 ** (i - 2)) for i, s in enumerate(SHAPES)] for _ in range(steps)]


def _sched(opt):
    return torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5 ** s)       # (powers of two: lr stays fp32-representable)


def _drive(m, opt, grads, sched=None, fresh=False):
    """One optimiser step per entry of `grads`; fresh: hand the gradient over as a NEW tensor (what a caller or
    GradientBuckets._write_back does) instead of writing it into the existing .grad."""
    ws = [getattr(m, f"w{i}") for i in range(len(SHAPES))]
    for k, gs in enumerate(grads):
        for i, (w, g) in enumerate(zip(ws, gs)):
            if w.grad is None or fresh or (i + k) % 2:
                w.grad = g.to(DEV).clone()
            else:
                w.grad.copy_(g.to(DEV))
        opt.step()
        opt.zero_grad(set_to_none=True)
        if sched is not None:
            sched.step()


def _fp64_module(m0, grads, lrs, wds, t0=0, state=None, halve=True):
    """fp64 restatement for the four trained tensors; lr halves every step when `halve` (the LambdaLR above)."""
    out = []
    for i in range(len(SHAPES)):
        p = m0[i].double().cpu()
        mm, vv = (torch.zeros_like(p), torch.zeros_like(p)) if state is None else state[i]
        gi = 0 if i < 2 else 1
        for k, gs in enumerate(grads):
            lr = lrs[gi] * (0.5 ** (t0 + k) if halve else 1.0)
            p, mm, vv = R.adamw_step(p, gs[i].double(), mm, vv, t0 + k + 1, lr, B1, B2, EPS, wds[gi])
        out.append(p)
    return out


def _errors(m, refs, p0s):
    return max(R.ulps(getattr(m, f"w{i}").detach(), refs[i], [p0s[i]]) for i in range(len(SHAPES)))


def test_class_against_torch(hip_lib):
    from ctrlv_amd.optim import AdamW
    grads = _grads(5)
    mt, mh = _module(), _module()
    p0s = [getattr(mt, f"w{i}").detach().clone() for i in range(4)]
    frozen0 = mh.frozen.detach().clone()
    kw = dict(betas=(B1, B2), eps=EPS)
    ot = torch.optim.AdamW(_groups(mt), foreach=False, fused=False, **kw)
    oh = AdamW(_groups(mh), **kw)
    _drive(mt, ot, grads, _sched(ot))
    _drive(mh, oh, grads, _sched(oh))
    torch.cuda.synchronize()
    assert oh.param_groups[0]["lr"] == ot.param_groups[0]["lr"] == R.f32(1e-3) / 32          # the LambdaLR drove both
    refs = _fp64_module(p0s, grads, [R.f32(1e-3), R.f32(3e-4)], [R.f32(1e-2), 0.0])
    e_hip, e_torch = _errors(mh, refs, p0s), _errors(mt, refs, p0s)
    print(f"  class, 5 steps, 2 groups, LambdaLR: max error in ulps of p: hip {e_hip:.3f}  torch {e_torch:.3f}")
    assert R.within_rule(e_hip, e_torch), (e_hip, e_torch)
    assert torch.equal(mh.frozen.detach(), frozen0) and mh.frozen.grad is None               # a frozen parameter keeps its bits
    assert torch.equal(mt.frozen.detach(), frozen0)
    assert all(not torch.equal(getattr(mh, f"w{i}").detach(), p0s[i]) for i in range(4))
    pbuf, offsets = oh.flat_buffers(0)[0], oh.flat_buffers(0)[4]
    pad = torch.ones_like(pbuf, dtype=torch.bool)
    for p, off in zip(oh.param_groups[0]["params"], offsets):
        pad[off:off + p.numel()] = False
    assert float(pbuf[pad].abs().sum()) == 0.0                                               # padding stays zero
    assert sorted(oh.state_dict()["state"]) == sorted(ot.state_dict()["state"])              # no state for the frozen one


# ------------------------------------------------------------------------------------------------ 5. versions and caches
def test_version_counters_and_caches(hip_lib):
    from ctrlv_amd import frozen
    from ctrlv_amd.optim import AdamW
    m = _module()
    opt = AdamW(_groups(m), betas=(B1, B2), eps=EPS)
    built = []

    def build():
        built.append(1)
        return len(built)

    trained = [getattr(m, f"w{i}") for i in range(4)]
    assert frozen.frozen_module(m, "probe", build) == 1 and frozen.frozen_module(m, "probe", build) == 1
    for k, gs in enumerate(_grads(3)):
        versions = [p._version for p in trained]
        fv = m.frozen._version
        _drive(m, opt, [gs])
        assert all(p._version > v for p, v in zip(trained, versions)), k
        assert m.frozen._version == fv
        assert frozen.frozen_module(m, "probe", build) == k + 2                              # rebuilt after every step
        assert frozen.frozen_module(m, "probe", build) == k + 2
    m.to(torch.float64)
    for w, g in zip(trained, _grads(1)[0]):
        w.grad = g.to(DEV, torch.float64)
    with pytest.raises(ValueError, match="parameter 0 of group 0"):
        opt.step()


# ------------------------------------------------------------------------------------------------ 6. state-dict interop
@pytest.mark.parametrize("direction", ["torch_to_hip", "hip_to_torch"])
def test_state_dict_interop(hip_lib, direction):
    from ctrlv_amd.optim import AdamW
    grads = _grads(4, seed=5)
    kw = dict(betas=(B1, B2), eps=EPS)
    lrs, wds = [R.f32(1e-3), R.f32(3e-4)], [R.f32(1e-2), 0.0]
    make = {"torch": lambda mod: torch.optim.AdamW(_groups(mod), foreach=False, fused=False, **kw), "hip": lambda mod: AdamW(_groups(mod), **kw)}
    first, second = ("torch", "hip") if direction == "torch_to_hip" else ("hip", "torch")
    # uninterrupted torch run: the reference side of the rule
    mt = _module(frozen=False)
    p0s = [getattr(mt, f"w{i}").detach().clone() for i in range(4)]
    _drive(mt, make["torch"](mt), grads, fresh=True)
    # two steps in `first`, state dict into `second` (a new module with the same values), two more steps
    ma = _module(frozen=False)
    oa = make[first](ma)
    _drive(ma, oa, grads[:2], fresh=True)
    mb = _module(frozen=False)
    with torch.no_grad():
        for i in range(4):
            getattr(mb, f"w{i}").copy_(getattr(ma, f"w{i}"))
    ob = make[second](mb)
    ob.load_state_dict(oa.state_dict())
    _drive(mb, ob, grads[2:], fresh=True)
    torch.cuda.synchronize()
    assert all(float(ob.state[getattr(mb, f"w{i}")]["step"]) == 4.0 for i in range(4))
    refs = _fp64_module(p0s, grads, lrs, wds, halve=False)
    e_hip, e_torch = _errors(mb, refs, p0s), _errors(mt, refs, p0s)
    print(f"  {direction}: 2 + 2 steps against 4 uninterrupted torch steps: max error in ulps of p: resumed {e_hip:.3f}  torch {e_torch:.3f}")
    assert R.within_rule(e_hip, e_torch), (e_hip, e_torch)


# ------------------------------------------------------------------------------------------------ 7. EMAModel
@pytest.mark.parametrize("path", ["flat", "foreach"])
def test_ema_against_fp64(hip_lib, path):
    from ctrlv_amd.optim import AdamW, EMAModel
    m = _module()
    params = list(m.parameters())
    ema = EMAModel(m.parameters())                          # built BEFORE the optimiser, as the reference does
    if path == "flat":
        opt = AdamW(_groups(m), betas=(B1, B2), eps=EPS)
    ref = [p.detach().double().cpu() for p in params]
    scale = [r.abs() for r in ref]
    gen = torch.Generator().manual_seed(11)
    for step in range(1, 6):
        with torch.no_grad():
            for p in params:
                if p.requires_grad:
                    p.add_((torch.randn(p.shape, generator=gen) * 0.05).to(DEV))
        ema.step(m.parameters())
        d = R.ema_decay(step)
        assert ema.cur_decay_value == pytest.approx(d, rel=1e-15) and ema.optimization_step == step
        ref = [R.ema_step(r, p.detach().double().cpu(), d) if p.requires_grad else p.detach().double().cpu() for r, p in zip(ref, params)]
        scale = [torch.maximum(s, torch.maximum(r.abs(), p.detach().double().cpu().abs())) for s, r, p in zip(scale, ref, params)]
    torch.cuda.synchronize()
    if path == "flat":
        shadow = ema._shadow_flat(opt, 0)
        assert shadow is not None and ema.shadow_params[0].data_ptr() == shadow.data_ptr()              # the flat mirror is in use
        assert ema.shadow_params[3].data_ptr() == ema._shadow_flat(opt, 1).data_ptr() + 4 * opt.flat_buffers(1)[4][1]
    else:
        assert not ema._flats
    errs = [R.ulps(s, r, [sc]) for s, r, sc in zip(ema.shadow_params, ref, scale)]
    print(f"  EMA, 5 steps, {path}: max error in ulps {max(errs):.3f} (bound 10)")
    assert max(errs) <= 10.0, errs
    assert torch.equal(ema.shadow_params[4], m.frozen.detach())
    # store / copy_to / restore give the parameters back bit for bit
    before = [p.detach().clone() for p in params]
    versions = [p._version for p in params]
    ema.store(m.parameters())
    ema.copy_to(m.parameters())
    assert all(torch.equal(p.detach(), s) for p, s in zip(params, ema.shadow_params))
    assert all(p._version > v for p, v in zip(params, versions))
    ema.restore(m.parameters())
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    if path == "flat":                                      # the parameters are still at home: the next step runs
        _drive(m, opt, _grads(1))


def test_fused_ema_in_the_class_equals_the_two_calls(hip_lib):
    from ctrlv_amd.optim import AdamW, EMAModel
    out = []
    for fused in (False, True):
        m = _module()
        ema = EMAModel(m.parameters())
        opt = AdamW(_groups(m), betas=(B1, B2), eps=EPS)
        if fused:
            opt.attach_ema(ema)
        for gs in _grads(4):
            _drive(m, opt, [gs])
            if not fused:
                ema.step(m.parameters())
        torch.cuda.synchronize()
        assert ema.optimization_step == 4
        out.append(([p.detach().clone() for p in m.parameters()], [s.clone() for s in ema.shadow_params]))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert torch.equal(a, b)
    assert not torch.equal(out[1][1][2], out[1][0][2])


def test_ema_save_and_load_pretrained_on_the_tiny_unet(hip_lib, tmp_path):
    import ctrlv_ref as Ref
    from ctrlv_amd.models import UNetSpatioTemporalConditionModel
    from ctrlv_amd.optim import EMAModel
    torch.manual_seed(3)
    unet = UNetSpatioTemporalConditionModel(**dict(Ref.TINY_CONFIG)).to(DEV)
    ema = EMAModel(unet.parameters(), model_cls=UNetSpatioTemporalConditionModel, model_config=unet.config, decay=R.f32(0.999),
                   use_ema_warmup=True, power=0.75)
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for s in ema.shadow_params:                         # shadows that differ from the model's weights
            s.add_((torch.randn(s.shape, generator=gen) * 0.01).to(DEV))
    ema.optimization_step = 7
    ema.save_pretrained(str(tmp_path / "unet_ema"))
    back = EMAModel.from_pretrained(str(tmp_path / "unet_ema"), UNetSpatioTemporalConditionModel)
    assert back.optimization_step == 7 and back.decay == R.f32(0.999) and back.use_ema_warmup is True and back.power == 0.75
    assert len(back.shadow_params) == len(ema.shadow_params)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(back.shadow_params, ema.shadow_params))
    loaded = UNetSpatioTemporalConditionModel.from_pretrained(str(tmp_path / "unet_ema"))      # a plain model directory as well
    assert all(torch.equal(a.cpu(), b.detach().cpu()) for a, b in zip(ema.shadow_params, loaded.parameters()))
    # the reference's resume: load_state_dict(load_model.state_dict()), then .to(device)
    ema2 = EMAModel(unet.parameters(), model_cls=UNetSpatioTemporalConditionModel, model_config=unet.config)
    ema2.load_state_dict(back.state_dict())
    ema2.to(DEV)
    assert ema2.optimization_step == 7 and all(torch.equal(a, b) for a, b in zip(ema2.shadow_params, ema.shadow_params))


# ------------------------------------------------------------------------------------------------ 8. the training steps
def _step_parity(tag, make, run, trainable, ema_leg=False):
    """make() -> a fresh model set with identical weights; run(models, optimizer) -> loss.  One step without an optimiser gives
    the gradients (bit-reproducible); then three steps with torch's optimiser and three with ours."""
    from ctrlv_amd.optim import AdamW, EMAModel
    from ctrlv_amd.training import GradientBuckets
    kw = dict(lr=R.f32(1e-3), betas=(B1, B2), eps=EPS, weight_decay=R.f32(1e-2))
    a = make()
    pa = trainable(a)
    p0 = [p.detach().clone() for p in pa]
    run(a, None, None)
    g = [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu() for p in pa]
    refs = [R.adamw_step(p.double().cpu(), gg, torch.zeros_like(gg), torch.zeros_like(gg), 1, kw["lr"], B1, B2, EPS, kw["weight_decay"])[0]
            for p, gg in zip(p0, g)]
    del a, pa
    results = {}
    for side in ("torch", "hip"):
        mods = make()
        ps = trainable(mods)
        assert all(torch.equal(p.detach(), q) for p, q in zip(ps, p0))
        if side == "torch":
            opt = torch.optim.AdamW(ps, foreach=False, fused=False, **kw)
        else:
            opt = AdamW(ps, **kw)
        ema = None
        if ema_leg:
            ema = EMAModel(ps)
            ema_ref = [p.double().cpu() for p in p0]
            ema_scale = [e.abs() for e in ema_ref]
            if side == "hip":
                opt.attach_ema(ema)                         # optimizer.step(ema=...) inside the step; no ema.step line
        buckets = GradientBuckets(ps)                       # single process: inactive; the copy-in rule is what is exercised
        losses = []
        for k in range(3):
            losses.append(float(run(mods, opt, buckets)))
            if ema_leg and side == "torch":
                ema.step(ps)
            if ema_leg:
                ema_ref = [R.ema_step(e, p.detach().double().cpu(), R.ema_decay(k + 1)) for e, p in zip(ema_ref, ps)]
                ema_scale = [torch.maximum(s, torch.maximum(e.abs(), p.detach().double().cpu().abs())) for s, e, p in zip(ema_scale, ema_ref, ps)]
            if k == 0:
                torch.cuda.synchronize()
                results[side] = max(R.ulps(p.detach(), r, [q]) for p, r, q in zip(ps, refs, p0))
        assert all(math.isfinite(v) for v in losses), (side, losses)
        if ema_leg:
            err = max(R.ulps(s, e, [sc]) for s, e, sc in zip(ema.shadow_params, ema_ref, ema_scale))
            print(f"  {tag}, {side}: EMA shadows after 3 steps: {err:.3f} ulps (bound 6)")
            assert ema.optimization_step == 3 and err <= 6.0, (side, err)
        del mods, ps, opt
    print(f"  {tag}: max error in ulps of p after step 1: hip {results['hip']:.3f}  torch {results['torch']:.3f}")
    assert R.within_rule(results["hip"], results["torch"]), results


def test_controlnet_train_step_with_the_hip_optimizer(hip_lib):
    import ctrlv_ref as Ref
    from tests.parity_utils import make_pair
    from tests.test_train_gpu import _batch
    from ctrlv_amd.training import train_step
    config = dict(Ref.TINY_CONFIG)
    bd = {k: v.to(DEV) for k, v in _batch(config, 1, 3, 16, 16, seed=9).items()}

    def make():
        _, _, hu, hc = make_pair(config, DEV, seed=4)
        hc.float()
        for p in hu.parameters():
            p.requires_grad_(False)
        return hu, hc

    _step_parity("ControlNet train_step", make, lambda ms, opt, b: train_step(ms[1], ms[0], bd, optimizer=opt, buckets=b),
                 lambda ms: [p for p in ms[1].parameters() if p.requires_grad])


def test_unet_train_step_with_the_hip_optimizer_and_fused_ema(hip_lib):
    import ctrlv_ref as Ref
    from tests.parity_utils import make_pair
    from tests.test_train_unet_gpu import _batch
    from ctrlv_amd.training import unet_train_step
    config = dict(Ref.TINY_CONFIG)
    bd = {k: v.to(DEV) for k, v in _batch(config, 1, 3, 16, 16, seed=9).items()}

    def make():
        _, _, hu, _ = make_pair(config, DEV, seed=6)
        hu.float()
        hu.enable_grad(all=True)
        return (hu,)

    _step_parity("unet_train_step", make, lambda ms, opt, b: unet_train_step(ms[0], bd, opt, buckets=b),
                 lambda ms: list(ms[0].get_parameters_with_grad()), ema_leg=True)


def test_vae_train_step_with_the_hip_optimizer(hip_lib):
    import copy
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    from ctrlv_amd.training import vae_train_step
    torch.manual_seed(5)
    base = AutoencoderKLTemporalDecoder().eval()
    with torch.no_grad():
        for name, p in base.named_parameters():
            if name.endswith("mix_factor"):
                p.fill_(0.4)
            p.copy_(p.to(torch.bfloat16).float())
    px = (torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(21)) * 2 - 1).to(DEV)

    def make():
        m = copy.deepcopy(base).to(DEV)
        for n, p in m.named_parameters():
            p.requires_grad_(n.startswith("decoder."))
        return (m,)

    def run(ms, opt, b):
        return vae_train_step(ms[0], {"pixel_values": px}, opt, num_frames=2, generator=torch.Generator(device=DEV).manual_seed(9), buckets=b)

    _step_parity("vae_train_step", make, run, lambda ms: list(ms[0].decoder.parameters()))
