"""Global gradient-norm clipping on the GPU: ctrlv_grad_sumsq / ctrlv_grad_finish / ctrlv_adamw_step_dev (csrc/optim.hip) and
`ctrlv_amd.optim.AdamW.step(max_grad_norm=...)`.

Bounds.  The norm: the kernels add exact fp64 products in fp64 (relative error below n * 2^-53, far under an fp32 ulp for every
n here) and round ONCE to fp32, so the norm lies within 1 fp32 ulp of the fp64 reference (tests/grad_clip_ref.py), and may in no
case be further from it than torch's own clip_grad_norm_ total norm in fp32 on the device unless that is below 1 ulp.  The
coefficient, the clipped step, the unclipped equivalence and the skipped step are compared bit for bit."""
import ctypes
import math

import pytest
import torch

from tests import grad_clip_ref as G
from tests import optim_ref as R
from tests.guarded import as_int, check_written_only_inside, guarded_flat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, B1, B2, EPS = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8)
ONE_BITS = 0x3F800000


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hip_norm(lib, g, max_norm=math.inf, grad_scale=1.0, partials=None, state=None, slot0=0):
    """Stage 1 and stage 2 on a flat fp32 tensor: (partials, state); state = int32[4]: norm, coef (fp32 bits), skip, skipped_total."""
    from ctrlv_amd import _lib
    n = g.numel()
    slots = lib.ctrlv_grad_sumsq_partials(n)
    assert slots == (n + G.BLOCK - 1) // G.BLOCK
    if partials is None:
        partials = torch.full((slot0 + slots,), math.nan, dtype=torch.float64, device=DEV)
    if state is None:
        state = torch.zeros(4, dtype=torch.int32, device=DEV)
    _lib.check(lib.ctrlv_grad_sumsq(_ptr(g), n, _ptr(partials), partials.numel(), slot0, _stream()), "ctrlv_grad_sumsq", lib)
    _lib.check(lib.ctrlv_grad_finish(ctypes.c_void_p(partials.data_ptr() + 8 * slot0), slots, grad_scale, max_norm, _ptr(state),
                                     _stream()), "ctrlv_grad_finish", lib)
    return partials, state


def _f(state, i):
    return state[i].view(torch.float32)


def _torch_norm(g):
    p = torch.nn.Parameter(torch.zeros_like(g))
    p.grad = g.clone()
    return float(torch.nn.utils.clip_grad_norm_([p], math.inf))


# ------------------------------------------------------------------------------------------------ 1. norm against fp64
@pytest.mark.parametrize("kind", ["mixed", "huge"])
@pytest.mark.parametrize("n", G.SIZES)
def test_norm_against_fp64(hip_lib, n, kind):
    g = G.case(n, steps=1)[1][0] if kind == "mixed" else G.huge_case(n)
    ref = G.total_norm([g])
    gd = g.to(DEV)
    _, state = _hip_norm(hip_lib, gd)
    torch.cuda.synchronize()
    norm = float(_f(state, 0))
    e_hip, e_torch = G.ulps_of(norm, ref), G.ulps_of(_torch_norm(gd), ref)
    print(f"  n={n} {kind}: norm {norm!r} (fp64 {ref!r}); error in fp32 ulps: hip {e_hip:.3f}  torch {e_torch:.3f}")
    assert math.isfinite(norm) and int(state[2]) == 0 and int(state[3]) == 0
    assert float(_f(state, 1)) == 1.0                       # max_norm = +inf: no clipping
    assert e_hip <= 1.0, (e_hip, e_torch)
    assert e_hip <= max(1.0, e_torch), (e_hip, e_torch)


# ------------------------------------------------------------------------------------------------ 2. determinism and layout
@pytest.mark.parametrize("n", G.SIZES)
def test_two_runs_give_the_same_bits(hip_lib, n):
    g = G.case(n, steps=1)[1][0].to(DEV)
    a, b = _hip_norm(hip_lib, g, max_norm=1.0), _hip_norm(hip_lib, g, max_norm=1.0)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(a[0]).all())                 # every slot was written


LAYOUT_SHAPES = [(5,), (4099,), (320, 3, 3), (2 * G.BLOCK + 3,)]        # two groups; a frozen parameter sits between the first two


def _layout_module(seed=1):
    gen = torch.Generator().manual_seed(seed)
    m = torch.nn.Module()
    for i, shape in enumerate(LAYOUT_SHAPES):
        m.register_parameter(f"w{i}", torch.nn.Parameter(torch.randn(*shape, generator=gen) * 0.1))
    m.register_parameter("frozen", torch.nn.Parameter(torch.randn(9, generator=gen), requires_grad=False))
    return m.to(DEV)


def _layout_groups(m):
    return [{"params": [m.w0, m.frozen, m.w1], "lr": R.f32(1e-3), "weight_decay": R.f32(1e-2)},
            {"params": [m.w2, m.w3], "lr": R.f32(3e-4), "weight_decay": 0.0}]


def test_one_run_and_the_optimisers_layout_agree(hip_lib):
    """The same gradient as ONE run and as the optimiser's layout (two groups, three runs: the frozen parameter splits the first
    group): each norm within 1 ulp of the fp64 reference (bit-identity across different partitions is not promised)."""
    from ctrlv_amd.optim import AdamW
    m = _layout_module()
    opt = AdamW(_layout_groups(m), betas=(B1, B2), eps=EPS)
    gen = torch.Generator().manual_seed(7)
    grads = [torch.randn(*s, generator=gen) * (10.0 ** (i - 1)) for i, s in enumerate(LAYOUT_SHAPES)]
    for i, g in enumerate(grads):
        getattr(m, f"w{i}").grad.copy_(g.to(DEV))
    assert len(opt._runs(0, opt.param_groups[0])) == 2 and len(opt._runs(1, opt.param_groups[1])) == 1
    frozen0 = m.frozen.detach().clone()
    opt.step(max_grad_norm=math.inf)
    st = {k: v.clone() for k, v in opt.grad_state().items()}
    _, one = _hip_norm(hip_lib, torch.cat([g.reshape(-1) for g in grads]).to(DEV))
    torch.cuda.synchronize()
    ref = G.total_norm(grads)
    e_layout, e_one = G.ulps_of(float(st["norm"]), ref), G.ulps_of(float(_f(one, 0)), ref)
    print(f"  layout: norm {float(st['norm'])!r}, one run {float(_f(one, 0))!r}, fp64 {ref!r}: {e_layout:.3f} / {e_one:.3f} ulps")
    assert e_layout <= 1.0 and e_one <= 1.0
    assert int(st["skip"]) == 0 and int(st["skipped_total"]) == 0 and float(st["coef"]) == 1.0
    assert torch.equal(m.frozen.detach(), frozen0)
    # padding took no part and stays zero
    for gi in range(2):
        pbuf, gbuf, _, _, offsets = opt.flat_buffers(gi)
        pad = torch.ones_like(pbuf, dtype=torch.bool)
        for p, off in zip(opt.param_groups[gi]["params"], offsets):
            pad[off:off + p.numel()] = False
        assert float(pbuf[pad].abs().sum()) == 0.0 and float(gbuf[pad].abs().sum()) == 0.0


@pytest.mark.parametrize("n", G.SIZES)
def test_guard_bands(hip_lib, n):
    """Only slots [slot0, slot0 + slots) of the partials array and the 16 bytes of the record are written; g keeps its bits."""
    slots, slot0 = (n + G.BLOCK - 1) // G.BLOCK, 2
    g_buf, g = guarded_flat(n, torch.float32, DEV, fill="poison")
    g.copy_(G.case(n, steps=1)[1][0].to(DEV))
    p_buf, p32 = guarded_flat(2 * (slot0 + slots + 3), torch.float32, DEV, fill="sentinel")    # fp64 slots as pairs of words
    s_buf, s32 = guarded_flat(4, torch.float32, DEV, fill="sentinel")
    partials, state = p32.view(torch.float64), s32.view(torch.int32)
    assert g.data_ptr() % 16 == 0 and partials.data_ptr() % 8 == 0 and state.data_ptr() % 16 == 0
    state[3] = 0                                            # the running count is read: the caller zero-initialises the record
    before = {"g": g_buf.clone(), "partials": p_buf.clone(), "state": s_buf.clone()}
    _hip_norm(hip_lib, g, max_norm=1.0, partials=partials, state=state, slot0=slot0)
    torch.cuda.synchronize()
    assert torch.equal(as_int(g_buf), as_int(before["g"]))
    check_written_only_inside(before["state"], s_buf, s32.view(1, 4), what="state")
    written = p32[2 * slot0:2 * (slot0 + slots)]
    changed = as_int(p_buf) != as_int(before["partials"])
    assert int(changed.sum()) == int((as_int(written) != as_int(before["partials"][1, 64 + 2 * slot0:64 + 2 * (slot0 + slots)])).sum())
    got = partials[slot0:slot0 + slots]
    assert bool(torch.isfinite(got).all())                  # no sentinel (a NaN as an fp64 too) is left in the run's slots
    want = torch.stack([(b.double() ** 2).sum() for b in g.cpu().split(G.BLOCK)])
    assert torch.allclose(got.cpu(), want, rtol=1e-12, atol=0.0)
    assert G.ulps_of(float(_f(state, 0)), G.total_norm([g])) <= 1.0


# ------------------------------------------------------------------------------------------------ 3. coefficient
@pytest.mark.parametrize("max_norm", [1.0, 1e-3, 1e6])
@pytest.mark.parametrize("n", G.SIZES)
def test_coefficient(hip_lib, n, max_norm):
    g = G.case(n, steps=1)[1][0].to(DEV)
    _, state = _hip_norm(hip_lib, g, max_norm=max_norm)
    norm = _f(state, 0)
    want = torch.clamp(torch.tensor(max_norm, dtype=torch.float32, device=DEV) / (norm + 1e-6), max=1.0)
    torch.cuda.synchronize()
    assert want.dtype == torch.float32
    assert int(state[1]) == int(want.view(torch.int32)), (float(_f(state, 1)), float(want))
    assert (float(want) < 1.0) == (R.f32(max_norm) < float(norm) + 1e-6)


def test_coefficient_below_and_above_the_norm(hip_lib):
    g = G.case(4099, steps=1)[1][0].to(DEV)
    coefs = [float(_f(_hip_norm(hip_lib, g, max_norm=mn)[1], 1)) for mn in (1.0, 1e-3, 1e6)]
    assert coefs[0] < 1.0 and coefs[1] < coefs[0] and coefs[2] == 1.0, coefs


# ------------------------------------------------------------------------------------------------ 4. clipped step against torch
@pytest.mark.parametrize("grad_scale", [1.0, 2.0 ** -7])
@pytest.mark.parametrize("wd", [0.0, R.f32(1e-2)])
@pytest.mark.parametrize("n", G.SIZES)
def test_clipped_step_against_torch_bit_for_bit(hip_lib, n, wd, grad_scale):
    """Three steps.  torch's side: the gradient times grad_scale (`mul_`), times the kernel's own coefficient (`mul_`), then one
    torch.optim.AdamW(foreach=False, fused=False) step; ours: step(max_grad_norm=1, grad_scale=...).  p, exp_avg and exp_avg_sq
    are compared with torch.equal."""
    from ctrlv_amd.optim import AdamW
    p0, grads = G.case(n)
    kw = dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    ph, pt = torch.nn.Parameter(p0.to(DEV).clone()), torch.nn.Parameter(p0.to(DEV).clone())
    oh, ot = AdamW([ph], **kw), torch.optim.AdamW([pt], foreach=False, fused=False, **kw)
    coefs = []
    for g in grads:
        ph.grad.copy_(g.to(DEV))
        oh.step(max_grad_norm=1.0, grad_scale=grad_scale)
        coef = oh.grad_state()["coef"].clone()
        pt.grad = g.to(DEV).clone()
        if grad_scale != 1.0:
            pt.grad.mul_(grad_scale)
        pt.grad.mul_(coef)
        ot.step()
        coefs.append(coef)
    torch.cuda.synchronize()
    assert float(oh.state[ph]["step"]) == 3.0 and int(oh.grad_state()["skipped_total"]) == 0
    if n >= 5:
        assert all(float(c) < 1.0 for c in coefs), coefs                 # the clip was active
    for name, a, b in (("p", ph.detach(), pt.detach()), ("exp_avg", oh.state[ph]["exp_avg"], ot.state[pt]["exp_avg"]),
                       ("exp_avg_sq", oh.state[ph]["exp_avg_sq"], ot.state[pt]["exp_avg_sq"])):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert not torch.equal(ph.detach(), p0.to(DEV))


# ------------------------------------------------------------------------------------------------ 5. unclipped equivalence
@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("n", G.SIZES)
def test_step_dev_with_a_unit_record_equals_the_plain_step(hip_lib, n, with_ema):
    from ctrlv_amd import _lib
    p0, grads = G.case(n)
    state = torch.tensor([0, ONE_BITS, 0, 0], dtype=torch.int32, device=DEV)       # coef = 1, skip = 0
    grads = [g.to(DEV) for g in grads]
    out = []
    for dev_path in (False, True):
        p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        e = (p0 * 1.5).to(DEV) if with_ema else None
        for t, g in enumerate(grads, 1):
            args = (_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), n, LR, B1, B2, EPS, R.f32(1e-2), 1.0 - B1 ** t, 1.0 - B2 ** t,
                    R.f32(0.5), R.f32(0.75))
            if dev_path:
                _lib.check(hip_lib.ctrlv_adamw_step_dev(*args, _ptr(state), _stream()), "ctrlv_adamw_step_dev", hip_lib)
            else:
                _lib.check(hip_lib.ctrlv_adamw_step(*args, _stream()), "ctrlv_adamw_step", hip_lib)
        torch.cuda.synchronize()
        out.append((p, m, v) + ((e,) if with_ema else ()))
    for a, b, name in zip(out[0], out[1], ("p", "m", "v", "ema")):
        assert torch.equal(a, b), name
    assert not torch.equal(out[1][0], p0.to(DEV))
    assert state.tolist() == [0, ONE_BITS, 0, 0]            # the record is only read


def test_infinite_max_grad_norm_equals_the_plain_step(hip_lib):
    from ctrlv_amd.optim import AdamW, EMAModel
    gen = torch.Generator().manual_seed(7)
    steps = [[torch.randn(*s, generator=gen) * (10.0 ** (i - 1)) for i, s in enumerate(LAYOUT_SHAPES)] for _ in range(3)]
    out = []
    for max_grad_norm in (None, math.inf):
        m = _layout_module()
        ema = EMAModel(m.parameters())
        opt = AdamW(_layout_groups(m), betas=(B1, B2), eps=EPS)
        for grads in steps:
            for i, g in enumerate(grads):
                getattr(m, f"w{i}").grad.copy_(g.to(DEV))
            opt.step(ema=ema, max_grad_norm=max_grad_norm)
            opt.zero_grad()
        torch.cuda.synchronize()
        out.append([p.detach().clone() for p in m.parameters()] + [s.clone() for s in ema.shadow_params]
                   + [t.clone() for gi in range(2) for t in opt.flat_buffers(gi)[2:4]])
        assert all(float(opt.state[getattr(m, f"w{i}")]["step"]) == 3.0 for i in range(4)) and ema.optimization_step == 3
    assert len(out[0]) == len(out[1]) and all(torch.equal(a, b) for a, b in zip(out[0], out[1]))
    assert float(opt.grad_state()["coef"]) == 1.0 and int(opt.grad_state()["skip"]) == 0


# ------------------------------------------------------------------------------------------------ 6. skip
@pytest.mark.parametrize("bad", [math.inf, math.nan])
@pytest.mark.parametrize("n,pos", [(4099, 0), (4099, 4098), (4099, 4096), (4099, 4095), (4096, 4095), (2 * G.BLOCK - 1, G.BLOCK)])
def test_skipped_step(hip_lib, n, pos, bad):
    """A finite clipped step, two steps whose gradient holds one inf / NaN (element 0, the last element, the n % 4 tail, the last
    vector, another block), a finite step again.  Nothing is read from the device before the comparisons at the end.

    The finite step that follows runs at t = 4, the attempted count.  It is compared (a) bit for bit with `ctrlv_adamw_step` at
    t = 4 on the state the skips left alone, (b) with torch's step at t = 4: exp_avg and exp_avg_sq bit for bit, p by the parity rule
    of tests/test_optim_gpu.py (`optim_ref.within_rule` against the fp64 restatement).  p is NOT bit-equal to torch's from t = 4 on,
    with or without a skip and in `ctrlv_adamw_step` as it was before this feature: the kernel multiplies sqrt(v) by
    1.0f / fp32(sqrt(bias2)), torch by fp32(1.0 / sqrt(bias2)) -- the same fp32 number at t = 1, 2, 3, 5, 7, 8 and neighbours one ulp
    apart at t = 4 and 6 (15.823354721 against 15.823353767 at t = 4).  Measured at n = 4099 without any skip: no differing bit
    after steps 1-3, 65 of 4099 elements of p after step 4, by at most 24 units in the last place of small |p|.  Measured here
    (hip / torch, ulps of p against fp64 at t = 4): n = 4099: 1.820 / 3.320; 4096: 1.705 / 2.455; 8191: 2.339 / 2.751."""
    from ctrlv_amd import _lib
    from ctrlv_amd.optim import AdamW, EMAModel
    p0, grads = G.case(n)
    kw = dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=R.f32(1e-2))
    ph, pt = torch.nn.Parameter(p0.to(DEV).clone()), torch.nn.Parameter(p0.to(DEV).clone())
    ema = EMAModel([ph])
    oh, ot = AdamW([ph], **kw), torch.optim.AdamW([pt], foreach=False, fused=False, **kw)

    def torch_step(g, coef):
        pt.grad = g.to(DEV).clone()
        pt.grad.mul_(coef)
        ot.step()

    # step 1: finite
    ph.grad.copy_(grads[0].to(DEV))
    oh.step(ema=ema, max_grad_norm=1.0)
    torch_step(grads[0], oh.grad_state()["coef"].clone())
    kept = [ph.detach().clone(), oh.state[ph]["exp_avg"].clone(), oh.state[ph]["exp_avg_sq"].clone()]
    ema.shadow_params[0].add_(0.01)                         # (the first EMA step has decay 0: move the shadow off the parameter)
    shadow = ema.shadow_params[0].clone()
    shadow0 = shadow.clone()
    # steps 2 and 3: skipped
    g_bad = grads[1].clone()
    g_bad[pos] = bad
    seen = []
    for k in (2, 3):
        ph.grad.copy_(g_bad.to(DEV))
        oh.step(ema=ema, max_grad_norm=1.0)
        seen.append({key: val.clone() for key, val in oh.grad_state().items()})
        _lib.check(hip_lib.ctrlv_ema_step(_ptr(shadow), _ptr(kept[0]), n, ema.get_decay(k), _stream()), "ctrlv_ema_step", hip_lib)
        assert ema.optimization_step == k and ema.cur_decay_value == ema.get_decay(k)
    after_skip = [ph.detach().clone(), oh.state[ph]["exp_avg"].clone(), oh.state[ph]["exp_avg_sq"].clone(), ema.shadow_params[0].clone()]
    # step 4: finite again; the attempted count is what both sides use as t
    ph.grad.copy_(grads[2].to(DEV))
    oh.step(ema=ema, max_grad_norm=1.0)
    last = {key: val.clone() for key, val in oh.grad_state().items()}
    ot.state[pt]["step"] += 2
    torch_step(grads[2], last["coef"])
    # ... and the same step by the plain kernel, from the state the skipped steps must have left alone, at t = 4
    g4 = grads[2].to(DEV) * last["coef"]
    plain = [t.clone() for t in kept]
    _lib.check(hip_lib.ctrlv_adamw_step(_ptr(plain[0]), _ptr(g4), _ptr(plain[1]), _ptr(plain[2]), None, n, LR, B1, B2, EPS, R.f32(1e-2),
                                        1.0 - B1 ** 4, 1.0 - B2 ** 4, 1.0, 0.0, _stream()), "ctrlv_adamw_step", hip_lib)
    # ---- the comparisons
    torch.cuda.synchronize()
    assert float(oh.state[ph]["step"]) == float(ot.state[pt]["step"]) == 4.0
    for a, b, name in zip(after_skip, kept + [shadow], ("p", "exp_avg", "exp_avg_sq", "shadow")):
        assert torch.equal(a, b), f"{name} after the skipped steps"
    assert not torch.equal(after_skip[3], after_skip[0]) and not torch.equal(after_skip[3], shadow0)     # the shadow moved
    assert [int(s["skip"]) for s in seen] == [1, 1] and [int(s["skipped_total"]) for s in seen] == [1, 2]
    assert all(not math.isfinite(float(s["norm"])) for s in seen)
    assert int(last["skip"]) == 0 and int(last["skipped_total"]) == 2 and 0.0 < float(last["coef"]) < 1.0
    mine = (ph.detach(), oh.state[ph]["exp_avg"], oh.state[ph]["exp_avg_sq"])
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), mine, plain):
        assert torch.equal(a, b), f"{name} after the finite step that followed, against ctrlv_adamw_step at t = 4"
    assert torch.equal(mine[1], ot.state[pt]["exp_avg"]) and torch.equal(mine[2], ot.state[pt]["exp_avg_sq"])       # torch's moments
    ref = R.adamw_step(kept[0].double().cpu(), g4.double().cpu(), kept[1].double().cpu(), kept[2].double().cpu(), 4, LR, B1, B2, EPS,
                       R.f32(1e-2))[0]
    e_hip, e_torch = R.ulps(mine[0], ref, [kept[0]]), R.ulps(pt.detach(), ref, [kept[0]])
    print(f"  n={n} pos={pos} {bad}: step t = 4 after two skips: error in ulps of p: hip {e_hip:.3f}  torch {e_torch:.3f}   "
          f"(elements whose bits differ from torch's: {int((mine[0] != pt.detach()).sum())})")
    assert R.within_rule(e_hip, e_torch), (e_hip, e_torch)
    assert not torch.equal(ph.detach(), kept[0])


# ------------------------------------------------------------------------------------------------ 7. through unet_train_step
def test_through_unet_train_step(hip_lib):
    """The tiny UNet: a clipped step equals the unclipped gradients (bit-reproducible) times the reported
    coefficient, stepped by the existing path; max_grad_norm=None equals the step without the argument."""
    import ctrlv_ref as Ref
    from tests.parity_utils import make_pair
    from tests.test_train_unet_gpu import _batch
    from ctrlv_amd.optim import AdamW
    from ctrlv_amd.training import unet_train_step
    config = dict(Ref.TINY_CONFIG)
    bd = {k: v.to(DEV) for k, v in _batch(config, 1, 3, 16, 16, seed=9).items()}
    kw = dict(lr=R.f32(1e-3), betas=(B1, B2), eps=EPS, weight_decay=R.f32(1e-2))

    def make():
        _, _, hu, _ = make_pair(config, DEV, seed=6)
        hu.float()
        hu.enable_grad(all=True)
        ps = list(hu.get_parameters_with_grad())
        return hu, ps, AdamW(ps, **kw)

    def by_hand(coef):
        hu, ps, opt = make()
        unet_train_step(hu, bd, None)                       # the gradients land in the optimiser's views
        if coef is not None:
            for p in ps:
                p.grad.mul_(coef)
        opt.step()
        return [p.detach().clone() for p in ps]

    hu, ps, opt = make()
    p0 = [p.detach().clone() for p in ps]
    loss = unet_train_step(hu, bd, opt, max_grad_norm=1e-3)
    st = {k: v.clone() for k, v in opt.grad_state().items()}
    clipped = [p.detach().clone() for p in ps]
    want = by_hand(st["coef"])
    hu2, ps2, opt2 = make()
    unet_train_step(hu2, bd, opt2, max_grad_norm=None)
    hu3, ps3, opt3 = make()
    unet_train_step(hu3, bd, opt3)
    plain = by_hand(None)
    torch.cuda.synchronize()
    print(f"  unet_train_step: loss {float(loss):.6f}  norm {float(st['norm']):.6g}  coef {float(st['coef']):.6g}")
    assert math.isfinite(float(loss)) and int(st["skip"]) == 0 and 0.0 < float(st["coef"]) < 1.0
    assert all(torch.equal(a, b) for a, b in zip(clipped, want))
    assert any(not torch.equal(a, b) for a, b in zip(clipped, p0))
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps2, plain)) and all(torch.equal(p.detach(), b) for p, b in zip(ps3, plain))
    assert any(not torch.equal(a, b) for a, b in zip(clipped, plain))
    assert all(float(p.grad.abs().sum()) == 0.0 for p in ps[:3])                                   # zero_grad ran after the step
    with pytest.raises(RuntimeError, match="grad_state"):
        opt2.grad_state()                                   # None took the plain path: no record was made
